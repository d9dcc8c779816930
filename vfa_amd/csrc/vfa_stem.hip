// vfa_stem.hip -- the stem of the ResNet trunk at inference (reference resnet.py:100-102, 139-140: a 7 x 7 stride-2 convolution of three
// channels without bias, GroupNorm, ReLU, a 3 x 3 stride-2 max pooling): float32 in and out, the images (B, 3, L, W) read through their
// four element strides, the outputs contiguous.  Fixed summation order, no atomics: the same bits on every run, and an image gives the
// same bits alone and in a batch.  The GroupNorm between the two kernels is vfa_group_norm_affine_f32 on the raw map.  The integer
// rules: vfa_stem.h.
//
//   1. stem_pack_kernel: the weight (O, 3, 7, 7) into the packed form of vfa_stem.h (148 x 64 floats, zeros past O and at k = 147), in
//      front of every convolution: 38 KB, cheaper than keeping it.
//   2. stem_conv_kernel: an implicit GEMM on the exact f32 MFMA v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain, one rounding per
//      product): M = outputs, N = output cells, K = 148.  A workgroup of 4 waves copies the packed weight to LDS once and walks
//      over tiles of 4 x 32 output cells of one image, wave w taking row w: per tile the 3 x 13 x 69 window is loaded in image
//      order (consecutive threads on consecutive addresses; a position outside the image is a zero and is never addressed) and stored
//      at its LOCATION; the next tile's window is in flight in registers under this tile's products.  Per k pair a lane reads its B
//      operand (cell rx = lane & 31, k = 2 s + (lane >> 5)) with one 4-byte LDS read -- 32 consecutive floats per half wave -- and
//      both A operands (outputs r and 32 + r) with one 8-byte read.  ONE chain per output over k = (c 7 + ky) 7 + kx ascending; the
//      padded k = 147 is a zero times a zero.  The output is stored as MFMA rows: 32 consecutive floats of an NCHW row.
//   3. stem_pool_kernel: out = max over the 3 x 3 taps inside the map of max(fmaf(a[b, c], y, b[b, c]), 0); a NaN tap makes the cell
//      a NaN, as torch's pooling does.  One thread per output cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"
#include "vfa_stem.h"

namespace {

using namespace vfa_stem;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWinLoads = (kWinValues + kThreads - 1) / kThreads; // 11
constexpr int kTargetGroups = 1536; // workgroups of a launch where there are that many tiles: six per compute unit
static_assert(kThreads / 64 == kTileRows, "one wave per row of a tile");
static_assert(kPackedFloats % 4 == 0, "the packed weight is copied in 16-byte pieces");
static_assert(cell_base(kTileRows - 1, kTileCols - 1) + tap_offset(kK - 1) < kWinLocations, "the last tap of the last cell lies inside the window");

struct Image {
    const float *x;
    long long s_frame;         // element strides, >= 0; inside an image every offset fits 31 bits (the entry point refuses others)
    int s_chan, s_row, s_col;
    int B, L, W;
};

__global__ __launch_bounds__(kThreads) void stem_pack_kernel(const float *__restrict__ weight, int O, float *__restrict__ packed)
{
    const int i = blockIdx.x * kThreads + threadIdx.x; // = packed_index(o, k)
    if (i >= kPackedFloats) return;
    const int k = i / kMaxOut, o = 32 * (i & 1) + (i % kMaxOut) / 2;
    packed[i] = k < kK && o < O ? weight[o * kK + k] : 0.0f;
}

// value e = tid + kThreads j of a tile's window: channel c and position q = wy kWinCols + wx, consecutive threads on consecutive
// addresses of the image (CHAN_FAST: a channels-last image).  The empty asm makes e opaque: (c, q) are a few integer operations per
// tile, and the compiler would otherwise keep all of them in registers across the products.
template <bool CHAN_FAST> __device__ __forceinline__ int value_of(int tid, int j, int &c, int &q)
{
    int e = tid + kThreads * j;
    asm volatile("" : "+v"(e));
    if (CHAN_FAST) { c = e % kChannels; q = e / kChannels; }
    else { c = e / (kWinRows * kWinCols); q = e % (kWinRows * kWinCols); }
    return e;
}

// A position outside the image is a zero; its lane reads the image's first element instead (no branch, and no address outside).
template <bool CHAN_FAST> __device__ __forceinline__ void window_load(const Image m, int b, int y0, int x0, int tid, float (&v)[kWinLoads])
{
    const float *image = m.x + b * m.s_frame;
#pragma unroll
    for (int j = 0; j < kWinLoads; ++j) {
        int c, q, cc, y, x;
        const int e = value_of<CHAN_FAST>(tid, j, c, q);
        const bool ok = window_position(c * (kWinRows * kWinCols) + q, y0, x0, m.L, m.W, cc, y, x) && e < kWinValues;
        const unsigned at = (unsigned)c * (unsigned)m.s_chan + (unsigned)y * (unsigned)m.s_row + (unsigned)x * (unsigned)m.s_col;
        const float t = image[ok ? at : 0u];
        v[j] = ok ? t : 0.0f;
    }
}

template <bool CHAN_FAST> __device__ __forceinline__ void window_store(float *win, int tid, const float (&v)[kWinLoads])
{
#pragma unroll
    for (int j = 0; j < kWinLoads; ++j) {
        int c, q;
        const int e = value_of<CHAN_FAST>(tid, j, c, q);
        if (e < kWinValues) win[window_location(c, q / kWinCols, q % kWinCols)] = v[j];
    }
}

constexpr int kGroup = 8, kGroups = (kSteps + kGroup - 1) / kGroup;

constexpr bool pair_slots_known()
{
    for (int s = 0; s < kSteps; ++s)
        if (pair_slot(s) < 0) return false;
    return true;
}
static_assert(pair_slots_known(), "every k pair has one of the kPairDeltas distances between its two taps");

// the operands of the k pairs s = kGroup g .. of a lane: B from the window at b_half[slot] + an offset that is the same for both
// halves of the wave (a padded k: a zero whatever the window holds), both A from the packed weight
__device__ __forceinline__ void read_operands(const float *a_mine, const float *const (&b_half)[kPairDeltas], int h, int g, float2 (&av)[kGroup],
                                              float (&bv)[kGroup])
{
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
        const int s = g * kGroup + j;
        if (s >= kSteps) continue;
        bv[j] = b_half[pair_slot(s)][tap_offset(2 * s)];
        if (2 * s + 1 >= kK) bv[j] = h ? 0.0f : bv[j];
        av[j] = *(const float2 *)(a_mine + 2 * s * kMaxOut);
    }
}

// grid (workgroups of an image, image); workgroup g takes the tiles g, g + gridDim.x, ...
template <bool CHAN_FAST>
__global__ __launch_bounds__(kThreads, 3) void stem_conv_kernel(const Image m, const float *__restrict__ packed, int O, int Lo, int Wo, float *__restrict__ out)
{
    __shared__ __align__(16) float lds[kPackedFloats + kWinLocations];
    float *win = lds + kPackedFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, n_tiles = tiles_x(Wo) * tiles_y(Lo);

    int tile = blockIdx.x, y0, x0;
    float v[kWinLoads];
    tile_origin(tile, Wo, y0, x0);
    window_load<CHAN_FAST>(m, b, y0, x0, tid, v);
    for (int i = tid; i < kPackedFloats / 4; i += kThreads) ((float4 *)lds)[i] = ((const float4 *)packed)[i];
    window_store<CHAN_FAST>(win, tid, v);
    __syncthreads();

    const float *a_mine = lds + h * kMaxOut + 2 * r; // row k = 2 s + h of the packed weight, the pair of outputs (r, 32 + r)
    const float *b_mine = win + cell_base(wave, r);
    const float *const b_half[kPairDeltas] = {b_mine + h * pair_delta(0), b_mine + h * pair_delta(1), b_mine + h * pair_delta(2), b_mine + h * pair_delta(3),
                                             b_mine + h * pair_delta(4)};
    while (true) {
        const int next = tile + (int)gridDim.x;
        const bool more = next < n_tiles; // (uniform)
        int ny0 = 0, nx0 = 0;
        if (more) {
            tile_origin(next, Wo, ny0, nx0);
            window_load<CHAN_FAST>(m, b, ny0, nx0, tid, v);
        }
        f32x16 acc[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[n][i] = 0.0f;
        // groups of kGroup k pairs: the next group's operands are read under this group's products, and a scheduling fence between
        // the groups keeps the compiler from reading all 74 pairs ahead (which costs the registers of two workgroups per unit)
        float bv[2][kGroup];
        float2 av[2][kGroup];
        read_operands(a_mine, b_half, h, 0, av[0], bv[0]);
#pragma unroll
        for (int g = 0; g < kGroups; ++g) { // A: rows = outputs, lane (r, h) holds k = 2 s + h; B: columns = cells
            if (g + 1 < kGroups) read_operands(a_mine, b_half, h, g + 1, av[(g + 1) & 1], bv[(g + 1) & 1]);
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                if (g * kGroup + j >= kSteps) continue;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][j].x, bv[g & 1][j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][j].y, bv[g & 1][j], acc[1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int y = y0 + wave, x = x0 + r;
        if (y < Lo && x < Wo) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) { // C/D: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
                    const int o = 32 * n + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (o < O) out[(((size_t)b * O + o) * Lo + y) * Wo + x] = acc[n][i];
                }
        }
        if (!more) break;
        __syncthreads(); // every wave has read this tile's window
        window_store<CHAN_FAST>(win, tid, v);
        __syncthreads();
        tile = next;
        y0 = ny0;
        x0 = nx0;
    }
}

// grid (blocks of 1024 output positions of a plane, (image, channel) pairs in a grid-stride loop)
constexpr int kPoolPerThread = 4;
__global__ __launch_bounds__(kThreads) void stem_pool_kernel(const float *__restrict__ y, const float *__restrict__ a, const float *__restrict__ b, int BC,
                                                             int L, int W, int Lo, int Wo, float *__restrict__ out)
{
    const int plane = Lo * Wo;
    for (int bc = blockIdx.y; bc < BC; bc += gridDim.y) {
        const float ya = a[bc], yb = b[bc];
        const float *src = y + (size_t)bc * L * W;
#pragma unroll
        for (int k = 0; k < kPoolPerThread; ++k) {
            const int p = (blockIdx.x * kPoolPerThread + k) * kThreads + threadIdx.x;
            if (p >= plane) break;
            const int oy = p / Wo, ox = p - oy * Wo;
            const int x_first = pool_first(ox), x_last = pool_last(ox, W);
            float best = -INFINITY; // (every cell has its centre tap, and a tap is >= 0 or a NaN)
            for (int ty = pool_first(oy); ty <= pool_last(oy, L); ++ty)
                for (int tx = x_first; tx <= x_last; ++tx) {
                    float t = fmaf(ya, src[(size_t)ty * W + tx], yb);
                    t = t < 0.0f ? 0.0f : t;                 // (a NaN stays a NaN)
                    best = (t > best || t != t) ? t : best; // ... and takes the cell: nothing is greater than a NaN
                }
            out[(size_t)bc * plane + p] = best;
        }
    }
}

} // namespace

extern "C" {

size_t vfa_stem_workspace_bytes(int O)
{
    if (O < 1 || O > kMaxOut) return 0;
    return kPackedFloats * sizeof(float);
}

int vfa_stem_conv_f32(const float *x, const long long *x_stride, const float *weight, int B, int C, int L, int W, int O, float *out, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    if (B < 0 || C < 1 || L < 0 || W < 0 || O < 1) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || (long long)L * W == 0) return 0;
    if (!x || !x_stride || !weight || !out) return VFA_ERR_BAD_ARGUMENT;
    if (x_stride[0] < 0 || x_stride[1] < 0 || x_stride[2] < 0 || x_stride[3] < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2) return VFA_ERR_UNSUPPORTED;
    if (C != kChannels || O > kMaxOut) return VFA_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < vfa_stem_workspace_bytes(O)) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if ((kChannels - 1) * x_stride[1] + (L - 1) * x_stride[2] + (W - 1) * x_stride[3] > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const Image m = {x, x_stride[0], (int)x_stride[1], (int)x_stride[2], (int)x_stride[3], B, L, W};
    float *packed = (float *)workspace;
    hipLaunchKernelGGL(stem_pack_kernel, dim3((kPackedFloats + kThreads - 1) / kThreads), dim3(kThreads), 0, s, weight, O, packed);
    const int Lo = conv_out(L), Wo = conv_out(W), n_tiles = tiles_x(Wo) * tiles_y(Lo);
    // the same number of tiles for every workgroup, up to one: the weight is copied to LDS once per workgroup
    const long long per_group = ((long long)n_tiles * B + kTargetGroups - 1) / kTargetGroups;
    const int groups = (int)((n_tiles + per_group - 1) / per_group);
    const dim3 grid((unsigned)groups, (unsigned)B);
    if (m.s_chan == 1) hipLaunchKernelGGL(stem_conv_kernel<true>, grid, dim3(kThreads), 0, s, m, packed, O, Lo, Wo, out);
    else hipLaunchKernelGGL(stem_conv_kernel<false>, grid, dim3(kThreads), 0, s, m, packed, O, Lo, Wo, out);
    return (int)hipGetLastError();
}

int vfa_stem_pool_f32(const float *y, const float *a, const float *b, int B, int C, int L, int W, float *out, void *stream)
{
    if (B < 0 || C < 0 || L < 0 || W < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || C == 0 || (long long)L * W == 0) return 0;
    if (!y || !a || !b || !out) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const int Lo = pool_out(L), Wo = pool_out(W), BC = B * C, per_block = kThreads * kPoolPerThread;
    const dim3 grid((unsigned)((Lo * Wo + per_block - 1) / per_block), (unsigned)(BC < 65535 ? BC : 65535));
    hipLaunchKernelGGL(stem_pool_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, y, a, b, BC, L, W, Lo, Wo, out);
    return (int)hipGetLastError();
}

} // extern "C"
