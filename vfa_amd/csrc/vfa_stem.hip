// vfa_stem.hip -- the stem of the ResNet trunk, at inference and with gradients (reference resnet.py:100-102, 139-140: a 7 x 7
// stride-2 convolution of three channels without bias, GroupNorm, ReLU, a 3 x 3 stride-2 max pooling): float32 in and out, the images (B, 3, L, W) read through their
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
//
// With gradients (ops.stem_train) the forward is the same three launches; the backward is vfa_group_norm_backward_f32 between two
// kernels of this file:
//   4. stem_pool_backward_kernel: u = the gradient behind the ReLU, a gather per element of u.  A workgroup stages the taps of a
//      32 x 64 tile of the raw map in LDS (recomputed with the forward's bits: the forward saves no winner), decides every window's
//      winner once under the forward's rule, and adds to each position the gout of the windows it won in ascending window order.
//   5. stem_wgrad_kernel + stem_wgrad_merge_kernel: the weight gradient as an implicit GEMM on the same f32 MFMA with the output
//      cells as K: M = outputs, N = 147 taps padded to 160.  The cells are cut into slabs by a rule of (Lo, Wo) alone; a workgroup
//      owns one (image, slab), its four waves split K (a row of every tile each) and hold all ten 32 x 32 accumulators, merged in
//      LDS in wave order; the (image, slab) partials are added in float64 in ascending order and rounded once.
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

// ---- training: the two backward kernels of the stem the library does not already have ----------------------------------------------

// grid (tiles of kPoolTileRows x kPoolTileCols positions of a plane, (image, channel) pairs in a grid-stride loop).  Three passes over
// LDS: the tile's taps max(fmaf(a, y, b), 0) with the forward's bits; per window its winner under the forward's rule and its gout;
// per position of u the windows that contain it, ascending, those it won added from +0.
__global__ __launch_bounds__(kThreads) void stem_pool_backward_kernel(const float *__restrict__ y, const float *__restrict__ a, const float *__restrict__ b,
                                                                      const float *__restrict__ gout, int BC, int L, int W, int Lo, int Wo,
                                                                      float *__restrict__ u)
{
    __shared__ float taps[kPoolTapRows * kPoolTapCols];
    __shared__ float gwin[kPoolWinRows * kPoolWinCols];
    __shared__ unsigned char winner[kPoolWinRows * kPoolWinCols];
    const int tid = threadIdx.x, tx_count = pool_tiles_x(W);
    const int p0 = ((int)blockIdx.x / tx_count) * kPoolTileRows, q0 = ((int)blockIdx.x % tx_count) * kPoolTileCols;
    const int i0 = p0 / 2, j0 = q0 / 2;
    for (int bc = blockIdx.y; bc < BC; bc += gridDim.y) {
        const float ya = a[bc], yb = b[bc];
        const float *src = y + (size_t)bc * L * W;
        const float *gsrc = gout + (size_t)bc * Lo * Wo;
        for (int e = tid; e < kPoolTapRows * kPoolTapCols; e += kThreads) {
            const int r = e / kPoolTapCols, c = e - r * kPoolTapCols, p = p0 - 1 + r, q = q0 - 1 + c;
            if (p >= 0 && p < L && q >= 0 && q < W) { // (a position outside the map is never read below: the taps are pool_first .. pool_last)
                const float t = fmaf(ya, src[(size_t)p * W + q], yb);
                taps[e] = t < 0.0f ? 0.0f : t;
            }
        }
        __syncthreads();
        for (int e = tid; e < kPoolWinRows * kPoolWinCols; e += kThreads) {
            const int wi = e / kPoolWinCols, i = i0 + wi, j = j0 + e - wi * kPoolWinCols;
            int code = kNoWinner;
            float g = 0.0f;
            if (i < Lo && j < Wo) {
                float best = -INFINITY;
                const int x_first = pool_first(j), x_last = pool_last(j, W);
                for (int ty = pool_first(i); ty <= pool_last(i, L); ++ty)
                    for (int tx = x_first; tx <= x_last; ++tx) { // the forward's scan and the forward's rule
                        const float t = taps[(ty - p0 + 1) * kPoolTapCols + (tx - q0 + 1)];
                        if (t > best || t != t) {
                            best = t;
                            code = pool_tap_code(i, j, ty, tx);
                        }
                    }
                g = gsrc[(size_t)i * Wo + j];
            }
            winner[e] = (unsigned char)code;
            gwin[e] = g;
        }
        __syncthreads();
        for (int e = tid; e < kPoolTileRows * kPoolTileCols; e += kThreads) {
            const int ly = e / kPoolTileCols, p = p0 + ly, q = q0 + e - ly * kPoolTileCols;
            if (p < L && q < W) {
                float s = 0.0f;
                const int j_first = pool_window_first(q), j_last = pool_window_last(q, Wo);
                for (int i = pool_window_first(p); i <= pool_window_last(p, Lo); ++i)
                    for (int j = j_first; j <= j_last; ++j) {
                        const int w = (i - i0) * kPoolWinCols + (j - j0);
                        if (winner[w] == pool_tap_code(i, j, p, q)) s += gwin[w];
                    }
                u[(size_t)bc * L * W + (size_t)p * W + q] = s;
            }
        }
        __syncthreads(); // the next plane overwrites the three arrays
    }
}

// The weight gradient: M = outputs (two 32-row blocks), N = the 147 taps padded to kNBlocks 32-column blocks, K = output cells, two
// per v_mfma_f32_32x32x2_f32.  grid (slab, image); a workgroup walks its slab's tiles ascending.  Per tile the window of x is staged
// as the forward stages it (the B operand of tap k and cell (ry, rx) is the forward's location cell_base + tap_offset), and the
// 64 x 4 x 32 tile of g as [cell][output] with a pitch of kGPitch floats, zeros past O and past the map.  Wave w takes row w of the
// tile -- the waves split K -- and holds all 2 x kNBlocks accumulators (one workgroup per compute unit; the next tile's operands wait in registers): per pair of cells 2 reads of g, kNBlocks reads of the window,
// 2 kNBlocks products.  A cell past the map and a padded tap are zero OPERANDS on both sides.  At the end the four waves' sums are
// merged through LDS as ((w0 + w1) + w2) + w3 and written as the (image, slab) partial.
constexpr int kGPitch = kMaxOut + 1;
constexpr int kGFloats = kTileRows * kTileCols * kGPitch;
constexpr int kGLoads = kMaxOut * kTileRows * kTileCols / kThreads; // 32
constexpr int kAccFloats = 2 * kNBlocks * 16 * 64;
static_assert(kAccFloats <= kGFloats + kWinLocations, "the waves' sums are merged in the LDS of the operands");
static_assert(kTileCols % 2 == 0 && kNBlocks * 32 >= kK, "two cells per product; every tap has a column");

// element e = tid + kThreads j of a tile of g: output e >> 7 = (tid >> 7) + 2 j, row (tid >> 5) & 3, column tid & 31 -- a thread keeps
// its cell and walks the outputs, consecutive threads on consecutive addresses; an output past O and a cell past the map are zeros
// (their lanes read the map's first element instead).  The loaded values stay untouched until they are stored, so that nothing waits
// for a load under the products of the tile before -> whether the thread's cell lies in the map.
__device__ __forceinline__ bool g_load(const float *__restrict__ gp, int O, int Lo, int Wo, int y0, int x0, int tid, float (&gv)[kGLoads])
{
    const int yy = y0 + ((tid >> 5) & 3), xx = x0 + (tid & 31), o0 = tid >> 7;
    const bool cell_ok = yy < Lo && xx < Wo;
    const size_t plane = (size_t)Lo * Wo, first = (size_t)o0 * plane + (size_t)(yy * Wo + xx);
#pragma unroll
    for (int j = 0; j < kGLoads; ++j) gv[j] = gp[cell_ok && o0 + 2 * j < O ? first + (size_t)(2 * j) * plane : (size_t)0];
    return cell_ok;
}

__device__ __forceinline__ void g_store(float *gl, int tid, const float (&gv)[kGLoads], bool cell_ok, int O)
{
    const int o0 = tid >> 7;
#pragma unroll
    for (int j = 0; j < kGLoads; ++j) gl[(tid & 127) * kGPitch + o0 + 2 * j] = cell_ok && o0 + 2 * j < O ? gv[j] : 0.0f;
}

// value_of without its fence: one workgroup per unit has the registers to keep what depends on the thread alone across the tiles
template <bool CHAN_FAST> __device__ __forceinline__ int value_kept(int tid, int j, int &c, int &q)
{
    const int e = tid + kThreads * j;
    if (CHAN_FAST) { c = e % kChannels; q = e / kChannels; }
    else { c = e / (kWinRows * kWinCols); q = e % (kWinRows * kWinCols); }
    return e;
}

// window_load and window_store in the same form: the zero of a position outside the image is applied at the store
template <bool CHAN_FAST> __device__ __forceinline__ unsigned window_load_raw(const Image m, int b, int y0, int x0, int tid, float (&v)[kWinLoads])
{
    const float *image = m.x + b * m.s_frame;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < kWinLoads; ++j) {
        int c, q, cc, y, x;
        const int e = value_kept<CHAN_FAST>(tid, j, c, q);
        const bool ok = window_position(c * (kWinRows * kWinCols) + q, y0, x0, m.L, m.W, cc, y, x) && e < kWinValues;
        const unsigned at = (unsigned)c * (unsigned)m.s_chan + (unsigned)y * (unsigned)m.s_row + (unsigned)x * (unsigned)m.s_col;
        v[j] = image[ok ? at : 0u];
        mask |= (unsigned)ok << j;
    }
    return mask;
}

template <bool CHAN_FAST> __device__ __forceinline__ void window_store_masked(float *win, int tid, const float (&v)[kWinLoads], unsigned ok)
{
#pragma unroll
    for (int j = 0; j < kWinLoads; ++j) {
        int c, q;
        const int e = value_kept<CHAN_FAST>(tid, j, c, q);
        if (e < kWinValues) win[window_location(c, q / kWinCols, q % kWinCols)] = (ok >> j & 1u) ? v[j] : 0.0f;
    }
}

// the operands of the pairs of cells s = kPairGroup g ..: both A (outputs r and 32 + r) and the kNBlocks B (this lane's taps)
constexpr int kPairGroup = 2, kPairGroups = kTileCols / 2 / kPairGroup;
__device__ __forceinline__ void read_pairs(const float *ga, const float *wb, const int (&toff)[kNBlocks], int g, float (&av)[kPairGroup][2],
                                           float (&bv)[kPairGroup][kNBlocks])
{
#pragma unroll
    for (int j = 0; j < kPairGroup; ++j) {
        const int s = g * kPairGroup + j;
        av[j][0] = ga[2 * s * kGPitch];
        av[j][1] = ga[2 * s * kGPitch + 32];
#pragma unroll
        for (int nb = 0; nb < kNBlocks; ++nb) bv[j][nb] = wb[toff[nb] + 2 * s];
    }
}

template <bool CHAN_FAST>
__global__ __launch_bounds__(kThreads, 1) void stem_wgrad_kernel(const Image m, const float *__restrict__ g, int O, int Lo, int Wo, int n_slabs,
                                                                 float *__restrict__ partial)
{
    __shared__ __align__(16) float lds[kGFloats + kWinLocations];
    float *gl = lds, *win = lds + kGFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int slab = blockIdx.x, b = blockIdx.y;
    const int t_begin = wgrad_slab_begin(slab, Lo, Wo), t_end = wgrad_slab_begin(slab + 1, Lo, Wo);
    const float *gp = g + (size_t)b * O * Lo * Wo;

    f32x16 acc[2][kNBlocks];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < kNBlocks; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.0f;
    int toff[kNBlocks]; // this lane's taps k = 32 nb + r: where they lie behind a cell's base, and whether they are taps at all
    bool kok[kNBlocks];
#pragma unroll
    for (int nb = 0; nb < kNBlocks; ++nb) {
        toff[nb] = tap_offset(32 * nb + r);
        kok[nb] = 32 * nb + r < kK;
    }
    const float *ga = gl + (wave * kTileCols + h) * kGPitch + r;
    const float *wb = win + cell_base(wave, h);

    int tile = t_begin, y0, x0;
    float v[kWinLoads], gv[kGLoads];
    tile_origin(tile, Wo, y0, x0);
    unsigned v_ok = window_load_raw<CHAN_FAST>(m, b, y0, x0, tid, v);
    bool g_ok = g_load(gp, O, Lo, Wo, y0, x0, tid, gv);
    window_store_masked<CHAN_FAST>(win, tid, v, v_ok);
    g_store(gl, tid, gv, g_ok, O);
    __syncthreads();
    while (true) {
        const int next = tile + 1;
        const bool more = next < t_end; // (uniform)
        int ny0 = 0, nx0 = 0;
        if (more) { // the next tile's operands are in flight in registers under this tile's products
            tile_origin(next, Wo, ny0, nx0);
            v_ok = window_load_raw<CHAN_FAST>(m, b, ny0, nx0, tid, v);
            g_ok = g_load(gp, O, Lo, Wo, ny0, nx0, tid, gv);
        }
        if (y0 + wave < Lo) { // (uniform in a wave)
            // groups of kPairGroup pairs: the next group's operands are read under this group's products (a scheduling fence between
            // the groups keeps that order); a pair of cells past the map is zeros times zeros
            float av[2][kPairGroup][2], bv[2][kPairGroup][kNBlocks];
            read_pairs(ga, wb, toff, 0, av[0], bv[0]);
#pragma unroll
            for (int g2 = 0; g2 < kPairGroups; ++g2) {
                if (g2 + 1 < kPairGroups) read_pairs(ga, wb, toff, g2 + 1, av[(g2 + 1) & 1], bv[(g2 + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0); // (the reads are issued in front of the products, not among them)
#pragma unroll
                for (int j = 0; j < kPairGroup; ++j) {
                    const bool cell_ok = x0 + 2 * (g2 * kPairGroup + j) + h < Wo;
#pragma unroll
                    for (int nb = 0; nb < kNBlocks; ++nb) { // A: rows = outputs, lane (r, h) holds cell 2 s + h; B: columns = taps
                        const float t = kok[nb] && cell_ok ? bv[g2 & 1][j][nb] : 0.0f;
                        acc[0][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g2 & 1][j][0], t, acc[0][nb], 0, 0, 0);
                        acc[1][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g2 & 1][j][1], t, acc[1][nb], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!more) break;
        __syncthreads(); // every wave has read this tile's operands
        window_store_masked<CHAN_FAST>(win, tid, v, v_ok);
        g_store(gl, tid, gv, g_ok, O);
        __syncthreads();
        tile = next;
        y0 = ny0;
        x0 = nx0;
    }

    __syncthreads();
    float *ml = lds + lane; // the sums of the waves before this one, [accumulator register][lane]
#pragma unroll
    for (int w = 0; w < kTileRows; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < kNBlocks; ++nb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int at = ((mb * kNBlocks + nb) * 16 + i) * 64;
                        if (w > 0) acc[mb][nb][i] = ml[at] + acc[mb][nb][i];
                        if (w < kTileRows - 1) ml[at] = acc[mb][nb][i];
                    }
        }
        if (w < kTileRows - 1) __syncthreads();
    }
    if (wave != kTileRows - 1) return;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < kNBlocks; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { // C/D: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
                const int o = 32 * mb + (i & 3) + 8 * (i >> 2) + 4 * h, k = 32 * nb + r;
                if (o < O && k < kK) partial[wgrad_partial_index(b, slab, n_slabs, o, k, O)] = acc[mb][nb][i];
            }
}

// one thread per element (o, k) of dw: the partials in ascending (image, slab) order, summed in float64, rounded once
constexpr int kMergeAhead = 32;
__global__ __launch_bounds__(kThreads) void stem_wgrad_merge_kernel(const float *__restrict__ partial, int n_partials, int per, float *__restrict__ dw)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= per) return;
    double sum = 0.0;
    int k = 0;
    for (; k + kMergeAhead <= n_partials; k += kMergeAhead) { // the loads of a batch are in flight together; the additions stay in order
        float t[kMergeAhead];
#pragma unroll
        for (int j = 0; j < kMergeAhead; ++j) t[j] = partial[(size_t)(k + j) * per + i];
#pragma unroll
        for (int j = 0; j < kMergeAhead; ++j) sum += (double)t[j];
    }
    for (; k < n_partials; ++k) sum += (double)partial[(size_t)k * per + i];
    dw[i] = (float)sum;
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

int vfa_stem_pool_backward_f32(const float *gout, const float *y, const float *a, const float *b, int B, int C, int L, int W, float *u, void *stream)
{
    if (B < 0 || C < 0 || L < 0 || W < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || C == 0 || (long long)L * W == 0) return 0;
    if (!gout || !y || !a || !b || !u) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const int Lo = pool_out(L), Wo = pool_out(W), BC = B * C;
    const dim3 grid((unsigned)(pool_tiles_x(W) * pool_tiles_y(L)), (unsigned)(BC < 65535 ? BC : 65535));
    hipLaunchKernelGGL(stem_pool_backward_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, y, a, b, gout, BC, L, W, Lo, Wo, u);
    return (int)hipGetLastError();
}

// 0: no such problem, or an empty one
size_t vfa_stem_conv_wgrad_workspace_bytes(int B, int O, int L, int W)
{
    if (B <= 0 || O < 1 || O > kMaxOut || L <= 0 || W <= 0 || B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2) return 0;
    return (size_t)B * wgrad_slabs(conv_out(L), conv_out(W)) * wgrad_partial_floats(O) * sizeof(float);
}

int vfa_stem_conv_wgrad_f32(const float *g, const float *x, const long long *x_stride, int B, int L, int W, int O, float *dw, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (B < 0 || L < 0 || W < 0 || O < 1 || !dw) return VFA_ERR_BAD_ARGUMENT;
    if (O > kMaxOut || B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2) return VFA_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || (long long)L * W == 0) return (int)hipMemsetAsync(dw, 0, (size_t)O * kK * sizeof(float), s); // an empty sum
    if (!g || !x || !x_stride) return VFA_ERR_BAD_ARGUMENT;
    if (x_stride[0] < 0 || x_stride[1] < 0 || x_stride[2] < 0 || x_stride[3] < 0) return VFA_ERR_BAD_ARGUMENT;
    if ((kChannels - 1) * x_stride[1] + (L - 1) * x_stride[2] + (W - 1) * x_stride[3] > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < vfa_stem_conv_wgrad_workspace_bytes(B, O, L, W)) return VFA_ERR_BAD_ARGUMENT;
    const Image m = {x, x_stride[0], (int)x_stride[1], (int)x_stride[2], (int)x_stride[3], B, L, W};
    const int Lo = conv_out(L), Wo = conv_out(W), n_slabs = wgrad_slabs(Lo, Wo), per = (int)wgrad_partial_floats(O);
    float *partial = (float *)workspace;
    const dim3 grid((unsigned)n_slabs, (unsigned)B);
    if (m.s_chan == 1) hipLaunchKernelGGL(stem_wgrad_kernel<true>, grid, dim3(kThreads), 0, s, m, g, O, Lo, Wo, n_slabs, partial);
    else hipLaunchKernelGGL(stem_wgrad_kernel<false>, grid, dim3(kThreads), 0, s, m, g, O, Lo, Wo, n_slabs, partial);
    hipLaunchKernelGGL(stem_wgrad_merge_kernel, dim3((unsigned)((per + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, partial, B * n_slabs, per, dw);
    return (int)hipGetLastError();
}

} // extern "C"
