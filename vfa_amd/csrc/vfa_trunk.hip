// vfa_trunk.hip -- the residual stages of the ResNet trunk at inference (reference resnet.py:26-57, a block: conv3x3 - GroupNorm - ReLU -
// conv3x3 - GroupNorm, a 1x1 projection with its GroupNorm or the identity as the shortcut, the join and a ReLU): float32 in and out,
// the input (B, C, L, W) read through its four element strides, the outputs contiguous.  Fixed summation order, no float atomics: the
// same bits on every run, and an image gives the same bits alone and in a batch.  The integer rules: vfa_trunk.h.
//
//   1. trunk_absmax_kernel: per image (and once per weight) the maximum of the bit patterns of the finite values the products will
//      see -- AFTER the prologue, and with one tap at the strided positions only -- merged with an integer atomicMax per block: the
//      operand's power-of-two scale of the fp16 split (vfa_split.h).  A pre-pass of its own: the value depends on the image alone.
//   2. trunk_pack_kernel: the weight (O, C, 3, 3) or (O, C, 1, 1) scaled and split into the packed hi / lo fp16 planes, once per weight.
//   3. trunk_conv_kernel<TAPS, S, TWO>: the dense kernel of vfa_conv.hip (implicit GEMM, M = outputs, N = output cells, K = TAPS C;
//      a workgroup of 4 waves owns 4 x 32 output cells and 128 outputs; chunks of 32 channels, the chunk's window split under
//      MODE.FP16_OVFL into two fp16 planes in LDS, the weights tap by tap through a double-buffered LDS stage, three
//      v_mfma_f32_32x32x16_f16 per product outside the saturation mode) with a stride S of 1 or 2, TAPS of 9 or 1, and an optional
//      prologue: a window position inside the map is staged as max(fmaf(a[b, c], x, b[b, c]), 0), one outside is a zero AFTER that
//      (the rule of vfa_conv3x3_few_f32).  The window is loaded in map order (consecutive threads on consecutive addresses) and
//      stored at its LOCATION (vfa_trunk.h: at stride 2 the even and the odd window columns in separate halves of a row).
//      TWO (C > 256): the chunks of the first half of the channels are summed in accumulators of their own and the two halves are
//      added once in fp32, first + second: the rounding error grows with the length of an fp32 chain.
//      The output is the raw convolution acc 2^-(ea + ew), stored as MFMA rows: 32 consecutive floats of an NCHW row.
//   4. residual_join_kernel: out = max(fmaf(a, y, b) + (r | fmaf(ra, r, rb)), 0), one rounding per written operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"
#include "vfa_split.h"
#include "vfa_trunk.h"

namespace {

using namespace vfa_trunk;
using vfa_dev::f16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kExp = 14; // as vfa_conv.hip: both operands in [2^14, 2^15)

struct Map {
    const float *x;
    long long s_frame, s_chan, s_row, s_col; // element strides, >= 0
    int B, C, L, W;
};

__device__ __forceinline__ float prologue(float a, float x, float b)
{
    const float t = fmaf(a, x, b);
    return t < 0.0f ? 0.0f : t; // (a NaN stays a NaN)
}

// grid (256 positions of the Lv x Wv visited positions, 32 channels, image); visited position (yv, xv) is map position (yv step,
// xv step).  As conv_absmax_kernel of vfa_conv.hip, with the prologue.
constexpr int kAbsmaxChannels = 32;
__global__ __launch_bounds__(kThreads) void trunk_absmax_kernel(const Map m, const float *__restrict__ pa, const float *__restrict__ pb, int Lv, int Wv,
                                                                int step, unsigned *__restrict__ absmax)
{
    __shared__ unsigned wave_best[kThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.z, c0 = blockIdx.y * kAbsmaxChannels;
    const int cn = m.C - c0 < kAbsmaxChannels ? m.C - c0 : kAbsmaxChannels;
    const int plane = Lv * Wv;
    const float *frame = m.x + b * m.s_frame + c0 * m.s_chan;
    const float *fa = pa ? pa + (size_t)b * m.C + c0 : nullptr, *fb = pa ? pb + (size_t)b * m.C + c0 : nullptr;
    unsigned best = 0;
    if (m.s_chan == 1 && cn == kAbsmaxChannels) { // channels-last: 32 lanes on 32 consecutive channels, 8 positions per pass
        const int c = tid & 31;
        const float a = fa ? fa[c] : 1.0f, bb = fa ? fb[c] : 0.0f;
        for (int k = 0; k < kThreads / 8; ++k) {
            const int p = blockIdx.x * kThreads + k * 8 + (tid >> 5);
            if (p >= plane) break;
            const int y = p / Wv, x = p - y * Wv;
            float val = frame[c + y * step * m.s_row + x * step * m.s_col];
            if (fa) val = prologue(a, val, bb);
            const unsigned bits = __float_as_uint(val) & 0x7fffffffu;
            if (bits < 0x7f800000u && bits > best) best = bits;
        }
    } else {
        const int p = blockIdx.x * kThreads + tid;
        if (p < plane) {
            const int y = p / Wv, x = p - y * Wv;
            const float *src = frame + y * step * m.s_row + x * step * m.s_col;
            for (int c = 0; c < cn; ++c) {
                float val = src[c * m.s_chan];
                if (fa) val = prologue(fa[c], val, fb[c]);
                const unsigned bits = __float_as_uint(val) & 0x7fffffffu;
                if (bits < 0x7f800000u && bits > best) best = bits;
            }
        }
    }
    best = vfa_dev::wave_max_u32(best);
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < kThreads / 64; ++i) best = wave_best[i] > best ? wave_best[i] : best;
        if (best > __hip_atomic_load(absmax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(absmax + b, best);
    }
}

// one thread per four channels of one (output, tap): both pieces
__global__ __launch_bounds__(kThreads) void trunk_pack_kernel(const float *__restrict__ weight, int O, int C, int taps, unsigned char *__restrict__ packed)
{
    const size_t per_piece = packed_halves(O, C, taps) / 8; // quads of one piece: a thread writes its hi quad and its lo quad
    const size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= per_piece) return;
    const int ew = vfa_dev::split_exponent(*(const unsigned *)packed, kExp);
    const float sw = vfa_dev::pow2f(ew);
    const int quads_per_slice_piece = kChunkC * kTileOut / 4;
    const size_t slice = q / quads_per_slice_piece;
    const int in = (int)(q - slice * quads_per_slice_piece);
    const int j4 = in & 1, ol = (in >> 1) % kTileOut, k8 = (in >> 1) / kTileOut;
    const int t = (int)(slice % taps);
    const size_t sc = slice / taps;
    const int n_chunks = C / kChunkC;
    const int ch = (int)(sc % n_chunks), ot = (int)(sc / n_chunks);
    const int o = ot * kTileOut + ol, c = ch * kChunkC + k8 * 8 + j4 * 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (o < O) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = weight[((size_t)o * C + c + j) * taps + t] * sw;
    }
    uint2 hi, lo;
    vfa_dev::fp16_saturate_mode(true);
    vfa_dev::split_f16x4(v[0], v[1], v[2], v[3], hi, lo);
    vfa_dev::fp16_saturate_mode(false);
    _Float16 *planes = (_Float16 *)(packed + kPackHeaderBytes);
    *(uint2 *)(planes + packed_index(o, c, t, 0, C, taps)) = hi;
    *(uint2 *)(planes + packed_index(o, c, t, 1, C, taps)) = lo;
}

template <int TAPS, int S> struct Win {
    static constexpr int kCols = window_cols(TAPS, S);
    static constexpr int kLoc = window_locations(TAPS, S);
    static constexpr int kQuads = kLoc * (kChunkC / 4);
    static constexpr int kLoads = (kQuads + kThreads - 1) / kThreads;
    static constexpr int kPlaneHalves = kLoc * kLocHalves;
    static constexpr int kLdsBytes = (2 * kPlaneHalves + 2 * kSliceHalves) * 2 + 2 * kChunkC * (int)sizeof(float); // planes, slices, a | b of a chunk
    static_assert(kLoads <= 32, "the inside-the-map bits of a thread's quads are one word");
};

// quad e of a chunk's window: (window position p in map order, four channels 4 c4 .. 4 c4 + 3), consecutive threads on consecutive
// addresses of the map
template <int TAPS, int S> __device__ __forceinline__ void quad_of(int e, bool chan_fast, int &p, int &c4)
{
    if (chan_fast) { c4 = e & 7; p = e >> 3; }
    else { c4 = e / Win<TAPS, S>::kLoc; p = e - c4 * Win<TAPS, S>::kLoc; }
}

// -> the bits of the quads that lie inside the map
template <int TAPS, int S>
__device__ __forceinline__ unsigned window_load(const Map m, int b, int y0, int x0, int c0, bool chan_fast, int tid, float (&v)[Win<TAPS, S>::kLoads][4])
{
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < Win<TAPS, S>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4, y, x;
        quad_of<TAPS, S>(e, chan_fast, p, c4);
        const bool ok = e < Win<TAPS, S>::kQuads && window_position(p, y0, x0, TAPS, S, m.L, m.W, y, x);
        const float *src = m.x + (ok ? b * m.s_frame + (long long)(c0 + 4 * c4) * m.s_chan + y * m.s_row + x * m.s_col : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = ok ? src[k * m.s_chan] : 0.0f;
        inside |= (ok ? 1u : 0u) << j;
    }
    return inside;
}

template <int TAPS, int S>
__device__ __forceinline__ void window_store(_Float16 *a_hi, _Float16 *a_lo, const float *ab, bool pro, unsigned inside, float sa, bool chan_fast, int tid,
                                             const float (&v)[Win<TAPS, S>::kLoads][4])
{
    vfa_dev::fp16_saturate_mode(true);
#pragma unroll
    for (int j = 0; j < Win<TAPS, S>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4;
        quad_of<TAPS, S>(e, chan_fast, p, c4);
        float t[4] = {v[j][0], v[j][1], v[j][2], v[j][3]};
        if (pro) { // (uniform)
            const bool ok = (inside >> j) & 1u;
            const int cq = e < Win<TAPS, S>::kQuads ? 4 * c4 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float val = prologue(ab[cq + k], t[k], ab[kChunkC + cq + k]);
                t[k] = ok ? val : 0.0f; // the zero padding comes after the prologue
            }
        }
        uint2 hi, lo;
        vfa_dev::split_f16x4(t[0] * sa, t[1] * sa, t[2] * sa, t[3] * sa, hi, lo);
        if (e < Win<TAPS, S>::kQuads) {
            const int loc = window_location(p / Win<TAPS, S>::kCols, p % Win<TAPS, S>::kCols, TAPS, S);
            *(uint2 *)(a_hi + loc * kLocHalves + 4 * c4) = hi;
            *(uint2 *)(a_lo + loc * kLocHalves + 4 * c4) = lo;
        }
    }
    vfa_dev::fp16_saturate_mode(false);
}

template <int TAPS, int S, bool TWO>
__global__ __launch_bounds__(kThreads) void trunk_conv_kernel(const Map m, const float *__restrict__ pa, const float *__restrict__ pb,
                                                              const unsigned *__restrict__ absmax, const unsigned char *__restrict__ packed, int O, int Lo,
                                                              int Wo, float *__restrict__ out)
{
    typedef Win<TAPS, S> WN;
    extern __shared__ __align__(16) unsigned char lds[];
    _Float16 *a_hi = (_Float16 *)lds, *a_lo = a_hi + WN::kPlaneHalves, *b_lds = a_lo + WN::kPlaneHalves;
    float *ab = (float *)(b_lds + 2 * kSliceHalves);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, ot = blockIdx.y;
    int y0, x0;
    tile_origin((int)blockIdx.x, Wo, y0, x0);
    const bool chan_fast = m.s_chan == 1, pro = pa != nullptr;
    const int ea = vfa_dev::split_exponent(absmax[b], kExp), ew = vfa_dev::split_exponent(*(const unsigned *)packed, kExp);
    const float sa = vfa_dev::pow2f(ea);
    const int n_chunks = m.C / kChunkC, n_iter = n_chunks * TAPS, n_first = first_chunks(m.C);
    const u32x4 *slices = (const u32x4 *)(packed + kPackHeaderBytes) + (size_t)ot * n_iter * (kSliceHalves / 8);
    const float *ab_src = pro ? (tid < kChunkC ? pa : pb) + (size_t)b * m.C + (tid & (kChunkC - 1)) : nullptr; // threads 0 .. 63

    float v[WN::kLoads][4];
    u32x4 w[4];
    unsigned inside = window_load<TAPS, S>(m, b, y0, x0, 0, chan_fast, tid, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = slices[tid + kThreads * q];
    if (pro) {
        if (tid < 2 * kChunkC) ab[tid] = ab_src[0];
        __syncthreads();
    }
    window_store<TAPS, S>(a_hi, a_lo, ab, pro, inside, sa, chan_fast, tid, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) ((u32x4 *)b_lds)[tid + kThreads * q] = w[q];
    __syncthreads();

    f32x16 acc[2][2], first[TWO ? 2 : 1][TWO ? 2 : 1]; // [output sub-tile][cell row]
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[n][mi][i] = 0.0f;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const bool more = ch + 1 < n_chunks; // (uniform)
        if (TWO && ch == n_first) { // the second half of the channels starts a chain of its own
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    first[TWO ? n : 0][TWO ? mi : 0] = acc[n][mi];
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[n][mi][i] = 0.0f;
                }
        }
        if (more) {
            inside = window_load<TAPS, S>(m, b, y0, x0, (ch + 1) * kChunkC, chan_fast, tid, v);
            // a | b of the next chunk: the last reader of `ab` (window_store) is behind a barrier, the next one behind the taps' barriers
            if (pro && tid < 2 * kChunkC) ab[tid] = ab_src[(ch + 1) * kChunkC];
        }
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int it = ch * TAPS + t;
            const int next = it + 1 < n_iter ? it + 1 : it; // (the last iteration reloads its own slice into the idle buffer)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = slices[(size_t)next * (kSliceHalves / 8) + tid + kThreads * q];
            const _Float16 *bw = b_lds + (it & 1) * kSliceHalves;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k8 = 2 * s + h;
                f16x8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const int at = tap_location(2 * wm + mi, r, t, TAPS, S) * kLocHalves + 8 * k8;
                    xh[mi] = *(const f16x8 *)(a_hi + at);
                    xl[mi] = *(const f16x8 *)(a_lo + at);
                }
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int at = (k8 * kTileOut + (2 * wn + n) * 32 + r) * 8;
                    wh[n] = *(const f16x8 *)(bw + at);
                    wl[n] = *(const f16x8 *)(bw + 4 * kTileOut * 8 + at);
                }
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) { // rows = outputs, columns = cells
                        acc[n][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[n], xh[mi], acc[n][mi], 0, 0, 0);
                        acc[n][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[n], xh[mi], acc[n][mi], 0, 0, 0);
                        acc[n][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[n], xl[mi], acc[n][mi], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) ((u32x4 *)(b_lds + ((it + 1) & 1) * kSliceHalves))[tid + kThreads * q] = w[q];
            __syncthreads(); // the next slice is in LDS; this slice's buffer (and after the last tap the window) is free
        }
        if (more) {
            window_store<TAPS, S>(a_hi, a_lo, ab, pro, inside, sa, chan_fast, tid, v);
            __syncthreads();
        }
    }

    const float inv = vfa_dev::pow2f(-(ea + ew));
    const int x = x0 + r;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) { // C/D: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
            const int o = ot * kTileOut + (2 * wn + n) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (o >= O) continue;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int y = y0 + 2 * wm + mi;
                if (y >= Lo || x >= Wo) continue;
                const float sum = TWO ? first[TWO ? n : 0][TWO ? mi : 0][i] + acc[n][mi][i] : acc[n][mi][i];
                out[(((size_t)b * O + o) * Lo + y) * Wo + x] = sum * inv;
            }
        }
}

// grid (blocks of 1024 positions of a plane, (image, channel) pairs in a grid-stride loop)
constexpr int kJoinPerThread = 4;
__global__ __launch_bounds__(kThreads) void residual_join_kernel(const float *y, const float *__restrict__ a, const float *__restrict__ b, const float *r,
                                                                 const float *__restrict__ ra, const float *__restrict__ rb, int BC, int plane, float *out)
{
    for (int bc = blockIdx.y; bc < BC; bc += gridDim.y) {
        const float ya = a[bc], yb = b[bc], sa = ra ? ra[bc] : 1.0f, sb = ra ? rb[bc] : 0.0f;
        const size_t base = (size_t)bc * plane;
#pragma unroll
        for (int k = 0; k < kJoinPerThread; ++k) {
            const int p = (blockIdx.x * kJoinPerThread + k) * kThreads + threadIdx.x;
            if (p >= plane) break;
            const float shortcut = ra ? fmaf(sa, r[base + p], sb) : r[base + p];
            const float val = fmaf(ya, y[base + p], yb) + shortcut;
            out[base + p] = val < 0.0f ? 0.0f : val; // (a NaN stays a NaN)
        }
    }
}

// 0: run; 1: nothing to do; otherwise the error
int check_map(const float *x, const long long *stride, int B, int C, int L, int W, Map &m)
{
    if (B < 0 || C < 1 || L < 0 || W < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || (long long)L * W == 0) return 1;
    if (!x || !stride) return VFA_ERR_BAD_ARGUMENT;
    if (stride[0] < 0 || stride[1] < 0 || stride[2] < 0 || stride[3] < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2) return VFA_ERR_UNSUPPORTED;
    m.x = x;
    m.s_frame = stride[0];
    m.s_chan = stride[1];
    m.s_row = stride[2];
    m.s_col = stride[3];
    m.B = B;
    m.C = C;
    m.L = L;
    m.W = W;
    return 0;
}

void launch_absmax(const Map &m, const float *a, const float *b, int Lv, int Wv, int step, unsigned *absmax, hipStream_t s)
{
    const dim3 grid((unsigned)((Lv * Wv + kThreads - 1) / kThreads), (unsigned)((m.C + kAbsmaxChannels - 1) / kAbsmaxChannels), (unsigned)m.B);
    hipLaunchKernelGGL(trunk_absmax_kernel, grid, dim3(kThreads), 0, s, m, a, b, Lv, Wv, step, absmax);
}

template <int TAPS, int S, bool TWO>
int launch_conv(const Map &m, const float *a, const float *b, const unsigned *absmax, const unsigned char *packed, int O, float *out, hipStream_t s)
{
    // The attribute belongs to the kernel ON A DEVICE: one flag per device (past kAttrDevices the call is made every time).
    // Idempotent: a race only repeats the call.
    constexpr int kAttrDevices = 64;
    static bool attr_set[kAttrDevices] = {};
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return (int)e;
    if (device < 0 || device >= kAttrDevices || !attr_set[device]) {
        e = hipFuncSetAttribute((const void *)trunk_conv_kernel<TAPS, S, TWO>, hipFuncAttributeMaxDynamicSharedMemorySize, Win<TAPS, S>::kLdsBytes);
        if (e != hipSuccess) return (int)e;
        if (device >= 0 && device < kAttrDevices) attr_set[device] = true;
    }
    const int Lo = out_size(m.L, S), Wo = out_size(m.W, S);
    const dim3 grid((unsigned)(tiles_x(Wo) * tiles_y(Lo)), (unsigned)out_tiles(O), (unsigned)m.B);
    constexpr int lds_bytes = Win<TAPS, S>::kLdsBytes;
    hipLaunchKernelGGL((trunk_conv_kernel<TAPS, S, TWO>), grid, dim3(kThreads), lds_bytes, s, m, a, b, absmax, packed, O, Lo, Wo, out);
    return (int)hipGetLastError();
}

template <int TAPS, int S>
int launch_conv_c(const Map &m, const float *a, const float *b, const unsigned *absmax, const unsigned char *packed, int O, float *out, hipStream_t s)
{
    return m.C > kSplitC ? launch_conv<TAPS, S, true>(m, a, b, absmax, packed, O, out, s) : launch_conv<TAPS, S, false>(m, a, b, absmax, packed, O, out, s);
}

} // namespace

extern "C" {

size_t vfa_trunk_packed_bytes(int O, int C, int taps)
{
    if (O < 1 || C < 1 || (taps != 1 && taps != 9) || C % kChunkC != 0 || (long long)O * C * taps > INT32_MAX / 2) return 0;
    return kPackHeaderBytes + packed_halves(O, C, taps) * 2;
}

int vfa_trunk_pack_weights_f32(const float *weight, int O, int C, int taps, void *packed, size_t packed_bytes, void *stream)
{
    if (O < 1 || C < 1 || (taps != 1 && taps != 9) || !weight || !packed) return VFA_ERR_BAD_ARGUMENT;
    const size_t need = vfa_trunk_packed_bytes(O, C, taps);
    if (need == 0 || out_tiles(O) > 65535) return VFA_ERR_UNSUPPORTED;
    if (packed_bytes != need || ((uintptr_t)packed & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(packed, 0, kPackHeaderBytes, s);
    if (e != hipSuccess) return (int)e;
    Map m = {weight, 0, 0, 0, 1, 1, 1, 1, O * C * taps};
    launch_absmax(m, nullptr, nullptr, 1, m.W, 1, (unsigned *)packed, s);
    const size_t quads = packed_halves(O, C, taps) / 8;
    hipLaunchKernelGGL(trunk_pack_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, weight, O, C, taps,
                       (unsigned char *)packed);
    return (int)hipGetLastError();
}

size_t vfa_trunk_workspace_bytes(int B)
{
    if (B <= 0) return 0;
    return ((size_t)B * sizeof(unsigned) + 255) / 256 * 256;
}

int vfa_trunk_conv_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *a, const float *b, int B,
                       int C, int L, int W, int O, int taps, int stride, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (O < 1 || !valid(taps, stride) || (a == nullptr) != (b == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!packed || !out || !workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < vfa_trunk_workspace_bytes(B)) return VFA_ERR_BAD_ARGUMENT;
    if (C % kChunkC != 0 || out_tiles(O) > 65535 || vfa_trunk_packed_bytes(O, C, taps) == 0) return VFA_ERR_UNSUPPORTED;
    if (packed_bytes != vfa_trunk_packed_bytes(O, C, taps) || ((uintptr_t)packed & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, vfa_trunk_workspace_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    // the values the products see: with nine taps every position of the map, with one tap the strided positions
    if (taps == 9) launch_absmax(m, a, b, L, W, 1, (unsigned *)workspace, s);
    else launch_absmax(m, a, b, out_size(L, stride), out_size(W, stride), stride, (unsigned *)workspace, s);
    const unsigned *absmax = (const unsigned *)workspace;
    const unsigned char *pk = (const unsigned char *)packed;
    if (taps == 9) return stride == 1 ? launch_conv_c<9, 1>(m, a, b, absmax, pk, O, out, s) : launch_conv_c<9, 2>(m, a, b, absmax, pk, O, out, s);
    return stride == 1 ? launch_conv_c<1, 1>(m, a, b, absmax, pk, O, out, s) : launch_conv_c<1, 2>(m, a, b, absmax, pk, O, out, s);
}

int vfa_residual_join_f32(const float *y, const float *a, const float *b, const float *r, const float *ra, const float *rb, int B, int C, int L,
                          int W, float *out, void *stream)
{
    if (B < 0 || C < 0 || L < 0 || W < 0 || (ra == nullptr) != (rb == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || C == 0 || (long long)L * W == 0) return 0;
    if (!y || !a || !b || !r || !out) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const int plane = L * W, BC = B * C, per_block = kThreads * kJoinPerThread;
    const dim3 grid((unsigned)((plane + per_block - 1) / per_block), (unsigned)(BC < 65535 ? BC : 65535));
    hipLaunchKernelGGL(residual_join_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, y, a, b, r, ra, rb, BC, plane, out);
    return (int)hipGetLastError();
}

} // extern "C"
