// vfa_conv.hip -- the dense 3x3 convolutions of the BEV heads at inference (reference vfanet.py:131-149: fuse, map_classifier,
// tytx_pred, thtwtl_pred): stride 1, zero padding = dilation, dilation 1..4, float32 in and out, the input (B, C, L, W) read through
// its four element strides, the output contiguous (B, O, L, W).  Fixed summation order, no float atomics: the same bits on every run,
// and a frame gives the same bits alone and in a batch.  The integer rules: vfa_conv.h.
//
//   1. conv_absmax_kernel: per frame (and once per weight) the maximum of the bit patterns of the finite values, merged with an
//      integer atomicMax per block -- the operand's power-of-two scale of the fp16 split (vfa_split.h).
//   2. conv_pack_kernel: the weight (O, C, 3, 3) scaled and split into the packed hi / lo fp16 planes of vfa_conv.h, once per weight;
//      or the planes of its transposed, tap-mirrored form, with which this file's dense kernel gives the input gradient
//      (vfa_conv_grad.hip has the weight gradient).
//   3. conv_dense_kernel<D>: an implicit GEMM with M = outputs, N = cells, K = 9 C.  A workgroup of 4 waves owns a tile of 4 map rows x
//      32 columns and 128 outputs; wave (wm, wn) takes the rows 2 wm, 2 wm + 1 and the outputs 64 wn .. 64 wn + 63: four 32 x 32
//      accumulators.  K runs in chunks of 32 channels: the tile's window (the tile grown by the dilation) of the chunk is loaded
//      through the strides, scaled, split under MODE.FP16_OVFL and kept in LDS as two fp16 planes [location][channel]; nine taps read it
//      at nine offsets, so there is no im2col buffer.  The weights come tap by tap as 16 KiB slices through a double-buffered LDS
//      stage.  The next chunk's window and the next tap's slice are in flight under the products.  A product is the three
//      v_mfma_f32_32x32x16_f16 of vfa_split.h (x_hi w_lo, x_hi w_hi, x_lo w_hi), not under the saturation mode.
//      Epilogue per output channel: out = act(acc 2^-(ea + ew) * scale[o] + shift[o]).
//   4. conv_few_kernel<O>: the layers with 1..4 outputs, plain fmaf: a workgroup takes 64 cells of a map row, its four waves a
//      quarter of the channels each (channel-ascending, tap-ascending chains), merged as (p0 + p1) + (p2 + p3).  Optional
//      prologue relu(a[b, c] x + b[b, c]) applied as a tap is read; a tap outside the map is a zero AFTER the prologue.
//   5. gn_partial_kernel / gn_affine_kernel: per (frame, group) sum and sum of squares in float64 (32 parts in a fixed tree, merged
//      in ascending order), then a = gamma rstd, b = beta - mean a per (frame, channel).
//   6. bn_fold_kernel: scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale from the running statistics on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_conv.h"
#include "vfa_hip.h"
#include "vfa_split.h"

namespace {

using namespace vfa_conv;
using vfa_dev::f16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kExp = 14;      // both operands are scaled into [2^14, 2^15): below fp16's 65504, and 9 C products stay far inside fp32
constexpr int kGnParts = 32;  // partial sums per (frame, group)

struct Map {
    const float *x;
    long long s_frame, s_chan, s_row, s_col; // element strides, >= 0
    int B, C, L, W;
};

// grid (256 positions of the plane, kAbsmaxChannels channels, frame): 32-bit index arithmetic, one division per position.  A block
// merges its maximum in LDS and issues its atomicMax only where it would raise the value it reads first (a maximum does not
// depend on who is skipped).
constexpr int kAbsmaxChannels = 32;
__global__ __launch_bounds__(kThreads) void conv_absmax_kernel(const Map m, unsigned *__restrict__ absmax)
{
    __shared__ unsigned wave_best[kThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.z, c0 = blockIdx.y * kAbsmaxChannels;
    const int cn = m.C - c0 < kAbsmaxChannels ? m.C - c0 : kAbsmaxChannels;
    const int plane = m.L * m.W;
    const float *frame = m.x + b * m.s_frame + c0 * m.s_chan;
    unsigned best = 0;
    if (m.s_chan == 1 && cn == kAbsmaxChannels) { // channels-last: 32 lanes on 32 consecutive channels, 8 positions per pass
        for (int k = 0; k < kThreads / 8; ++k) {
            const int p = blockIdx.x * kThreads + k * 8 + (tid >> 5);
            if (p >= plane) break;
            const int y = p / m.W, x = p - y * m.W;
            const unsigned bits = __float_as_uint(frame[(tid & 31) + y * m.s_row + x * m.s_col]) & 0x7fffffffu;
            if (bits < 0x7f800000u && bits > best) best = bits;
        }
    } else {
        const int p = blockIdx.x * kThreads + tid;
        if (p < plane) {
            const int y = p / m.W, x = p - y * m.W;
            const float *src = frame + y * m.s_row + x * m.s_col;
            for (int c = 0; c < cn; ++c) {
                const unsigned bits = __float_as_uint(src[c * m.s_chan]) & 0x7fffffffu;
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

// one thread per four channels of one (output, tap): both pieces.  transposed: `weight` is (C, O, 3, 3) and the planes are those of
// its transposed, tap-mirrored form w'[o, c, t] = weight[c, o, 8 - t], the weight of the convolution's input gradient
__global__ __launch_bounds__(kThreads) void conv_pack_kernel(const float *__restrict__ weight, int O, int C, int transposed,
                                                             unsigned char *__restrict__ packed)
{
    const size_t per_piece = packed_halves(O, C) / 8; // quads of one piece: a thread writes its hi quad and its lo quad
    const size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= per_piece) return;
    const int ew = vfa_dev::split_exponent(*(const unsigned *)packed, kExp);
    const float sw = vfa_dev::pow2f(ew);
    const int quads_per_slice_piece = kChunkC * kTileOut / 4;
    const size_t slice = q / quads_per_slice_piece;
    const int in = (int)(q - slice * quads_per_slice_piece);
    const int j4 = in & 1, ol = (in >> 1) % kTileOut, k8 = (in >> 1) / kTileOut;
    const int t = (int)(slice % kTaps);
    const size_t sc = slice / kTaps;
    const int n_chunks = C / kChunkC;
    const int ch = (int)(sc % n_chunks), ot = (int)(sc / n_chunks);
    const int o = ot * kTileOut + ol, c = ch * kChunkC + k8 * 8 + j4 * 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (o < O) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = (transposed ? weight[((size_t)(c + j) * O + o) * kTaps + (kTaps - 1 - t)] : weight[((size_t)o * C + c + j) * kTaps + t]) * sw;
    }
    uint2 hi, lo;
    vfa_dev::fp16_saturate_mode(true);
    vfa_dev::split_f16x4(v[0], v[1], v[2], v[3], hi, lo);
    vfa_dev::fp16_saturate_mode(false);
    _Float16 *planes = (_Float16 *)(packed + kPackHeaderBytes);
    *(uint2 *)(planes + packed_index(o, c, t, 0, C)) = hi;
    *(uint2 *)(planes + packed_index(o, c, t, 1, C)) = lo;
}

template <int D> struct Dense {
    static constexpr int kLoc = (kTileRows + 2 * D) * (kTileCols + 2 * D);
    static constexpr int kQuads = kLoc * (kChunkC / 4);
    static constexpr int kLoads = (kQuads + kThreads - 1) / kThreads;
    static constexpr int kPlaneHalves = kLoc * kLocHalves;
    static constexpr int kLdsBytes = (2 * kPlaneHalves + 2 * kSliceHalves) * 2;
};

// quad e of a chunk's window: (location, four channels 4 c4 .. 4 c4 + 3), consecutive threads on consecutive addresses of the map
template <int D> __device__ __forceinline__ void quad_of(int e, bool chan_fast, int &loc, int &c4)
{
    if (chan_fast) { c4 = e & 7; loc = e >> 3; }
    else { c4 = e / Dense<D>::kLoc; loc = e - c4 * Dense<D>::kLoc; }
}

template <int D>
__device__ __forceinline__ void window_load(const Map m, int b, int y0, int x0, int c0, bool chan_fast, int tid, float (&v)[Dense<D>::kLoads][4])
{
#pragma unroll
    for (int j = 0; j < Dense<D>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int loc, c4, y, x;
        quad_of<D>(e, chan_fast, loc, c4);
        const bool ok = e < Dense<D>::kQuads && window_position(loc, y0, x0, D, m.L, m.W, y, x);
        const float *p = m.x + (ok ? b * m.s_frame + (long long)(c0 + 4 * c4) * m.s_chan + y * m.s_row + x * m.s_col : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = ok ? p[k * m.s_chan] : 0.0f;
    }
}

template <int D>
__device__ __forceinline__ void window_store(_Float16 *a_hi, _Float16 *a_lo, float sa, bool chan_fast, int tid, const float (&v)[Dense<D>::kLoads][4])
{
    vfa_dev::fp16_saturate_mode(true);
#pragma unroll
    for (int j = 0; j < Dense<D>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int loc, c4;
        quad_of<D>(e, chan_fast, loc, c4);
        uint2 hi, lo;
        vfa_dev::split_f16x4(v[j][0] * sa, v[j][1] * sa, v[j][2] * sa, v[j][3] * sa, hi, lo);
        if (e < Dense<D>::kQuads) {
            *(uint2 *)(a_hi + loc * kLocHalves + 4 * c4) = hi;
            *(uint2 *)(a_lo + loc * kLocHalves + 4 * c4) = lo;
        }
    }
    vfa_dev::fp16_saturate_mode(false);
}

template <int D>
__global__ __launch_bounds__(kThreads) void conv_dense_kernel(const Map m, const unsigned *__restrict__ absmax, const unsigned char *__restrict__ packed,
                                                              const float *__restrict__ scale, const float *__restrict__ shift, int relu, int O,
                                                              float *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char lds[];
    _Float16 *a_hi = (_Float16 *)lds, *a_lo = a_hi + Dense<D>::kPlaneHalves, *b_lds = a_lo + Dense<D>::kPlaneHalves;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, ot = blockIdx.y;
    int y0, x0;
    tile_origin((int)blockIdx.x, m.W, y0, x0);
    const bool chan_fast = m.s_chan == 1;
    const int ea = vfa_dev::split_exponent(absmax[b], kExp), ew = vfa_dev::split_exponent(*(const unsigned *)packed, kExp);
    const float sa = vfa_dev::pow2f(ea);
    const int n_chunks = m.C / kChunkC, n_iter = n_chunks * kTaps;
    const u32x4 *slices = (const u32x4 *)(packed + kPackHeaderBytes) + (size_t)ot * n_iter * (kSliceHalves / 8);

    float v[Dense<D>::kLoads][4];
    u32x4 w[4];
    window_load<D>(m, b, y0, x0, 0, chan_fast, tid, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = slices[tid + kThreads * q];
    window_store<D>(a_hi, a_lo, sa, chan_fast, tid, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) ((u32x4 *)b_lds)[tid + kThreads * q] = w[q];
    __syncthreads();

    f32x16 acc[2][2]; // [output sub-tile][cell row]
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[n][mi][i] = 0.0f;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const bool more = ch + 1 < n_chunks; // (uniform)
        if (more) window_load<D>(m, b, y0, x0, (ch + 1) * kChunkC, chan_fast, tid, v);
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            const int it = ch * kTaps + t;
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
                    const int at = window_index(2 * wm + mi, r, t, D) * kLocHalves + 8 * k8;
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
            __syncthreads(); // the next slice is in LDS; this slice's buffer (and after tap 8 the window) is free
        }
        if (more) {
            window_store<D>(a_hi, a_lo, sa, chan_fast, tid, v);
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
            const float sc = scale ? scale[o] : 1.0f, sh = shift ? shift[o] : 0.0f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int y = y0 + 2 * wm + mi;
                if (y >= m.L || x >= m.W) continue;
                float val = fmaf(acc[n][mi][i] * inv, sc, sh);
                if (relu) val = val < 0.0f ? 0.0f : val; // (a NaN stays a NaN)
                out[(((size_t)b * O + o) * m.L + y) * m.W + x] = val;
            }
        }
}

template <int NO>
__global__ __launch_bounds__(kThreads) void conv_few_kernel(const Map m, const float *__restrict__ weight, const float *__restrict__ pa,
                                                            const float *__restrict__ pb, int d, float *__restrict__ out)
{
    __shared__ float part[4][NO][64];
    const int tid = threadIdx.x, cell = tid & 63, p = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = blockIdx.x * 64 + cell, y = blockIdx.y, b = blockIdx.z;
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0f;
    long long off[kTaps];
    bool ok[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const int ty = y + (t / 3 - 1) * d, tx = x + (t % 3 - 1) * d;
        ok[t] = x < m.W && ty >= 0 && ty < m.L && tx >= 0 && tx < m.W;
        off[t] = ok[t] ? b * m.s_frame + ty * m.s_row + tx * m.s_col : 0;
    }
    const int per = m.C / 4;
    for (int c = p * per; c < (p + 1) * per; ++c) { // ascending channels, ascending taps
        const float a = pa ? pa[(size_t)b * m.C + c] : 1.0f, bb = pa ? pb[(size_t)b * m.C + c] : 0.0f;
        const float *xc = m.x + (long long)c * m.s_chan;
        const float *wc = weight + (size_t)c * kTaps;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            float val = ok[t] ? xc[off[t]] : 0.0f;
            if (pa) {
                val = fmaf(a, val, bb);
                val = val < 0.0f ? 0.0f : val;
                val = ok[t] ? val : 0.0f; // the zero padding comes after the prologue
            }
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[o] = fmaf(val, wc[(size_t)o * m.C * kTaps + t], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) part[p][o][cell] = acc[o];
    __syncthreads();
    if (tid < 64 && x < m.W) {
#pragma unroll
        for (int o = 0; o < NO; ++o)
            out[(((size_t)b * NO + o) * m.L + y) * m.W + x] = (part[0][o][cell] + part[1][o][cell]) + (part[2][o][cell] + part[3][o][cell]);
    }
}

__global__ __launch_bounds__(kThreads) void gn_partial_kernel(const Map m, int groups, double *__restrict__ partial)
{
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x, p = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int cg = m.C / groups;
    const long long plane = (long long)m.L * m.W;
    const int begin = (int)(plane * p / kGnParts), end = (int)(plane * (p + 1) / kGnParts); // part p: a range of positions, every channel
    const float *group = m.x + b * m.s_frame + (long long)g * cg * m.s_chan;
    double s = 0.0, q = 0.0;
    for (int i = begin + tid; i < end; i += kThreads) {
        const int y = i / m.W, x = i - y * m.W;
        const float *src = group + y * m.s_row + x * m.s_col;
        for (int c = 0; c < cg; ++c) {
            const double val = (double)src[c * m.s_chan];
            s += val;
            q += val * val;
        }
    }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) { // a fixed tree
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double *dst = partial + (((size_t)b * groups + g) * kGnParts + p) * 2;
        dst[0] = red[0][0];
        dst[1] = red[1][0];
    }
}

// one thread per (frame, channel)
__global__ __launch_bounds__(kThreads) void gn_affine_kernel(const double *__restrict__ partial, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, double eps, int B, int C, int groups, double count,
                                                             float *__restrict__ a, float *__restrict__ bb)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C, g = c / (C / groups);
    const double *src = partial + ((size_t)b * groups + g) * kGnParts * 2;
    double s = 0.0, q = 0.0;
    for (int p = 0; p < kGnParts; ++p) { // ascending parts
        s += src[2 * p];
        q += src[2 * p + 1];
    }
    const double mean = s / count;
    double var = q / count - mean * mean; // biased
    var = var < 0.0 ? 0.0 : var;
    const double rstd = 1.0 / sqrt(var + eps);
    const double ga = gamma ? (double)gamma[c] : 1.0, be = beta ? (double)beta[c] : 0.0;
    a[i] = (float)(ga * rstd);
    bb[i] = (float)(be - mean * ga * rstd);
}

__global__ __launch_bounds__(kThreads) void bn_fold_kernel(const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                           const float *__restrict__ var, const float *__restrict__ bias, double eps, int O,
                                                           float *__restrict__ scale, float *__restrict__ shift)
{
    const int o = blockIdx.x * kThreads + threadIdx.x;
    if (o >= O) return;
    const double sc = (gamma ? (double)gamma[o] : 1.0) / sqrt((double)var[o] + eps);
    scale[o] = (float)sc;
    shift[o] = (float)((beta ? (double)beta[o] : 0.0) + ((bias ? (double)bias[o] : 0.0) - (double)mean[o]) * sc);
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

dim3 absmax_grid(const Map &m)
{
    return dim3((unsigned)((m.L * m.W + kThreads - 1) / kThreads), (unsigned)((m.C + kAbsmaxChannels - 1) / kAbsmaxChannels), (unsigned)m.B);
}

template <int D>
int launch_dense(const Map &m, const unsigned *absmax, const unsigned char *packed, const float *scale, const float *shift, int relu, int O,
                 float *out, hipStream_t s)
{
    static bool attr_set = false; // idempotent: a race only repeats the call
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void *)conv_dense_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, Dense<D>::kLdsBytes);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const dim3 grid((unsigned)(tiles_x(m.W) * tiles_y(m.L)), (unsigned)out_tiles(O), (unsigned)m.B);
    hipLaunchKernelGGL(conv_dense_kernel<D>, grid, dim3(kThreads), Dense<D>::kLdsBytes, s, m, absmax, packed, scale, shift, relu, O, out);
    return (int)hipGetLastError();
}

int pack_weights(const float *weight, int O, int C, int transposed, void *packed, size_t packed_bytes, void *stream)
{
    if (O < 1 || C < 1 || !weight || !packed) return VFA_ERR_BAD_ARGUMENT;
    const size_t need = vfa_conv3x3_packed_bytes(O, C);
    if (need == 0 || out_tiles(O) > 65535) return VFA_ERR_UNSUPPORTED;
    if (packed_bytes != need || ((uintptr_t)packed & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(packed, 0, kPackHeaderBytes, s);
    if (e != hipSuccess) return (int)e;
    Map m = {weight, 0, 0, 0, 1, 1, 1, 1, O * C * kTaps};
    hipLaunchKernelGGL(conv_absmax_kernel, absmax_grid(m), dim3(kThreads), 0, s, m, (unsigned *)packed);
    const size_t quads = packed_halves(O, C) / 8;
    hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, weight, O, C, transposed,
                       (unsigned char *)packed);
    return (int)hipGetLastError();
}

} // namespace

int vfa_conv::frame_absmax(const float *x, const long long *stride, int B, int C, int L, int W, unsigned *absmax, void *stream)
{
    Map m = {};
    const int status = check_map(x, stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    hipLaunchKernelGGL(conv_absmax_kernel, absmax_grid(m), dim3(kThreads), 0, (hipStream_t)stream, m, absmax);
    return (int)hipGetLastError();
}

extern "C" {

size_t vfa_conv3x3_packed_bytes(int O, int C)
{
    if (O < 1 || C < 1 || C % kChunkC != 0 || (long long)O * C * kTaps > INT32_MAX / 2) return 0;
    return kPackHeaderBytes + packed_halves(O, C) * 2;
}

int vfa_conv3x3_pack_weights_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream)
{
    return pack_weights(weight, O, C, 0, packed, packed_bytes, stream);
}

int vfa_conv3x3_pack_weights_transposed_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream)
{
    return pack_weights(weight, C, O, 1, packed, packed_bytes, stream); // the planes of a convolution with O inputs and C outputs
}

size_t vfa_conv3x3_workspace_bytes(int B)
{
    if (B <= 0) return 0;
    return ((size_t)B * sizeof(unsigned) + 255) / 256 * 256;
}

int vfa_conv3x3_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *scale,
                    const float *shift, int relu, int B, int C, int L, int W, int O, int dilation, float *out, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (O < 1 || dilation < 1) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!packed || !out || !workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < vfa_conv3x3_workspace_bytes(B))
        return VFA_ERR_BAD_ARGUMENT;
    if (C % kChunkC != 0 || dilation > kMaxDilation || out_tiles(O) > 65535 || vfa_conv3x3_packed_bytes(O, C) == 0) return VFA_ERR_UNSUPPORTED;
    if (packed_bytes != vfa_conv3x3_packed_bytes(O, C) || ((uintptr_t)packed & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, vfa_conv3x3_workspace_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(conv_absmax_kernel, absmax_grid(m), dim3(kThreads), 0, s, m, (unsigned *)workspace);
    const unsigned *absmax = (const unsigned *)workspace;
    const unsigned char *pk = (const unsigned char *)packed;
    switch (dilation) {
    case 1: return launch_dense<1>(m, absmax, pk, scale, shift, relu, O, out, s);
    case 2: return launch_dense<2>(m, absmax, pk, scale, shift, relu, O, out, s);
    case 3: return launch_dense<3>(m, absmax, pk, scale, shift, relu, O, out, s);
    default: return launch_dense<4>(m, absmax, pk, scale, shift, relu, O, out, s);
    }
}

int vfa_bn_fold_f32(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias, float eps, int O,
                    float *scale, float *shift, void *stream)
{
    if (O < 0 || (O > 0 && (!mean || !var || !scale || !shift))) return VFA_ERR_BAD_ARGUMENT;
    if (O == 0) return 0;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)((O + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gamma, beta,
                       mean, var, bias, (double)eps, O, scale, shift);
    return (int)hipGetLastError();
}

int vfa_conv3x3_few_f32(const float *x, const long long *x_stride, const float *weight, const float *a, const float *b, int B, int C, int L,
                        int W, int O, int dilation, float *out, void *stream)
{
    Map m = {};
    if (O < 1 || dilation < 1) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!weight || !out || (a == nullptr) != (b == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    if (O > 4 || C % 4 != 0 || dilation > kMaxDilation) return VFA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)L, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    switch (O) {
    case 1: hipLaunchKernelGGL(conv_few_kernel<1>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    case 2: hipLaunchKernelGGL(conv_few_kernel<2>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    case 3: hipLaunchKernelGGL(conv_few_kernel<3>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    default: hipLaunchKernelGGL(conv_few_kernel<4>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    }
    return (int)hipGetLastError();
}

size_t vfa_group_norm_workspace_bytes(int B, int groups)
{
    if (B <= 0 || groups <= 0) return 0;
    return (size_t)B * (size_t)groups * kGnParts * 2 * sizeof(double);
}

int vfa_group_norm_affine_f32(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C,
                              int L, int W, int groups, float *a, float *b, void *workspace, size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (groups < 1 || C < 1 || C % groups != 0) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!a || !b || !workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < vfa_group_norm_workspace_bytes(B, groups))
        return VFA_ERR_BAD_ARGUMENT;
    if (groups > 65535 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_partial_kernel, dim3(kGnParts, (unsigned)groups, (unsigned)B), dim3(kThreads), 0, s, m, groups, (double *)workspace);
    hipLaunchKernelGGL(gn_affine_kernel, dim3((unsigned)((B * C + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const double *)workspace,
                       gamma, beta, (double)eps, B, C, groups, (double)(C / groups) * (double)L * (double)W, a, b);
    return (int)hipGetLastError();
}

} // extern "C"
