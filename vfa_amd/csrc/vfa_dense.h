// vfa_dense.h -- the dense convolution on the matrix pipe, stated once for the BEV heads (vfa_conv.hip) and the ResNet trunk
// (vfa_trunk.hip): device and host code in an anonymous namespace, so each unit that includes it instantiates its own kernels and no
// device code crosses a unit.  float32 in and out, the input (B, C, L, W) read through its four element strides, the output
// contiguous (B, O, Lo, Wo).  Fixed summation order, no float atomics: the same bits on every run, and a frame gives the same bits
// alone and in a batch.  The integer rules: vfa_conv.h.
//
//   1. absmax_kernel: per frame (and once per weight) the maximum of the bit patterns of the finite values the products will see --
//      AFTER the optional prologue, and at the visited positions (yv step, xv step) only -- merged with an integer atomicMax per
//      block: the operand's power-of-two scale of the fp16 split (vfa_split.h).  A pre-pass of its own: the value depends on the frame
//      alone.
//   2. pack_kernel: the weight (O, C, 3, 3) or (O, C, 1, 1) scaled and split into the packed hi / lo fp16 planes of vfa_conv.h, once
//      per weight; or the planes of the transposed, tap-mirrored form of a (C, O, 3, 3) weight, with which the dense kernel gives the
//      convolution's input gradient.
//   3. dense_kernel<TAPS, S, D, TWO, PRO, Epi>: an implicit GEMM with M = outputs, N = output cells, K = TAPS C.  A workgroup of 4
//      waves owns a tile of 4 output rows x 32 columns and 128 outputs; wave (wm, wn) takes the rows 2 wm, 2 wm + 1 and the outputs
//      64 wn .. 64 wn + 63: four 32 x 32 accumulators.  K runs in chunks of 32 channels: the tile's window of the chunk is loaded through
//      the strides in map order (consecutive threads on consecutive addresses), scaled, split under MODE.FP16_OVFL and kept in LDS
//      as two fp16 planes [location][channel]; the taps read it at TAPS offsets, so there is no im2col buffer.  The weights come tap
//      by tap as 16 KiB slices through a double-buffered LDS stage.  The next chunk's window and the next tap's slice are in flight
//      under the products.  A product is the three v_mfma_f32_32x32x16_f16 of vfa_split.h (x_hi w_lo, x_hi w_hi, x_lo w_hi), not
//      under the saturation mode.
//      PRO: a prologue may be given (pa != nullptr, uniform): a window position inside the map is staged as
//      max(fmaf(a[b, c], x, b[b, c]), 0), one outside is a zero AFTER that (the rule of vfa_conv3x3_few_f32); a | b of a chunk lie
//      behind the slices in LDS.  Without PRO that region, the inside-the-map bits and the arguments pa, pb do not exist.
//      TWO (C > kSplitC): the chunks of the first half of the channels are summed in accumulators of their own and the two halves
//      are added once in fp32, first + second: the rounding error grows with the length of an fp32 chain.
//      Epi: what becomes of v = sum 2^-(ea + ew), stored as MFMA rows (32 consecutive floats of an NCHW row): EpiRaw stores v,
//      EpiAffine act(fmaf(v, scale[o] | 1, shift[o] | 0)).  Its per-output part is read once per output, outside the cell rows.
//      Epi::at says where an element goes: contiguous (B, O, Lo, Wo), or (EpiDown) every other row and column of a larger map.
//      TAPS may also be a BLOCK of taps (vfa_conv.h: 11, 21, 12, 22), whose slices are a run of the nine of a nine-tap pack: the
//      parity classes of a stride-2 convolution's input gradient (vfa_conv_grad.h, vfa_trunk.hip).
#ifndef VFA_DENSE_H
#define VFA_DENSE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_conv.h"
#include "vfa_conv_grad.h"
#include "vfa_hip.h"
#include "vfa_split.h"

namespace {

using namespace vfa_conv;
using vfa_dev::f16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kExp = 14; // both operands are scaled into [2^14, 2^15): below fp16's 65504, and 9 C products stay far inside fp32

struct Map {
    const float *x;
    long long s_frame, s_chan, s_row, s_col; // element strides, >= 0
    int B, C, L, W;
};

// 0: run; 1: nothing to do; otherwise the error
inline int check_map(const float *x, const long long *stride, int B, int C, int L, int W, Map &m)
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

__device__ __forceinline__ float prologue(float a, float x, float b)
{
    const float t = fmaf(a, x, b);
    return t < 0.0f ? 0.0f : t; // (a NaN stays a NaN)
}

// grid (256 positions of the Lv x Wv visited positions, kAbsmaxChannels channels, frame); visited position (yv, xv) is map position
// (yv step, xv step): 32-bit index arithmetic, one division per position.  A block merges its maximum in LDS and issues its
// atomicMax only where it would raise the value it reads first (a maximum does not depend on who is skipped).
constexpr int kAbsmaxChannels = 32;
__global__ __launch_bounds__(kThreads) void absmax_kernel(const Map m, const float *__restrict__ pa, const float *__restrict__ pb, int Lv, int Wv, int step,
                                                          unsigned *__restrict__ absmax)
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

inline void launch_absmax(const Map &m, const float *a, const float *b, int Lv, int Wv, int step, unsigned *absmax, hipStream_t s)
{
    const dim3 grid((unsigned)((Lv * Wv + kThreads - 1) / kThreads), (unsigned)((m.C + kAbsmaxChannels - 1) / kAbsmaxChannels), (unsigned)m.B);
    hipLaunchKernelGGL(absmax_kernel, grid, dim3(kThreads), 0, s, m, a, b, Lv, Wv, step, absmax);
}

// one thread per four channels of one (output, tap): both pieces.  transposed 1: `weight` is (C, O, 3, 3) and the planes are those of
// its transposed, tap-mirrored form w'[o, c, t] = weight[c, o, taps - 1 - t], the weight of the convolution's input gradient;
// transposed 2 (taps 9): w'[o, c, t] = weight[c, o, down_source_tap(t)], the four class blocks of a stride-2 convolution's input
// gradient behind one another (vfa_conv_grad.h)
__global__ __launch_bounds__(kThreads) void pack_kernel(const float *__restrict__ weight, int O, int C, int taps, int transposed,
                                                        unsigned char *__restrict__ packed)
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
        for (int j = 0; j < 4; ++j)
            v[j] = (transposed ? weight[((size_t)(c + j) * O + o) * taps + (transposed == 2 ? vfa_conv_grad::down_source_tap(t) : taps - 1 - t)]
                               : weight[((size_t)o * C + c + j) * taps + t]) * sw;
    }
    uint2 hi, lo;
    vfa_dev::fp16_saturate_mode(true);
    vfa_dev::split_f16x4(v[0], v[1], v[2], v[3], hi, lo);
    vfa_dev::fp16_saturate_mode(false);
    _Float16 *planes = (_Float16 *)(packed + kPackHeaderBytes);
    *(uint2 *)(planes + packed_index(o, c, t, 0, C, taps)) = hi;
    *(uint2 *)(planes + packed_index(o, c, t, 1, C, taps)) = lo;
}

// bytes of the packed planes of an (O, C) weight with `taps` taps, header included; 0: no such planes
inline size_t packed_bytes_of(int O, int C, int taps)
{
    if (O < 1 || C < 1 || (taps != 1 && taps != 9) || C % kChunkC != 0 || (long long)O * C * taps > INT32_MAX / 2) return 0;
    return kPackHeaderBytes + packed_halves(O, C, taps) * 2;
}

// what the dense entry points ask of the planes they are handed: 0, or the error
inline int check_packed(const void *packed, size_t packed_bytes, int O, int C, int taps)
{
    const size_t need = packed_bytes_of(O, C, taps);
    if (need == 0 || out_tiles(O) > 65535) return VFA_ERR_UNSUPPORTED;
    if (packed_bytes != need || ((uintptr_t)packed & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    return 0;
}

// the weight's absmax into the header, then the planes: O outputs and C inputs of the PACKED convolution (transposed: `weight` is
// (C, O, 3, 3))
inline int pack_weights(const float *weight, int O, int C, int taps, int transposed, void *packed, size_t packed_bytes, void *stream)
{
    if (O < 1 || C < 1 || (taps != 1 && taps != 9) || !weight || !packed) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_packed(packed, packed_bytes, O, C, taps);
    if (status != 0) return status;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(packed, 0, kPackHeaderBytes, s);
    if (e != hipSuccess) return (int)e;
    Map m = {weight, 0, 0, 0, 1, 1, 1, 1, O * C * taps};
    launch_absmax(m, nullptr, nullptr, 1, m.W, 1, (unsigned *)packed, s);
    const size_t quads = packed_halves(O, C, taps) / 8;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, weight, O, C, taps, transposed,
                       (unsigned char *)packed);
    return (int)hipGetLastError();
}

// the per-frame scales of a call: B words, padded
inline size_t scales_workspace_bytes(int B) { return B <= 0 ? 0 : ((size_t)B * sizeof(unsigned) + 255) / 256 * 256; }

// ---- the epilogues: output(o) once per output channel, then (per-output part, v = sum 2^-(ea + ew)) -> the stored value ----------

// at(): where element (b, o, y, x) of the (B, O, Lo, Wo) result is stored
__device__ __forceinline__ size_t contiguous_at(int b, int o, int y, int x, int O, int Lo, int Wo) { return (((size_t)b * O + o) * Lo + y) * Wo + x; }

struct EpiRaw { // the raw convolution
    struct Out {};
    __device__ __forceinline__ size_t at(int b, int o, int y, int x, int O, int Lo, int Wo) const { return contiguous_at(b, o, y, x, O, Lo, Wo); }
    __device__ __forceinline__ Out output(int) const { return {}; }
    __device__ __forceinline__ float operator()(Out, float v, const float *) const { return v; }
};

// a parity class of a stride-2 convolution's input gradient: cell (y, x) of the class is position (2 y + py, 2 x + px) of the
// contiguous (B, O, L, W) gradient; add: the stored value is what lies there + v, in that order (the second term of a sum)
struct EpiDown {
    int L, W, py, px, add;
    struct Out {};
    __device__ __forceinline__ size_t at(int b, int o, int y, int x, int O, int, int) const
    {
        return (((size_t)b * O + o) * L + 2 * y + py) * W + 2 * x + px;
    }
    __device__ __forceinline__ Out output(int) const { return {}; }
    __device__ __forceinline__ float operator()(Out, float v, const float *dst) const { return add ? *dst + v : v; }
};

struct EpiAffine { // act(v scale[o] + shift[o]); scale / shift: nullptr = 1 / 0
    const float *__restrict__ scale, *__restrict__ shift;
    int relu;
    __device__ __forceinline__ size_t at(int b, int o, int y, int x, int O, int Lo, int Wo) const { return contiguous_at(b, o, y, x, O, Lo, Wo); }
    struct Out {
        float sc, sh;
    };
    __device__ __forceinline__ Out output(int o) const { return {scale ? scale[o] : 1.0f, shift ? shift[o] : 0.0f}; }
    __device__ __forceinline__ float operator()(Out p, float v, const float *) const
    {
        float val = fmaf(v, p.sc, p.sh);
        if (relu) val = val < 0.0f ? 0.0f : val; // (a NaN stays a NaN)
        return val;
    }
};

// ---- the kernel ------------------------------------------------------------------------------------------------------------------

template <int TAPS, int S, int D, bool PRO> struct Win {
    static constexpr int kCols = window_cols(TAPS, S, D);
    static constexpr int kLoc = window_locations(TAPS, S, D);
    static constexpr int kQuads = kLoc * (kChunkC / 4);
    static constexpr int kLoads = (kQuads + kThreads - 1) / kThreads;
    static constexpr int kPlaneHalves = kLoc * kLocHalves;
    static constexpr int kLdsBytes = (2 * kPlaneHalves + 2 * kSliceHalves) * 2 + (PRO ? 2 * kChunkC * (int)sizeof(float) : 0); // planes, slices, a | b of a chunk
    static_assert(kLoads <= 32, "the inside-the-map bits of a thread's quads are one word");
};

// quad e of a chunk's window of LOC positions: (window position p in map order, four channels 4 c4 .. 4 c4 + 3), consecutive threads
// on consecutive addresses of the map
template <int LOC> __device__ __forceinline__ void quad_of(int e, bool chan_fast, int &p, int &c4)
{
    if (chan_fast) { c4 = e & 7; p = e >> 3; }
    else { c4 = e / LOC; p = e - c4 * LOC; }
}

// -> the bits of the quads that lie inside the map
template <class WN, int TAPS, int S, int D>
__device__ __forceinline__ unsigned window_load(const Map m, int b, int y0, int x0, int c0, bool chan_fast, int tid, float (&v)[WN::kLoads][4])
{
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < WN::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4, y, x;
        quad_of<WN::kLoc>(e, chan_fast, p, c4);
        const bool ok = e < WN::kQuads && window_position(p, y0, x0, TAPS, S, D, m.L, m.W, y, x);
        const float *src = m.x + (ok ? b * m.s_frame + (long long)(c0 + 4 * c4) * m.s_chan + y * m.s_row + x * m.s_col : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = ok ? src[k * m.s_chan] : 0.0f;
        inside |= (ok ? 1u : 0u) << j;
    }
    return inside;
}

// pro (uniform; false without PRO): the prologue with the chunk's a | b in `ab`
template <class WN, int TAPS, int S, int D>
__device__ __forceinline__ void window_store(_Float16 *a_hi, _Float16 *a_lo, const float *ab, bool pro, unsigned inside, float sa, bool chan_fast, int tid,
                                             const float (&v)[WN::kLoads][4])
{
    vfa_dev::fp16_saturate_mode(true);
#pragma unroll
    for (int j = 0; j < WN::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4;
        quad_of<WN::kLoc>(e, chan_fast, p, c4);
        float t[4] = {v[j][0], v[j][1], v[j][2], v[j][3]};
        if (pro) {
            const bool ok = (inside >> j) & 1u;
            const int cq = e < WN::kQuads ? 4 * c4 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float val = prologue(ab[cq + k], t[k], ab[kChunkC + cq + k]);
                t[k] = ok ? val : 0.0f; // the zero padding comes after the prologue
            }
        }
        uint2 hi, lo;
        vfa_dev::split_f16x4(t[0] * sa, t[1] * sa, t[2] * sa, t[3] * sa, hi, lo);
        if (e < WN::kQuads) {
            int loc = p; // only the even / odd column split of stride 2 moves a position
            if constexpr (TAPS == 9 && S == 2) loc = window_location(p / WN::kCols, p % WN::kCols, TAPS, S, D);
            *(uint2 *)(a_hi + loc * kLocHalves + 4 * c4) = hi;
            *(uint2 *)(a_lo + loc * kLocHalves + 4 * c4) = lo;
        }
    }
    vfa_dev::fp16_saturate_mode(false);
}

template <int TAPS, int S, int D, bool TWO, bool PRO, class Epi>
__global__ __launch_bounds__(kThreads) void dense_kernel(const Map m, const float *__restrict__ pa, const float *__restrict__ pb,
                                                         const unsigned *__restrict__ absmax, const unsigned char *__restrict__ packed, const Epi epi, int O,
                                                         int Lo, int Wo, float *__restrict__ out)
{
    typedef Win<TAPS, S, D, PRO> WN;
    extern __shared__ __align__(16) unsigned char lds[];
    _Float16 *a_hi = (_Float16 *)lds, *a_lo = a_hi + WN::kPlaneHalves, *b_lds = a_lo + WN::kPlaneHalves;
    float *ab = (float *)(b_lds + 2 * kSliceHalves); // (PRO)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, ot = blockIdx.y;
    int y0, x0;
    tile_origin((int)blockIdx.x, Wo, y0, x0);
    const bool chan_fast = m.s_chan == 1, pro = PRO && pa != nullptr;
    const int ea = vfa_dev::split_exponent(absmax[b], kExp), ew = vfa_dev::split_exponent(*(const unsigned *)packed, kExp);
    const float sa = vfa_dev::pow2f(ea);
    // NT taps; a block's slices are NT of the nine of a (chunk) of the stride-2 input gradient's pack, from its class's first
    constexpr int NT = tap_count(TAPS), PT = is_block(TAPS) ? kTaps : NT, T0 = is_block(TAPS) ? vfa_conv_grad::down_class_first(TAPS) : 0;
    const int n_chunks = m.C / kChunkC, n_iter = n_chunks * NT, n_first = first_chunks(m.C);
    const u32x4 *slices = (const u32x4 *)(packed + kPackHeaderBytes) + ((size_t)ot * n_chunks * PT + T0) * (kSliceHalves / 8);
    const float *ab_src = pro ? (tid < kChunkC ? pa : pb) + (size_t)b * m.C + (tid & (kChunkC - 1)) : nullptr; // threads 0 .. 63

    float v[WN::kLoads][4];
    u32x4 w[4];
    unsigned inside = window_load<WN, TAPS, S, D>(m, b, y0, x0, 0, chan_fast, tid, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = slices[tid + kThreads * q];
    if (pro) {
        if (tid < 2 * kChunkC) ab[tid] = ab_src[0];
        __syncthreads();
    }
    window_store<WN, TAPS, S, D>(a_hi, a_lo, ab, pro, inside, sa, chan_fast, tid, v);
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
            inside = window_load<WN, TAPS, S, D>(m, b, y0, x0, (ch + 1) * kChunkC, chan_fast, tid, v);
            // a | b of the next chunk: the last reader of `ab` (window_store) is behind a barrier, the next one behind the taps' barriers
            if (pro && tid < 2 * kChunkC) ab[tid] = ab_src[(ch + 1) * kChunkC];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int it = ch * NT + t;
            int next = it + 1 < n_iter ? it + 1 : it; // (the last iteration reloads its own slice into the idle buffer)
            if constexpr (PT != NT) next = (next / NT) * PT + next % NT;
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = slices[(size_t)next * (kSliceHalves / 8) + tid + kThreads * q];
            const _Float16 *bw = b_lds + (it & 1) * kSliceHalves;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k8 = 2 * s + h;
                f16x8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const int at = tap_location(2 * wm + mi, r, t, TAPS, S, D) * kLocHalves + 8 * k8;
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
            window_store<WN, TAPS, S, D>(a_hi, a_lo, ab, pro, inside, sa, chan_fast, tid, v);
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
            const typename Epi::Out per_output = epi.output(o);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int y = y0 + 2 * wm + mi;
                if (y >= Lo || x >= Wo) continue;
                const float sum = TWO ? first[TWO ? n : 0][TWO ? mi : 0][i] + acc[n][mi][i] : acc[n][mi][i];
                float *dst = out + epi.at(b, o, y, x, O, Lo, Wo);
                *dst = epi(per_output, sum * inv, dst);
            }
        }
}

// the grid of output tiles ((Lo_, Wo_): the cells to compute where they are not the convolution's own -- a class of EpiDown); the
// kernel's dynamic LDS is allowed once per device (vfa_conv.h: DynamicLds)
template <int TAPS, int S, int D, bool TWO, bool PRO, class Epi>
int launch_dense(const Map &m, const float *a, const float *b, const unsigned *absmax, const unsigned char *packed, const Epi &epi, int O, float *out,
                 hipStream_t s, int Lo_ = -1, int Wo_ = -1)
{
    static DynamicLds lds;
    constexpr int lds_bytes = Win<TAPS, S, D, PRO>::kLdsBytes;
    const int status = lds.allow((const void *)dense_kernel<TAPS, S, D, TWO, PRO, Epi>, lds_bytes);
    if (status != 0) return status;
    const int Lo = Lo_ < 0 ? out_size(m.L, S) : Lo_, Wo = Lo_ < 0 ? out_size(m.W, S) : Wo_;
    const dim3 grid((unsigned)(tiles_x(Wo) * tiles_y(Lo)), (unsigned)out_tiles(O), (unsigned)m.B);
    hipLaunchKernelGGL((dense_kernel<TAPS, S, D, TWO, PRO, Epi>), grid, dim3(kThreads), lds_bytes, s, m, a, b, absmax, packed, epi, O, Lo, Wo, out);
    return (int)hipGetLastError();
}

} // namespace
#endif // VFA_DENSE_H
