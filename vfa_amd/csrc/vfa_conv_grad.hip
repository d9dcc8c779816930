// vfa_conv_grad.hip -- the weight gradient of the dense 3x3 convolution of vfa_conv.hip (stride 1, zero padding = dilation, dilation
// 1..4), for training the 256 -> 256 layers of the BEV heads:
//
//     dW[o, c, ty, tx] = sum_b sum_(l, w) g[b, o, l, w] x[b, c, l + (ty - 1) d, w + (tx - 1) d]        db[o] = sum_b sum_(l, w) g[b, o, l, w]
//
// g (B, O, L, W) and x (B, C, L, W) float32, both read through their four element strides; dW (O, C, 3, 3) contiguous.  Fixed summation
// order, no float atomics: the same bits on every run.  (The input gradient is the forward kernel on g with the transposed,
// tap-mirrored weight: vfa_conv3x3_pack_weights_transposed_f32.)  The integer rules: vfa_conv_grad.h.
//
//   1. absmax_kernel of vfa_dense.h (vfa_conv::frame_absmax) on g and on x: per frame the power-of-two scale of the fp16 split (vfa_split.h).
//   2. wgrad_kernel<D>: an implicit GEMM with M = outputs, N = inputs, K = cells, once per tap.  A workgroup of 4 waves owns one
//      (frame, slab of cells) and a tile of 128 outputs x 32 inputs x 9 taps; wave w takes the outputs 32 w .. 32 w + 31: nine 32 x 32
//      accumulators.  K runs in the forward kernel's tiles of 4 map rows x 32 columns: the tile's cells of g (128 outputs) and the
//      tile's window of x (the tile grown by the dilation, 32 inputs) are loaded through the strides, scaled, split under
//      MODE.FP16_OVFL and kept in LDS as two fp16 planes each, [cell][channel]; the next tile is in flight under the products.  Both
//      MFMA operands want 8 consecutive k of ONE channel per lane, which in these planes is a column: ds_read_b64_tr_b16, the
//      transposed LDS read, delivers it.  A tap moves the window location of a cell, never the alignment of a read, so the nine
//      taps read the one window at nine offsets.  A product is the three v_mfma_f32_32x32x16_f16 of vfa_split.h (g_lo x_hi, g_hi x_hi,
//      g_hi x_lo).  Epilogue: the partial acc 2^-(eg + ex) of the frame's two scales to the workspace, [frame][slab][tap][o][c].
//      PRO (the trunk's layers, vfa_trunk_conv_wgrad_f32, wgrad_kernel<1, true>): the x operand is max(fmaf(a[b, c], x, b[b, c]), 0), the
//      GroupNorm affine and the ReLU in front of the convolution, applied in x_load as a value arrives; a window position outside the
//      map is a zero AFTER that.  a | b of the workgroup's 32 inputs lie behind the planes in LDS, read from memory once; the absmax
//      pre-pass sees the same values.  Without PRO that region does not exist and pa, pb are not read.
//   3. wgrad_merge_kernel: per element of dW the partials in ascending (frame, slab) order, summed in float64, rounded once.
//   4. bias_grad_kernel: per output a workgroup; thread i sums the cells i, i + 256, .. of frame 0, then of frame 1, .. in float64,
//      the 256 sums are merged in a fixed tree and rounded once.
//   5. wgrad_down_kernel<9 | 1> (vfa_trunk_down_wgrad_f32): the weight gradient of the trunk's stride-2 convolutions, 3 x 3 with
//      padding 1 and 1 x 1: wgrad_kernel on K tiles of 2 x 32 cells of g, whose 5 x 65 window of x is stored by column parity so that
//      a tap still only moves an offset of the transposed reads; partials with 9 or 1 planes, merged by wgrad_merge_kernel<9 | 1>.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_conv.h"
#include "vfa_conv_grad.h"
#include "vfa_hip.h"
#include "vfa_split.h"

namespace {

using namespace vfa_conv;
using namespace vfa_conv_grad;
using vfa_dev::f16x4;
using vfa_dev::f16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));

constexpr int kThreads = 256;
constexpr int kExp = 14;  // both operands are scaled into [2^14, 2^15): a product is below 2^30 and a slab's sum far inside fp32
constexpr int kTileCells = kTileRows * kTileCols;
constexpr int kGQuads = kTileCells * (kTileO / 4);
constexpr int kGLoads = kGQuads / kThreads;
constexpr int kGPlaneHalves = kTileCells * kGHalves;

struct Map {
    const float *x;
    long long s_frame, s_chan, s_row, s_col; // element strides, >= 0
};

template <int D> struct Grad {
    static constexpr int kLoc = (kTileRows + 2 * D) * (kTileCols + 2 * D);
    static constexpr int kQuads = kLoc * (kTileC / 4);
    static constexpr int kLoads = (kQuads + kThreads - 1) / kThreads;
    static constexpr int kPlaneHalves = kLoc * kLocHalves;
    static constexpr int kPlaneBytes = (2 * kPlaneHalves + 2 * kGPlaneHalves) * 2;
    static constexpr int kLdsBytes = kPlaneBytes;                                      // without the prologue
    static constexpr int kLdsBytesPro = kPlaneBytes + 2 * kTileC * (int)sizeof(float); // a | b of the tile's inputs behind the planes
};

// quad e of the window of x: (location, four inputs 4 c4 .. 4 c4 + 3), consecutive threads on consecutive addresses of the map
template <int D> __device__ __forceinline__ void x_quad_of(int e, bool chan_fast, int &loc, int &c4)
{
    if (chan_fast) { c4 = e & 7; loc = e >> 3; }
    else { c4 = e / Grad<D>::kLoc; loc = e - c4 * Grad<D>::kLoc; }
}
// quad e of the tile of g: (cell of the tile, four outputs); CELLS: the cells of the tile, whole rows of it
template <int CELLS = kTileCells> __device__ __forceinline__ void g_quad_of(int e, bool chan_fast, int &cell, int &c4)
{
    if (chan_fast) { c4 = e & (kTileO / 4 - 1); cell = e / (kTileO / 4); }
    else { c4 = e / CELLS; cell = e & (CELLS - 1); }
}

__device__ __forceinline__ float prologue(float a, float x, float b)
{
    const float t = fmaf(a, x, b);
    return t < 0.0f ? 0.0f : t; // (a NaN stays a NaN)
}

// PRO: a value inside the map becomes max(fmaf(a, x, b), 0) with a | b of the tile's inputs in `ab`; a position outside the map is a
// zero, after that
template <int D, bool PRO>
__device__ __forceinline__ void x_load(const Map m, const float *ab, int L, int W, int b, int y0, int x0, int c0, bool chan_fast, int tid,
                                       float (&v)[Grad<D>::kLoads][4])
{
#pragma unroll
    for (int j = 0; j < Grad<D>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int loc, c4, y, x;
        x_quad_of<D>(e, chan_fast, loc, c4);
        const bool ok = e < Grad<D>::kQuads && window_position(loc, y0, x0, D, L, W, y, x);
        const float *p = m.x + (ok ? b * m.s_frame + (long long)(c0 + 4 * c4) * m.s_chan + y * m.s_row + x * m.s_col : 0);
        const int cq = ok ? 4 * c4 : 0; // (PRO)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (PRO) v[j][k] = ok ? prologue(ab[cq + k], p[k * m.s_chan], ab[kTileC + cq + k]) : 0.0f;
            else v[j][k] = ok ? p[k * m.s_chan] : 0.0f;
        }
    }
}

template <int D>
__device__ __forceinline__ void x_store(_Float16 *x_hi, _Float16 *x_lo, float sx, bool chan_fast, int tid, const float (&v)[Grad<D>::kLoads][4])
{
#pragma unroll
    for (int j = 0; j < Grad<D>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int loc, c4;
        x_quad_of<D>(e, chan_fast, loc, c4);
        uint2 hi, lo;
        vfa_dev::split_f16x4(v[j][0] * sx, v[j][1] * sx, v[j][2] * sx, v[j][3] * sx, hi, lo);
        if (e < Grad<D>::kQuads) {
            *(uint2 *)(x_hi + loc * kLocHalves + 4 * c4) = hi;
            *(uint2 *)(x_lo + loc * kLocHalves + 4 * c4) = lo;
        }
    }
}

// the tile's cells of g: outputs o0 .. o0 + 127; a cell outside the map and an output past O are zeros
template <int CELLS = kTileCells>
__device__ __forceinline__ void g_load(const Map m, int L, int W, int O, int b, int y0, int x0, int o0, bool chan_fast, int tid,
                                       float (&v)[kGLoads * CELLS / kTileCells][4])
{
#pragma unroll
    for (int j = 0; j < kGLoads * CELLS / kTileCells; ++j) {
        int cell, c4;
        g_quad_of<CELLS>(tid + kThreads * j, chan_fast, cell, c4);
        const int y = y0 + cell / kTileCols, x = x0 + cell % kTileCols, o = o0 + 4 * c4;
        const bool ok = y < L && x < W && o < O; // (O % 4 == 0: a quad is inside or outside)
        const float *p = m.x + (ok ? b * m.s_frame + (long long)o * m.s_chan + y * m.s_row + x * m.s_col : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = ok ? p[k * m.s_chan] : 0.0f;
    }
}

template <int CELLS = kTileCells>
__device__ __forceinline__ void g_store(_Float16 *g_hi, _Float16 *g_lo, float sg, bool chan_fast, int tid, const float (&v)[kGLoads * CELLS / kTileCells][4])
{
#pragma unroll
    for (int j = 0; j < kGLoads * CELLS / kTileCells; ++j) {
        int cell, c4;
        g_quad_of<CELLS>(tid + kThreads * j, chan_fast, cell, c4);
        uint2 hi, lo;
        vfa_dev::split_f16x4(v[j][0] * sg, v[j][1] * sg, v[j][2] * sg, v[j][3] * sg, hi, lo);
        *(uint2 *)(g_hi + cell * kGHalves + 4 * c4) = hi;
        *(uint2 *)(g_lo + cell * kGHalves + 4 * c4) = lo;
    }
}

// ds_read_b64_tr_b16: per group of 16 lanes a block of 4 rows x 16 columns of the [cell][channel] plane, column-major -- lane 4 q + p of
// the group gives the address of row q, columns 4 p .. 4 p + 3 (8-byte aligned), lane i receives column i, row q in element q.
// Every lane of the wave must be active.
__device__ __forceinline__ f16x4 read_transposed(const _Float16 *p)
{
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)p));
}
// the 32x32x16 operand of 32 channels x 16 cells: `p` is this lane's address in the first of its 8 cells, `step` the halves between
// two cells; element j of the lane is cell 8 h + j of the step (h = lane >> 5), its channel lane & 31
__device__ __forceinline__ f16x8 operand(const _Float16 *p, int step)
{
    const f16x4 a = read_transposed(p), b = read_transposed(p + 4 * step);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int D, bool PRO = false>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const Map mg, const Map mx, const float *__restrict__ pa, const float *__restrict__ pb,
                                                         const unsigned *__restrict__ absmax, int B, int C, int L, int W, int O,
                                                         float *__restrict__ partial)
{
    extern __shared__ __align__(16) unsigned char lds[];
    _Float16 *x_hi = (_Float16 *)lds, *x_lo = x_hi + Grad<D>::kPlaneHalves, *g_hi = x_lo + Grad<D>::kPlaneHalves, *g_lo = g_hi + kGPlaneHalves;
    const float *ab = (const float *)(lds + Grad<D>::kPlaneBytes); // (PRO)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int slab = blockIdx.x, b = blockIdx.z, n_c = C / kTileC;
    const int o0 = ((int)blockIdx.y / n_c) * kTileO, c0 = ((int)blockIdx.y % n_c) * kTileC;
    const bool g_fast = mg.s_chan == 1, x_fast = mx.s_chan == 1;
    const int eg = vfa_dev::split_exponent(absmax[b], kExp), ex = vfa_dev::split_exponent(absmax[B + b], kExp);
    const float sg = vfa_dev::pow2f(eg), sx = vfa_dev::pow2f(ex);
    const int n_slabs = (int)gridDim.x; // slabs(L, W), or the trunk's slabs_for(L, W, O, C)
    const int tile_begin = slab_begin_of(slab, n_slabs, L, W), tile_end = slab_begin_of(slab + 1, n_slabs, L, W);

    // this lane's part of the transposed reads: row q of its group's block is cell 8 h + q of the step, columns 4 p .. of the
    // group's 16 channels
    const int q = (lane >> 2) & 3, p = lane & 3, half16 = (lane >> 4) & 1;
    const int k_lane = 8 * h + q, ch_lane = 16 * half16 + 4 * p;

    float vx[Grad<D>::kLoads][4], vg[kGLoads][4];
    int y0, x0;
    tile_origin(tile_begin, W, y0, x0);
    if constexpr (PRO) { // a | b of this workgroup's inputs, once: threads 0 .. 63
        if (tid < 2 * kTileC) ((float *)(lds + Grad<D>::kPlaneBytes))[tid] = (tid < kTileC ? pa : pb)[(size_t)b * C + c0 + (tid & (kTileC - 1))];
        __syncthreads();
    }
    x_load<D, PRO>(mx, ab, L, W, b, y0, x0, c0, x_fast, tid, vx);
    g_load(mg, L, W, O, b, y0, x0, o0, g_fast, tid, vg);
    vfa_dev::fp16_saturate_mode(true);
    x_store<D>(x_hi, x_lo, sx, x_fast, tid, vx);
    g_store(g_hi, g_lo, sg, g_fast, tid, vg);
    vfa_dev::fp16_saturate_mode(false);
    __syncthreads();

    f32x16 acc[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const bool more = tile + 1 < tile_end; // (uniform)
        if (more) {
            tile_origin(tile + 1, W, y0, x0);
            x_load<D, PRO>(mx, ab, L, W, b, y0, x0, c0, x_fast, tid, vx);
            g_load(mg, L, W, O, b, y0, x0, o0, g_fast, tid, vg);
        }
#pragma unroll 1
        for (int ks = 0; ks < kTileCells / 16; ++ks) { // 16 cells of one tile row
            const int ry = ks >> 1, rx = (ks & 1) * 16 + k_lane;
            const int g_at = (ry * kTileCols + rx) * kGHalves + wave * 32 + ch_lane;
            const f16x8 gh = operand(g_hi + g_at, kGHalves), gl = operand(g_lo + g_at, kGHalves);
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const int x_at = window_index(ry, rx, t, D) * kLocHalves + ch_lane;
                const f16x8 xh = operand(x_hi + x_at, kLocHalves), xl = operand(x_lo + x_at, kLocHalves);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, xh, acc[t], 0, 0, 0); // rows = outputs, columns = inputs
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xl, acc[t], 0, 0, 0);
            }
        }
        __syncthreads(); // the planes are free
        if (more) {
            vfa_dev::fp16_saturate_mode(true);
            x_store<D>(x_hi, x_lo, sx, x_fast, tid, vx);
            g_store(g_hi, g_lo, sg, g_fast, tid, vg);
            vfa_dev::fp16_saturate_mode(false);
            __syncthreads();
        }
    }

    const float inv = vfa_dev::pow2f(-(eg + ex));
    const int c = c0 + r;
#pragma unroll
    for (int t = 0; t < kTaps; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { // C/D: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
            const int o = o0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (o < O) partial[partial_index_of(b, slab, n_slabs, t, o, c, O, C)] = acc[t][i] * inv;
        }
}

// ---- stride 2 (vfa_trunk_down_wgrad_f32; the rules: vfa_conv_grad.h) -------------------------------------------------------------------
// TAPS 9: the 3 x 3 weight with padding 1; TAPS 1: the 1 x 1 weight.  g is (Lo, Wo), x (L, W).  wgrad_kernel with K tiles of 2 x 32
// cells (64 cells of g, a 5 x 65 window of x stored by column parity: 52 000 + 34 816 bytes), two per tile of the slab walk.
template <int TAPS> struct Down {
    static constexpr int kCells = kDownRows * kTileCols;
    static constexpr int kLoc = down_window_locations(TAPS);
    static constexpr int kQuads = kLoc * (kTileC / 4);
    static constexpr int kLoads = (kQuads + kThreads - 1) / kThreads;
    static constexpr int kGLoadsDown = kGLoads * kCells / kTileCells;
    static constexpr int kPlaneHalves = kLoc * kLocHalves;
    static constexpr int kGPlaneHalvesDown = kCells * kGHalves;
    static constexpr int kLdsBytes = (2 * kPlaneHalves + 2 * kGPlaneHalvesDown) * 2;
    static_assert(kCells % 16 == 0 && kGQuads % kThreads == 0 && (kCells * (kTileO / 4)) % kThreads == 0, "whole steps, whole loads");
    static_assert(kLdsBytes <= 160 * 1024, "the window of x and the cells of g of one K tile share the CU's LDS");
};

// quad e of the K tile's window: (window position in map order, four inputs)
template <int TAPS> __device__ __forceinline__ void down_quad_of(int e, bool chan_fast, int &p, int &c4)
{
    if (chan_fast) { c4 = e & 7; p = e >> 3; }
    else { c4 = e / Down<TAPS>::kLoc; p = e - c4 * Down<TAPS>::kLoc; }
}

template <int TAPS>
__device__ __forceinline__ void down_x_load(const Map m, int L, int W, int b, int y0, int x0, int c0, bool chan_fast, int tid,
                                            float (&v)[Down<TAPS>::kLoads][4])
{
#pragma unroll
    for (int j = 0; j < Down<TAPS>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4, y, x;
        down_quad_of<TAPS>(e, chan_fast, p, c4);
        const bool ok = e < Down<TAPS>::kQuads && down_window_position(p, y0, x0, TAPS, L, W, y, x);
        const float *src = m.x + (ok ? b * m.s_frame + (long long)(c0 + 4 * c4) * m.s_chan + y * m.s_row + x * m.s_col : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = ok ? src[k * m.s_chan] : 0.0f;
    }
}

template <int TAPS>
__device__ __forceinline__ void down_x_store(_Float16 *x_hi, _Float16 *x_lo, float sx, bool chan_fast, int tid, const float (&v)[Down<TAPS>::kLoads][4])
{
#pragma unroll
    for (int j = 0; j < Down<TAPS>::kLoads; ++j) {
        const int e = tid + kThreads * j;
        int p, c4;
        down_quad_of<TAPS>(e, chan_fast, p, c4);
        uint2 hi, lo;
        vfa_dev::split_f16x4(v[j][0] * sx, v[j][1] * sx, v[j][2] * sx, v[j][3] * sx, hi, lo);
        if (e < Down<TAPS>::kQuads) {
            const int loc = down_window_location(p, TAPS);
            *(uint2 *)(x_hi + loc * kLocHalves + 4 * c4) = hi;
            *(uint2 *)(x_lo + loc * kLocHalves + 4 * c4) = lo;
        }
    }
}

// grid (slabs of (Lo, Wo), output tiles x input chunks, frames), as wgrad_kernel
template <int TAPS>
__global__ __launch_bounds__(kThreads) void wgrad_down_kernel(const Map mg, const Map mx, const unsigned *__restrict__ absmax, int B, int C, int L, int W,
                                                              int Lo, int Wo, int O, float *__restrict__ partial)
{
    typedef Down<TAPS> DN;
    extern __shared__ __align__(16) unsigned char lds[];
    _Float16 *x_hi = (_Float16 *)lds, *x_lo = x_hi + DN::kPlaneHalves, *g_hi = x_lo + DN::kPlaneHalves, *g_lo = g_hi + DN::kGPlaneHalvesDown;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int slab = blockIdx.x, b = blockIdx.z, n_c = C / kTileC;
    const int o0 = ((int)blockIdx.y / n_c) * kTileO, c0 = ((int)blockIdx.y % n_c) * kTileC;
    const bool g_fast = mg.s_chan == 1, x_fast = mx.s_chan == 1;
    const int eg = vfa_dev::split_exponent(absmax[b], kExp), ex = vfa_dev::split_exponent(absmax[B + b], kExp);
    const float sg = vfa_dev::pow2f(eg), sx = vfa_dev::pow2f(ex);
    const int n_slabs = (int)gridDim.x; // slabs_for(Lo, Wo, O, C)
    const int k_begin = slab_begin_of(slab, n_slabs, Lo, Wo) * kDownHalves, k_end = slab_begin_of(slab + 1, n_slabs, Lo, Wo) * kDownHalves;

    const int q = (lane >> 2) & 3, p = lane & 3, half16 = (lane >> 4) & 1; // (the transposed reads: wgrad_kernel)
    const int k_lane = 8 * h + q, ch_lane = 16 * half16 + 4 * p;

    float vx[DN::kLoads][4], vg[DN::kGLoadsDown][4];
    int y0, x0;
    down_origin(k_begin / kDownHalves, k_begin % kDownHalves, Wo, y0, x0);
    down_x_load<TAPS>(mx, L, W, b, y0, x0, c0, x_fast, tid, vx);
    g_load<DN::kCells>(mg, Lo, Wo, O, b, y0, x0, o0, g_fast, tid, vg);
    vfa_dev::fp16_saturate_mode(true);
    down_x_store<TAPS>(x_hi, x_lo, sx, x_fast, tid, vx);
    g_store<DN::kCells>(g_hi, g_lo, sg, g_fast, tid, vg);
    vfa_dev::fp16_saturate_mode(false);
    __syncthreads();

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    for (int k = k_begin; k < k_end; ++k) { // K tiles: ascending tiles, the upper half of a tile first
        const bool more = k + 1 < k_end; // (uniform)
        if (more) {
            down_origin((k + 1) / kDownHalves, (k + 1) % kDownHalves, Wo, y0, x0);
            down_x_load<TAPS>(mx, L, W, b, y0, x0, c0, x_fast, tid, vx);
            g_load<DN::kCells>(mg, Lo, Wo, O, b, y0, x0, o0, g_fast, tid, vg);
        }
#pragma unroll 1
        for (int ks = 0; ks < DN::kCells / 16; ++ks) { // 16 cells of one row of the K tile
            const int ry = ks >> 1, rx = (ks & 1) * 16 + k_lane;
            const int g_at = (ry * kTileCols + rx) * kGHalves + wave * 32 + ch_lane;
            const f16x8 gh = operand(g_hi + g_at, kGHalves), gl = operand(g_lo + g_at, kGHalves);
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int x_at = down_tap_location(ry, rx, t, TAPS) * kLocHalves + ch_lane;
                const f16x8 xh = operand(x_hi + x_at, kLocHalves), xl = operand(x_lo + x_at, kLocHalves);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, xh, acc[t], 0, 0, 0); // rows = outputs, columns = inputs
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, xl, acc[t], 0, 0, 0);
            }
        }
        __syncthreads(); // the planes are free
        if (more) {
            vfa_dev::fp16_saturate_mode(true);
            down_x_store<TAPS>(x_hi, x_lo, sx, x_fast, tid, vx);
            g_store<DN::kCells>(g_hi, g_lo, sg, g_fast, tid, vg);
            vfa_dev::fp16_saturate_mode(false);
            __syncthreads();
        }
    }

    const float inv = vfa_dev::pow2f(-(eg + ex));
    const int c = c0 + r;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { // C/D: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
            const int o = o0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (o < O) partial[down_partial_index(b, slab, n_slabs, t, o, c, O, C, TAPS)] = acc[t][i] * inv;
        }
}

// one thread per element (t, o, c) of a partial: consecutive threads on consecutive addresses of every partial
template <int TAPS = kTaps>
__global__ __launch_bounds__(kThreads) void wgrad_merge_kernel(const float *__restrict__ partial, int n_partials, int O, int C, float *__restrict__ dw)
{
    const size_t per = down_partial_floats(O, C, TAPS), i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= per) return;
    double sum = 0.0;
    for (int k = 0; k < n_partials; ++k) sum += (double)partial[(size_t)k * per + i]; // ascending (frame, slab)
    const size_t oc = i % ((size_t)O * C), t = i / ((size_t)O * C);
    dw[oc * TAPS + t] = (float)sum;
}

// grid (O): thread i takes the cells i, i + 256, .. of frame 0, then of frame 1, ..
__global__ __launch_bounds__(kThreads) void bias_grad_kernel(const Map mg, int B, int L, int W, float *__restrict__ db)
{
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, o = blockIdx.x, plane = L * W;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float *src = mg.x + b * mg.s_frame + (long long)o * mg.s_chan;
        for (int i = tid; i < plane; i += kThreads) {
            const int y = i / W, x = i - y * W;
            s += (double)src[y * mg.s_row + x * mg.s_col];
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) { // a fixed tree
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) db[o] = (float)red[0];
}

size_t scales_bytes(int B) { return ((size_t)2 * B * sizeof(unsigned) + 255) / 256 * 256; }

template <int D, bool PRO = false>
int launch_wgrad(const Map &mg, const Map &mx, const float *a, const float *b, const unsigned *absmax, int B, int C, int L, int W, int O, int n_slabs,
                 float *partial, hipStream_t s)
{
    static DynamicLds lds; // (vfa_conv.h: once per device)
    constexpr int lds_bytes = PRO ? Grad<D>::kLdsBytesPro : Grad<D>::kLdsBytes;
    const int status = lds.allow((const void *)wgrad_kernel<D, PRO>, lds_bytes);
    if (status != 0) return status;
    const dim3 grid((unsigned)n_slabs, (unsigned)(((O + kTileO - 1) / kTileO) * (C / kTileC)), (unsigned)B);
    hipLaunchKernelGGL((wgrad_kernel<D, PRO>), grid, dim3(kThreads), lds_bytes, s, mg, mx, a, b, absmax, B, C, L, W, O, partial);
    return (int)hipGetLastError();
}

bool sizes_ok(int B, int O, int C, int L, int W)
{
    return B <= 65535 && L <= 65535 && (long long)L * W <= INT32_MAX / 2 && (long long)O * C * kTaps <= INT32_MAX / 2 &&
           (long long)((O + kTileO - 1) / kTileO) * (C / kTileC) <= 65535;
}

template <int TAPS>
int launch_wgrad_down(const Map &mg, const Map &mx, const unsigned *absmax, int B, int C, int L, int W, int O, int n_slabs, float *partial,
                             float *dw, hipStream_t s)
{
    static DynamicLds lds; // (vfa_conv.h: once per device)
    const int status = lds.allow((const void *)wgrad_down_kernel<TAPS>, Down<TAPS>::kLdsBytes);
    if (status != 0) return status;
    const int Lo = out_size(L, 2), Wo = out_size(W, 2);
    const dim3 grid((unsigned)n_slabs, (unsigned)(((O + kTileO - 1) / kTileO) * (C / kTileC)), (unsigned)B);
    hipLaunchKernelGGL((wgrad_down_kernel<TAPS>), grid, dim3(kThreads), Down<TAPS>::kLdsBytes, s, mg, mx, absmax, B, C, L, W, Lo, Wo, O, partial);
    const size_t per = down_partial_floats(O, C, TAPS);
    hipLaunchKernelGGL(wgrad_merge_kernel<TAPS>, dim3((unsigned)((per + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, partial, B * n_slabs, O, C, dw);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

// 0: no such problem, or an empty one
static size_t wgrad_workspace_bytes(int B, int O, int C, int L, int W, bool trunk)
{
    if (B <= 0 || O < 1 || C < 1 || L <= 0 || W <= 0 || O % 32 != 0 || C % kTileC != 0 || !sizes_ok(B, O, C, L, W)) return 0;
    return scales_bytes(B) + (size_t)B * (trunk ? slabs_for(L, W, O, C) : slabs(L, W)) * partial_floats(O, C) * sizeof(float);
}

size_t vfa_conv3x3_wgrad_workspace_bytes(int B, int O, int C, int L, int W) { return wgrad_workspace_bytes(B, O, C, L, W, false); }

size_t vfa_trunk_conv_wgrad_workspace_bytes(int B, int O, int C, int L, int W) { return wgrad_workspace_bytes(B, O, C, L, W, true); }

// the entry points' common body; a, b: both nullptr, or the (B, C) prologue of x (dilation 1); trunk: the slabs of slabs_for
static int wgrad(const float *g, const long long *g_stride, const float *x, const long long *x_stride, const float *a, const float *b, int B, int C,
                 int L, int W, int O, int dilation, bool trunk, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || C < 1 || L < 0 || W < 0 || O < 1 || dilation < 1 || !dw) return VFA_ERR_BAD_ARGUMENT;
    if (O % 32 != 0 || C % kTileC != 0 || dilation > kMaxDilation || !sizes_ok(B, O, C, L, W)) return VFA_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || (long long)L * W == 0) { // an empty sum
        hipError_t e = hipMemsetAsync(dw, 0, (size_t)O * C * kTaps * sizeof(float), s);
        if (e == hipSuccess && db) e = hipMemsetAsync(db, 0, (size_t)O * sizeof(float), s);
        return (int)e;
    }
    if (!g || !g_stride || !x || !x_stride) return VFA_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i)
        if (g_stride[i] < 0 || x_stride[i] < 0) return VFA_ERR_BAD_ARGUMENT;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < wgrad_workspace_bytes(B, O, C, L, W, trunk)) return VFA_ERR_BAD_ARGUMENT;
    const int n_slabs = trunk ? slabs_for(L, W, O, C) : slabs(L, W);
    const Map mg = {g, g_stride[0], g_stride[1], g_stride[2], g_stride[3]}, mx = {x, x_stride[0], x_stride[1], x_stride[2], x_stride[3]};
    unsigned *absmax = (unsigned *)workspace;
    float *partial = (float *)((unsigned char *)workspace + scales_bytes(B));
    const hipError_t e = hipMemsetAsync(absmax, 0, scales_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    int status = vfa_conv::frame_absmax(g, g_stride, B, O, L, W, absmax, stream);
    if (status == 0) status = vfa_conv::frame_absmax(x, x_stride, a, b, B, C, L, W, absmax + B, stream);
    if (status != 0) return status;
    if (a) status = launch_wgrad<1, true>(mg, mx, a, b, absmax, B, C, L, W, O, n_slabs, partial, s);
    else
        switch (dilation) {
        case 1: status = launch_wgrad<1>(mg, mx, a, b, absmax, B, C, L, W, O, n_slabs, partial, s); break;
        case 2: status = launch_wgrad<2>(mg, mx, a, b, absmax, B, C, L, W, O, n_slabs, partial, s); break;
        case 3: status = launch_wgrad<3>(mg, mx, a, b, absmax, B, C, L, W, O, n_slabs, partial, s); break;
        default: status = launch_wgrad<4>(mg, mx, a, b, absmax, B, C, L, W, O, n_slabs, partial, s); break;
        }
    if (status != 0) return status;
    const size_t per = partial_floats(O, C);
    hipLaunchKernelGGL(wgrad_merge_kernel<kTaps>, dim3((unsigned)((per + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, partial, B * n_slabs, O, C, dw);
    if (db) hipLaunchKernelGGL(bias_grad_kernel, dim3((unsigned)O), dim3(kThreads), 0, s, mg, B, L, W, db);
    return (int)hipGetLastError();
}

int vfa_conv3x3_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, int B, int C, int L, int W,
                          int O, int dilation, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream)
{
    return wgrad(g, g_stride, x, x_stride, nullptr, nullptr, B, C, L, W, O, dilation, false, dw, db, workspace, workspace_bytes, stream);
}

int vfa_trunk_conv_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, const float *a, const float *b,
                             int B, int C, int L, int W, int O, float *dw, void *workspace, size_t workspace_bytes, void *stream)
{
    if ((a == nullptr) != (b == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    return wgrad(g, g_stride, x, x_stride, a, b, B, C, L, W, O, 1, true, dw, nullptr, workspace, workspace_bytes, stream);
}

// (L, W): the size of x; kernel 3 | 1.  0: no such problem, or an empty one
size_t vfa_trunk_down_wgrad_workspace_bytes(int B, int O, int C, int L, int W, int kernel)
{
    if (B <= 0 || O < 1 || C < 1 || L <= 0 || W <= 0 || (kernel != 3 && kernel != 1) || O % 32 != 0 || C % kTileC != 0 || !sizes_ok(B, O, C, L, W)) return 0;
    return scales_bytes(B) + (size_t)B * slabs_for(out_size(L, 2), out_size(W, 2), O, C) * down_partial_floats(O, C, kernel * kernel) * sizeof(float);
}

int vfa_trunk_down_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, int B, int C, int L, int W, int O,
                             int kernel, float *dw, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || C < 1 || L < 0 || W < 0 || O < 1 || (kernel != 3 && kernel != 1) || !dw) return VFA_ERR_BAD_ARGUMENT;
    if (O % 32 != 0 || C % kTileC != 0 || !sizes_ok(B, O, C, L, W)) return VFA_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || (long long)L * W == 0) return (int)hipMemsetAsync(dw, 0, (size_t)O * C * kernel * kernel * sizeof(float), s); // an empty sum
    if (!g || !g_stride || !x || !x_stride) return VFA_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i)
        if (g_stride[i] < 0 || x_stride[i] < 0) return VFA_ERR_BAD_ARGUMENT;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < vfa_trunk_down_wgrad_workspace_bytes(B, O, C, L, W, kernel))
        return VFA_ERR_BAD_ARGUMENT;
    const int Lo = out_size(L, 2), Wo = out_size(W, 2), n_slabs = slabs_for(Lo, Wo, O, C);
    const Map mg = {g, g_stride[0], g_stride[1], g_stride[2], g_stride[3]}, mx = {x, x_stride[0], x_stride[1], x_stride[2], x_stride[3]};
    unsigned *absmax = (unsigned *)workspace;
    float *partial = (float *)((unsigned char *)workspace + scales_bytes(B));
    const hipError_t e = hipMemsetAsync(absmax, 0, scales_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    int status = vfa_conv::frame_absmax(g, g_stride, B, O, Lo, Wo, absmax, stream);
    if (status == 0) status = vfa_conv::frame_absmax(x, x_stride, B, C, L, W, absmax + B, stream); // (1 x 1: a scale of the whole of x serves)
    if (status != 0) return status;
    return kernel == 3 ? launch_wgrad_down<9>(mg, mx, absmax, B, C, L, W, O, n_slabs, partial, dw, s)
                       : launch_wgrad_down<1>(mg, mx, absmax, B, C, L, W, O, n_slabs, partial, dw, s);
}

} // extern "C"
