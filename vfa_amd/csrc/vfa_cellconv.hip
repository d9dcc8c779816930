// vfa_cellconv.hip -- a 3x3 dilated convolution (C -> O channels, zero padding = dilation, no bias) evaluated ONLY at listed cells
// of a batch of BEV maps, with its backward: the orientation head of VFANet (256 -> 360, dilation 4) is read at the top-k cells of
// the decode in inference and at the positive cells of the loss in training, so the dense (B, O, L, W) map is never made.
// The same function as the dense convolution gathered at the cells, up to the fp32 summation order.
//
// A gather-GEMM: M = B * k rows (cells), N = O, K = 9 C, the weight (O, C, 3, 3) read as an (O, K) matrix whose k = 9 c + t.
// The integer logic (skipped rows, tap locations, the zero border, who writes a location of d_feat): vfa_cellconv.h.
//
//   1. cellconv_forward_kernel, one workgroup of 4 waves per tile of 16 rows x 64 outputs.  K runs in chunks of 32 channels (288
//      k): the 256 threads gather the chunk's taps of the 16 rows into LDS through feat's four strides (4-byte loads; a tap outside
//      the map and every tap of a skipped row is a zero and forms no address), the next chunk's loads -- taps and weights -- in flight under this
//      chunk's products.  Products: the exact f32 MFMA v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain).  Wave (h, p) takes half h of the
//      chunk's k (9 steps of 16) for the output tiles 2 p and 2 p + 1; the halves are combined in LDS as (half 0) + (half 1).  A
//      fixed order, no atomics: the same bits on every run, and the logits do not know whether the rotation is wanted.
//   2. cellconv_rotation_kernel, one wave per row: the decode's rotation rule (vfa_rotation.h) on the row's logits.
//   3. cellconv_grad_weight_kernel, one workgroup per (32 channels, 32 outputs): the same gather, row tile by row tile, and
//      d_weight[o, k] += d_logits[row, o] * tap[row, k] as one fmaf chain in ASCENDING row order.
//   4. cellconv_grad_feat_kernel, one workgroup per row, one thread per channel, after the map was cleared: the nine taps'
//      sums over o from nine contiguous weights; a location is written by the lowest row with a tap on it, which then adds the
//      later rows' pairs in ascending order (vfa_cellconv.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_cellconv.h"
#include "vfa_hip.h"
#include "vfa_rotation.h"

namespace {

using namespace vfa_cellconv;

constexpr int kThreads = 256;
constexpr int kRows = 16;               // rows of a tile: the M of one MFMA
constexpr int kChunkC = 32;             // channels of an LDS chunk (C % 32 == 0)
constexpr int kChunkK = kChunkC * kTaps; // 288 = 18 steps of 16 k
constexpr int kStride = kChunkK + 4;    // LDS row stride in floats: 16-byte aligned rows, 4 banks apart
constexpr int kSteps = kChunkK / 16;    // 18
constexpr int kHalf = kSteps / 2;       // steps of one wave: half of a chunk's k
constexpr int kLoads = kRows * kChunkK / kThreads; // 18 gathered values per thread and chunk
constexpr int kOutTile = 64;            // outputs of a forward workgroup: 2 wave pairs x 2 MFMA tiles of 16
constexpr int kGradO = 32;              // outputs of a grad-weight workgroup
constexpr int kGradAcc = kGradO * kChunkK / kThreads; // 36

static_assert(kRows * kChunkK % kThreads == 0 && kSteps % 2 == 0 && kGradO * kChunkK % kThreads == 0, "tiling");

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct Cells {
    const float *feat;
    long long s_frame, s_chan, s_row, s_col; // element strides of feat (B, C, L, W), >= 0
    const int *cell;                          // (B, k)
    long long M;                              // B * k
    int C, L, W, O, k, dilation;
};

// The offsets of the 9 taps of the 16 rows from `row0` on (without the channel term), -1: no load (outside the map, a skipped row, a
// row past M); row_ok: the row exists and is not skipped.  Threads 0 .. 143; the caller synchronises.
__device__ __forceinline__ void tile_offsets(const Cells &a, long long row0, long long *tap_off, int *row_ok, int tid)
{
    if (tid < kRows * kTaps) {
        const int i = tid / kTaps, t = tid - i * kTaps;
        const long long row = row0 + i;
        long long off = -1;
        bool ok = false;
        if (row < a.M) {
            const int cell = a.cell[row];
            ok = cell_valid(cell, a.L, a.W);
            int y, x;
            if (ok && tap_location(cell, t, a.L, a.W, a.dilation, y, x)) off = (row / a.k) * a.s_frame + y * a.s_row + x * a.s_col;
        }
        tap_off[tid] = off;
        if (t == 0) row_ok[i] = ok;
    }
}

// value e = tid + 256 j of a chunk is (row i = e / 288, k = e % 288 = 9 c + t): consecutive threads, consecutive LDS words
__device__ __forceinline__ void gather_load(const Cells &a, const long long *tap_off, int c0, int tid, float (&v)[kLoads])
{
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
        const int e = tid + kThreads * j, i = e / kChunkK, kk = e - i * kChunkK, c = kk / kTaps, t = kk - c * kTaps;
        const long long off = tap_off[i * kTaps + t];
        v[j] = off < 0 ? 0.0f : a.feat[off + (long long)(c0 + c) * a.s_chan];
    }
}
__device__ __forceinline__ void gather_store(float *taps, int tid, const float (&v)[kLoads])
{
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
        const int e = tid + kThreads * j, i = e / kChunkK, kk = e - i * kChunkK;
        taps[i * kStride + kk] = v[j];
    }
}

// a wave's weights of one chunk: 9 steps of 16 k for two output tiles, 16 bytes per lane and step
__device__ __forceinline__ void load_weights(const float *const (&w_row)[2], int chunk, f32x4 (&bw)[2][kHalf])
{
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int s = 0; s < kHalf; ++s) bw[n][s] = *(const f32x4 *)(w_row[n] + (long long)chunk * kChunkK + 16 * s);
}

__global__ __launch_bounds__(kThreads) void cellconv_forward_kernel(const Cells a, const float *__restrict__ weight, float *__restrict__ logits)
{
    __shared__ __attribute__((aligned(16))) float taps[2][kRows * kStride];
    __shared__ __attribute__((aligned(16))) f32x4 part[2][2][64];
    __shared__ long long tap_off[kRows * kTaps];
    __shared__ int row_ok[kRows];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = wave & 1, pair = wave >> 1;
    const int i = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * kRows;
    const int o0 = blockIdx.y * kOutTile + pair * 32;
    const long long K = (long long)a.C * kTaps;

    tile_offsets(a, row0, tap_off, row_ok, tid);
    __syncthreads();

    // this lane's weight rows of the two output tiles, from its half of a chunk on (past O: row O - 1 is read and a zero is used)
    const float *w_row[2];
    bool w_ok[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int o = o0 + 16 * n + i;
        w_ok[n] = o < a.O;
        w_row[n] = weight + (long long)(w_ok[n] ? o : a.O - 1) * K + 16 * half * kHalf + 4 * g;
    }

    float v[kLoads];
    gather_load(a, tap_off, 0, tid, v);
    f32x4 bw[2][kHalf], bw_next[2][kHalf]; // this chunk's weights and the next one's: every load of a chunk is in flight at once
    load_weights(w_row, 0, bw);
    gather_store(taps[0], tid, v);
    __syncthreads();

    f32x4 acc[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n_chunks = a.C / kChunkC;
    for (int ch = 0; ch < n_chunks; ++ch) {
        const bool more = ch + 1 < n_chunks; // (uniform)
        if (more) {
            gather_load(a, tap_off, (ch + 1) * kChunkC, tid, v);
            load_weights(w_row, ch + 1, bw_next);
        }
        const float *mine = taps[ch & 1] + i * kStride + 16 * half * kHalf + 4 * g;
#pragma unroll
        for (int s = 0; s < kHalf; ++s) { // lane (i, g) holds k = 16 (9 half + s) + 4 g .. + 3 of row i and of output i
            const f32x4 av = *(const f32x4 *)(mine + 16 * s);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const f32x4 bv = w_ok[n] ? bw[n][s] : zero;
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[n], 0, 0, 0);
            }
        }
        if (more) {
            gather_store(taps[(ch + 1) & 1], tid, v);
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int s = 0; s < kHalf; ++s) bw[n][s] = bw_next[n][s];
        }
        __syncthreads(); // the next chunk is in LDS, and this chunk's buffer is free for the one after it
    }

    if (half == 1) { part[pair][0][lane] = acc[0]; part[pair][1][lane] = acc[1]; }
    __syncthreads();
    if (half == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const f32x4 sum = acc[n] + part[pair][n][lane]; // (half 0) + (half 1)
            const int o = o0 + 16 * n + i;                  // C/D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ri = 4 * g + r;
                const long long row = row0 + ri;
                if (row < a.M && o < a.O) logits[row * a.O + o] = row_ok[ri] ? sum[r] : 0.0f;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void cellconv_rotation_kernel(const int *cell, const float *logits, float *rotation, long long M,
                                                                      int L, int W, int O)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= M) return; // (uniform per wave)
    float value = 0.0f;
    if (cell_valid(cell[row], L, W)) value = vfa_rotation::wave_rotation(logits + row * O, 1, O, lane);
    if (lane == 0) rotation[row] = value;
}

__global__ __launch_bounds__(kThreads) void cellconv_grad_weight_kernel(const Cells a, const float *__restrict__ d_logits,
                                                                         float *__restrict__ d_weight)
{
    __shared__ float taps[kRows * kStride];
    __shared__ float grad[kRows * kGradO];
    __shared__ long long tap_off[kRows * kTaps];
    __shared__ int row_ok[kRows];

    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kChunkC, o0 = blockIdx.y * kGradO;
    float acc[kGradAcc];
#pragma unroll
    for (int j = 0; j < kGradAcc; ++j) acc[j] = 0.0f;

    for (long long row0 = 0; row0 < a.M; row0 += kRows) { // ascending rows
        tile_offsets(a, row0, tap_off, row_ok, tid);
        __syncthreads();
        float v[kLoads];
        gather_load(a, tap_off, c0, tid, v);
        gather_store(taps, tid, v);
        for (int e = tid; e < kRows * kGradO; e += kThreads) {
            const int i = e / kGradO, o = o0 + (e - i * kGradO);
            grad[e] = row_ok[i] && o < a.O ? d_logits[(row0 + i) * a.O + o] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kGradAcc; ++j) {
            const int e = tid + kThreads * j, ol = e / kChunkK, kk = e - ol * kChunkK;
#pragma unroll
            for (int i = 0; i < kRows; ++i) acc[j] = fmaf(grad[i * kGradO + ol], taps[i * kStride + kk], acc[j]);
        }
        __syncthreads();
    }
    const long long K = (long long)a.C * kTaps;
#pragma unroll
    for (int j = 0; j < kGradAcc; ++j) {
        const int e = tid + kThreads * j, ol = e / kChunkK, kk = e - ol * kChunkK;
        if (o0 + ol < a.O) d_weight[(long long)(o0 + ol) * K + (long long)c0 * kTaps + kk] = acc[j];
    }
}

// d_feat (B, C, L, W) contiguous, cleared before.  Workgroup = row, thread = channel.
__global__ __launch_bounds__(kThreads) void cellconv_grad_feat_kernel(const Cells a, const float *__restrict__ d_logits,
                                                                       const float *__restrict__ weight, float *__restrict__ d_feat)
{
    __shared__ signed char land[kTaps][kMaxRows]; // land[t][j]: the tap of row j of the frame on the location of my tap t, -1: none
    __shared__ int loc_y[kTaps], loc_x[kTaps], owned[kTaps], later[kTaps];

    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const long long frame = row / a.k;
    const int mine = (int)(row - frame * a.k);
    const int *cells = a.cell + frame * a.k;
    const int cell = cells[mine];
    if (!cell_valid(cell, a.L, a.W)) return; // (uniform) a skipped row writes nothing and forms no address

    if (tid < kTaps) {
        int y = -1, x = -1;
        tap_location(cell, tid, a.L, a.W, a.dilation, y, x);
        loc_y[tid] = y;
        loc_x[tid] = x;
    }
    __syncthreads();
    for (int e = tid; e < kTaps * a.k; e += kThreads) {
        const int t = e / a.k, j = e - t * a.k;
        const int other = cells[j];
        land[t][j] = (signed char)(loc_y[t] >= 0 && cell_valid(other, a.L, a.W) ? tap_landing_on(other, loc_y[t], loc_x[t], a.W, a.dilation) : -1);
    }
    __syncthreads();
    if (tid < kTaps) { // the owner is the lowest row with a tap on the location (pair_owns of vfa_cellconv.h)
        bool own = loc_y[tid] >= 0, more = false;
        for (int j = 0; j < mine; ++j) own = own && land[tid][j] < 0;
        for (int j = mine + 1; j < a.k; ++j) more = more || land[tid][j] >= 0;
        owned[tid] = own;
        later[tid] = own && more;
    }
    __syncthreads();

    const long long K = (long long)a.C * kTaps;
    const size_t plane = (size_t)a.L * a.W;
    for (int c = tid; c < a.C; c += kThreads) {
        float acc[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) acc[t] = 0.0f;
        const float *g = d_logits + row * a.O;
        const float *w = weight + (long long)c * kTaps;
#pragma unroll 8
        for (int o = 0; o < a.O; ++o) { // my own pairs: ascending o, nine contiguous weights (unrolled: 72 loads in flight)
            const float go = g[o];
#pragma unroll
            for (int t = 0; t < kTaps; ++t) acc[t] = fmaf(go, w[o * K + t], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            if (!owned[t]) continue; // (uniform)
            if (later[t])
                for (int j = mine + 1; j < a.k; ++j) { // the later rows' pairs, ascending
                    const int t2 = land[t][j];
                    if (t2 < 0) continue;
                    const float *g2 = d_logits + (frame * a.k + j) * a.O;
                    for (int o = 0; o < a.O; ++o) acc[t] = fmaf(g2[o], w[o * K + t2], acc[t]);
                }
            d_feat[((size_t)frame * a.C + c) * plane + (size_t)loc_y[t] * a.W + loc_x[t]] = acc[t];
        }
    }
}

// 0: run; 1: nothing to do; otherwise the error
int check(const float *feat, const long long *stride, const float *weight, const int *cell, int B, int C, int L, int W, int O, int k,
          int dilation, Cells &a)
{
    if (B < 0 || C < 1 || L < 0 || W < 0 || O < 1 || k < 0 || dilation < 1) return VFA_ERR_BAD_ARGUMENT;
    if ((long long)B * k == 0) return 1;
    if (!feat || !stride || !weight || !cell) return VFA_ERR_BAD_ARGUMENT;
    if (stride[0] < 0 || stride[1] < 0 || stride[2] < 0 || stride[3] < 0) return VFA_ERR_BAD_ARGUMENT;
    if (C % kChunkC != 0 || (long long)L * W > INT32_MAX || (long long)B * k > INT32_MAX - kRows || O > 65535 * kGradO ||
        ((uintptr_t)weight & 15) != 0)
        return VFA_ERR_UNSUPPORTED;
    a.feat = feat;
    a.s_frame = stride[0];
    a.s_chan = stride[1];
    a.s_row = stride[2];
    a.s_col = stride[3];
    a.cell = cell;
    a.M = (long long)B * k;
    a.C = C;
    a.L = L;
    a.W = W;
    a.O = O;
    a.k = k;
    a.dilation = dilation;
    return 0;
}

} // namespace

extern "C" {

size_t vfa_conv3x3_at_cells_workspace_bytes(int B, int k, int O)
{
    if (B <= 0 || k <= 0 || O <= 0) return 0;
    return (size_t)B * (size_t)k * (size_t)O * sizeof(float);
}

int vfa_conv3x3_at_cells_f32(const float *feat, const long long *feat_stride, const float *weight, const int *cell, int B, int C, int L,
                             int W, int O, int k, int dilation, float *logits, float *rotation, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    Cells a = {};
    const int status = check(feat, feat_stride, weight, cell, B, C, L, W, O, k, dilation, a);
    if (status != 0) return status == 1 ? 0 : status;
    if (!logits && !rotation) return VFA_ERR_BAD_ARGUMENT;
    if (!logits) { // the rotation alone: the logits are staged in the caller's workspace
        if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < vfa_conv3x3_at_cells_workspace_bytes(B, k, O))
            return VFA_ERR_BAD_ARGUMENT;
        logits = (float *)workspace;
    }
    const unsigned row_tiles = (unsigned)((a.M + kRows - 1) / kRows);
    hipLaunchKernelGGL(cellconv_forward_kernel, dim3(row_tiles, (O + kOutTile - 1) / kOutTile), dim3(kThreads), 0, (hipStream_t)stream, a,
                       weight, logits);
    if (rotation)
        hipLaunchKernelGGL(cellconv_rotation_kernel, dim3((unsigned)((a.M + 3) / 4)), dim3(kThreads), 0, (hipStream_t)stream, cell, logits,
                           rotation, a.M, L, W, O);
    return (int)hipGetLastError();
}

int vfa_conv3x3_at_cells_backward_f32(const float *d_logits, const float *feat, const long long *feat_stride, const float *weight,
                                      const int *cell, int B, int C, int L, int W, int O, int k, int dilation, float *d_feat,
                                      float *d_weight, void *stream)
{
    Cells a = {};
    if (B < 0 || C < 1 || L < 0 || W < 0 || O < 1 || k < 0 || dilation < 1 || (!d_feat && !d_weight)) return VFA_ERR_BAD_ARGUMENT;
    const size_t feat_bytes = (size_t)B * C * L * W * sizeof(float), weight_bytes = (size_t)O * C * kTaps * sizeof(float);
    if ((long long)B * k == 0) { // no row: both gradients are zeros, and both are still written
        if (d_feat && feat_bytes) { const hipError_t e = hipMemsetAsync(d_feat, 0, feat_bytes, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
        if (d_weight) { const hipError_t e = hipMemsetAsync(d_weight, 0, weight_bytes, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    const int status = check(feat, feat_stride, weight, cell, B, C, L, W, O, k, dilation, a);
    if (status != 0) return status;
    if (!d_logits) return VFA_ERR_BAD_ARGUMENT;
    if (d_feat && k > kMaxRows) return VFA_ERR_UNSUPPORTED;
    if (d_weight)
        hipLaunchKernelGGL(cellconv_grad_weight_kernel, dim3(C / kChunkC, (O + kGradO - 1) / kGradO), dim3(kThreads), 0, (hipStream_t)stream,
                           a, d_logits, d_weight);
    if (d_feat) {
        const hipError_t e = hipMemsetAsync(d_feat, 0, feat_bytes, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(cellconv_grad_feat_kernel, dim3((unsigned)a.M), dim3(kThreads), 0, (hipStream_t)stream, a, d_logits, weight,
                           d_feat);
    }
    return (int)hipGetLastError();
}

} // extern "C"
