// vfa_decode.hip -- the decode half of the reference's ObjectEncoder (vfa/data/encoder.py:230-305) for a batch of frames in one
// stream-ordered call with outputs of a fixed shape: peaks, the top-k of every frame in a deterministic order, the box arithmetic
// and the rotation arg-max at the selected cells only.
//
//   1. vfa_bev_nms_batch_f32 (vfa_eval.hip) writes conf (B, L, W) into the caller's workspace: the confidences ARE that kernel's.
//   2. bev_decode_kernel, ONE WORKGROUP OF 16 WAVES PER FRAME:
//      - select: the k-th largest key of the frame's candidates (conf > thresh) by a radix select, one 8-bit digit per pass over the
//        map (which stays in L2), 256 bins in LDS; the logic, the key and the bounds of every loop: vfa_decode.h;
//      - collect: the candidates with key >= threshold, at most k, into LDS (slots from an LDS counter: any order), padded with zero
//        keys to a power of two and ordered by a bitonic network.  Keys are unique, so the order does not depend on the slots;
//      - decode: the waves take the selected cells in turn; lane 0 does the box arithmetic, the 64 lanes reduce the cell's rotation
//        logits by (sigmoid value, lowest index): vfa_rotation.h.  Rows from the frame's count on are written as zeros, cell -1.
// fp32, one operation per reference operation, no contraction (-ffp-contract=off); expf is the device's.  No atomics on memory:
// every call gives the same bits.  A NaN logit is no candidate (the NMS writes 0 for it) and never wins the arg-max.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_decode.h"
#include "vfa_hip.h"
#include "vfa_rotation.h"

namespace {

using namespace vfa_decode;
using vfa_rotation::sigmoid;

constexpr int kThreads = 1024, kWaves = kThreads / 64;

struct Strides { long long frame, row, col, chan; };

struct DecodeArgs {
    const float *conf_map;                   // (B, L, W), the NMS output
    const float *loc, *dim, *rot;            // heads, strided; dim == rot == nullptr: 2D
    Strides loc_s, dim_s, rot_s;
    int L, W, n_rot, k;
    float thresh, grid0, grid1, world0, world1, mean0, mean1, mean2;
    int yx_first;
    int *count, *cell;
    float *conf, *location, *dimension, *rotation;
};

__global__ __launch_bounds__(kThreads) void bev_decode_kernel(const DecodeArgs a)
{
    __shared__ unsigned hist[kBins];
    __shared__ uint64_t keys[kMaxTopk];
    __shared__ Select sel;
    __shared__ unsigned n_taken;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cells = a.L * a.W, k = a.k;
    const float *conf_map = a.conf_map + (size_t)b * n_cells;

    // ---- select
    if (tid == 0) { sel = select_begin(k, n_cells); n_taken = 0; }
    __syncthreads();
    Select s = sel;
    for (int pass = 0; pass < kPasses; ++pass) {
        if (!pass_counts(pass, n_cells)) continue; // (uniform)
        if (tid < kBins) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n_cells; i += kThreads) {
            const float c = conf_map[i];
            if (!(c > a.thresh)) continue;
            const uint64_t key = pack_key(__float_as_uint(c), (uint32_t)i);
            if (select_matches(s, key)) atomicAdd(&hist[key_digit(key, pass)], 1u);
        }
        __syncthreads();
        if (tid == 0) { select_advance(s, hist, pass); sel = s; }
        __syncthreads();
        s = sel;
        if (s.done) break; // (uniform: every thread reads the same LDS word)
    }

    // ---- collect and order
    for (int i = tid; i < n_cells; i += kThreads) {
        const float c = conf_map[i];
        if (!(c > a.thresh)) continue;
        const uint64_t key = pack_key(__float_as_uint(c), (uint32_t)i);
        if (!select_takes(s, key)) continue;
        const unsigned slot = atomicAdd(&n_taken, 1u);
        if (slot < (unsigned)k) keys[slot] = key;
    }
    __syncthreads();
    const int n = (int)min(n_taken, (unsigned)k);
    const int padded = pow2_at_least(n);
    if (tid >= n && tid < padded) keys[tid] = 0;
    __syncthreads();
    for (int size = 2; size <= padded; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < (padded >> 1)) bitonic_exchange(keys, tid, size, stride);
            __syncthreads();
        }

    // ---- decode
    if (tid == 0) a.count[b] = n;
    const bool three_d = a.rot != nullptr;
    for (int r = wave; r < k; r += kWaves) { // (uniform per wave)
        const size_t row = (size_t)b * k + r;
        const uint64_t key = r < n ? keys[r] : 0;
        const uint32_t cell = key_cell(key);
        if (r >= n || cell >= (uint32_t)n_cells) {
            if (lane == 0) {
                a.conf[row] = 0.0f;
                a.cell[row] = -1;
                a.location[3 * row] = a.location[3 * row + 1] = a.location[3 * row + 2] = 0.0f;
                if (three_d) {
                    a.dimension[3 * row] = a.dimension[3 * row + 1] = a.dimension[3 * row + 2] = 0.0f;
                    a.rotation[row] = 0.0f;
                }
            }
            continue;
        }
        const int l = (int)(cell / (uint32_t)a.W), w = (int)(cell - (uint32_t)l * (uint32_t)a.W);
        if (lane == 0) {
            const float *t = a.loc + b * a.loc_s.frame + l * a.loc_s.row + w * a.loc_s.col;
            const float cy = ((float)l + sigmoid(t[0])) / a.grid0 * a.world0;
            const float cx = ((float)w + sigmoid(t[a.loc_s.chan])) / a.grid1 * a.world1;
            a.conf[row] = __uint_as_float(key_conf_bits(key));
            a.cell[row] = (int)cell;
            a.location[3 * row] = a.yx_first ? cy : cx;
            a.location[3 * row + 1] = a.yx_first ? cx : cy;
            a.location[3 * row + 2] = 0.0f;
            if (three_d) {
                const float *d = a.dim + b * a.dim_s.frame + l * a.dim_s.row + w * a.dim_s.col;
                a.dimension[3 * row] = expf(d[0]) * a.mean0;
                a.dimension[3 * row + 1] = expf(d[a.dim_s.chan]) * a.mean1;
                a.dimension[3 * row + 2] = expf(d[2 * a.dim_s.chan]) * a.mean2;
            }
        }
        if (three_d) {
            const float *o = a.rot + b * a.rot_s.frame + l * a.rot_s.row + w * a.rot_s.col;
            const float rotation = vfa_rotation::wave_rotation(o, a.rot_s.chan, a.n_rot, lane); // (the rule: vfa_rotation.h)
            if (lane == 0) a.rotation[row] = rotation;
        }
    }
}

} // namespace

extern "C" {

size_t vfa_bev_decode_workspace_bytes(int B, int L, int W, int topk)
{
    if (B <= 0 || L <= 0 || W <= 0 || topk <= 0) return 0;
    return (size_t)B * (size_t)L * (size_t)W * sizeof(float);
}

int vfa_bev_decode_f32(const float *heatmap, const float *loc_offset, const long long *loc_stride, const float *dim_offset,
                       const long long *dim_stride, const float *rotation, const long long *rot_stride, int B, int L, int W, int n_rot,
                       int topk, float cls_thresh, float grid0, float grid1, float world0, float world1, const float *dimension_mean,
                       int yx_first, void *workspace, size_t workspace_bytes, int *count, float *conf, float *location, int *cell,
                       float *dimension, float *rotation_out, void *stream)
{
    if (B < 0 || L < 0 || W < 0 || topk < 1 || n_rot < 0 || !(cls_thresh >= 0.0f)) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || L == 0 || W == 0) return 0;
    if (B > 65535 || topk > kMaxTopk || (long long)L * W > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const bool three_d = dim_offset != nullptr || rotation != nullptr;
    if (!heatmap || !loc_offset || !loc_stride || !count || !conf || !location || !cell) return VFA_ERR_BAD_ARGUMENT;
    if (three_d && (!dim_offset || !rotation || !dim_stride || !rot_stride || !dimension_mean || !dimension || !rotation_out ||
                    n_rot < 1))
        return VFA_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < vfa_bev_decode_workspace_bytes(B, L, W, topk)) return VFA_ERR_BAD_ARGUMENT;

    const int status = vfa_bev_nms_batch_f32(heatmap, (float *)workspace, B, L, W, stream);
    if (status != 0) return status;

    DecodeArgs a = {};
    a.conf_map = (const float *)workspace;
    a.loc = loc_offset;
    a.loc_s = {loc_stride[0], loc_stride[1], loc_stride[2], loc_stride[3]};
    if (three_d) {
        a.dim = dim_offset;
        a.rot = rotation;
        a.dim_s = {dim_stride[0], dim_stride[1], dim_stride[2], dim_stride[3]};
        a.rot_s = {rot_stride[0], rot_stride[1], rot_stride[2], rot_stride[3]};
        a.mean0 = dimension_mean[0];
        a.mean1 = dimension_mean[1];
        a.mean2 = dimension_mean[2];
    }
    a.L = L;
    a.W = W;
    a.n_rot = n_rot;
    a.k = (long long)L * W < topk ? L * W : topk;
    a.thresh = cls_thresh;
    a.grid0 = grid0;
    a.grid1 = grid1;
    a.world0 = world0;
    a.world1 = world1;
    a.yx_first = yx_first;
    a.count = count;
    a.cell = cell;
    a.conf = conf;
    a.location = location;
    a.dimension = dimension;
    a.rotation = rotation_out;
    hipLaunchKernelGGL(bev_decode_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // extern "C"
