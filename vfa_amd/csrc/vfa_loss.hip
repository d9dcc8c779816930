// vfa_loss.hip -- the two steps between the heads and backward of a training step, without a host wait: the encode half of the
// reference's ObjectEncoder (vfa/data/encoder.py:152-217) in the sparse form VFANet.heads(rotation_at=cells) defines, and the
// detection loss (vfa/model/loss.py) with its backward.  The rules and the per-element arithmetic: vfa_loss.h.
//
//   vfa_det_targets_f32           det_targets_kernel, ONE WORKGROUP PER FRAME: cells of the objects into LDS, duplicates resolved and the
//                                 live objects ranked by counting (no sort library), rows written at their rank, padding behind them.
//   vfa_det_loss_f32              det_loss_dense_kernel: the heat-map focal loss, 1024 cells per workgroup -> one partial per workgroup
//                                 in the workspace; det_loss_frame_kernel, one workgroup per frame: adds the frame's partials, the
//                                 three sparse terms over the positive-cell list, the weighted sum.
//   vfa_det_loss_backward_f32     det_loss_dense_backward_kernel (d heatmap, every cell) and det_loss_rows_backward_kernel (one
//                                 workgroup per listed row: its d rotation_at row, its entries of d loc_offset / d dim_offset, which a
//                                 memset zeroed).  Nothing accumulates across threads.
// Sums: the float32 elements are added in float64 (what is left of the error is the elements' own): wave shuffle -> LDS ->
// per-workgroup partial -> the frame kernel, every step in a fixed order that depends on (L, W, k, R) only, never on B: a frame of
// a batch has the bits of its single-frame call.  No float atomics, no waiting between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"
#include "vfa_loss.h"

namespace {

using namespace vfa_loss;

constexpr int kEncThreads = 256;
constexpr int kDenseThreads = 256, kCellsPerThread = 4, kCellsPerGroup = kDenseThreads * kCellsPerThread;
constexpr int kFrameThreads = 1024;
constexpr int kRowThreads = 256;

struct Map3 { long long frame, row, col; };        // heat maps
struct Map4 { long long frame, row, col, chan; };  // heads (B, L, W, C) through their strides
struct Rows { long long frame, row, chan; };       // rotation_at (B, k, R)

struct Partial { double pos, neg; int n_pos, n_neg; };

// sum over the workgroup, the result on thread 0: shuffle inside the wave, the waves' sums through LDS in wave order
template <typename T, int kThreads> __device__ T group_sum(T v, T *lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // (the previous sum's readers are done with lds)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    T s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) s += lds[w];
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- encoder
struct TargetArgs {
    const float *location, *dimension, *rotation;
    const int *count;
    int loc_width, K, L, W, kind;
    float world0, world1, mean0, mean1, mean2;
    int *cells, *n_pos, *angle_label;
    float *loc_offset, *dim_offset;
};

__global__ __launch_bounds__(kEncThreads) void det_targets_kernel(const TargetArgs a)
{
    __shared__ int cell[kMaxObjects], key[kMaxObjects];
    __shared__ float off[kMaxObjects][2];
    __shared__ int n_live;

    const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
    int n = a.count[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    if (tid == 0) n_live = 0;
    for (int i = tid; i < n; i += kEncThreads) {
        const float *loc = a.location + ((size_t)b * K + i) * a.loc_width;
        const Assigned as = assign_cell(loc[0], loc[1], a.world0, a.world1, a.L, a.W, a.kind);
        cell[i] = as.cell;
        off[i][0] = as.off_x;
        off[i][1] = as.off_y;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kEncThreads) {
        const int c = live_key(cell, n, i);
        key[i] = c;
        if (c >= 0) atomicAdd(&n_live, 1);  // (an integer counter in LDS)
    }
    __syncthreads();
    const int live = n_live;
    if (tid == 0) a.n_pos[b] = live;
    const bool three_d = a.dimension != nullptr;
    for (int i = tid; i < n; i += kEncThreads) {
        if (key[i] < 0) continue;
        const size_t row = (size_t)b * K + rank_of(key, n, i);  // (rank < live <= K)
        a.cells[row] = key[i];
        a.loc_offset[2 * row] = off[i][0];
        a.loc_offset[2 * row + 1] = off[i][1];
        if (three_d) {
            const float *dim = a.dimension + ((size_t)b * K + i) * 3;
            a.dim_offset[3 * row] = logf(dim[0] / a.mean0);
            a.dim_offset[3 * row + 1] = logf(dim[1] / a.mean1);
            a.dim_offset[3 * row + 2] = logf(dim[2] / a.mean2);
            a.angle_label[row] = angle_label(a.rotation[(size_t)b * K + i]);
        }
    }
    for (int r = live + tid; r < K; r += kEncThreads) {  // the padding: rows no object writes
        const size_t row = (size_t)b * K + r;
        a.cells[row] = -1;
        a.loc_offset[2 * row] = a.loc_offset[2 * row + 1] = 0.0f;
        if (three_d) {
            a.dim_offset[3 * row] = a.dim_offset[3 * row + 1] = a.dim_offset[3 * row + 2] = 0.0f;
            a.angle_label[row] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- loss
struct LossArgs {
    const float *heat, *gt, *loc, *dim, *rot;
    Map3 heat_s, gt_s;
    Map4 loc_s, dim_s;
    Rows rot_s;
    const int *cells, *n_pos, *label;
    const float *loc_t, *dim_t, *table;
    int L, W, k, R, n_groups;
    float w_hm, w_pos, w_dim, w_ang;
    Partial *partial;  // (B, n_groups)
    // forward outputs
    float *terms, *loss;
    int *counts;  // (B, 4): heat-map positives, negatives, angle positives, negatives
    // backward
    const float *coef;
    const int *counts_in;
    float *d_heat, *d_loc, *d_dim, *d_rot;
};

__global__ __launch_bounds__(kDenseThreads) void det_loss_dense_kernel(const LossArgs a)
{
    __shared__ double fsum[kDenseThreads / 64];
    __shared__ int isum[kDenseThreads / 64];
    const int b = blockIdx.y, tid = threadIdx.x, n_cells = a.L * a.W;
    double pos = 0.0, neg = 0.0;
    int n_pos = 0, n_neg = 0;
    for (int j = 0; j < kCellsPerThread; ++j) {
        const int i = blockIdx.x * kCellsPerGroup + j * kDenseThreads + tid;
        if (i >= n_cells) break;
        const int l = i / a.W, w = i - l * a.W;
        const float x = a.heat[b * a.heat_s.frame + l * a.heat_s.row + w * a.heat_s.col];
        const float gt = a.gt[b * a.gt_s.frame + l * a.gt_s.row + w * a.gt_s.col];
        const float p = clamp_prob(sigmoid(x));
        if (gt == 1.0f) {
            pos += (double)focal_pos(p);
            n_pos += 1;
        } else {
            neg += (double)focal_neg(p, gt);
            n_neg += 1;
        }
    }
    Partial part;
    part.pos = group_sum<double, kDenseThreads>(pos, fsum);
    part.neg = group_sum<double, kDenseThreads>(neg, fsum);
    part.n_pos = group_sum<int, kDenseThreads>(n_pos, isum);
    part.n_neg = group_sum<int, kDenseThreads>(n_neg, isum);
    if (tid == 0) a.partial[(size_t)b * a.n_groups + blockIdx.x] = part;
}

// the listed row r of frame b is read: behind the frame's count, or a cell outside the map, it is not
__device__ __forceinline__ int live_rows(const LossArgs &a, int b)
{
    const int n = a.n_pos[b];
    return n < 0 ? 0 : (n > a.k ? a.k : n);
}

__global__ __launch_bounds__(kFrameThreads) void det_loss_frame_kernel(const LossArgs a)
{
    __shared__ double fsum[kFrameThreads / 64];
    __shared__ int isum[kFrameThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, n_cells = a.L * a.W, k = a.k, R = a.R;

    // ---- heat map: the frame's partials, each thread its own in index order
    double pos = 0.0, neg = 0.0;
    int n_pos = 0, n_neg = 0;
    for (int g = tid; g < a.n_groups; g += kFrameThreads) {
        const Partial part = a.partial[(size_t)b * a.n_groups + g];
        pos += part.pos;
        neg += part.neg;
        n_pos += part.n_pos;
        n_neg += part.n_neg;
    }
    pos = group_sum<double, kFrameThreads>(pos, fsum);
    neg = group_sum<double, kFrameThreads>(neg, fsum);
    n_pos = group_sum<int, kFrameThreads>(n_pos, isum);
    n_neg = group_sum<int, kFrameThreads>(n_neg, isum);
    const float heat_term = focal_mean((float)pos, (float)neg, n_pos, n_neg);

    // ---- the sparse terms
    const int n = live_rows(a, b);
    const float per = (float)(n > 1 ? n : 1);  // max(n_pos, 1), loss.py:58-62
    const int *cells = a.cells + (size_t)b * k;
    double loc = 0.0, dim = 0.0, apos = 0.0, aneg = 0.0;
    int an_pos = 0, an_neg = 0;
    for (int e = tid; e < 2 * n; e += kFrameThreads) {
        const int r = e >> 1, c = e & 1, cell = cells[r];
        if (cell < 0 || cell >= n_cells) continue;
        const int l = cell / a.W, w = cell - l * a.W;
        const float x = a.loc[b * a.loc_s.frame + l * a.loc_s.row + w * a.loc_s.col + c * a.loc_s.chan];
        loc += (double)(smooth_l1(sigmoid(x) - a.loc_t[((size_t)b * k + r) * 2 + c]) / per);
    }
    if (a.dim != nullptr) {
        for (int e = tid; e < 3 * n; e += kFrameThreads) {
            const int r = e / 3, c = e - 3 * r, cell = cells[r];
            if (cell < 0 || cell >= n_cells) continue;
            const int l = cell / a.W, w = cell - l * a.W;
            const float x = a.dim[b * a.dim_s.frame + l * a.dim_s.row + w * a.dim_s.col + c * a.dim_s.chan];
            dim += (double)(smooth_l1(x - a.dim_t[((size_t)b * k + r) * 3 + c]) / per);
        }
        for (int e = tid; e < n * R; e += kFrameThreads) {
            const int r = e / R, j = e - r * R, cell = cells[r];
            if (cell < 0 || cell >= n_cells) continue;
            const float gt = a.table[table_index(j, label_shift(a.label[(size_t)b * k + r], R), R)];
            const float p = clamp_prob(sigmoid(a.rot[b * a.rot_s.frame + r * a.rot_s.row + j * a.rot_s.chan]));
            if (gt == 1.0f) {
                apos += (double)focal_pos(p);
                an_pos += 1;
            } else {
                aneg += (double)focal_neg(p, gt);
                an_neg += 1;
            }
        }
    }
    loc = group_sum<double, kFrameThreads>(loc, fsum);
    dim = group_sum<double, kFrameThreads>(dim, fsum);
    apos = group_sum<double, kFrameThreads>(apos, fsum);
    aneg = group_sum<double, kFrameThreads>(aneg, fsum);
    an_pos = group_sum<int, kFrameThreads>(an_pos, isum);
    an_neg = group_sum<int, kFrameThreads>(an_neg, isum);
    if (tid == 0) {
        const float ang = focal_mean((float)apos, (float)aneg, an_pos, an_neg), loc_term = (float)loc, dim_term = (float)dim;
        a.terms[4 * b] = heat_term;
        a.terms[4 * b + 1] = loc_term;
        a.terms[4 * b + 2] = dim_term;
        a.terms[4 * b + 3] = ang;
        a.loss[b] = loc_term * a.w_pos + dim_term * a.w_dim + heat_term * a.w_hm + ang * a.w_ang;  // (the order of loss.py:66-67)
        a.counts[4 * b] = n_pos;
        a.counts[4 * b + 1] = n_neg;
        a.counts[4 * b + 2] = an_pos;
        a.counts[4 * b + 3] = an_neg;
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(kDenseThreads) void det_loss_dense_backward_kernel(const LossArgs a)
{
    const int b = blockIdx.y, n_cells = a.L * a.W;
    const int i = blockIdx.x * kDenseThreads + threadIdx.x;
    if (i >= n_cells) return;
    const int n_pos = a.counts_in[4 * b], n_neg = a.counts_in[4 * b + 1];
    const float coef = a.coef[4 * b];
    const int l = i / a.W, w = i - l * a.W;
    const float x = a.heat[b * a.heat_s.frame + l * a.heat_s.row + w * a.heat_s.col];
    const float gt = a.gt[b * a.gt_s.frame + l * a.gt_s.row + w * a.gt_s.col];
    const float s = sigmoid(x), p = clamp_prob(s), slope = prob_slope(s);
    float g = 0.0f;
    if (slope != 0.0f) {  // (a NaN is not 0: it goes through)
        if (gt == 1.0f) g = coef / (float)n_pos * focal_pos_slope(p) * slope;  // (this cell is one: n_pos > 0)
        else g = coef / (float)n_neg * focal_neg_slope(p, gt) * slope;
    }
    a.d_heat[(size_t)b * n_cells + i] = g;
}

__global__ __launch_bounds__(kRowThreads) void det_loss_rows_backward_kernel(const LossArgs a)
{
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, n_cells = a.L * a.W, k = a.k, R = a.R;
    const int n = live_rows(a, b);
    const int cell = a.cells[(size_t)b * k + r];
    const bool live = r < n && cell >= 0 && cell < n_cells;
    if (a.d_rot != nullptr) {
        float *d_row = a.d_rot + ((size_t)b * k + r) * R;
        if (!live) {
            for (int j = tid; j < R; j += kRowThreads) d_row[j] = 0.0f;
        } else {
            const int an_pos = a.counts_in[4 * b + 2], an_neg = a.counts_in[4 * b + 3];
            const float coef = a.coef[4 * b + 3];
            const int shift = label_shift(a.label[(size_t)b * k + r], R);
            for (int j = tid; j < R; j += kRowThreads) {
                const float gt = a.table[table_index(j, shift, R)];
                const float s = sigmoid(a.rot[b * a.rot_s.frame + r * a.rot_s.row + j * a.rot_s.chan]);
                const float p = clamp_prob(s), slope = prob_slope(s);
                float g = 0.0f;
                if (slope != 0.0f) {
                    if (gt == 1.0f) g = coef / (float)an_pos * focal_pos_slope(p) * slope;
                    else g = coef / (float)an_neg * focal_neg_slope(p, gt) * slope;
                }
                d_row[j] = g;
            }
        }
    }
    if (!live || tid >= 5) return;
    const float per = (float)(n > 1 ? n : 1);
    const int l = cell / a.W, w = cell - l * a.W;
    if (tid < 2) {
        const float s = sigmoid(a.loc[b * a.loc_s.frame + l * a.loc_s.row + w * a.loc_s.col + tid * a.loc_s.chan]);
        const float d = s - a.loc_t[((size_t)b * k + r) * 2 + tid];
        a.d_loc[((size_t)b * n_cells + cell) * 2 + tid] = a.coef[4 * b + 1] / per * smooth_l1_slope(d) * (s * (1.0f - s));
    } else if (a.d_dim != nullptr) {
        const int c = tid - 2;
        const float x = a.dim[b * a.dim_s.frame + l * a.dim_s.row + w * a.dim_s.col + c * a.dim_s.chan];
        const float d = x - a.dim_t[((size_t)b * k + r) * 3 + c];
        a.d_dim[((size_t)b * n_cells + cell) * 3 + c] = a.coef[4 * b + 2] / per * smooth_l1_slope(d);
    }
}

bool any_negative(const long long *s, int n)
{
    for (int i = 0; i < n; ++i)
        if (s[i] < 0) return true;
    return false;
}

// what the forward and the backward check alike; 0: go on, 1: nothing to do
int check_loss_shapes(const float *heatmap, const long long *heat_stride, const float *gt_heatmap, const long long *gt_stride,
                      const float *loc, const long long *loc_stride, const float *dim, const long long *dim_stride, const float *rot,
                      const long long *rot_stride, const int *cells, const int *n_pos, const float *loc_target, const float *dim_target,
                      const int *angle_label, const float *table, int B, int L, int W, int k, int R, bool *three_d, bool *empty)
{
    *three_d = dim != nullptr || rot != nullptr;
    *empty = false;
    if (B < 0 || L < 0 || W < 0 || k < 0 || R < 0) return VFA_ERR_BAD_ARGUMENT;
    if (k > kMaxObjects || R > kMaxRot || (*three_d && (R & 1))) return VFA_ERR_UNSUPPORTED;
    if (B == 0 || L == 0 || W == 0) {
        *empty = true;
        return 0;
    }
    if (B > 65535 || (long long)L * W > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    if (!heatmap || !heat_stride || !gt_heatmap || !gt_stride || !loc || !loc_stride || !n_pos) return VFA_ERR_BAD_ARGUMENT;
    if (k > 0 && (!cells || !loc_target)) return VFA_ERR_BAD_ARGUMENT;
    if (any_negative(heat_stride, 3) || any_negative(gt_stride, 3) || any_negative(loc_stride, 4)) return VFA_ERR_BAD_ARGUMENT;
    if (*three_d) {
        if (!dim || !dim_stride || !rot_stride || R < 2 || (k > 0 && (!rot || !dim_target || !angle_label || !table)))
            return VFA_ERR_BAD_ARGUMENT;
        if (any_negative(dim_stride, 4) || any_negative(rot_stride, 3)) return VFA_ERR_BAD_ARGUMENT;
    }
    return 0;
}

LossArgs loss_args(const float *heatmap, const long long *heat_stride, const float *gt_heatmap, const long long *gt_stride,
                   const float *loc, const long long *loc_stride, const float *dim, const long long *dim_stride, const float *rot,
                   const long long *rot_stride, const int *cells, const int *n_pos, const float *loc_target, const float *dim_target,
                   const int *angle_label, const float *table, int L, int W, int k, int R, bool three_d)
{
    LossArgs a = {};
    a.heat = heatmap;
    a.gt = gt_heatmap;
    a.loc = loc;
    a.heat_s = {heat_stride[0], heat_stride[1], heat_stride[2]};
    a.gt_s = {gt_stride[0], gt_stride[1], gt_stride[2]};
    a.loc_s = {loc_stride[0], loc_stride[1], loc_stride[2], loc_stride[3]};
    if (three_d) {
        a.dim = dim;
        a.rot = rot;
        a.dim_s = {dim_stride[0], dim_stride[1], dim_stride[2], dim_stride[3]};
        a.rot_s = {rot_stride[0], rot_stride[1], rot_stride[2]};
        a.label = angle_label;
        a.dim_t = dim_target;
        a.table = table;
    }
    a.cells = cells;
    a.n_pos = n_pos;
    a.loc_t = loc_target;
    a.L = L;
    a.W = W;
    a.k = k;
    a.R = three_d ? R : 0;
    a.n_groups = (int)(((long long)L * W + kCellsPerGroup - 1) / kCellsPerGroup);
    return a;
}

}  // namespace

extern "C" {

int vfa_det_targets_f32(const float *location, int loc_width, const int *count, const float *dimension, const float *rotation,
                        const float *dimension_mean, int B, int K, int L, int W, float world0, float world1, int kind, int *cells,
                        int *n_pos, float *loc_offset, float *dim_offset, int *angle_label, void *stream)
{
    if (B < 0 || K < 0 || L < 0 || W < 0 || (loc_width != 2 && loc_width != 3) || kind < 0 || kind > 2) return VFA_ERR_BAD_ARGUMENT;
    if (!(world0 > 0.0f) || !(world1 > 0.0f)) return VFA_ERR_BAD_ARGUMENT;
    if (K > kMaxObjects) return VFA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (B > 65535 || (long long)L * W > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const bool three_d = dimension != nullptr || rotation != nullptr;
    if (!count || !n_pos || (K > 0 && (!location || !cells || !loc_offset))) return VFA_ERR_BAD_ARGUMENT;
    if (three_d && (!dimension || !rotation || !dimension_mean || (K > 0 && (!dim_offset || !angle_label)))) return VFA_ERR_BAD_ARGUMENT;

    TargetArgs a = {};
    a.location = location;
    a.dimension = dimension;
    a.rotation = rotation;
    a.count = count;
    a.loc_width = loc_width;
    a.K = K;
    a.L = L;
    a.W = W;
    a.kind = kind;
    a.world0 = world0;
    a.world1 = world1;
    if (three_d) {
        a.mean0 = dimension_mean[0];
        a.mean1 = dimension_mean[1];
        a.mean2 = dimension_mean[2];
    }
    a.cells = cells;
    a.n_pos = n_pos;
    a.angle_label = angle_label;
    a.loc_offset = loc_offset;
    a.dim_offset = dim_offset;
    hipLaunchKernelGGL(det_targets_kernel, dim3(B), dim3(kEncThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

size_t vfa_det_loss_workspace_bytes(int B, int L, int W)
{
    if (B <= 0 || L <= 0 || W <= 0) return 0;
    return (size_t)B * (size_t)(((long long)L * W + kCellsPerGroup - 1) / kCellsPerGroup) * sizeof(Partial);
}

int vfa_det_loss_f32(const float *heatmap, const long long *heat_stride, const float *gt_heatmap, const long long *gt_stride,
                     const float *loc_offset, const long long *loc_stride, const float *dim_offset, const long long *dim_stride,
                     const float *rotation_at, const long long *rot_stride, const int *cells, const int *n_pos, const float *loc_target,
                     const float *dim_target, const int *angle_label, const float *table, const float *loss_weight, int B, int L, int W,
                     int k, int R, void *workspace, size_t workspace_bytes, float *terms, float *loss, int *counts, void *stream)
{
    bool three_d, empty;
    const int status = check_loss_shapes(heatmap, heat_stride, gt_heatmap, gt_stride, loc_offset, loc_stride, dim_offset, dim_stride,
                                         rotation_at, rot_stride, cells, n_pos, loc_target, dim_target, angle_label, table, B, L, W, k, R,
                                         &three_d, &empty);
    if (status != 0 || empty) return status;
    if (!loss_weight || !terms || !loss || !counts) return VFA_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < vfa_det_loss_workspace_bytes(B, L, W)) return VFA_ERR_BAD_ARGUMENT;

    LossArgs a = loss_args(heatmap, heat_stride, gt_heatmap, gt_stride, loc_offset, loc_stride, dim_offset, dim_stride, rotation_at,
                           rot_stride, cells, n_pos, loc_target, dim_target, angle_label, table, L, W, k, R, three_d);
    a.w_hm = loss_weight[0];
    a.w_pos = loss_weight[1];
    a.w_dim = loss_weight[2];
    a.w_ang = loss_weight[3];
    a.partial = (Partial *)workspace;
    a.terms = terms;
    a.loss = loss;
    a.counts = counts;
    hipLaunchKernelGGL(det_loss_dense_kernel, dim3(a.n_groups, B), dim3(kDenseThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(det_loss_frame_kernel, dim3(B), dim3(kFrameThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int vfa_det_loss_backward_f32(const float *coef, const float *heatmap, const long long *heat_stride, const float *gt_heatmap,
                              const long long *gt_stride, const float *loc_offset, const long long *loc_stride, const float *dim_offset,
                              const long long *dim_stride, const float *rotation_at, const long long *rot_stride, const int *cells,
                              const int *n_pos, const float *loc_target, const float *dim_target, const int *angle_label,
                              const float *table, const int *counts, int B, int L, int W, int k, int R, float *d_heatmap,
                              float *d_loc_offset, float *d_dim_offset, float *d_rotation_at, void *stream)
{
    bool three_d, empty;
    const int status = check_loss_shapes(heatmap, heat_stride, gt_heatmap, gt_stride, loc_offset, loc_stride, dim_offset, dim_stride,
                                         rotation_at, rot_stride, cells, n_pos, loc_target, dim_target, angle_label, table, B, L, W, k, R,
                                         &three_d, &empty);
    if (status != 0 || empty) return status;
    if (!coef || !counts || !d_heatmap || !d_loc_offset) return VFA_ERR_BAD_ARGUMENT;
    if (three_d && (!d_dim_offset || (k > 0 && !d_rotation_at))) return VFA_ERR_BAD_ARGUMENT;

    LossArgs a = loss_args(heatmap, heat_stride, gt_heatmap, gt_stride, loc_offset, loc_stride, dim_offset, dim_stride, rotation_at,
                           rot_stride, cells, n_pos, loc_target, dim_target, angle_label, table, L, W, k, R, three_d);
    a.coef = coef;
    a.counts_in = counts;
    a.d_heat = d_heatmap;
    a.d_loc = d_loc_offset;
    a.d_dim = three_d ? d_dim_offset : nullptr;
    a.d_rot = three_d ? d_rotation_at : nullptr;
    const size_t n_cells = (size_t)L * W;
    hipError_t err = hipMemsetAsync(d_loc_offset, 0, (size_t)B * n_cells * 2 * sizeof(float), (hipStream_t)stream);
    if (err == hipSuccess && three_d) err = hipMemsetAsync(d_dim_offset, 0, (size_t)B * n_cells * 3 * sizeof(float), (hipStream_t)stream);
    if (err != hipSuccess) return (int)err;
    const int groups = (int)((n_cells + kDenseThreads - 1) / kDenseThreads);
    hipLaunchKernelGGL(det_loss_dense_backward_kernel, dim3(groups, B), dim3(kDenseThreads), 0, (hipStream_t)stream, a);
    if (k > 0) hipLaunchKernelGGL(det_loss_rows_backward_kernel, dim3(k, B), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
