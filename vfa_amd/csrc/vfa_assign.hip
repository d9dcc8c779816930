// vfa_assign.hip -- the match tables of the CLEAR-MOD metric (MODA / MODP, reference vfa/evaluation/pyeval/CLEAR_MOD_HUN.py:44-93)
// for a whole evaluation set in one launch: one wave per frame, grid = n_frames.  A workgroup loads its frame's coordinates into
// LDS, writes the distance matrix when asked to, solves the assignment (vfa_assign.h) and writes its frame's rows of the tables.
// Workgroups share nothing: no tickets, no atomics, no workspace; every run gives the same bits.  float64 throughout, like the
// reference's numpy.
#include <hip/hip_runtime.h>

#include "vfa_assign.h"
#include "vfa_hip.h"

static_assert(VFA_CLEAR_MOD_MAX_SIDE == vfa_assign::kMaxSide, "the cap of the header is the solver's");

namespace {

using namespace vfa_assign;

__global__ __launch_bounds__(kLanes) void clear_mod_frames_kernel(const double *__restrict__ det_xy, const int *__restrict__ det_begin,
                                                                  const double *__restrict__ gt_xy, const int *__restrict__ gt_begin,
                                                                  int n_det, int n_gt, double td, const long long *__restrict__ pair_begin,
                                                                  long long n_pairs, double *__restrict__ dist, int *__restrict__ gt_match,
                                                                  double *__restrict__ gt_dist, long long *__restrict__ frame_counts,
                                                                  double *__restrict__ frame_cost, int *__restrict__ frame_status)
{
    __shared__ State S;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int d0 = det_begin[f], d1 = det_begin[f + 1], g0 = gt_begin[f], g1 = gt_begin[f + 1];
    // offsets that do not describe rows of the arrays (not the caller's contract) are not followed
    if (d0 < 0 || d1 < d0 || d1 > n_det || g0 < 0 || g1 < g0 || g1 > n_gt) {
        if (lane == 0) frame_status[f] = VFA_CLEAR_MOD_BAD_OFFSETS;
        return;
    }
    const int P = d1 - d0, G = g1 - g0;
    if (P > kMaxSide || G > kMaxSide) {
        for (int o = lane; o < G; o += kLanes) { gt_match[g0 + o] = -1; gt_dist[g0 + o] = INFINITY; }
        if (lane == 0) frame_status[f] = VFA_CLEAR_MOD_TOO_LARGE;
        return;
    }
    for (int o = lane; o < G; o += kLanes) { S.gx[o] = gt_xy[2 * (size_t)(g0 + o)]; S.gy[o] = gt_xy[2 * (size_t)(g0 + o) + 1]; }
    for (int e = lane; e < P; e += kLanes) { S.ex[e] = det_xy[2 * (size_t)(d0 + e)]; S.ey[e] = det_xy[2 * (size_t)(d0 + e) + 1]; }
    __syncthreads();
    if (dist) { // the reference's dist[o, e] (CLEAR_MOD_HUN.py:58-63), before the threshold
        const long long q0 = pair_begin[f];
        if (q0 >= 0 && q0 + (long long)G * P <= n_pairs) {
            for (int q = lane; q < G * P; q += kLanes) {
                const int o = q / P, e = q - o * P;
                dist[q0 + q] = pair_distance(S.gx[o], S.gy[o], S.ex[e], S.ey[e]);
            }
        }
    }
    const FrameTotals t = solve_frame(S, G, P, td, gt_match + g0, gt_dist + g0);
    if (lane == 0) {
        frame_counts[4 * (size_t)f + 0] = G;
        frame_counts[4 * (size_t)f + 1] = P;
        frame_counts[4 * (size_t)f + 2] = t.matched;
        frame_counts[4 * (size_t)f + 3] = t.beyond;
        frame_cost[f] = t.cost;
        frame_status[f] = t.flags ? VFA_CLEAR_MOD_SOLVER_FLAG : 0;
    }
}

} // namespace

extern "C" {

int vfa_clear_mod_frames_f64(const double *det_xy, const int *det_begin, const double *gt_xy, const int *gt_begin, int n_frames, int n_det,
                             int n_gt, double td, const long long *pair_begin, long long n_pairs, double *dist, int *gt_match,
                             double *gt_dist, long long *frame_counts, double *frame_cost, int *frame_status, void *stream)
{
    if (n_frames < 0 || n_det < 0 || n_gt < 0 || n_pairs < 0) return VFA_ERR_BAD_ARGUMENT;
    if (n_frames == 0) return 0;
    if (!det_begin || !gt_begin || !frame_counts || !frame_cost || !frame_status) return VFA_ERR_BAD_ARGUMENT;
    if ((n_det > 0 && !det_xy) || (n_gt > 0 && (!gt_xy || !gt_match || !gt_dist))) return VFA_ERR_BAD_ARGUMENT;
    if (dist && !pair_begin) return VFA_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(clear_mod_frames_kernel, dim3((unsigned)n_frames), dim3(kLanes), 0, (hipStream_t)stream, det_xy, det_begin, gt_xy,
                       gt_begin, n_det, n_gt, td, pair_begin, n_pairs, dist, gt_match, gt_dist, frame_counts, frame_cost, frame_status);
    return (int)hipGetLastError();
}

} // extern "C"
