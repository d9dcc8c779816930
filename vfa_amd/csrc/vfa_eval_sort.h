// vfa_eval_sort.h -- the vertex-ordering rule of the AP/AOS metric's rotated-box IoU as device code, shared by the two kernels that
// need it: vfa_sort_vertices_f32 (vfa_eval.hip, the drop-in for the reference's CUDA op) and the fused box-pair IoU of vfa_iou.hip.
// One statement of the comparison and of the selection loop (sort_vert_kernel.cu:15-40, :68-121); the callers differ only in where
// the candidate vertices live (global memory there, LDS here), which they hand in as two small functors.
#ifndef VFA_EVAL_SORT_H
#define VFA_EVAL_SORT_H
#include <hip/hip_runtime.h>

namespace vfa_eval {

constexpr int kMaxVertIdx = 9;         // MAX_NUM_VERT_IDX   sort_vert_kernel.cu:6
constexpr int kIntersectionOffset = 8; // INTERSECTION_OFFSET :7
constexpr double kEps = 1e-8;          // EPSILON            :8 (a double literal in the reference)

// "vertex 1 comes before vertex 2", vertices normalised around (0, 0): smallest on the positive x axis, growing anticlockwise
// (sort_vert_kernel.cu:15-40; the reference falls off the end -- undefined -- when a y is exactly 0: false here).
// Kept out of line: inlined twice into the selection loop, hipcc 7.2 at -O1 and above folds the second call to "false"
// (every pick after the first stayed 0 on gfx950; -O0 and the out-of-line call agree with the CPU restatement).
__device__ __noinline__ static bool before(float x1, float y1, float x2, float y2)
{
    if ((double)fabsf(x1 - x2) < kEps && (double)fabsf(y2 - y1) < kEps) return false;
    if (y1 > 0 && y2 < 0) return true;
    if (y1 < 0 && y2 > 0) return false;
    const float n1 = (float)((double)(x1 * x1 + y1 * y1) + kEps);
    const float n2 = (float)((double)(x2 * x2 + y2 * y2) + kEps);
    const float d = fabsf(x1) * x1 / n1 - fabsf(x2) * x2 / n2;
    if (y1 > 0 && y2 > 0) return (double)d > kEps;
    if (y1 < 0 && y2 < 0) return (double)d < kEps;
    return false;
}

// order[0 .. 8] of one polygon: the nv valid ones of its m candidate vertices anticlockwise, the first index repeated, then `pad`
// (an invalid intersection index).  vertex(k, x, y) loads candidate k (normalised around the polygon's centre), valid(k) its mask.
// The pick loop is written with a constant trip count and an early exit so that every order[] index is a constant once it is
// unrolled: the array stays in registers (a runtime-indexed per-lane array goes to scratch on this target).
template <class Vertex, class Valid>
__device__ __forceinline__ void order_polygon(Vertex vertex, Valid valid, int nv, int m, int pad, int (&order)[kMaxVertIdx])
{
#pragma unroll
    for (int j = 0; j < kMaxVertIdx; ++j) order[j] = pad;
    if (nv < 3) return; // not enough vertices
    // selection sort: the j-th vertex is the smallest one that is larger than the (j - 1)-th          (:68-93)
    float px = 0.0f, py = 0.0f; // previous pick
#pragma unroll
    for (int j = 0; j < kMaxVertIdx - 1; ++j) {
        if (j >= nv) break;
        float x_min = 1.0f, y_min = (float)-kEps;
        int take = 0;
#pragma unroll 1
        for (int k = 0; k < m; ++k) {
            float x, y;
            vertex(k, x, y);
            if (valid(k) && before(x, y, x_min, y_min) && (j == 0 || before(px, py, x, y))) {
                x_min = x; y_min = y; take = k;
            }
        }
        order[j] = take;
        vertex(take, px, py);
    }
    const int nvc = nv < kMaxVertIdx - 1 ? nv : kMaxVertIdx - 1;
#pragma unroll
    for (int j = 0; j < kMaxVertIdx; ++j)
        if (j == nvc) order[j] = order[0]; // duplicate the first index                                (:96)
    // two identical boxes: the four corners of box 1 equal those of box 2                              (:107-121)
    if (nv == 8) {
        int counter = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 4; k < kIntersectionOffset; ++k)
                if (order[k] == order[j]) ++counter;
        if (counter == 4) {
            order[4] = order[0];
#pragma unroll
            for (int j = 5; j < kMaxVertIdx; ++j) order[j] = pad;
        }
    }
}

} // namespace vfa_eval
#endif // VFA_EVAL_SORT_H
