// vfa_iou.hip -- the rotated-box 3D IoU of the AP/AOS metric (vfa/evaluation/pyeval/IoU.py:6-225) and the per-detection best
// match of its evaluation loop (evaluateAPAOS.py:74-92) as HIP kernels for wave64.
//
// ONE LANE per box pair runs the whole of IoU3D: corners of both boxes, the 16 edge-edge intersections, the two corner-inside
// tests, the 24 candidate vertices with their masks, their mean, the anticlockwise ordering (vfa_eval_sort.h: the same device
// code as vfa_sort_vertices_f32), the shoelace over the un-normalised candidates, union, BEV IoU, z overlap (NOT clamped), 3D
// IoU.  Per pair, HBM sees 14 input floats and the results; the 24 candidates live in LDS as [candidate][lane] planes (the
// ordering loop and the shoelace read them by a runtime index; the plane layout makes a wave's access to one candidate 64
// consecutive words), their masks as one 24-bit word in a register.
//
// Arithmetic: fp32, one operation per reference operation in the reference's order; the file is compiled with
// -ffp-contract=off, so no multiply and add are merged.  The reference sums the 24 masked candidates and the 8 shoelace terms
// with torch.sum, whose order is not specified; here both sums run in index order.  cosf / sinf are the device's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_eval_sort.h"
#include "vfa_hip.h"

namespace {

using vfa_eval::kIntersectionOffset;
using vfa_eval::kMaxVertIdx;

constexpr int kBlock = 64;  // one wave per block: a set of 20 000 detections still spreads over every CU
constexpr int kCand = 24; // 4 + 4 corners, 16 edge-edge intersections   (IoU.py:133)

// the candidates of the block's lanes: plane k holds candidate k of every lane (12 KB per block of the CU's 160 KB)
struct Candidates {
    float x[kCand][kBlock];
    float y[kCand][kBlock];
};

// torch.min / torch.max propagate NaN
__device__ __forceinline__ float min_t(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float max_t(float a, float b) { return (a != a || a > b) ? a : b; }

// boxes2corners (IoU.py:6-35): (x, y, w, h, alpha) -> 4 corners, txty @ [[cos, sin], [-sin, cos]] + (x, y)
__device__ __forceinline__ void corners_of(float x, float y, float w, float h, float alpha, float (&cx)[4], float (&cy)[4])
{
    const float c = cosf(alpha), s = sinf(alpha), ns = -s;
    const float sx[4] = {0.5f, -0.5f, -0.5f, 0.5f}, sy[4] = {0.5f, 0.5f, -0.5f, -0.5f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float tx = sx[k] * w, ty = sy[k] * h;
        cx[k] = x + (tx * c + ty * ns);
        cy[k] = y + (tx * s + ty * c);
    }
}

// box1_in_box2 (IoU.py:89-117): which corners of `p` lie inside the rectangle `q` (projections on its edges ab and ad)
__device__ __forceinline__ unsigned inside_mask(const float (&px)[4], const float (&py)[4], const float (&qx)[4], const float (&qy)[4])
{
    const float abx = qx[1] - qx[0], aby = qy[1] - qy[0], adx = qx[3] - qx[0], ady = qy[3] - qy[0];
    const float norm_ab = abx * abx + aby * aby, norm_ad = adx * adx + ady * ady;
    const float lo = (float)-1e-6, hi = (float)(1. + 1e-6); // the reference compares fp32 tensors with these Python floats
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float amx = px[k] - qx[0], amy = py[k] - qy[0];
        const float r_ab = (amx * abx + amy * aby) / norm_ab, r_ad = (amx * adx + amy * ady) / norm_ad;
        if (r_ab > lo && r_ab < hi && r_ad > lo && r_ad < hi) bits |= 1u << k;
    }
    return bits;
}

// IoU3D of one pair (IoU.py:206-225) with IoUs2D (:178-204) inside; b1, b2 -> x y z l w h alpha.  Every lane of the block may
// call it (also repeatedly): a lane touches only its own column of `cand`.
__device__ void pair_iou(const float *__restrict__ b1, const float *__restrict__ b2, Candidates &cand, int lane, float &iou_bev,
                         float &iou_3d)
{
    const float x1 = b1[0], y1 = b1[1], z1 = b1[2], l1 = b1[3], w1 = b1[4], h1 = b1[5], a1 = b1[6];
    const float x2 = b2[0], y2 = b2[1], z2 = b2[2], l2 = b2[3], w2 = b2[4], h2 = b2[5], a2 = b2[6];
    float c1x[4], c1y[4], c2x[4], c2y[4];
    corners_of(x1, y1, l1, w1, a1, c1x, c1y);
    corners_of(x2, y2, l2, w2, a2, c2x, c2y);

    unsigned mask = inside_mask(c1x, c1y, c2x, c2y) | (inside_mask(c2x, c2y, c1x, c1y) << 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cand.x[k][lane] = c1x[k];
        cand.y[k][lane] = c1y[k];
        cand.x[4 + k][lane] = c2x[k];
        cand.y[4 + k][lane] = c2y[k];
    }
    // boxes_intersection (IoU.py:38-86): edge i of box 1 against edge j of box 2, candidate 8 + 4 i + j
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float ax = c1x[i], ay = c1y[i], bx = c1x[(i + 1) & 3], by = c1y[(i + 1) & 3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float cx = c2x[j], cy = c2y[j], dx = c2x[(j + 1) & 3], dy = c2y[(j + 1) & 3];
            const float den = (ax - bx) * (cy - dy) - (ay - by) * (cx - dx);
            const float mol_t = (ax - cx) * (cy - dy) - (ay - cy) * (cx - dx);
            const float mol_u = (bx - ax) * (ay - cy) - (by - ay) * (ax - cx);
            const float t = mol_t / den, u = mol_u / den;
            const bool hit = t > 0.f && t < 1.f && u > 0.f && u < 1.f; // open intervals; a zero denominator gives inf / NaN: no hit
            const float t2 = mol_t / (den + (float)1e-8);
            const float keep = hit ? 1.0f : 0.0f; // multiplied like the reference's mask.float(): a NaN stays a NaN
            const int k = kIntersectionOffset + 4 * i + j;
            cand.x[k][lane] = (ax + t2 * (bx - ax)) * keep;
            cand.y[k][lane] = (ay + t2 * (by - ay)) * keep;
            if (hit) mask |= 1u << k;
        }
    }
    // sort_vertices (IoU.py:139-155): centre of the valid candidates, then the ordering of the kernel
    const int nv = __popc(mask);
    float sum_x = 0.0f, sum_y = 0.0f;
#pragma unroll 1
    for (int k = 0; k < kCand; ++k) {
        const float keep = (mask >> k & 1u) ? 1.0f : 0.0f;
        sum_x += cand.x[k][lane] * keep;
        sum_y += cand.y[k][lane] * keep;
    }
    const float mean_x = sum_x / (float)nv, mean_y = sum_y / (float)nv; // (0 / 0 = NaN with no valid candidate: never read then)
    int pad = kCand - 1; // an invalid intersection: zeroed above, its shoelace terms vanish
#pragma unroll 1
    for (int k = kIntersectionOffset; k < kCand; ++k)
        if (!(mask >> k & 1u)) { pad = k; break; }
    int order[kMaxVertIdx];
    vfa_eval::order_polygon([&](int k, float &x, float &y) { x = cand.x[k][lane] - mean_x; y = cand.y[k][lane] - mean_y; },
                            [&](int k) { return (mask >> k & 1u) != 0; }, nv, kCand, pad, order);
    // calculate_area (IoU.py:158-175): open shoelace over the 9 indices on the UN-normalised candidates
    float total = 0.0f;
    float qx = cand.x[order[0]][lane], qy = cand.y[order[0]][lane];
#pragma unroll
    for (int k = 1; k < kMaxVertIdx; ++k) {
        const float rx = cand.x[order[k]][lane], ry = cand.y[order[k]][lane];
        total += qx * ry - qy * rx;
        qx = rx; qy = ry;
    }
    const float overlap = fabsf(total) / 2;
    // IoUs2D tail (:200-203), IoU3D (:215-225)
    const float uni = l1 * w1 + l2 * w2 - overlap;
    iou_bev = overlap / uni;
    const float zmax1 = z1 + 0.5f * h1, zmin1 = z1 - 0.5f * h1, zmax2 = z2 + 0.5f * h2, zmin2 = z2 - 0.5f * h2;
    const float z_overlap = min_t(zmax1, zmax2) - max_t(zmin1, zmin2); // not clamped: negative for boxes apart in z
    const float inter = iou_bev * uni * z_overlap;
    const float u3d = l1 * w1 * h1 + l2 * w2 * h2 - inter;
    iou_3d = inter / u3d;
}

__global__ __launch_bounds__(kBlock) void iou3d_pairs_kernel(const float *__restrict__ box1, const float *__restrict__ box2,
                                                             float *__restrict__ iou3d, float *__restrict__ iou_bev, long long count)
{
    __shared__ Candidates cand;
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    float bev, vol;
    pair_iou(box1 + i * 7, box2 + i * 7, cand, threadIdx.x, bev, vol);
    iou3d[i] = vol;
    if (iou_bev) iou_bev[i] = bev;
}

// the frame whose range of `begin` (n + 1 non-decreasing offsets) holds `q`: the last f with begin[f] <= q
template <class T>
__device__ __forceinline__ int frame_of(const T *__restrict__ begin, int n, long long q)
{
    int lo = 0, hi = n; // begin[lo] <= q < begin[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)begin[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// one lane per (detection, ground truth) pair of a frame; the packed matrices of the frames follow one another in `iou`
__global__ __launch_bounds__(kBlock) void iou3d_frames_kernel(const float *__restrict__ det, const int *__restrict__ det_begin,
                                                              const float *__restrict__ gt, const int *__restrict__ gt_begin, int n_frames,
                                                              int n_det, int n_gt, const long long *__restrict__ pair_begin,
                                                              long long n_pairs, float *__restrict__ iou)
{
    __shared__ Candidates cand;
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n_pairs || q < pair_begin[0] || q >= pair_begin[n_frames]) return;
    const int f = frame_of(pair_begin, n_frames, q);
    const int d0 = det_begin[f], d1 = det_begin[f + 1], g0 = gt_begin[f], g1 = gt_begin[f + 1];
    const long long local = q - pair_begin[f];
    // offsets that do not describe this matrix (not the caller's contract) write nothing rather than read out of bounds
    if (d0 < 0 || d1 > n_det || g0 < 0 || g1 > n_gt || g1 <= g0 || d1 <= d0 || local >= (long long)(d1 - d0) * (g1 - g0)) return;
    const int i = (int)(local / (g1 - g0)), j = (int)(local % (g1 - g0));
    float bev, vol;
    pair_iou(det + (size_t)(d0 + i) * 7, gt + (size_t)(g0 + j) * 7, cand, threadIdx.x, bev, vol);
    iou[q] = vol;
}

// kSlots lanes per detection: lane s takes the ground truths s, s + kSlots, ... of the detection's frame, keeps the best of its own
// and the group then keeps the largest value, the LOWEST INDEX among equal ones -- what a scan in index order would keep, whatever
// the order of the combination; NaN never wins.  FROM_MATRIX reads the row the pair kernel wrote, otherwise the lanes compute the
// IoUs themselves (no matrix in memory): the same device function on the same operands, so both give the same bits.
constexpr int kSlots = 16;
template <bool FROM_MATRIX>
__global__ __launch_bounds__(kBlock) void best_match_kernel(const float *__restrict__ det, const int *__restrict__ det_begin,
                                                            const float *__restrict__ gt, const int *__restrict__ gt_begin, int n_frames,
                                                            int n_det, int n_gt, const long long *__restrict__ pair_begin,
                                                            long long n_pairs, const float *__restrict__ iou,
                                                            int *__restrict__ best_idx, float *__restrict__ best_iou)
{
    __shared__ Candidates cand;
    const long long p = (long long)blockIdx.x * (kBlock / kSlots) + threadIdx.x / kSlots; // (every lane stays for the shuffles)
    const int slot = threadIdx.x % kSlots;
    int best = -1;
    float value = -1.0f;
    if (p < n_det && p >= det_begin[0] && p < det_begin[n_frames]) {
        const int f = frame_of(det_begin, n_frames, p);
        const int d0 = det_begin[f], g0 = gt_begin[f], g1 = gt_begin[f + 1];
        if (g0 >= 0 && g1 <= n_gt) {
            for (int j = slot; j < g1 - g0; j += kSlots) {
                float v, bev;
                if (FROM_MATRIX) {
                    const long long q = pair_begin[f] + (p - d0) * (g1 - g0) + j;
                    if (q < 0 || q >= n_pairs) break; // (offsets that do not describe the matrix)
                    v = iou[q];
                } else pair_iou(det + (size_t)p * 7, gt + (size_t)(g0 + j) * 7, cand, threadIdx.x, bev, v);
                if (v == v && (best < 0 || v > value)) { best = j; value = v; }
            }
        }
    }
#pragma unroll
    for (int step = kSlots / 2; step > 0; step >>= 1) {
        const int other = __shfl_xor(best, step, kSlots);
        const float theirs = __shfl_xor(value, step, kSlots);
        if (other >= 0 && (best < 0 || theirs > value || (theirs == value && other < best))) { best = other; value = theirs; }
    }
    if (slot == 0 && p < n_det) {
        best_idx[p] = best;
        best_iou[p] = value;
    }
}

} // namespace

extern "C" {

int vfa_iou3d_f32(const float *box1, const float *box2, float *iou3d, float *iou_bev, long long count, void *stream)
{
    if (count < 0) return VFA_ERR_BAD_ARGUMENT;
    if (count == 0) return 0;
    if (!box1 || !box2 || !iou3d) return VFA_ERR_BAD_ARGUMENT;
    const long long blocks = (count + kBlock - 1) / kBlock;
    if (blocks >= (1ll << 31)) return VFA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(iou3d_pairs_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, box1, box2, iou3d, iou_bev, count);
    return (int)hipGetLastError();
}

int vfa_iou3d_frames_f32(const float *det, const int *det_begin, const float *gt, const int *gt_begin, int n_frames, int n_det, int n_gt,
                         const long long *pair_begin, long long n_pairs, float *iou, int *best_idx, float *best_iou, void *stream)
{
    if (n_frames < 0 || n_det < 0 || n_gt < 0 || n_pairs < 0) return VFA_ERR_BAD_ARGUMENT;
    if ((best_idx == nullptr) != (best_iou == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    if (n_frames == 0 || n_det == 0) return 0;
    if (!det || !det_begin || !gt_begin || (n_gt > 0 && !gt)) return VFA_ERR_BAD_ARGUMENT;
    if (iou && !pair_begin) return VFA_ERR_BAD_ARGUMENT;
    if (iou && n_pairs > 0) {
        const long long blocks = (n_pairs + kBlock - 1) / kBlock;
        if (blocks >= (1ll << 31)) return VFA_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(iou3d_frames_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, det, det_begin, gt, gt_begin,
                           n_frames, n_det, n_gt, pair_begin, n_pairs, iou);
    }
    if (best_idx) {
        const dim3 grid((unsigned)(((long long)n_det * kSlots + kBlock - 1) / kBlock));
        if (iou)
            hipLaunchKernelGGL(best_match_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, det, det_begin, gt, gt_begin, n_frames,
                               n_det, n_gt, pair_begin, n_pairs, iou, best_idx, best_iou);
        else
            hipLaunchKernelGGL(best_match_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, det, det_begin, gt, gt_begin, n_frames,
                               n_det, n_gt, pair_begin, n_pairs, iou, best_idx, best_iou);
    }
    return (int)hipGetLastError();
}

} // extern "C"
