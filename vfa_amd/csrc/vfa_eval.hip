// vfa_eval.hip -- the two consumer-side kernels behind the path:
//   * sort_vertices   the reference's only native code, a CUDA op of its AP/AOS metric (vfa/evaluation/pyeval/cuda_op/
//                     sort_vert_kernel.cu:42-134, called from IoU.py through cuda_ext.py and hard-wired to device('cuda') in
//                     evaluateAPAOS.py:79-83): orders the <= 8 valid vertices of a rectangle-rectangle intersection polygon
//                     anticlockwise for the shoelace area.  Rewritten for wave64: ONE LANE per polygon (the polygons are
//                     independent, 24 candidate vertices each, all state in registers), 256-thread blocks over b * n.
//   * bev_nms         sigmoid + 5 x 5 max-pool non-maximum suppression of the heat map (vfa/data/encoder.py:230-232, first
//                     lines of decode3d / decode2d :238, :278): conf = (maxpool5(s) == s) * s with s = sigmoid(heatmap).
// Both are index / comparison work; the arithmetic inside the comparisons keeps the reference's operand types (float
// products, double constants).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_eval_sort.h"
#include "vfa_hip.h"

namespace {

using vfa_eval::kIntersectionOffset;
using vfa_eval::kMaxVertIdx;

__global__ __launch_bounds__(256) void sort_vertices_kernel(const float *__restrict__ vertices, const uint8_t *__restrict__ mask,
                                                            const int *__restrict__ num_valid, int *__restrict__ idx, long long total,
                                                            int m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x; // polygon
    if (i >= total) return;
    const float *v = vertices + i * m * 2;
    const uint8_t *mk = mask + i * m;
    int *out = idx + i * kMaxVertIdx;
    const int nv = num_valid[i];
    int pad = m - 1; // an arbitrary INVALID intersection point (the reference leaves it uninitialised when there is none)
    for (int j = kIntersectionOffset; j < m; ++j)
        if (!mk[j]) { pad = j; break; }
    int order[kMaxVertIdx]; // the comparison and the selection loop: vfa_eval_sort.h, shared with the fused IoU kernel (vfa_iou.hip)
    vfa_eval::order_polygon([&](int k, float &x, float &y) { x = v[2 * k]; y = v[2 * k + 1]; }, [&](int k) { return mk[k] != 0; }, nv, m,
                            pad, order);
#pragma unroll
    for (int j = 0; j < kMaxVertIdx; ++j) out[j] = order[j];
}

// conf[l, w] = s if s == max over the 5 x 5 neighbourhood (padding 2, -inf outside) else 0, s = 1 / (1 + exp(-heatmap[l, w]))
// Batched (vfa_bev_nms_batch_f32): frame blockIdx.z, its own (L, W) map -- the window stops at the frame's edges like the padding of
// one map, so a peak of frame b + 1 never suppresses one of frame b
__global__ __launch_bounds__(256) void bev_nms_kernel(const float *__restrict__ heat, float *__restrict__ conf, int L, int W)
{
    heat += (size_t)blockIdx.z * L * W;
    conf += (size_t)blockIdx.z * L * W;
    const int w = blockIdx.x * 32 + (threadIdx.x & 31), l = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (l >= L || w >= W) return;
    auto sig = [](float x) { return 1.0f / (1.0f + expf(-x)); };
    const float s = sig(heat[(size_t)l * W + w]);
    float mx = s;
    for (int dl = -2; dl <= 2; ++dl)
        for (int dw = -2; dw <= 2; ++dw) {
            const int ll = l + dl, ww = w + dw;
            if (ll >= 0 && ll < L && ww >= 0 && ww < W) mx = fmaxf(mx, sig(heat[(size_t)ll * W + ww]));
        }
    conf[(size_t)l * W + w] = (mx == s) ? s : 0.0f;
}

} // namespace

extern "C" {

int vfa_sort_vertices_f32(const float *vertices, const uint8_t *mask, const int *num_valid, int *idx, int b, int n, int m, void *stream)
{
    if (b < 0 || n < 0 || m <= kIntersectionOffset) return VFA_ERR_BAD_ARGUMENT;
    const long long total = (long long)b * n;
    if (total == 0) return 0;
    if ((total + 255) / 256 >= (1ll << 31)) return VFA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(sort_vertices_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, mask,
                       num_valid, idx, total, m);
    return (int)hipGetLastError();
}

int vfa_bev_nms_f32(const float *heatmap, float *conf, int L, int W, void *stream)
{
    if (L < 0 || W < 0) return VFA_ERR_BAD_ARGUMENT;
    if (L == 0 || W == 0) return 0;
    hipLaunchKernelGGL(bev_nms_kernel, dim3((W + 31) / 32, (L + 7) / 8), dim3(256), 0, (hipStream_t)stream, heatmap, conf, L, W);
    return (int)hipGetLastError();
}

int vfa_bev_nms_batch_f32(const float *heatmap, float *conf, int B, int L, int W, void *stream)
{
    if (B < 0 || L < 0 || W < 0) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || L == 0 || W == 0) return 0;
    if (B > 65535) return VFA_ERR_UNSUPPORTED; // (grid z)
    hipLaunchKernelGGL(bev_nms_kernel, dim3((W + 31) / 32, (L + 7) / 8, B), dim3(256), 0, (hipStream_t)stream, heatmap, conf, L, W);
    return (int)hipGetLastError();
}

} // extern "C"
