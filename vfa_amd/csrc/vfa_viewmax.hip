// vfa_viewmax.hip -- hand-written HIP (gfx950 / CDNA4, wave64) kernels of the max-over-cameras BEV fusion, behind the C ABI of
// include/vfa_hip.h.
//
//   vfa_scale_view_max_f32           ortho = max over cameras of ((relu(lin8+b8) + relu(lin16+b16)) + relu(lin32+b32)), with the
//                                    winning camera per element (the reference's scale sum, vfa/model/vfanet.py:79, followed by
//                                    a maximum where :82 adds)
//   vfa_scale_view_max_backward_f32  its gradient: every element's gradient goes to the winning camera only, through that
//                                    camera's three ReLU masks; the other cameras get zeros
//
// Both kernels stream from memory: one thread owns 4 channels of one cell (16-byte loads), the forward keeps the loads of
// kMaxAhead cameras in flight, nothing goes through LDS.  There are no float atomics: the bias gradients are column sums in a
// fixed order (vfa_column_sum_f32), so the backward gives the same bits on every run.
//
// Compiled with -ffp-contract=off: an FMA appears only where fmaf() is written (none here).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "vfa_geom.h"

namespace {
using vfa_dev::relu_t;

constexpr int kMaxAhead = 4;       // cameras whose three lin rows a forward thread loads before it compares
constexpr int kMaxViews = 256;     // the winner index is one byte

// vfanet.py:79 for one element, in the reference's association order
__device__ __forceinline__ float scale_sum(float x8, float x16, float x32, float c8, float c16, float c32)
{
    float s = relu_t(x8 + c8) + relu_t(x16 + c16);
    return s + relu_t(x32 + c32);
}

// torch.max(dim=0)'s rule for a scan in camera order: the first NaN wins, otherwise a strictly larger value (ties keep the
// lower camera)
__device__ __forceinline__ void take_max(float t, int v, float &best, int &idx)
{
    const bool best_nan = best != best;
    if (!best_nan && (t > best || t != t)) {
        best = t;
        idx = v;
    }
}

template <int VEC>
__device__ __forceinline__ void load_vec(const float *__restrict__ p, float (&x)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *__restrict__ p, const float (&x)[VEC])
{
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else p[0] = x[0];
}

// grid-stride over groups of VEC elements of the (M, N) map; VEC = 4 needs 4 | N and 16-byte aligned rows (the host checks)
template <int VEC>
__global__ __launch_bounds__(256) void scale_view_max_kernel(const float *__restrict__ l8, const float *__restrict__ l16,
                                                             const float *__restrict__ l32, const float *__restrict__ b8,
                                                             const float *__restrict__ b16, const float *__restrict__ b32,
                                                             float *__restrict__ ortho, uint8_t *__restrict__ argmax, int n_views,
                                                             size_t MN, int N)
{
    const size_t stride = (size_t)gridDim.x * 256 * VEC;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC; i < MN; i += stride) {
        const int col = (int)(i % N);
        float c8[VEC], c16[VEC], c32[VEC], best[VEC];
        int idx[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            c8[k] = b8 ? b8[col + k] : 0.0f;
            c16[k] = b16 ? b16[col + k] : 0.0f;
            c32[k] = b32 ? b32[col + k] : 0.0f;
            best[k] = 0.0f; // n_views = 0: zeros, like the sum
            idx[k] = 0;
        }
        int v = 0;
        for (; v + kMaxAhead <= n_views; v += kMaxAhead) {
            float x8[kMaxAhead][VEC], x16[kMaxAhead][VEC], x32[kMaxAhead][VEC];
#pragma unroll
            for (int u = 0; u < kMaxAhead; ++u) { // every load of the group is issued before the first compare
                const size_t o = (size_t)(v + u) * MN + i;
                load_vec<VEC>(l8 + o, x8[u]);
                load_vec<VEC>(l16 + o, x16[u]);
                load_vec<VEC>(l32 + o, x32[u]);
            }
#pragma unroll
            for (int u = 0; u < kMaxAhead; ++u) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float t = scale_sum(x8[u][k], x16[u][k], x32[u][k], c8[k], c16[k], c32[k]);
                    if (v + u == 0) best[k] = t; // camera 0 is the first candidate, whatever its value (-0.0 and NaN included)
                    else take_max(t, v + u, best[k], idx[k]);
                }
            }
        }
        for (; v < n_views; ++v) {
            float x8[VEC], x16[VEC], x32[VEC];
            const size_t o = (size_t)v * MN + i;
            load_vec<VEC>(l8 + o, x8);
            load_vec<VEC>(l16 + o, x16);
            load_vec<VEC>(l32 + o, x32);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float t = scale_sum(x8[k], x16[k], x32[k], c8[k], c16[k], c32[k]);
                if (v == 0) best[k] = t;
                else take_max(t, v, best[k], idx[k]);
            }
        }
        store_vec<VEC>(ortho + i, best);
        if (argmax) {
            if constexpr (VEC == 4) {
                const uint32_t packed = (uint32_t)idx[0] | ((uint32_t)idx[1] << 8) | ((uint32_t)idx[2] << 16) | ((uint32_t)idx[3] << 24);
                *reinterpret_cast<uint32_t *>(argmax + i) = packed;
            } else {
                argmax[i] = (uint8_t)idx[0];
            }
        }
    }
}

// The winner's pre-activation of one scale at the VEC elements of group i, masked: out[k] = g[k] if lin[w[k]] + c[k] > 0 (strict),
// else 0.  A winner index outside [0, n_views) passes no gradient and reads nothing.
template <int VEC>
__device__ __forceinline__ void winner_masked(const float *__restrict__ lin, const float (&c)[VEC], const float (&g)[VEC],
                                              const int (&w)[VEC], bool same, int n_views, size_t MN, size_t i, float (&out)[VEC])
{
    if constexpr (VEC == 4) {
        if (same && w[0] < n_views) { // the common case: one camera wins all four channels -> one 16-byte load
            float x[4];
            load_vec<4>(lin + (size_t)w[0] * MN + i, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = (x[k] + c[k] > 0.0f) ? g[k] : 0.0f;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        out[k] = (w[k] < n_views && lin[(size_t)w[k] * MN + i + k] + c[k] > 0.0f) ? g[k] : 0.0f;
}

template <int VEC>
__global__ __launch_bounds__(256) void scale_view_max_backward_kernel(
    const float *__restrict__ grad, const float *__restrict__ l8, const float *__restrict__ l16, const float *__restrict__ l32,
    const float *__restrict__ b8, const float *__restrict__ b16, const float *__restrict__ b32, const uint8_t *__restrict__ argmax,
    float *__restrict__ g8, float *__restrict__ g16, float *__restrict__ g32, int n_views, size_t MN, int N)
{
    const size_t stride = (size_t)gridDim.x * 256 * VEC;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC; i < MN; i += stride) {
        const int col = (int)(i % N);
        float c8[VEC], c16[VEC], c32[VEC], g[VEC];
        int w[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            c8[k] = b8 ? b8[col + k] : 0.0f;
            c16[k] = b16 ? b16[col + k] : 0.0f;
            c32[k] = b32 ? b32[col + k] : 0.0f;
        }
        load_vec<VEC>(grad + i, g);
        if constexpr (VEC == 4) {
            const uint32_t packed = *reinterpret_cast<const uint32_t *>(argmax + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (int)((packed >> (8 * k)) & 0xffu);
        } else {
            w[0] = argmax[i];
        }
        bool same = true;
#pragma unroll
        for (int k = 1; k < VEC; ++k) same = same && w[k] == w[0];
        float o8[VEC], o16[VEC], o32[VEC];
        winner_masked<VEC>(l8, c8, g, w, same, n_views, MN, i, o8);
        winner_masked<VEC>(l16, c16, g, w, same, n_views, MN, i, o16);
        winner_masked<VEC>(l32, c32, g, w, same, n_views, MN, i, o32);
        // dense rows for every camera (the product backward takes them): the winner's masked gradient, zeros elsewhere
        for (int v = 0; v < n_views; ++v) {
            float y8[VEC], y16[VEC], y32[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const bool win = w[k] == v;
                y8[k] = win ? o8[k] : 0.0f;
                y16[k] = win ? o16[k] : 0.0f;
                y32[k] = win ? o32[k] : 0.0f;
            }
            const size_t o = (size_t)v * MN + i;
            store_vec<VEC>(g8 + o, y8);
            store_vec<VEC>(g16 + o, y16);
            store_vec<VEC>(g32 + o, y32);
        }
    }
}

inline int launch_status() { return (int)hipGetLastError(); }

inline unsigned elementwise_blocks(size_t n_items)
{
    const size_t want = (n_items + 255) / 256;
    const size_t cap = 256 * 8; // 256 CUs x 8 blocks, grid-stride beyond that
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

inline bool aligned16(const void *p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

} // namespace

extern "C" {

int vfa_scale_view_max_f32(const float *lin8, const float *lin16, const float *lin32, const float *bias8, const float *bias16,
                           const float *bias32, float *ortho, uint8_t *argmax, int n_views, size_t M, int N, void *stream)
{
    if (n_views < 0 || n_views > kMaxViews || N <= 0) return VFA_ERR_BAD_ARGUMENT;
    const size_t MN = M * (size_t)N;
    if (MN == 0) return 0;
    if (!ortho || (n_views > 0 && (!lin8 || !lin16 || !lin32))) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const bool vec4 = N % 4 == 0 && aligned16(lin8) && aligned16(lin16) && aligned16(lin32) && aligned16(ortho)
                      && ((uintptr_t)argmax & 3u) == 0;
    if (vec4)
        hipLaunchKernelGGL((scale_view_max_kernel<4>), dim3(elementwise_blocks(MN / 4)), dim3(256), 0, s, lin8, lin16, lin32, bias8,
                           bias16, bias32, ortho, argmax, n_views, MN, N);
    else
        hipLaunchKernelGGL((scale_view_max_kernel<1>), dim3(elementwise_blocks(MN)), dim3(256), 0, s, lin8, lin16, lin32, bias8,
                           bias16, bias32, ortho, argmax, n_views, MN, N);
    return launch_status();
}

int vfa_scale_view_max_backward_f32(const float *grad, const float *lin8, const float *lin16, const float *lin32, const float *bias8,
                                    const float *bias16, const float *bias32, const uint8_t *argmax, float *grad_lin8,
                                    float *grad_lin16, float *grad_lin32, float *grad_bias8, float *grad_bias16, float *grad_bias32,
                                    int n_views, size_t M, int N, void *stream)
{
    if (n_views < 0 || n_views > kMaxViews || N <= 0) return VFA_ERR_BAD_ARGUMENT;
    const size_t MN = M * (size_t)N;
    hipStream_t s = (hipStream_t)stream;
    if (MN > 0 && n_views > 0) {
        if (!grad || !lin8 || !lin16 || !lin32 || !argmax || !grad_lin8 || !grad_lin16 || !grad_lin32) return VFA_ERR_BAD_ARGUMENT;
        const bool vec4 = N % 4 == 0 && aligned16(grad) && aligned16(lin8) && aligned16(lin16) && aligned16(lin32)
                          && aligned16(grad_lin8) && aligned16(grad_lin16) && aligned16(grad_lin32) && ((uintptr_t)argmax & 3u) == 0;
        if (vec4)
            hipLaunchKernelGGL((scale_view_max_backward_kernel<4>), dim3(elementwise_blocks(MN / 4)), dim3(256), 0, s, grad, lin8,
                               lin16, lin32, bias8, bias16, bias32, argmax, grad_lin8, grad_lin16, grad_lin32, n_views, MN, N);
        else
            hipLaunchKernelGGL((scale_view_max_backward_kernel<1>), dim3(elementwise_blocks(MN)), dim3(256), 0, s, grad, lin8, lin16,
                               lin32, bias8, bias16, bias32, argmax, grad_lin8, grad_lin16, grad_lin32, n_views, MN, N);
        const int st = launch_status();
        if (st) return st;
    }
    // bias gradients: column sums of the dense rows in a fixed order (no atomics); rows = 0 writes zeros
    const long long rows = MN > 0 ? (long long)n_views * (long long)M : 0;
    const float *glin[3] = {grad_lin8, grad_lin16, grad_lin32};
    float *gbias[3] = {grad_bias8, grad_bias16, grad_bias32};
    for (int k = 0; k < 3; ++k) {
        if (!gbias[k]) continue;
        const int st = vfa_column_sum_f32(glin[k], gbias[k], rows, N, 0, stream);
        if (st) return st;
    }
    return 0;
}

} // extern "C"
