// vfa_trunk_grad.hip -- training the identity residual blocks of the ResNet trunk (reference resnet.py:26-57): the backward of a
// GroupNorm whose normalised map was never written, with the mask of the ReLU behind it folded in.  (The convolutions' gradients are
// vfa_trunk_conv_f32 on the output gradient with the transposed planes, and vfa_trunk_conv_wgrad_f32 of vfa_conv_grad.hip.)
//
// Forward: z = gamma (y - mean) rstd + beta per (image, group), the statistics over the group's channels and the plane; the consumer
// applied a ReLU whose mask is m, and u is the gradient behind that ReLU.  With N = (C / groups) L W values in a group,
//
//     S1[b, c] = sum m u                     S2[b, c] = sum m u y                                            (over the plane)
//     A[b, g]  = sum_c gamma_c S1[b, c]      K[b, g]  = rstd sum_c gamma_c (S2[b, c] - mean S1[b, c])        (over the group's channels)
//     dy = p (m u) + q y + r        p[b, c] = gamma_c rstd      q[b, g] = -rstd^2 K / N      r[b, g] = -rstd A / N - q mean
//     dgamma[c] = sum_b rstd (S2[b, c] - mean S1[b, c])         dbeta[c] = sum_b S1[b, c]
//
// float32 maps, contiguous (B, C, L, W); every sum in float64 in an order that depends on the shape alone, no atomics: the same bits
// on every run, and an image gives the same dy and dz bits alone and in a batch.
//
//   1. gnb_partial_kernel: per (image, channel) 32 parts of the plane (the cut of gn_partial_kernel: part k owns the positions
//      [P k / 32, P (k + 1) / 32), an empty part is a zero); a part's S1 | S2 from 256 threads' float64 sums in a fixed tree.  The
//      product of two float32 values is exact in float64.
//   2. gnb_coef_kernel: one thread per (image, channel): the parts in ascending order, the group's channels in ascending order, p, q, r
//      rounded to float32 once; the threads of image 0 also dgamma and dbeta over the images in ascending order, rounded once.
//   3. gnb_apply_kernel: dy = fmaf(p, m ? u : 0, fmaf(q, y, r)), and with the mask of a given map, dz = m ? u : 0.
// The mask: VFA_GN_MASK_PROLOGUE m = fmaf(a, y, b) > 0, the ReLU the next convolution applied as it read y (vfa_dense.h: prologue);
// VFA_GN_MASK_OUT m = out > 0 for a given map, the ReLU of the join.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kParts = 32;       // parts of a plane
constexpr int kPerThread = 4;    // positions of a thread of the elementwise kernel

template <bool OUT> __device__ __forceinline__ bool mask_of(float a, float y, float b, float out)
{
    return OUT ? out > 0.0f : fmaf(a, y, b) > 0.0f;
}

// grid (kParts, C, B)
template <bool OUT>
__global__ __launch_bounds__(kThreads) void gnb_partial_kernel(const float *__restrict__ y, const float *__restrict__ u, const float *__restrict__ pa,
                                                               const float *__restrict__ pb, const float *__restrict__ out, int C, int plane,
                                                               double *__restrict__ partial)
{
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x, part = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const size_t bc = (size_t)b * C + c, base = bc * plane;
    const int begin = (int)((long long)plane * part / kParts), end = (int)((long long)plane * (part + 1) / kParts);
    const float a = OUT ? 0.0f : pa[bc], bb = OUT ? 0.0f : pb[bc];
    double s1 = 0.0, s2 = 0.0;
    for (int i = begin + tid; i < end; i += kThreads) {
        const float yv = y[base + i], uv = u[base + i];
        if (mask_of<OUT>(a, yv, bb, OUT ? out[base + i] : 0.0f)) {
            s1 += (double)uv;
            s2 += (double)uv * (double)yv;
        }
    }
    red[0][tid] = s1;
    red[1][tid] = s2;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) { // a fixed tree
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double *dst = partial + (bc * kParts + part) * 2;
        dst[0] = red[0][0];
        dst[1] = red[1][0];
    }
}

// S1 | S2 of (image, channel) bc: the parts in ascending order
__device__ __forceinline__ void sums_of(const double *__restrict__ partial, size_t bc, double &s1, double &s2)
{
    const double *src = partial + bc * kParts * 2;
    s1 = 0.0;
    s2 = 0.0;
    for (int k = 0; k < kParts; ++k) {
        s1 += src[2 * k];
        s2 += src[2 * k + 1];
    }
}

// one thread per (image, channel); coef: p | q | r, (B, C) floats each
__global__ __launch_bounds__(kThreads) void gnb_coef_kernel(const double *__restrict__ partial, const float *__restrict__ gamma,
                                                            const double *__restrict__ stats, int B, int C, int groups, double count,
                                                            float *__restrict__ coef, float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C, cg = C / groups, g = c / cg;
    const double mean = stats[((size_t)b * groups + g) * 2], rstd = stats[((size_t)b * groups + g) * 2 + 1];
    double A = 0.0, K = 0.0;
    for (int k = g * cg; k < (g + 1) * cg; ++k) { // the group's channels in ascending order
        double s1, s2;
        sums_of(partial, (size_t)b * C + k, s1, s2);
        const double ga = gamma ? (double)gamma[k] : 1.0;
        A += ga * s1;
        K += ga * (s2 - mean * s1);
    }
    K *= rstd;
    const double q = -(rstd * rstd) * K / count, r = -(rstd * A) / count - q * mean;
    const size_t n = (size_t)B * C;
    coef[i] = (float)((gamma ? (double)gamma[c] : 1.0) * rstd);
    coef[n + i] = (float)q;
    coef[2 * n + i] = (float)r;
    if (b == 0 && (dgamma || dbeta)) { // the images in ascending order
        double dg = 0.0, db = 0.0;
        for (int k = 0; k < B; ++k) {
            double s1, s2;
            sums_of(partial, (size_t)k * C + c, s1, s2);
            const double mk = stats[((size_t)k * groups + g) * 2], rk = stats[((size_t)k * groups + g) * 2 + 1];
            dg += rk * (s2 - mk * s1);
            db += s1;
        }
        if (dgamma) dgamma[c] = (float)dg;
        if (dbeta) dbeta[c] = (float)db;
    }
}

// grid (blocks of 1024 positions of a plane, (image, channel) pairs in a grid-stride loop)
template <bool OUT>
__global__ __launch_bounds__(kThreads) void gnb_apply_kernel(const float *__restrict__ y, const float *__restrict__ u, const float *__restrict__ pa,
                                                             const float *__restrict__ pb, const float *__restrict__ out,
                                                             const float *__restrict__ coef, int BC, int plane, float *__restrict__ dy,
                                                             float *__restrict__ dz)
{
    for (int bc = blockIdx.y; bc < BC; bc += gridDim.y) {
        const float p = coef[bc], q = coef[(size_t)BC + bc], r = coef[2 * (size_t)BC + bc];
        const float a = OUT ? 0.0f : pa[bc], bb = OUT ? 0.0f : pb[bc];
        const size_t base = (size_t)bc * plane;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
            if (i >= plane) break;
            const float yv = y[base + i], uv = u[base + i];
            const float mu = mask_of<OUT>(a, yv, bb, OUT ? out[base + i] : 0.0f) ? uv : 0.0f;
            dy[base + i] = fmaf(p, mu, fmaf(q, yv, r)); // (a NaN stays a NaN)
            if (OUT) dz[base + i] = mu;
        }
    }
}

size_t partial_bytes(int B, int C) { return (size_t)B * (size_t)C * kParts * 2 * sizeof(double); }

template <bool OUT>
void launch(const float *y, const float *u, const float *a, const float *b, const float *out, const float *gamma, const double *stats, int B, int C,
            int L, int W, int groups, float *dy, float *dz, float *dgamma, float *dbeta, void *workspace, hipStream_t s)
{
    const int plane = L * W, BC = B * C, per_block = kThreads * kPerThread;
    double *partial = (double *)workspace;
    float *coef = (float *)((unsigned char *)workspace + partial_bytes(B, C));
    hipLaunchKernelGGL(gnb_partial_kernel<OUT>, dim3(kParts, (unsigned)C, (unsigned)B), dim3(kThreads), 0, s, y, u, a, b, out, C, plane, partial);
    hipLaunchKernelGGL(gnb_coef_kernel, dim3((unsigned)((BC + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const double *)partial, gamma, stats, B,
                       C, groups, (double)(C / groups) * (double)L * (double)W, coef, dgamma, dbeta);
    const dim3 grid((unsigned)((plane + per_block - 1) / per_block), (unsigned)(BC < 65535 ? BC : 65535));
    hipLaunchKernelGGL(gnb_apply_kernel<OUT>, grid, dim3(kThreads), 0, s, y, u, a, b, out, (const float *)coef, BC, plane, dy, dz);
}

} // namespace

extern "C" {

size_t vfa_group_norm_backward_workspace_bytes(int B, int C)
{
    if (B <= 0 || C <= 0) return 0;
    return partial_bytes(B, C) + ((size_t)3 * B * C * sizeof(float) + 255) / 256 * 256;
}

int vfa_group_norm_backward_f32(const float *y, const float *u, const float *a, const float *b, const float *out, const float *gamma,
                                const double *stats, int mask, int B, int C, int L, int W, int groups, float *dy, float *dz, float *dgamma,
                                float *dbeta, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || C < 1 || L < 0 || W < 0 || groups < 1 || C % groups != 0 || (mask != VFA_GN_MASK_PROLOGUE && mask != VFA_GN_MASK_OUT))
        return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || (long long)L * W == 0) { // an empty sum; no element of dy or dz
        hipError_t e = dgamma ? hipMemsetAsync(dgamma, 0, (size_t)C * sizeof(float), s) : hipSuccess;
        if (e == hipSuccess && dbeta) e = hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), s);
        return (int)e;
    }
    if (!y || !u || !stats || !dy || ((uintptr_t)stats & 7) != 0) return VFA_ERR_BAD_ARGUMENT;
    if (mask == VFA_GN_MASK_OUT ? (!out || !dz) : (!a || !b)) return VFA_ERR_BAD_ARGUMENT;
    if (!workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < vfa_group_norm_backward_workspace_bytes(B, C)) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || C > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2 || (long long)B * C > INT32_MAX / 4) return VFA_ERR_UNSUPPORTED;
    if (mask == VFA_GN_MASK_OUT) launch<true>(y, u, a, b, out, gamma, stats, B, C, L, W, groups, dy, dz, dgamma, dbeta, workspace, s);
    else launch<false>(y, u, a, b, out, gamma, stats, B, C, L, W, groups, dy, dz, dgamma, dbeta, workspace, s);
    return (int)hipGetLastError();
}

} // extern "C"
