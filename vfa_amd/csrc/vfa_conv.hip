// vfa_conv.hip -- the dense 3x3 convolutions of the BEV heads (reference vfanet.py:131-149: fuse, map_classifier, tytx_pred,
// thtwtl_pred): stride 1, zero padding = dilation, dilation 1..4, float32 in and out, the input (B, C, L, W) read through its four
// element strides, the output contiguous (B, O, L, W).  Fixed summation order, no float atomics: the same bits on every run, and a
// frame gives the same bits alone and in a batch.
//
//   1. The dense kernel, its absmax pre-pass and its weight pack are vfa_dense.h's (the integer rules: vfa_conv.h).  The heads use
//      dense_kernel<9, 1, D, false, false, EpiAffine> for D = 1..4: nine taps, stride 1, the window grown by the dilation, one
//      accumulator chain for every C, no prologue, and the epilogue out = act(acc 2^-(ea + ew) * scale[o] + shift[o]) per output
//      channel.  The same kernel on the output gradient with the planes of the transposed, tap-mirrored weight gives the input
//      gradient (vfa_conv_grad.hip has the weight gradient, and takes its per-frame scales from frame_absmax here).
//   2. conv_few_kernel<O>: the layers with 1..4 outputs, plain fmaf: a workgroup takes 64 cells of a map row, its four waves a
//      quarter of the channels each (channel-ascending, tap-ascending chains), merged as (p0 + p1) + (p2 + p3).  Optional
//      prologue relu(a[b, c] x + b[b, c]) applied as a tap is read; a tap outside the map is a zero AFTER the prologue.
//   3. gn_partial_kernel / gn_affine_kernel: per (frame, group) sum and sum of squares in float64 (32 parts in a fixed tree, merged
//      in ascending order), then a = gamma rstd, b = beta - mean a per (frame, channel); where the caller keeps them for a backward
//      (vfa_group_norm_stats_f32), the mean and rstd of each (frame, group) as the float64 values a and b were made from.
//   4. bn_fold_kernel: scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale from the running statistics on the device.
#include "vfa_dense.h"

namespace {

constexpr int kGnParts = 32;  // partial sums per (frame, group)

template <int NO>
__global__ __launch_bounds__(kThreads) void conv_few_kernel(const Map m, const float *__restrict__ weight, const float *__restrict__ pa,
                                                            const float *__restrict__ pb, int d, float *__restrict__ out)
{
    __shared__ float part[4][NO][64];
    const int tid = threadIdx.x, cell = tid & 63, p = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = blockIdx.x * 64 + cell, y = blockIdx.y, b = blockIdx.z;
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0f;
    long long off[kTaps];
    bool ok[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const int ty = y + (t / 3 - 1) * d, tx = x + (t % 3 - 1) * d;
        ok[t] = x < m.W && ty >= 0 && ty < m.L && tx >= 0 && tx < m.W;
        off[t] = ok[t] ? b * m.s_frame + ty * m.s_row + tx * m.s_col : 0;
    }
    const int per = m.C / 4;
    for (int c = p * per; c < (p + 1) * per; ++c) { // ascending channels, ascending taps
        const float a = pa ? pa[(size_t)b * m.C + c] : 1.0f, bb = pa ? pb[(size_t)b * m.C + c] : 0.0f;
        const float *xc = m.x + (long long)c * m.s_chan;
        const float *wc = weight + (size_t)c * kTaps;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            float val = ok[t] ? xc[off[t]] : 0.0f;
            if (pa) {
                val = fmaf(a, val, bb);
                val = val < 0.0f ? 0.0f : val;
                val = ok[t] ? val : 0.0f; // the zero padding comes after the prologue
            }
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[o] = fmaf(val, wc[(size_t)o * m.C * kTaps + t], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) part[p][o][cell] = acc[o];
    __syncthreads();
    if (tid < 64 && x < m.W) {
#pragma unroll
        for (int o = 0; o < NO; ++o)
            out[(((size_t)b * NO + o) * m.L + y) * m.W + x] = (part[0][o][cell] + part[1][o][cell]) + (part[2][o][cell] + part[3][o][cell]);
    }
}

__global__ __launch_bounds__(kThreads) void gn_partial_kernel(const Map m, int groups, double *__restrict__ partial)
{
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x, p = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int cg = m.C / groups;
    const long long plane = (long long)m.L * m.W;
    const int begin = (int)(plane * p / kGnParts), end = (int)(plane * (p + 1) / kGnParts); // part p: a range of positions, every channel
    const float *group = m.x + b * m.s_frame + (long long)g * cg * m.s_chan;
    double s = 0.0, q = 0.0;
    for (int i = begin + tid; i < end; i += kThreads) {
        const int y = i / m.W, x = i - y * m.W;
        const float *src = group + y * m.s_row + x * m.s_col;
        for (int c = 0; c < cg; ++c) {
            const double val = (double)src[c * m.s_chan];
            s += val;
            q += val * val;
        }
    }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) { // a fixed tree
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double *dst = partial + (((size_t)b * groups + g) * kGnParts + p) * 2;
        dst[0] = red[0][0];
        dst[1] = red[1][0];
    }
}

// one thread per (frame, channel); stats (nullptr: not wanted): (B, groups, 2) mean | rstd, written by the group's first channel
__global__ __launch_bounds__(kThreads) void gn_affine_kernel(const double *__restrict__ partial, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, double eps, int B, int C, int groups, double count,
                                                             float *__restrict__ a, float *__restrict__ bb, double *__restrict__ stats)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C, g = c / (C / groups);
    const double *src = partial + ((size_t)b * groups + g) * kGnParts * 2;
    double s = 0.0, q = 0.0;
    for (int p = 0; p < kGnParts; ++p) { // ascending parts
        s += src[2 * p];
        q += src[2 * p + 1];
    }
    const double mean = s / count;
    double var = q / count - mean * mean; // biased
    var = var < 0.0 ? 0.0 : var;
    const double rstd = 1.0 / sqrt(var + eps);
    const double ga = gamma ? (double)gamma[c] : 1.0, be = beta ? (double)beta[c] : 0.0;
    a[i] = (float)(ga * rstd);
    bb[i] = (float)(be - mean * ga * rstd);
    if (stats && c == g * (C / groups)) {
        stats[((size_t)b * groups + g) * 2] = mean;
        stats[((size_t)b * groups + g) * 2 + 1] = rstd;
    }
}

__global__ __launch_bounds__(kThreads) void bn_fold_kernel(const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                           const float *__restrict__ var, const float *__restrict__ bias, double eps, int O,
                                                           float *__restrict__ scale, float *__restrict__ shift)
{
    const int o = blockIdx.x * kThreads + threadIdx.x;
    if (o >= O) return;
    const double sc = (gamma ? (double)gamma[o] : 1.0) / sqrt((double)var[o] + eps);
    scale[o] = (float)sc;
    shift[o] = (float)((beta ? (double)beta[o] : 0.0) + ((bias ? (double)bias[o] : 0.0) - (double)mean[o]) * sc);
}

template <int D>
int launch_heads(const Map &m, const unsigned *absmax, const unsigned char *packed, const EpiAffine &epi, int O, float *out, hipStream_t s)
{
    return launch_dense<kTaps, 1, D, false, false>(m, nullptr, nullptr, absmax, packed, epi, O, out, s);
}

// the two launches of the GroupNorm affine; stats: nullptr, or where the (frame, group) mean | rstd go
int group_norm(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C, int L, int W, int groups,
               float *a, float *b, double *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (groups < 1 || C < 1 || C % groups != 0) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!a || !b || !workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < vfa_group_norm_workspace_bytes(B, groups))
        return VFA_ERR_BAD_ARGUMENT;
    if (groups > 65535 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_partial_kernel, dim3(kGnParts, (unsigned)groups, (unsigned)B), dim3(kThreads), 0, s, m, groups, (double *)workspace);
    hipLaunchKernelGGL(gn_affine_kernel, dim3((unsigned)((B * C + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const double *)workspace,
                       gamma, beta, (double)eps, B, C, groups, (double)(C / groups) * (double)L * (double)W, a, b, stats);
    return (int)hipGetLastError();
}

} // namespace

int vfa_conv::frame_absmax(const float *x, const long long *stride, int B, int C, int L, int W, unsigned *absmax, void *stream)
{
    return frame_absmax(x, stride, nullptr, nullptr, B, C, L, W, absmax, stream);
}

int vfa_conv::frame_absmax(const float *x, const long long *stride, const float *a, const float *b, int B, int C, int L, int W, unsigned *absmax,
                           void *stream)
{
    Map m = {};
    const int status = check_map(x, stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    launch_absmax(m, a, b, L, W, 1, absmax, (hipStream_t)stream);
    return (int)hipGetLastError();
}

extern "C" {

size_t vfa_conv3x3_packed_bytes(int O, int C) { return packed_bytes_of(O, C, kTaps); }

int vfa_conv3x3_pack_weights_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream)
{
    return pack_weights(weight, O, C, kTaps, 0, packed, packed_bytes, stream);
}

int vfa_conv3x3_pack_weights_transposed_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream)
{
    return pack_weights(weight, C, O, kTaps, 1, packed, packed_bytes, stream); // the planes of a convolution with O inputs and C outputs
}

size_t vfa_conv3x3_workspace_bytes(int B) { return scales_workspace_bytes(B); }

int vfa_conv3x3_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *scale,
                    const float *shift, int relu, int B, int C, int L, int W, int O, int dilation, float *out, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (O < 1 || dilation < 1) return VFA_ERR_BAD_ARGUMENT;
    int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!packed || !out || !workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < scales_workspace_bytes(B)) return VFA_ERR_BAD_ARGUMENT;
    if (!valid(kTaps, 1, dilation)) return VFA_ERR_UNSUPPORTED;
    status = check_packed(packed, packed_bytes, O, C, kTaps);
    if (status != 0) return status;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, scales_workspace_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    launch_absmax(m, nullptr, nullptr, L, W, 1, (unsigned *)workspace, s);
    const unsigned *absmax = (const unsigned *)workspace;
    const unsigned char *pk = (const unsigned char *)packed;
    const EpiAffine epi = {scale, shift, relu};
    switch (dilation) {
    case 1: return launch_heads<1>(m, absmax, pk, epi, O, out, s);
    case 2: return launch_heads<2>(m, absmax, pk, epi, O, out, s);
    case 3: return launch_heads<3>(m, absmax, pk, epi, O, out, s);
    default: return launch_heads<4>(m, absmax, pk, epi, O, out, s);
    }
}

int vfa_bn_fold_f32(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias, float eps, int O,
                    float *scale, float *shift, void *stream)
{
    if (O < 0 || (O > 0 && (!mean || !var || !scale || !shift))) return VFA_ERR_BAD_ARGUMENT;
    if (O == 0) return 0;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)((O + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gamma, beta,
                       mean, var, bias, (double)eps, O, scale, shift);
    return (int)hipGetLastError();
}

int vfa_conv3x3_few_f32(const float *x, const long long *x_stride, const float *weight, const float *a, const float *b, int B, int C, int L,
                        int W, int O, int dilation, float *out, void *stream)
{
    Map m = {};
    if (O < 1 || dilation < 1) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!weight || !out || (a == nullptr) != (b == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    if (O > 4 || C % 4 != 0 || dilation > kMaxDilation) return VFA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)L, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    switch (O) {
    case 1: hipLaunchKernelGGL(conv_few_kernel<1>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    case 2: hipLaunchKernelGGL(conv_few_kernel<2>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    case 3: hipLaunchKernelGGL(conv_few_kernel<3>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    default: hipLaunchKernelGGL(conv_few_kernel<4>, grid, dim3(kThreads), 0, s, m, weight, a, b, dilation, out); break;
    }
    return (int)hipGetLastError();
}

size_t vfa_group_norm_workspace_bytes(int B, int groups)
{
    if (B <= 0 || groups <= 0) return 0;
    return (size_t)B * (size_t)groups * kGnParts * 2 * sizeof(double);
}

int vfa_group_norm_affine_f32(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C,
                              int L, int W, int groups, float *a, float *b, void *workspace, size_t workspace_bytes, void *stream)
{
    return group_norm(x, x_stride, gamma, beta, eps, B, C, L, W, groups, a, b, nullptr, workspace, workspace_bytes, stream);
}

int vfa_group_norm_stats_f32(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C,
                             int L, int W, int groups, float *a, float *b, double *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!stats || ((uintptr_t)stats & 7) != 0) return VFA_ERR_BAD_ARGUMENT;
    return group_norm(x, x_stride, gamma, beta, eps, B, C, L, W, groups, a, b, stats, workspace, workspace_bytes, stream);
}

} // extern "C"
