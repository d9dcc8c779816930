// vfa_trunk.hip -- the residual stages of the ResNet trunk at inference (reference resnet.py:26-57, a block: conv3x3 - GroupNorm - ReLU -
// conv3x3 - GroupNorm, a 1x1 projection with its GroupNorm or the identity as the shortcut, the join and a ReLU): float32 in and out,
// the input (B, C, L, W) read through its four element strides, the outputs contiguous.  Fixed summation order, no float atomics: the
// same bits on every run, and an image gives the same bits alone and in a batch.
//
//   1. The convolutions are the dense kernel of vfa_dense.h with its absmax pre-pass and its weight pack (the integer rules:
//      vfa_conv.h).  The trunk uses dense_kernel<TAPS, S, 1, TWO, true, EpiRaw> for TAPS = 9 | 1, S = 1 | 2 and TWO = C > 256: dilation
//      1, the optional prologue max(fmaf(a[b, c], x, b[b, c]), 0) of the GroupNorm in front, two accumulator chains past 256
//      channels, and the raw convolution acc 2^-(ea + ew) as the output.  The absmax pre-pass sees what the products see: the values
//      AFTER the prologue, and with one tap the strided positions only.
//   2. residual_join_kernel: out = max(fmaf(a, y, b) + (r | fmaf(ra, r, rb)), 0), one rounding per written operation.
//   3. vfa_trunk_down_dgrad_f32, the input gradient of a stride-2 convolution (training the projection blocks): the four parity
//      classes of dx are dense_kernel<11 | 21 | 12 | 22, 1, 1, TWO, false, EpiDown> on the output gradient -- a block of 1, 2, 2 or 4
//      taps each, the classes' nine taps packed once per call from the weight as it lies (pack_kernel, transposed 2), the result
//      stored through doubled strides; a 1 x 1 weight's term is dense_kernel<1, ...> added to what class (0, 0) holds.
#include "vfa_dense.h"

namespace {

// grid (blocks of 1024 positions of a plane, (image, channel) pairs in a grid-stride loop)
constexpr int kJoinPerThread = 4;
__global__ __launch_bounds__(kThreads) void residual_join_kernel(const float *y, const float *__restrict__ a, const float *__restrict__ b, const float *r,
                                                                 const float *__restrict__ ra, const float *__restrict__ rb, int BC, int plane, float *out)
{
    for (int bc = blockIdx.y; bc < BC; bc += gridDim.y) {
        const float ya = a[bc], yb = b[bc], sa = ra ? ra[bc] : 1.0f, sb = ra ? rb[bc] : 0.0f;
        const size_t base = (size_t)bc * plane;
#pragma unroll
        for (int k = 0; k < kJoinPerThread; ++k) {
            const int p = (blockIdx.x * kJoinPerThread + k) * kThreads + threadIdx.x;
            if (p >= plane) break;
            const float shortcut = ra ? fmaf(sa, r[base + p], sb) : r[base + p];
            const float val = fmaf(ya, y[base + p], yb) + shortcut;
            out[base + p] = val < 0.0f ? 0.0f : val; // (a NaN stays a NaN)
        }
    }
}

template <int TAPS, int S>
int launch_trunk(const Map &m, const float *a, const float *b, const unsigned *absmax, const unsigned char *packed, int O, float *out, hipStream_t s)
{
    return m.C > kSplitC ? launch_dense<TAPS, S, 1, true, true>(m, a, b, absmax, packed, EpiRaw{}, O, out, s)
                         : launch_dense<TAPS, S, 1, false, true>(m, a, b, absmax, packed, EpiRaw{}, O, out, s);
}

// one parity class (py, px) of the stride-2 input gradient, or (TAPS 1) the term of a 1 x 1 weight in class (0, 0): the dense kernel on
// g (m) with the class's block of taps, stored through EpiDown; a class without positions is not launched
template <int TAPS>
int launch_down_class(const Map &m, const unsigned *absmax, const unsigned char *packed, int C, int L, int W, int py, int px, int add, float *dx,
                      hipStream_t s)
{
    const int Lc = vfa_conv_grad::down_class_size(L, py), Wc = vfa_conv_grad::down_class_size(W, px);
    if (Lc == 0 || Wc == 0) return 0;
    const EpiDown epi = {L, W, py, px, add};
    return m.C > kSplitC ? launch_dense<TAPS, 1, 1, true, false>(m, nullptr, nullptr, absmax, packed, epi, C, dx, s, Lc, Wc)
                         : launch_dense<TAPS, 1, 1, false, false>(m, nullptr, nullptr, absmax, packed, epi, C, dx, s, Lc, Wc);
}

} // namespace

extern "C" {

size_t vfa_trunk_packed_bytes(int O, int C, int taps) { return packed_bytes_of(O, C, taps); }

int vfa_trunk_pack_weights_f32(const float *weight, int O, int C, int taps, void *packed, size_t packed_bytes, void *stream)
{
    return pack_weights(weight, O, C, taps, 0, packed, packed_bytes, stream);
}

size_t vfa_trunk_workspace_bytes(int B) { return scales_workspace_bytes(B); }

int vfa_trunk_conv_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *a, const float *b, int B,
                       int C, int L, int W, int O, int taps, int stride, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (O < 1 || !valid(taps, stride, 1) || (a == nullptr) != (b == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    int status = check_map(x, x_stride, B, C, L, W, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!packed || !out || !workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < scales_workspace_bytes(B)) return VFA_ERR_BAD_ARGUMENT;
    status = check_packed(packed, packed_bytes, O, C, taps);
    if (status != 0) return status;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, scales_workspace_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    // the values the products see: with nine taps every position of the map, with one tap the strided positions
    if (taps == 9) launch_absmax(m, a, b, L, W, 1, (unsigned *)workspace, s);
    else launch_absmax(m, a, b, out_size(L, stride), out_size(W, stride), stride, (unsigned *)workspace, s);
    const unsigned *absmax = (const unsigned *)workspace;
    const unsigned char *pk = (const unsigned char *)packed;
    if (taps == 9) return stride == 1 ? launch_trunk<9, 1>(m, a, b, absmax, pk, O, out, s) : launch_trunk<9, 2>(m, a, b, absmax, pk, O, out, s);
    return stride == 1 ? launch_trunk<1, 1>(m, a, b, absmax, pk, O, out, s) : launch_trunk<1, 2>(m, a, b, absmax, pk, O, out, s);
}

size_t vfa_trunk_down_dgrad_workspace_bytes(int B, int O, int C, int kernel)
{
    if (B <= 0 || (kernel != 3 && kernel != 1) || C < 1 || C % 32 != 0) return 0;
    const size_t packed = packed_bytes_of(C, O, kernel * kernel); // the planes of a convolution with O inputs and C outputs
    return packed == 0 ? 0 : scales_workspace_bytes(B) + packed;
}

int vfa_trunk_down_dgrad_f32(const float *g, const long long *g_stride, const float *weight, int B, int O, int Lo, int Wo, int C, int L, int W,
                             int kernel, int accumulate, float *dx, void *workspace, size_t workspace_bytes, void *stream)
{
    Map m = {};
    if (C < 1 || O < 1 || L < 0 || W < 0 || (kernel != 3 && kernel != 1) || (accumulate != 0 && accumulate != 1)) return VFA_ERR_BAD_ARGUMENT;
    if (Lo != out_size(L, 2) || Wo != out_size(W, 2)) return VFA_ERR_BAD_ARGUMENT; // g is not the gradient of a stride-2 map of x's size
    int status = check_map(g, g_stride, B, O, Lo, Wo, m);
    if (status != 0) return status == 1 ? 0 : status;
    if (!weight || !dx || !workspace || ((uintptr_t)workspace & 15) != 0) return VFA_ERR_BAD_ARGUMENT;
    if (C % 32 != 0 || (kernel == 1 && !accumulate)) return VFA_ERR_UNSUPPORTED;
    const int taps = kernel * kernel;
    const size_t packed_bytes = packed_bytes_of(C, O, taps), scales = scales_workspace_bytes(B);
    if (packed_bytes == 0 || out_tiles(C) > 65535) return VFA_ERR_UNSUPPORTED;
    if (workspace_bytes < scales + packed_bytes) return VFA_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, scales, s);
    if (e != hipSuccess) return (int)e;
    launch_absmax(m, nullptr, nullptr, Lo, Wo, 1, (unsigned *)workspace, s); // the whole of g: one scale per image for every class
    unsigned char *packed = (unsigned char *)workspace + scales;
    status = pack_weights(weight, C, O, taps, kernel == 3 ? 2 : 1, packed, packed_bytes, stream);
    if (status != 0) return status;
    const unsigned *absmax = (const unsigned *)workspace;
    if (kernel == 1) return launch_down_class<1>(m, absmax, packed, C, L, W, 0, 0, 1, dx, s);
    status = launch_down_class<11>(m, absmax, packed, C, L, W, 0, 0, accumulate, dx, s);
    if (status == 0) status = launch_down_class<21>(m, absmax, packed, C, L, W, 1, 0, accumulate, dx, s);
    if (status == 0) status = launch_down_class<12>(m, absmax, packed, C, L, W, 0, 1, accumulate, dx, s);
    if (status == 0) status = launch_down_class<22>(m, absmax, packed, C, L, W, 1, 1, accumulate, dx, s);
    return status;
}

int vfa_residual_join_f32(const float *y, const float *a, const float *b, const float *r, const float *ra, const float *rb, int B, int C, int L,
                          int W, float *out, void *stream)
{
    if (B < 0 || C < 0 || L < 0 || W < 0 || (ra == nullptr) != (rb == nullptr)) return VFA_ERR_BAD_ARGUMENT;
    if (B == 0 || C == 0 || (long long)L * W == 0) return 0;
    if (!y || !a || !b || !r || !out) return VFA_ERR_BAD_ARGUMENT;
    if (B > 65535 || L > 65535 || (long long)L * W > INT32_MAX / 2 || (long long)B * C > INT32_MAX) return VFA_ERR_UNSUPPORTED;
    const int plane = L * W, BC = B * C, per_block = kThreads * kJoinPerThread;
    const dim3 grid((unsigned)((plane + per_block - 1) / per_block), (unsigned)(BC < 65535 ? BC : 65535));
    hipLaunchKernelGGL(residual_join_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, y, a, b, r, ra, rb, BC, plane, out);
    return (int)hipGetLastError();
}

} // extern "C"
