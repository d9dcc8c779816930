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
