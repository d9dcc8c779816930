// vfa_resize.h -- the rules of the image front end as plain host / device code: Pillow's antialiased bilinear resize of 8-bit
// images (the reference's transforms.Resize, vfa/data/dataset.py:63), ToTensor and the model's normalisation (vfanet.py:59), one
// operation per reference operation, so that tests/native/resize_harness.cpp compiles this file with g++ and checks it on the CPU
// against Pillow's own pixels (the pattern of vfa_heat.h).  NEVER CONTRACTED: every user compiles with -ffp-contract=off.
//
// Per axis, `in` source and `out` target length, everything in double:
//   scale = in / out, fs = max(scale, 1), support = fs, ksize = (int)ceil(support) * 2 + 1, ss = 1 / fs.
//   Output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
//   n = min((int)(center + support + 0.5), in) - xmin taps, w[x] = tri((x + xmin - center + 0.5) * ss) with
//   tri(a) = |a| < 1 ? 1 - |a| : 0, ww the LEFT-TO-RIGHT sum of w, w[x] /= ww where ww != 0, and the integer coefficient
//   k[x] = (int)(0.5 + w[x] * 2^22) (bilinear weights are never negative).
// A pass: acc = 2^21 + sum pixel * k[x] in int32, the result clip(acc >> 22, 0, 255) as a BYTE.  The horizontal pass runs first, into
//   a byte image; the vertical pass runs on those bytes.  An axis that keeps its length has the coefficients (2^22, 0): the identity.
// The tensor: t = (float)byte / 255.0f, value = (t - mean[c]) / std[c], each a correctly rounded float32 operation (an IEEE division,
//   no reciprocal): a byte has 256 values, so a channel's values are a 256-entry table.
#ifndef VFA_RESIZE_H
#define VFA_RESIZE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VFA_RESIZE_HD __host__ __device__ __forceinline__
#else
#define VFA_RESIZE_HD inline
#endif

namespace vfa_resize {

constexpr int kMaxTaps = 17;         // ksize of the strongest downscale taken, 8x (VFA_IMAGE_MAX_TAPS of include/vfa_hip.h)
constexpr int kMaxLength = 16384;    // the longest axis, source or target (VFA_IMAGE_MAX_LENGTH)
constexpr int kPrecisionBits = 22;   // Pillow's PRECISION_BITS
constexpr int kTableEntries = 3 * 256;

struct Axis {
    double scale, support, ss;
    int in, ksize;
};

VFA_RESIZE_HD Axis axis_of(int in, int out)
{
    Axis a;
    a.in = in;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = fs;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / fs;
    return a;
}

VFA_RESIZE_HD int ksize_of(int in, int out) { return axis_of(in, out).ksize; }

VFA_RESIZE_HD double triangle(double a)
{
    if (a < 0.0) a = -a;
    return a < 1.0 ? 1.0 - a : 0.0;
}

// the taps of output index xx: first source index *xmin, their number (the return value, 1 .. ksize)
VFA_RESIZE_HD int bounds(const Axis &a, int xx, int *xmin)
{
    const double center = ((double)xx + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + a.support + 0.5);
    if (hi > a.in) hi = a.in;
    *xmin = lo;
    return hi - lo;
}

// ... and their integer coefficients k[0 .. ksize), zero behind the taps
VFA_RESIZE_HD int coefficients(const Axis &a, int xx, int *xmin, int *k)
{
    const int n = bounds(a, xx, xmin);
    const double center = ((double)xx + 0.5) * a.scale;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += triangle(((double)(x + *xmin) - center + 0.5) * a.ss);
    for (int x = 0; x < a.ksize; ++x) {
        double w = 0.0;
        if (x < n) {
            w = triangle(((double)(x + *xmin) - center + 0.5) * a.ss);
            if (ww != 0.0) w /= ww;
        }
        k[x] = (int)(0.5 + w * (double)(1 << kPrecisionBits));
    }
    return n;
}

// ---- a pass, one pixel of one channel
VFA_RESIZE_HD int pass_begin() { return 1 << (kPrecisionBits - 1); }
VFA_RESIZE_HD int pass_tap(int acc, int pixel, int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return acc + __mul24(pixel, k);  // 0 <= pixel < 2^8, 0 <= k <= 2^22: the 24-bit multiply is exact, and full rate where the 32-bit one is not
#else
    return acc + pixel * k;
#endif
}
VFA_RESIZE_HD int pass_end(int acc)
{
    const int v = acc >> kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

VFA_RESIZE_HD uint8_t pass_pixel(const uint8_t *first, int stride, const int *k, int n)
{
    int acc = pass_begin();
    for (int x = 0; x < n; ++x) acc = pass_tap(acc, first[(long long)x * stride], k[x]);
    return (uint8_t)pass_end(acc);
}

// ---- ToTensor and the normalisation of one byte value
VFA_RESIZE_HD float table_entry(int byte, float mean, float std)
{
    const float t = (float)byte / 255.0f;
    return (t - mean) / std;
}

}  // namespace vfa_resize

#endif  // VFA_RESIZE_H
