// vfa_heat.h -- the rules of the two dense heat-map targets of the reference (vfa/data/GK.py: RotationGaussianKernel "RGK" and
// GaussianKernel "GK") as plain host / device code, one operation per reference operation, so that tests/native/heat_harness.cpp
// compiles this file with g++ and checks it on the CPU (the pattern of vfa_loss.h).  NEVER CONTRACTED: every user compiles with
// -ffp-contract=off; a fused multiply-add in the coordinate chain or the blend changes which cells are skipped.
//
// RGK, per object (GK.py:18-124; l along columns, w along rows, angle in degrees as annotated):
//   size     std = dim * alpha in float64; k = (int)(ceil(max(std_w, std_l)) * ratio); the kernel is n x n, n = k + 1, axis values
//            lo .. lo + k with lo = floor(-k / 2), as float32.
//   tap      A[r][c] = exp((-(x * x)) / d_l - (y * y) / d_w), x = lo + c, y = lo + r, float32 throughout with IEEE divisions;
//            d = (float)(2 * std * std), the float64 product rounded once.  The exp is the float64 exp of the float32 exponent rounded
//            once (numpy's float32 exp is correctly rounded to within its last bit; the tests bound the difference).
//   rotate   float64, separate multiplies and adds: a = deg * pi / 180, c = cos a, s = sin a, H = n;
//            d0 = i - 0.5 H, d1 = -j + 0.5 H; e0 = d0 c + d1 s, e1 = d0 (-s) + d1 c; f0 = e0 + 0.5 H, f1 = -e1 + 0.5 H;
//            ni = floor f0, nj = floor f1, u = f0 - ni, v = f1 - nj;
//            SKIP (0) if nj >= H or ni >= H or ni < 1 or nj < 1 or i + 1 >= H or j + 1 >= H; NEAREST A[ni][nj] if ni + 1 >= H or
//            nj + 1 >= H; else the blend (1-u)(1-v) A[ni][nj] + (1-u) v A[ni][nj+1] + u (1-v) A[ni+1][nj] + u v A[ni+1][nj+1] in
//            float64, left to right, rounded once to float32.
//   centre   the arg-max of the rotated kernel: value descending, then row-major index ascending (DEVIATION: the reference raises
//            on a tie).
//   paste    map[row - g_t + r][col - g_l + q] = max(old, rot[r][q]) with (row, col) the object's cell -- vfa_loss::assign_cell, the
//            function the target encoder uses -- then map[row][col] = 1.  DEVIATION: cells outside the map are dropped (the reference
//            raises when the window leaves its pad).  A pasted value is kept below 1 (`pasted`): only the centre of an object is 1,
//            so the cells of a map equal to 1 are the encoder's positive cells.  (Without an arg-max tie no other value reaches 1.)
//   An object whose kernel cannot be made -- k > kMaxK, k < 2, a non-positive or non-finite dimension or angle -- contributes its
//   centre only and is counted as clipped.
// GK, per frame (GK.py:148-182): occupancy 1 at every object's cell (a duplicate counts once), a (2r+1)^2 float32 table applied as
//   conv2d with zero padding: products in float32 (times 1: exact), summed in FLOAT64 in raster order of the table and rounded
//   once; occupied cells are then 1.  The table is the host's: (float)exp(-(x^2 + y^2) / (2 sigma^2)).
#ifndef VFA_HEAT_H
#define VFA_HEAT_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VFA_HEAT_HD __host__ __device__ __forceinline__
#else
#define VFA_HEAT_HD inline
#endif

namespace vfa_heat {

constexpr int kMaxKernel = 65;       // n of the largest kernel (VFA_HEAT_MAX_KERNEL of include/vfa_hip.h): k <= 64
constexpr int kMaxK = kMaxKernel - 1;
constexpr int kMaxRadius = 16;       // r of the GK table (VFA_HEAT_MAX_RADIUS)
constexpr uint32_t kOneBits = 0x3f800000u, kBelowOneBits = 0x3f7fffffu;

VFA_HEAT_HD uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

VFA_HEAT_HD float float_of(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- RGK: size
struct Kernel {
    bool ok;         // false: centre only (clipped)
    int k, n, lo;    // n = k + 1 taps per side, axis values lo .. lo + k
    float d_l, d_w;  // the two divisors of the tap
};

VFA_HEAT_HD Kernel kernel_of(float l, float w, double alpha, int ratio)
{
    Kernel g = {false, 0, 0, 0, 0.0f, 0.0f};
    const double std_w = (double)w * alpha, std_l = (double)l * alpha;
    const double m = std_w > std_l ? std_w : std_l;
    if (!(std_w > 0.0) || !(std_l > 0.0) || !(m <= 1.0e6) || ratio <= 0 || ratio > 1024) return g;
    const double size = ceil(m) * (double)ratio;
    if (!(size >= 2.0) || size > (double)kMaxK) return g;
    g.k = (int)size;
    g.n = g.k + 1;
    g.lo = -((g.k + 1) / 2);  // floor(-k / 2)
    g.d_l = (float)(2.0 * (std_l * std_l));
    g.d_w = (float)(2.0 * (std_w * std_w));
    g.ok = g.d_l > 0.0f && g.d_w > 0.0f;
    return g;
}

// ---- RGK: tap (r: row, y, w; c: column, x, l)
VFA_HEAT_HD float tap(const Kernel &g, int r, int c)
{
    const float x = (float)(g.lo + c), y = (float)(g.lo + r);
    const float e = (-(x * x)) / g.d_l - (y * y) / g.d_w;
    return (float)exp((double)e);
}

// ---- RGK: the coordinate chain and the branch of a kernel cell
struct Turn { bool ok; double c, s; };

VFA_HEAT_HD Turn turn_of(double deg)
{
    Turn t = {false, 1.0, 0.0};
    if (!(deg >= -1.0e9 && deg <= 1.0e9)) return t;  // (a NaN fails)
    const double a = deg * 3.141592653589793 / 180.0;
    t.c = cos(a);
    t.s = sin(a);
    t.ok = true;
    return t;
}

enum Branch { kSkip = 0, kNearest = 1, kBlend = 2 };
struct Source { int branch, ni, nj; double u, v; };

VFA_HEAT_HD Source source_of(int i, int j, int n, const Turn &t)
{
    Source q = {kSkip, 0, 0, 0.0, 0.0};
    const double half = 0.5 * (double)n;
    const double d0 = (double)i - half, d1 = -(double)j + half;
    const double e0 = d0 * t.c + d1 * t.s, e1 = d0 * (-t.s) + d1 * t.c;
    const double f0 = e0 + half, f1 = -e1 + half;
    const double g0 = floor(f0), g1 = floor(f1);  // |f| < 2 n: the conversions below are defined
    q.ni = (int)g0;
    q.nj = (int)g1;
    q.u = f0 - g0;
    q.v = f1 - g1;
    if (q.nj >= n || q.ni >= n || q.ni < 1 || q.nj < 1 || i + 1 >= n || j + 1 >= n) return q;
    q.branch = (q.ni + 1 >= n || q.nj + 1 >= n) ? kNearest : kBlend;
    return q;
}

// ---- RGK: the blend
VFA_HEAT_HD float blend(const Source &q, float a00, float a01, float a10, float a11)
{
    const double u = q.u, v = q.v;
    return (float)((1.0 - u) * (1.0 - v) * (double)a00 + (1.0 - u) * v * (double)a01 + u * (1.0 - v) * (double)a10 + u * v * (double)a11);
}

// the value of rotated cell (i, j) from the n x n taps (row-major)
VFA_HEAT_HD float rotated(const float *taps, int n, int i, int j, const Turn &t)
{
    const Source q = source_of(i, j, n, t);
    if (q.branch == kSkip) return 0.0f;
    const float *a = taps + q.ni * n + q.nj;
    if (q.branch == kNearest) return a[0];
    return blend(q, a[0], a[1], a[n], a[n + 1]);
}

// ---- RGK: the arg-max order.  The greater key wins: value descending (values are >= 0: their bit patterns order like the floats),
// then index ascending.
VFA_HEAT_HD unsigned long long rank_key(float value, int index)
{
    return ((unsigned long long)bits_of(value) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)index);
}
VFA_HEAT_HD int index_of_key(unsigned long long key) { return (int)(0xffffffffu - (uint32_t)(key & 0xffffffffu)); }

// ---- RGK: the paste.  Kernel cell (r, q) of an object at (row, col) whose arg-max is (g_t, g_l) lands on map cell
// (row - g_t + r, col - g_l + q); -1: outside the map, dropped.
VFA_HEAT_HD int paste_cell(int row, int col, int g_t, int g_l, int r, int q, int L, int W)
{
    const int y = row - g_t + r, x = col - g_l + q;
    return (y < 0 || x < 0 || y >= L || x >= W) ? -1 : y * W + x;
}

// what is pasted for a kernel value, as bits for the integer max (0: nothing to paste); the centre of an object is kOneBits
VFA_HEAT_HD uint32_t pasted(float value)
{
    const uint32_t b = bits_of(value);
    return b >= kOneBits ? kBelowOneBits : b;  // (values are in [0, 1]; a kernel is free of NaN by kernel_of)
}

// ---- GK: one output cell.  occ: the frame's occupancy bytes (L, W); table (2r+1)^2 row-major
VFA_HEAT_HD float gk_cell(const unsigned char *occ, const float *table, int r, int L, int W, int y, int x)
{
    if (occ[y * W + x]) return 1.0f;
    const int side = 2 * r + 1;
    double sum = 0.0;
    for (int i = 0; i < side; ++i) {
        const int yy = y + i - r;
        if (yy < 0 || yy >= L) continue;
        for (int j = 0; j < side; ++j) {
            const int xx = x + j - r;
            if (xx < 0 || xx >= W) continue;
            if (occ[yy * W + xx]) sum += (double)table[i * side + j];
        }
    }
    return (float)sum;
}

}  // namespace vfa_heat

#endif  // VFA_HEAT_H
