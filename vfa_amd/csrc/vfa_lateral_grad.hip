// vfa_lateral_grad.hip -- the backward of the producer for the training step: from d integral (the
// channels-last gradient the frame node accumulates) straight to d trunk output, d conv weight, d conv bias, d gamma and d beta of
//     integral = cumsum_H(cumsum_W(relu(GroupNorm16(conv1x1(f)))))      reference vfa/model/vfanet.py:37-42, 72-74 + vfa_op.py:172-173
// without an NCHW lateral map or an NCHW d lateral.  Per view n and group g (16 channels, P = h w pixels, N_g = 16 P), mu and r the
// group's mean and reciprocal standard deviation (vfa_lateral_convs_train_f32, double), y the convolution output, z = y * scale + shift
// with the two fp32 roundings of the forward's row scan (vfa_integral.hip, rows_hwc_kernel):
//   d a  = reverse cumsum of d integral along H, then along W, interior only (integral_cols_backward / integral_rows_backward order:
//          double accumulators rounded to fp32 per element, H first)                                           scan_cols_kernel, scan_rows_kernel
//   dz   = d a [z > 0]                                                                                         scan_rows_kernel
//   S1 = sum_p dz,  S2 = sum_p dz (y - mu),  T = sum_p (y - mu)        per (n, c) in double, around mu          scan_rows_kernel, stats_view_kernel
//   A_g = (1 / N_g) sum_{c in g} gamma_c S1,   B_g = (r / N_g) sum_{c in g} gamma_c S2
//   d y  = (r gamma_c) dz - r^2 B_g (y - mu) - r A_g                   formed on the fly by the convolution kernels (form_dy)
//   d beta_c = sum_n S1,  d gamma_c = sum_n r S2,  d b_c = sum_n (r gamma_c S1 - r^2 B_g T - P r A_g)    stats_sum_kernel (double)
//   d f[n, k, p] = sum_c W[c, k] d y[n, p, c]        (NCHW)                                                     grad_feat_kernel
//   d W[c, k]    = sum_{n, p} d y[n, p, c] f[n, k, p]                                                            grad_weight_kernel + _reduce
// d b is the exact sum of d y taken in double from the statistics the scan gathered anyway (no pass over d y for it).
// The two products run at the width of an sgemm: six bf16 MFMA products of a three-piece split of both operands with fp32
// accumulation, the arithmetic of vfa_lateral.hip and vfa_grad.hip.  Every sum has a fixed order (per-workgroup partials in fixed
// workspace slots, added in order by a second kernel; butterflies inside a wave): no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vfa_hip.h"
#include "vfa_geom.h"

namespace {
using namespace vfa_dev;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kCo = 256;      // lateral channels
constexpr int kGroups = 16;   // GroupNorm(16, 256)
constexpr int kGc = 16;       // channels per group = the reduction depth of one v_mfma_f32_32x32x16_bf16
constexpr int kMaxK = 1024;
constexpr int kMaxMaps = 3;
constexpr int kKBlocks = 4;   // 32-wide k blocks per wave (both products): 128 k per workgroup
constexpr int kDwUnits = 192; // d W workgroups per map the slabs aim at (partials: units x 256 x 128 floats)

// ---- workspace of one map: the scan call fills the first areas, the convolution call reads them ------------------------------
struct Layout {
    size_t part;   // double (n, H, 3, 256): per (view, row) sums S1, S2, T of every channel
    size_t chan;   // double (n, 3, 256): per (view, channel) d beta, d gamma, d b shares
    size_t coef;   // float (n, 256): r gamma_c
    size_t gk;     // float (n, 16, 2): r^2 B_g, r A_g
    size_t wfrag;  // bf16 (K / 32, 16, 3, 64) x 8: W^T as three planes in MFMA fragment order
    size_t dw;     // float (units, 256, K): d W partials
    size_t stats_end, total;
    int parts, ktiles; // d W slabs per view, 128-wide k tiles
};
__host__ __device__ inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline int dw_parts(int n_views, int HW, int K)
{
    const int ktiles = (K + 127) / 128;
    if (n_views <= 0) return 1;
    const long long steps = ((long long)HW + 15) / 16;
    long long p = ((long long)kDwUnits + (long long)n_views * ktiles - 1) / ((long long)n_views * ktiles);
    if (p > steps) p = steps;
    return p < 1 ? 1 : (int)p;
}
inline Layout layout_of(int n_views, int K, int H, int W)
{
    Layout l;
    size_t o = 0;
    l.part = o; o = align256(o + (size_t)n_views * H * 3 * kCo * sizeof(double));
    l.chan = o; o = align256(o + (size_t)n_views * 3 * kCo * sizeof(double));
    l.coef = o; o = align256(o + (size_t)n_views * kCo * sizeof(float));
    l.gk = o; o = align256(o + (size_t)n_views * kGroups * 2 * sizeof(float));
    l.stats_end = o;
    l.ktiles = (K + 127) / 128;
    l.parts = dw_parts(n_views, H * W, K);
    l.wfrag = o; o = align256(o + (size_t)(K / 32) * kGc * 3 * 64 * 16);
    l.dw = o; o = align256(o + (size_t)n_views * l.parts * kCo * K * sizeof(float));
    l.total = o;
    return l;
}

// ---- kernel 2: reverse scans + mask + statistics ---------------------------------------------------------------------------------
struct ScanMap {
    const float *gi;      // (n, H + 2, W + 2, 256) d integral
    const float *y;       // (n, H, W, 256)
    const float *scale, *shift; // (n, 256)
    const double *mean, *rstd;  // (n, 16)
    const float *gamma;   // (256)
    float *dz;            // (n, H, W, 256): first the H-scanned d integral, then dz in place
    unsigned char *ws;
    Layout l;
    float *g_bias, *g_gamma, *g_beta; // (256) or NULL
    int H, W;
    unsigned long long col_end; // cumulative threads of the column pass
    unsigned row_end;           // cumulative waves of the row pass
    unsigned view_end;          // cumulative workgroups of stats_view_kernel
};
struct ScanArgs { ScanMap m[kMaxMaps]; int n_maps, n_views; };

// pass H: one thread = four channels of one interior column of one view; reverse cumsum over the interior rows (double, rounded per
// element: integral_cols_backward_kernel's sequence), written to dz.  The border rows and columns of d integral are never read.
__global__ __launch_bounds__(256) void scan_cols_kernel(ScanArgs a)
{
    unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && i >= a.m[mi].col_end) ++mi;
    const ScanMap &m = a.m[mi];
    if (i >= m.col_end) return;
    if (mi > 0) i -= a.m[mi - 1].col_end;
    const int H = m.H, W = m.W;
    const int q = (int)(i % (kCo / 4));
    const unsigned long long rest = i / (kCo / 4);
    const int x = (int)(rest % (unsigned)W), v = (int)(rest / (unsigned)W);
    const size_t in_row = (size_t)(W + 2) * kCo / 4, out_row = (size_t)W * kCo / 4;
    const float4 *src = reinterpret_cast<const float4 *>(m.gi) + ((size_t)v * (H + 2) + 1) * in_row + (size_t)(x + 1) * (kCo / 4) + q;
    float4 *dst = reinterpret_cast<float4 *>(m.dz) + (size_t)v * H * out_row + (size_t)x * (kCo / 4) + q;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    constexpr int U = 8;
    int y = H - 1;
    for (; y - U + 1 >= 0; y -= U) {
        float4 t[U];
#pragma unroll
        for (int k = 0; k < U; ++k) t[k] = src[(size_t)(y - k) * in_row];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            a0 += (double)t[k].x; a1 += (double)t[k].y; a2 += (double)t[k].z; a3 += (double)t[k].w;
            dst[(size_t)(y - k) * out_row] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        }
    }
    for (; y >= 0; --y) {
        const float4 t = src[(size_t)y * in_row];
        a0 += (double)t.x; a1 += (double)t.y; a2 += (double)t.z; a3 += (double)t.w;
        dst[(size_t)y * out_row] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    }
}

// pass W: one wave = 64 channels of one row of one view; reverse cumsum along the row over the H-scanned values (double, rounded per
// element: integral_rows_backward_kernel's sequence), the mask of the forward's row scan recomputed from y, scale, shift in the same
// two fp32 operations, dz stored in place, and the row's S1, S2, T per channel (double, around the group mean).
__global__ __launch_bounds__(kWave) void scan_rows_kernel(ScanArgs a)
{
    unsigned b = blockIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && b >= a.m[mi].row_end) ++mi;
    const ScanMap &m = a.m[mi];
    if (mi > 0) b -= a.m[mi - 1].row_end;
    const int lane = threadIdx.x, H = m.H, W = m.W;
    const int row = (int)(b % (unsigned)H);
    const unsigned rest = b / (unsigned)H;
    const int c = (int)(rest % 4u) * kWave + lane, v = (int)(rest / 4u);
    const float sc = m.scale[(size_t)v * kCo + c], sh = m.shift[(size_t)v * kCo + c];
    const double mu = m.mean[(size_t)v * kGroups + c / kGc];
    const size_t base = ((size_t)v * H + row) * W * kCo + c;
    float *dz = m.dz + base;
    const float *yp = m.y + base;
    double acc = 0.0, s1 = 0.0, s2 = 0.0, t3 = 0.0;
    auto step = [&](float g, float yv, int x) {
        acc += (double)g;
        const float da = (float)acc;
        float t = yv * sc;
        t = t + sh;
        const float d = t > 0.0f ? da : 0.0f;
        dz[(size_t)x * kCo] = d;
        const double e = (double)yv - mu;
        s1 += (double)d;
        s2 += (double)d * e;
        t3 += e;
    };
    constexpr int U = 8;
    int x = W - 1;
    for (; x - U + 1 >= 0; x -= U) {
        float g[U], yv[U];
#pragma unroll
        for (int k = 0; k < U; ++k) { g[k] = dz[(size_t)(x - k) * kCo]; yv[k] = yp[(size_t)(x - k) * kCo]; }
#pragma unroll
        for (int k = 0; k < U; ++k) step(g[k], yv[k], x - k);
    }
    for (; x >= 0; --x) step(dz[(size_t)x * kCo], yp[(size_t)x * kCo], x);
    double *p = reinterpret_cast<double *>(m.ws + m.l.part) + ((size_t)v * H + row) * 3 * kCo + c;
    p[0] = s1; p[kCo] = s2; p[2 * kCo] = t3;
}

// per (map, view), thread = channel: the rows' sums in row order, the group sums by a fixed 16-lane butterfly, then the
// coefficients of d y and the view's shares of d beta, d gamma, d b
__global__ __launch_bounds__(kCo) void stats_view_kernel(ScanArgs a)
{
    unsigned b = blockIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && b >= a.m[mi].view_end) ++mi;
    const ScanMap &m = a.m[mi];
    if (mi > 0) b -= a.m[mi - 1].view_end;
    const int v = (int)b, c = threadIdx.x, g = c / kGc, H = m.H;
    const double *p = reinterpret_cast<const double *>(m.ws + m.l.part) + (size_t)v * H * 3 * kCo + c;
    double s1 = 0.0, s2 = 0.0, t3 = 0.0;
    constexpr int U = 8;
    int r = 0;
    for (; r + U <= H; r += U) {
        double x1[U], x2[U], x3[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const double *q = p + (size_t)(r + k) * 3 * kCo;
            x1[k] = q[0]; x2[k] = q[kCo]; x3[k] = q[2 * kCo];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) { s1 += x1[k]; s2 += x2[k]; t3 += x3[k]; }
    }
    for (; r < H; ++r) {
        const double *q = p + (size_t)r * 3 * kCo;
        s1 += q[0]; s2 += q[kCo]; t3 += q[2 * kCo];
    }
    const double rs = m.rstd[(size_t)v * kGroups + g];
    const double gam = (double)m.gamma[c];
    double x1 = gam * s1, x2 = gam * s2;
#pragma unroll
    for (int d = 1; d < kGc; d <<= 1) { // (commutative pairwise adds: every lane of the group ends with the same bits)
        x1 += __shfl_xor(x1, d);
        x2 += __shfl_xor(x2, d);
    }
    const double P = (double)H * m.W, Ng = P * kGc;
    const double A = x1 / Ng, B = rs * x2 / Ng;
    float *coef = reinterpret_cast<float *>(m.ws + m.l.coef);
    float *gk = reinterpret_cast<float *>(m.ws + m.l.gk);
    coef[(size_t)v * kCo + c] = (float)(rs * gam);
    if ((c & (kGc - 1)) == 0) {
        gk[((size_t)v * kGroups + g) * 2 + 0] = (float)(rs * rs * B);
        gk[((size_t)v * kGroups + g) * 2 + 1] = (float)(rs * A);
    }
    double *ch = reinterpret_cast<double *>(m.ws + m.l.chan) + (size_t)v * 3 * kCo + c;
    ch[0] = s1;
    ch[kCo] = rs * s2;
    ch[2 * kCo] = rs * gam * s1 - rs * rs * B * t3 - P * rs * A;
}

// per map, thread = channel: the views' shares in view order
__global__ __launch_bounds__(kCo) void stats_sum_kernel(ScanArgs a)
{
    const ScanMap &m = a.m[blockIdx.x];
    const int c = threadIdx.x;
    const double *ch = reinterpret_cast<const double *>(m.ws + m.l.chan) + c;
    double sb = 0.0, sg = 0.0, sbias = 0.0;
    for (int v = 0; v < a.n_views; ++v) {
        sb += ch[(size_t)v * 3 * kCo];
        sg += ch[(size_t)v * 3 * kCo + kCo];
        sbias += ch[(size_t)v * 3 * kCo + 2 * kCo];
    }
    if (m.g_beta) m.g_beta[c] = (float)sb;
    if (m.g_gamma) m.g_gamma[c] = (float)sg;
    if (m.g_bias) m.g_bias[c] = (float)sbias;
}

// ---- kernel 3: the convolution's two products --------------------------------------------------------------------------------
struct ConvMap {
    const float *dz, *y;  // (n, HW, 256)
    const double *mean;   // (n, 16)
    const float *feat;    // (n, K, HW)
    const float *w;       // (256, K)
    float *g_feat;        // (n, K, HW) or NULL
    float *g_w;           // (256, K) or NULL
    unsigned char *ws;
    Layout l;
    int K, HW;
    unsigned split_end, feat_end, dw_end; // cumulative workgroups of the three launches
    unsigned long long red_end;           // cumulative threads of the reduction
};
struct ConvArgs { ConvMap m[kMaxMaps]; int n_maps, n_views; };

__device__ __forceinline__ void split3(const float (&x)[8], bf16x8 &p0, bf16x8 &p1, bf16x8 &p2)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 q0 = (__bf16)x[j];
        const float r1 = x[j] - (float)q0;
        const __bf16 q1 = (__bf16)r1;
        p0[j] = q0; p1[j] = q1; p2[j] = (__bf16)(r1 - (float)q1);
    }
}
// d y of one element in fp32 from dz, y and the coefficients (y - mu formed in double: no cancellation when |mu| >> sigma).  Both
// products form it with this one sequence.
__device__ __forceinline__ float form_dy(float dz, float y, float a, float k1, float k0, double mu)
{
    const float e = (float)((double)y - mu);
    float t = k1 * e;
    t = t + k0;
    float d = a * dz;
    return d - t;
}
// D += A . B as six bf16 products, small terms first (the order of vfa_lateral.hip / vfa_grad.hip)
__device__ __forceinline__ void mfma6(f32x16 &acc, const bf16x8 &a0, const bf16x8 &a1, const bf16x8 &a2, const bf16x8 &b0,
                                      const bf16x8 &b1, const bf16x8 &b2)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
}

// W^T as three bf16 planes in MFMA fragment order (the forward's lateral_split_weight has the channels as rows and k as the
// reduction; d f needs the transpose):  frag[((cc * (K / 32) + kb) * 3 + plane) * 64 + lane] = W[c = 16 cc + 8 (lane >> 5) + j][k = 32 kb + (lane & 31)]
__global__ __launch_bounds__(256) void split_weight_t_kernel(ConvArgs a)
{
    unsigned b = blockIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && b >= a.m[mi].split_end) ++mi;
    const ConvMap &m = a.m[mi];
    if (mi > 0) b -= a.m[mi - 1].split_end;
    const int KB = m.K / 32;
    const int idx = (int)b * 256 + threadIdx.x; // (cc, kb, lane)
    if (idx >= kGc * KB * 64) return;
    const int lane = idx & 63, kb = (idx >> 6) % KB, cc = (idx >> 6) / KB;
    const float *src = m.w + (size_t)(16 * cc + 8 * (lane >> 5)) * m.K + 32 * kb + (lane & 31);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = src[(size_t)j * m.K];
    bf16x8 p0, p1, p2;
    split3(x, p0, p1, p2);
    bf16x8 *o = reinterpret_cast<bf16x8 *>(m.ws + m.l.wfrag) + ((size_t)cc * KB + kb) * 3 * 64 + lane;
    o[0] = p0; o[64] = p1; o[128] = p2;
}

// d f[n, k, p] = sum_c W[c, k] d y[n, p, c]: a workgroup = four waves = 128 pixels of one view x 128 k; wave w owns 32 pixels and the
// (up to) four 32-k blocks.  The k are the MFMA rows (W^T fragments from L2 / L1), the pixels its columns: lane (pixel, channel half)
// forms the eight d y of a 16-channel chunk -- one GroupNorm group -- from 32 contiguous bytes of dz and y and splits them in
// registers.  Register i of block kb is k = 32 kb + (i & 3) + 8 (i >> 2) + 4 half, pixel p0 + (lane & 31): a half wave stores 128
// contiguous bytes of one NCHW row.
__global__ __launch_bounds__(256) void grad_feat_kernel(ConvArgs a)
{
    unsigned b = blockIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && b >= a.m[mi].feat_end) ++mi;
    const ConvMap &m = a.m[mi];
    if (mi > 0) b -= a.m[mi - 1].feat_end;
    const int KB = m.K / 32, kgroups = (KB + kKBlocks - 1) / kKBlocks;
    const int pblocks = (m.HW + 127) / 128;
    const int kg = (int)(b % (unsigned)kgroups);
    const unsigned rest = b / (unsigned)kgroups;
    const int blk = (int)(rest % (unsigned)pblocks), v = (int)(rest / (unsigned)pblocks);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int p0 = blk * 128 + wave * 32;
    if (p0 >= m.HW) return;
    const int p = p0 + col;
    const bool on = p < m.HW;
    const int pc = on ? p : m.HW - 1;
    const int kb0 = kg * kKBlocks, nkb = min(kKBlocks, KB - kb0);
    const float *dzp = m.dz + ((size_t)v * m.HW + pc) * kCo + 8 * h;
    const float *yp = m.y + ((size_t)v * m.HW + pc) * kCo + 8 * h;
    const float *coef = reinterpret_cast<const float *>(m.ws + m.l.coef) + (size_t)v * kCo + 8 * h;
    const float *gk = reinterpret_cast<const float *>(m.ws + m.l.gk) + (size_t)v * kGroups * 2;
    const double *mean = m.mean + (size_t)v * kGroups;
    const bf16x8 *frag = reinterpret_cast<const bf16x8 *>(m.ws + m.l.wfrag) + lane;

    f32x16 acc[kKBlocks];
#pragma unroll
    for (int kb = 0; kb < kKBlocks; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[kb][i] = 0.0f;

    for (int cc = 0; cc < kGroups; ++cc) {
        const float4 d0 = *reinterpret_cast<const float4 *>(dzp + 16 * cc), d1 = *reinterpret_cast<const float4 *>(dzp + 16 * cc + 4);
        const float4 y0 = *reinterpret_cast<const float4 *>(yp + 16 * cc), y1 = *reinterpret_cast<const float4 *>(yp + 16 * cc + 4);
        const float4 c0 = *reinterpret_cast<const float4 *>(coef + 16 * cc), c1 = *reinterpret_cast<const float4 *>(coef + 16 * cc + 4);
        const float k1 = gk[2 * cc], k0 = gk[2 * cc + 1];
        const double mu = mean[cc];
        const float dzv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        const float yv[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
        const float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        float dy[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) dy[j] = on ? form_dy(dzv[j], yv[j], cv[j], k1, k0, mu) : 0.0f;
        bf16x8 q0, q1, q2;
        split3(dy, q0, q1, q2);
#pragma unroll
        for (int kb = 0; kb < kKBlocks; ++kb) {
            if (kb < nkb) {
                const bf16x8 *f = frag + ((size_t)cc * KB + kb0 + kb) * 3 * 64;
                const bf16x8 w0 = f[0], w1 = f[64], w2 = f[128];
                mfma6(acc[kb], w0, w1, w2, q0, q1, q2);
            }
        }
    }
    if (!on) return;
    float *dst = m.g_feat + (size_t)v * m.K * m.HW + p;
#pragma unroll
    for (int kb = 0; kb < kKBlocks; ++kb) {
        if (kb < nkb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = 32 * (kb0 + kb) + (i & 3) + 8 * (i >> 2) + 4 * h;
                dst[(size_t)k * m.HW] = acc[kb][i];
            }
        }
    }
}

// d W partials: a workgroup = one slab of 16-pixel steps of one view x 128 k; wave w owns channels 64 w .. 64 w + 63 (two 32-row
// blocks) and the (up to) four 32-k blocks.  The channels are the MFMA rows: lane (channel, pixel half) forms d y of eight
// consecutive pixels of its channel; the trunk map is the column operand: lane (k, pixel half) loads eight consecutive pixels of an
// NCHW row.  The partial of the slab goes to its own workspace slot ((view, slab) major, then channel, then k).
__global__ __launch_bounds__(256) void grad_weight_kernel(ConvArgs a)
{
    unsigned b = blockIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && b >= a.m[mi].dw_end) ++mi;
    const ConvMap &m = a.m[mi];
    if (mi > 0) b -= a.m[mi - 1].dw_end;
    const int KB = m.K / 32, ktiles = m.l.ktiles, parts = m.l.parts;
    const int kt = (int)(b % (unsigned)ktiles);
    const unsigned rest = b / (unsigned)ktiles;
    const int part = (int)(rest % (unsigned)parts), v = (int)(rest / (unsigned)parts);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int kb0 = kt * kKBlocks, nkb = min(kKBlocks, KB - kb0);
    const long long steps = ((long long)m.HW + 15) / 16;
    const int s0 = (int)(steps * part / parts), s1 = (int)(steps * (part + 1) / parts);

    // this lane's two channels (one per 32-row block) and their coefficients
    int cch[2];
    float ca[2], ck1[2], ck0[2];
    double cmu[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int c = 64 * wave + 32 * cb + col, g = c / kGc;
        cch[cb] = c;
        ca[cb] = reinterpret_cast<const float *>(m.ws + m.l.coef)[(size_t)v * kCo + c];
        ck1[cb] = reinterpret_cast<const float *>(m.ws + m.l.gk)[((size_t)v * kGroups + g) * 2];
        ck0[cb] = reinterpret_cast<const float *>(m.ws + m.l.gk)[((size_t)v * kGroups + g) * 2 + 1];
        cmu[cb] = m.mean[(size_t)v * kGroups + g];
    }
    const float *dzv = m.dz + (size_t)v * m.HW * kCo;
    const float *yv = m.y + (size_t)v * m.HW * kCo;
    const float *fv = m.feat + (size_t)v * m.K * m.HW;

    f32x16 acc[2][kKBlocks];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int kb = 0; kb < kKBlocks; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][kb][i] = 0.0f;

    for (int s = s0; s < s1; ++s) {
        const int q = 16 * s + 8 * h; // this lane's first pixel
        bf16x8 ap[2][3];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int px = q + j;
                const bool on = px < m.HW;
                const size_t o = (size_t)(on ? px : m.HW - 1) * kCo + cch[cb];
                const float g = dzv[o], yy = yv[o];
                d[j] = on ? form_dy(g, yy, ca[cb], ck1[cb], ck0[cb], cmu[cb]) : 0.0f;
            }
            split3(d, ap[cb][0], ap[cb][1], ap[cb][2]);
        }
#pragma unroll
        for (int kb = 0; kb < kKBlocks; ++kb) {
            if (kb < nkb) {
                const float *fr = fv + (size_t)(32 * (kb0 + kb) + col) * m.HW;
                float f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int px = q + j;
                    f[j] = px < m.HW ? fr[px] : 0.0f;
                }
                bf16x8 b0, b1, b2;
                split3(f, b0, b1, b2);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) mfma6(acc[cb][kb], ap[cb][0], ap[cb][1], ap[cb][2], b0, b1, b2);
            }
        }
    }
    float *dst = reinterpret_cast<float *>(m.ws + m.l.dw) + (size_t)(v * parts + part) * kCo * m.K;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int kb = 0; kb < kKBlocks; ++kb) {
            if (kb < nkb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 64 * wave + 32 * cb + (i & 3) + 8 * (i >> 2) + 4 * h;
                    dst[(size_t)c * m.K + 32 * (kb0 + kb) + col] = acc[cb][kb][i];
                }
            }
        }
}

// d W[c][k] = sum over the (view, slab) partials: four interleaved chains (partials u, u + 4, ...), then ((c0 + c1) + c2) + c3
__global__ __launch_bounds__(256) void grad_weight_reduce_kernel(ConvArgs a)
{
    unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    int mi = 0;
    while (mi + 1 < a.n_maps && i >= a.m[mi].red_end) ++mi;
    const ConvMap &m = a.m[mi];
    if (i >= m.red_end) return;
    if (mi > 0) i -= a.m[mi - 1].red_end;
    const int units = a.n_views * m.l.parts;
    const size_t stride = (size_t)kCo * m.K;
    const float *src = reinterpret_cast<const float *>(m.ws + m.l.dw) + i;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int u = 0;
    for (; u + 4 <= units; u += 4) {
        const float v0 = src[(size_t)u * stride], v1 = src[(size_t)(u + 1) * stride], v2 = src[(size_t)(u + 2) * stride],
                    v3 = src[(size_t)(u + 3) * stride];
        s[0] += v0; s[1] += v1; s[2] += v2; s[3] += v3;
    }
    for (int k = 0; u < units; ++u, ++k) s[k] += src[(size_t)u * stride];
    m.g_w[i] = ((s[0] + s[1]) + s[2]) + s[3];
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int shape_check(int n_maps, int n_views, const int *Ks, const int *feat_hw)
{
    if (n_maps < 1 || n_maps > kMaxMaps || n_views < 0 || !Ks || !feat_hw) return VFA_ERR_BAD_ARGUMENT;
    if (n_views > 65535) return VFA_ERR_UNSUPPORTED;
    for (int m = 0; m < n_maps; ++m) {
        const int K = Ks[m], H = feat_hw[2 * m], W = feat_hw[2 * m + 1];
        if (K <= 0 || H <= 0 || W <= 0) return VFA_ERR_BAD_ARGUMENT;
        if (K % 32 != 0 || K > kMaxK) return VFA_ERR_UNSUPPORTED;
        if ((long long)H * W * kCo * (long long)(n_views > 0 ? n_views : 1) >= (1ll << 40) || (long long)H * W >= (1ll << 28))
            return VFA_ERR_UNSUPPORTED;
    }
    return 0;
}

} // namespace

extern "C" {

size_t vfa_lateral_backward_workspace_bytes(int n_views, int K, int Hf, int Wf)
{
    if (n_views < 0 || K <= 0 || Hf <= 0 || Wf <= 0 || K % 32 != 0 || K > kMaxK) return 0;
    return layout_of(n_views, K, Hf, Wf).total;
}

int vfa_lateral_scan_backward_f32(int n_maps, const float *const *grad_integrals, const float *const *ys_hwc, const float *const *scales,
                                  const float *const *shifts, const double *const *means, const double *const *rstds,
                                  const float *const *gammas, float *const *dzs_hwc, float *const *grad_biases, float *const *grad_gammas,
                                  float *const *grad_betas, void *const *workspaces, const size_t *workspace_bytes, int n_views,
                                  const int *Ks, const int *feat_hw, void *stream)
{
    {
        const int st = shape_check(n_maps, n_views, Ks, feat_hw);
        if (st) return st;
    }
    if (!grad_integrals || !ys_hwc || !scales || !shifts || !means || !rstds || !gammas || !dzs_hwc || !workspaces || !workspace_bytes)
        return VFA_ERR_BAD_ARGUMENT;
    ScanArgs sa;
    sa.n_maps = n_maps;
    sa.n_views = n_views;
    unsigned long long cols = 0;
    unsigned long long rows = 0, views = 0;
    for (int m = 0; m < kMaxMaps; ++m) {
        ScanMap &s = sa.m[m];
        if (m >= n_maps) { s = sa.m[0]; s.col_end = cols; s.row_end = (unsigned)rows; s.view_end = (unsigned)views; continue; }
        const int H = feat_hw[2 * m], W = feat_hw[2 * m + 1];
        if (!grad_integrals[m] || !ys_hwc[m] || !scales[m] || !shifts[m] || !means[m] || !rstds[m] || !gammas[m] || !dzs_hwc[m])
            return VFA_ERR_BAD_ARGUMENT;
        s.l = layout_of(n_views, Ks[m], H, W);
        if (n_views > 0 && (!workspaces[m] || workspace_bytes[m] < s.l.total)) return VFA_ERR_BAD_ARGUMENT;
        if (!aligned16(grad_integrals[m]) || !aligned16(dzs_hwc[m]) || !aligned16(workspaces[m])) return VFA_ERR_UNSUPPORTED;
        s.gi = grad_integrals[m]; s.y = ys_hwc[m]; s.scale = scales[m]; s.shift = shifts[m]; s.mean = means[m]; s.rstd = rstds[m];
        s.gamma = gammas[m]; s.dz = dzs_hwc[m]; s.ws = static_cast<unsigned char *>(workspaces[m]);
        s.g_bias = grad_biases ? grad_biases[m] : nullptr;
        s.g_gamma = grad_gammas ? grad_gammas[m] : nullptr;
        s.g_beta = grad_betas ? grad_betas[m] : nullptr;
        s.H = H; s.W = W;
        cols += (unsigned long long)n_views * W * (kCo / 4);
        rows += (unsigned long long)n_views * H * 4;
        views += (unsigned long long)n_views;
        if (rows >= (1ull << 31) || (cols + 255) / 256 >= (1ull << 31)) return VFA_ERR_UNSUPPORTED;
        s.col_end = cols; s.row_end = (unsigned)rows; s.view_end = (unsigned)views;
    }
    if (n_views == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scan_cols_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, sa);
    int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(scan_rows_kernel, dim3((unsigned)rows), dim3(kWave), 0, st, sa);
    e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(stats_view_kernel, dim3((unsigned)views), dim3(kCo), 0, st, sa);
    e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(stats_sum_kernel, dim3((unsigned)n_maps), dim3(kCo), 0, st, sa);
    return (int)hipGetLastError();
}

int vfa_lateral_conv_backward_f32(int n_maps, const float *const *dzs_hwc, const float *const *ys_hwc, const double *const *means,
                                  const float *const *feats, const float *const *weights, float *const *grad_feats,
                                  float *const *grad_weights, void *const *workspaces, const size_t *workspace_bytes, int n_views,
                                  const int *Ks, const int *feat_hw, void *stream)
{
    {
        const int st = shape_check(n_maps, n_views, Ks, feat_hw);
        if (st) return st;
    }
    if (!dzs_hwc || !ys_hwc || !means || !feats || !weights || !workspaces || !workspace_bytes) return VFA_ERR_BAD_ARGUMENT;
    ConvArgs ca;
    ca.n_maps = n_maps;
    ca.n_views = n_views;
    unsigned long long split = 0, fb = 0, wb = 0, red = 0;
    bool any_f = false, any_w = false;
    for (int m = 0; m < kMaxMaps; ++m) {
        ConvMap &c = ca.m[m];
        if (m >= n_maps) { c = ca.m[0]; c.split_end = (unsigned)split; c.feat_end = (unsigned)fb; c.dw_end = (unsigned)wb; c.red_end = red; continue; }
        const int K = Ks[m], H = feat_hw[2 * m], W = feat_hw[2 * m + 1];
        if (!dzs_hwc[m] || !ys_hwc[m] || !means[m] || !feats[m] || !weights[m]) return VFA_ERR_BAD_ARGUMENT;
        if (!aligned16(dzs_hwc[m]) || !aligned16(ys_hwc[m]) || !aligned16(workspaces[m])) return VFA_ERR_UNSUPPORTED;
        c.l = layout_of(n_views, K, H, W);
        if (n_views > 0 && (!workspaces[m] || workspace_bytes[m] < c.l.total)) return VFA_ERR_BAD_ARGUMENT;
        c.dz = dzs_hwc[m]; c.y = ys_hwc[m]; c.mean = means[m]; c.feat = feats[m]; c.w = weights[m];
        c.g_feat = grad_feats ? grad_feats[m] : nullptr;
        c.g_w = grad_weights ? grad_weights[m] : nullptr;
        c.ws = static_cast<unsigned char *>(workspaces[m]);
        c.K = K; c.HW = H * W;
        const int KB = K / 32;
        if (c.g_feat) {
            any_f = true;
            split += (unsigned long long)(kGc * KB * 64 + 255) / 256;
            fb += (unsigned long long)n_views * ((c.HW + 127) / 128) * ((KB + kKBlocks - 1) / kKBlocks);
        }
        if (c.g_w) {
            any_w = true;
            wb += (unsigned long long)n_views * c.l.parts * c.l.ktiles;
            red += (unsigned long long)kCo * K;
        }
        if (fb >= (1ull << 31) || wb >= (1ull << 31)) return VFA_ERR_UNSUPPORTED;
        c.split_end = (unsigned)split; c.feat_end = (unsigned)fb; c.dw_end = (unsigned)wb; c.red_end = red;
    }
    if (n_views == 0) {
        for (int m = 0; m < n_maps; ++m) // (no pixel: d W is zero)
            if (ca.m[m].g_w) {
                const hipError_t e = hipMemsetAsync(ca.m[m].g_w, 0, (size_t)kCo * Ks[m] * sizeof(float), (hipStream_t)stream);
                if (e != hipSuccess) return (int)e;
            }
        return 0;
    }
    hipStream_t st = (hipStream_t)stream;
    int e = 0;
    if (any_f) {
        hipLaunchKernelGGL(split_weight_t_kernel, dim3((unsigned)split), dim3(256), 0, st, ca);
        if ((e = (int)hipGetLastError())) return e;
        hipLaunchKernelGGL(grad_feat_kernel, dim3((unsigned)fb), dim3(256), 0, st, ca);
        if ((e = (int)hipGetLastError())) return e;
    }
    if (any_w) {
        hipLaunchKernelGGL(grad_weight_kernel, dim3((unsigned)wb), dim3(256), 0, st, ca);
        if ((e = (int)hipGetLastError())) return e;
        hipLaunchKernelGGL(grad_weight_reduce_kernel, dim3((unsigned)((red + 255) / 256)), dim3(256), 0, st, ca);
        if ((e = (int)hipGetLastError())) return e;
    }
    return 0;
}

} // extern "C"
