// vfa_geom_grad.hip -- the gradient of the box pooling with respect to the GEOMETRY: the camera matrices and the ground grid.
// The reference's VFA.forward (vfa/model/vfa_op.py:61-125) is a chain of stock torch ops, so autograd differentiates the BEV map
// with respect to `calib` and `grid` whenever they require grad; this is that derivative, per box (view, layer, cell):
//
//   vox = N / area * visible,   N = LT + RB - RT - LB,   P = bilinear sample of the (unbordered) integral image at a box corner
//   dS/dx = (W/2) [(1-fy)(ne-nw) + fy(se-sw)],  dS/dy = (H/2) [(1-fx)(sw-nw) + fx(se-ne)]          (ATen grid_sampler_2d_backward)
//   with g = dL/dvox, A_p = sum_c g dS_p/dx, B_p = sum_c g dS_p/dy, Q = sum_c g vox:
//     dl = (A_LT - A_LB)/area + Q (b-t) HW/area      dr = (A_RB - A_RT)/area - Q (b-t) HW/area
//     dt = (B_LT - B_RT)/area + Q (r-l) HW/area      db = (B_RB - B_LB)/area - Q (r-l) HW/area
//   l = min_k nu_k (t, r, b likewise): the gradient goes to the corner torch.min / max selects (lowest index on ties); the clamp
//   passes it where cmin <= nu_pre <= cmax; nu = 2u/img_w - 1, u = h0/h2, v = h1/h2, h = P [X 1]:
//     dh0 = du/h2, dh1 = dv/h2, dh2 = -(du u + dv v)/h2;  dP[r][j] += dh_r X_j;  dX = sum_r dh_r P[r][0:3]
//   d grid = dX times the conversion's scale (1 MultiviewC, 1/40 MultiviewX, 2.5 Wildtrack), summed over corners, layers and views.
//
// Layout of the work -- bit-reproducible, no float atomics:
//   * a wave owns a tile of kTileCells = 8 consecutive cells and walks (view, cell, layer) of them in that order, one box at a time;
//   * lane = (cell slot grp = lane / 8, corner k = lane % 8).  Every lane projects corner k of the box with the forward's fp32
//     sequence (project_corner_ex); l / t / r / b and their corners come from an exact min / max butterfly over the eight corners;
//   * the channel sums run with the lanes over channels (16-byte loads of the 16 tap rows and the d vox row); everything after the
//     sums is linear in them, so each lane turns its partial sums into partial dl / dr / dt / db and ONE butterfly of four values
//     gives the box's;
//   * the corner chain rule is lane k's; the lanes of cell slot grp == cell keep the result: d grid of the cell (over views, layers)
//     and d P of the view (over the tile's cells and layers) in registers;
//   * per (tile, view) the 12-vector is reduced over the wave in a fixed butterfly and stored into its own workspace slot; per tile
//     the cells' d grid is reduced over the eight corners and stored directly;
//   * a second kernel sums the slots of every (view, element) in slot order: thread t of 256 takes slots t, t + 256, ..., then a
//     fixed LDS tree.
// The result is a function of the inputs and shapes only.  Compiled with -ffp-contract=off like its siblings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vfa_hip.h"
#include "vfa_geom.h"

namespace {
using namespace vfa_dev;

constexpr int kTileCells = 8;     // cells per wave (one per group of eight lanes)
constexpr int kWavesPerBlock = 4;
constexpr int kReduceThreads = 256;

struct GeomGradDims {
    int n_views, C, Hf, Wf, nl, cell_begin, cell_count, tiles;
    int accumulate;
};

template <int VEC> struct vec_t;
template <> struct vec_t<1> { typedef float type; };
template <> struct vec_t<4> { typedef float4 type; };

__device__ __forceinline__ float comp(const float &v, int) { return v; }
__device__ __forceinline__ float comp(const float4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
__device__ __forceinline__ float group8_sum(float v)
{
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
// exact min / max with the corner index over the eight lanes of a group; ties go to the lower corner (what torch.min / max select)
__device__ __forceinline__ void group8_argmin(float &v, int &k)
{
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) {
        const float ov = __shfl_xor(v, m, kWave);
        const int ok = __shfl_xor(k, m, kWave);
        if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
}
__device__ __forceinline__ void group8_argmax(float &v, int &k)
{
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) {
        const float ov = __shfl_xor(v, m, kWave);
        const int ok = __shfl_xor(k, m, kWave);
        if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
}
__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int VEC>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void geom_grad_kernel(const float *__restrict__ grad_vox,
                                                                          const float *__restrict__ integral, BoxGeom g, GeomGradDims d,
                                                                          float *__restrict__ grad_grid, float *__restrict__ slots)
{
    typedef typename vec_t<VEC>::type V;
    const int lane = threadIdx.x & (kWave - 1);
    const int tile = blockIdx.x * kWavesPerBlock + uniform_i(threadIdx.x >> 6);
    if (tile >= d.tiles) return;
    const int grp = lane >> 3, kc = lane & 7;
    const int cl0 = tile * kTileCells;
    const int nc = min(kTileCells, d.cell_count - cl0);
    const size_t Wp = (size_t)d.Wf + 2;
    const size_t img_floats = (size_t)(d.Hf + 2) * Wp * d.C;
    const float hw = (float)d.Hf * (float)d.Wf;
    const float half_w = (float)d.Wf * 0.5f, half_h = (float)d.Hf * 0.5f;
    const float grid_scale = g.conv_kind == VFA_CONV_WILDTRACK ? 2.5f : 1.0f;
    float dg[3] = {0.0f, 0.0f, 0.0f}; // d grid of cell slot grp, corner kc

    for (int v = 0; v < d.n_views; ++v) {
        const float *P = g.calibs + (size_t)v * 12;
        float pm[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) pm[j] = P[j];
        float dP[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) dP[j] = 0.0f;
        const float *img = integral + (size_t)v * img_floats;
        for (int ci = 0; ci < nc; ++ci) {
            const int cl = cl0 + ci, cell = d.cell_begin + cl;
            const float gx = g.grid[cell * 3 + 0] + 0.0f; // (the forward's sequence: + the int64 zeros of z_corners)
            const float gy = g.grid[cell * 3 + 1] + 0.0f;
            const float gz0 = g.grid[cell * 3 + 2];
            for (int layer = 0; layer < d.nl; ++layer) {
                const float gz = gz0 + g.z_layers[layer];
                float nu, nv, nu_pre, nv_pre, X[3], h[3];
                project_corner_ex(g, pm, gx, gy, gz, kc, nu, nv, nu_pre, nv_pre, X, h);
                // a NaN corner makes the forward's box NaN: not visible
                if (__ballot(nu != nu || nv != nv) != 0ull) continue;
                float l = nu, r = nu, t = nv, b = nv;
                int kl = kc, kr = kc, kt = kc, kb = kc;
                group8_argmin(l, kl); group8_argmax(r, kr);
                group8_argmin(t, kt); group8_argmax(b, kb);
                l = uniform_f(l); r = uniform_f(r); t = uniform_f(t); b = uniform_f(b);
                kl = uniform_i(kl); kr = uniform_i(kr); kt = uniform_i(kt); kb = uniform_i(kb);
                const float area = box_area(l, t, r, b, d.Hf, d.Wf);
                if (!box_visible(area, d.Hf, d.Wf)) continue; // masked boxes pass nothing
                const Axis xl = make_axis(l, d.Wf), xr = make_axis(r, d.Wf);
                const Axis yt = make_axis(t, d.Hf), yb = make_axis(b, d.Hf);
                // tap rows / columns as float offsets inside the view's padded image: out-of-image taps land on the zero border
                const int xs[4] = {xl.i0, xl.i0 + 1, xr.i0, xr.i0 + 1};
                const int ys[4] = {yt.i0, yt.i0 + 1, yb.i0, yb.i0 + 1};
                size_t col[4], row[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    col[q] = (size_t)(min(max(xs[q], -1), d.Wf) + 1) * d.C;
                    row[q] = (size_t)(min(max(ys[q], -1), d.Hf) + 1) * Wp * d.C;
                }
                // points: 0 = (l,t), 1 = (r,b), 2 = (r,t), 3 = (l,b): rows (ri), columns (cj) of their nw tap, and their axes
                const int pr[4] = {0, 2, 0, 2}, pc[4] = {0, 2, 2, 0};
                const float xlo[4] = {xl.lo, xr.lo, xr.lo, xl.lo}, xhi[4] = {xl.hi, xr.hi, xr.hi, xl.hi};
                const float ylo[4] = {yt.lo, yb.lo, yt.lo, yb.lo}, yhi[4] = {yt.hi, yb.hi, yt.hi, yb.hi};
                float wgt[4][4];
                bilinear_weights(wgt[0], xl, yt);
                bilinear_weights(wgt[1], xr, yb);
                bilinear_weights(wgt[2], xr, yt);
                bilinear_weights(wgt[3], xl, yb);
                const float *gv = grad_vox + ((((size_t)v * d.cell_count + cl) * d.nl) + layer) * d.C;
                float A[4] = {0.0f, 0.0f, 0.0f, 0.0f}, B[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qn = 0.0f;
                for (int c = lane * VEC; c < d.C; c += kWave * VEC) {
                    const V gval = *reinterpret_cast<const V *>(gv + c);
                    V tap[4][4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float *r0 = img + row[pr[p]] + c, *r1 = img + row[pr[p] + 1] + c;
                        tap[p][0] = *reinterpret_cast<const V *>(r0 + col[pc[p]]);
                        tap[p][1] = *reinterpret_cast<const V *>(r0 + col[pc[p] + 1]);
                        tap[p][2] = *reinterpret_cast<const V *>(r1 + col[pc[p]]);
                        tap[p][3] = *reinterpret_cast<const V *>(r1 + col[pc[p] + 1]);
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float gc = comp(gval, i);
                        float n_acc = 0.0f;
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            const float nw = comp(tap[p][0], i), ne = comp(tap[p][1], i), sw = comp(tap[p][2], i), se = comp(tap[p][3], i);
                            const float s = wgt[p][0] * nw + wgt[p][1] * ne + wgt[p][2] * sw + wgt[p][3] * se;
                            const float dx = ylo[p] * (ne - nw) + yhi[p] * (se - sw);
                            const float dy = xlo[p] * (sw - nw) + xhi[p] * (se - ne);
                            A[p] += gc * dx;
                            B[p] += gc * dy;
                            n_acc += (p < 2) ? s : -s;
                        }
                        qn += gc * n_acc;
                    }
                }
                // partial dl / dr / dt / db of this lane's channels (linear in the sums), then one butterfly
                const float inv = 1.0f / area;
                const float qa = qn * inv; // sum_c g vox
                const float wy = qa * ((b - t) * hw), wx = qa * ((r - l) * hw);
                float gl = ((A[0] - A[3]) * half_w + wy) * inv;
                float gr = ((A[1] - A[2]) * half_w - wy) * inv;
                float gt = ((B[0] - B[2]) * half_h + wx) * inv;
                float gb = ((B[1] - B[3]) * half_h - wx) * inv;
                gl = wave_sum(gl); gr = wave_sum(gr); gt = wave_sum(gt); gb = wave_sum(gb);
                // corner kc: which of l / r / t / b it carries, through the clamp, the normalisation and the division
                float dnu = (kc == kl ? gl : 0.0f) + (kc == kr ? gr : 0.0f);
                float dnv = (kc == kt ? gt : 0.0f) + (kc == kb ? gb : 0.0f);
                if (!(g.cmin <= nu_pre && nu_pre <= g.cmax)) dnu = 0.0f;
                if (!(g.cmin <= nv_pre && nv_pre <= g.cmax)) dnv = 0.0f;
                if (grp == ci && (dnu != 0.0f || dnv != 0.0f)) {
                    const float du = dnu * 2.0f / g.img_w, dv = dnv * 2.0f / g.img_h;
                    const float u = h[0] / h[2], w = h[1] / h[2];
                    const float dh[3] = {du / h[2], dv / h[2], -(du * u + dv * w) / h[2]};
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) {
                        dP[rr * 4 + 0] += dh[rr] * X[0];
                        dP[rr * 4 + 1] += dh[rr] * X[1];
                        dP[rr * 4 + 2] += dh[rr] * X[2];
                        dP[rr * 4 + 3] += dh[rr];
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        float s = dh[0] * pm[j] + dh[1] * pm[4 + j];
                        s = s + dh[2] * pm[8 + j];
                        dg[j] += g.conv_kind == VFA_CONV_MULTIVIEWX ? s / 40.0f : s * grid_scale;
                    }
                }
            }
        }
        if (slots) { // this (tile, view)'s 12-vector: a fixed butterfly over the wave, into its own slot
            float *dst = slots + ((size_t)tile * d.n_views + v) * 12;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const float s = wave_sum(dP[j]);
                if (lane == 0) dst[j] = s;
            }
        }
    }
    if (grad_grid) { // d grid of the tile's cells: the eight corners of a slot in a fixed butterfly
#pragma unroll
        for (int j = 0; j < 3; ++j) dg[j] = group8_sum(dg[j]);
        if (kc == 0 && grp < nc) {
            float *dst = grad_grid + (size_t)(cl0 + grp) * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[j] = d.accumulate ? dst[j] + dg[j] : dg[j];
        }
    }
}

// grad_calibs[v][j] (+)= sum over tiles of slots[tile][v][j]: one workgroup per (v, j); thread t adds slots t, t + 256, ... in order,
// then a fixed LDS tree.  Exactly one add into grad_calibs when accumulating.
__global__ __launch_bounds__(kReduceThreads) void geom_calib_reduce_kernel(const float *__restrict__ slots, float *__restrict__ grad_calibs,
                                                                          int n_views, int tiles, int accumulate)
{
    __shared__ float s_sum[kReduceThreads];
    const int vj = blockIdx.x, v = vj / 12, j = vj % 12, t = threadIdx.x;
    float s = 0.0f;
    for (int k = t; k < tiles; k += kReduceThreads) s += slots[((size_t)k * n_views + v) * 12 + j];
    s_sum[t] = s;
    __syncthreads();
#pragma unroll
    for (int off = kReduceThreads / 2; off > 0; off >>= 1) {
        if (t < off) s_sum[t] = s_sum[t] + s_sum[t + off];
        __syncthreads();
    }
    if (t == 0) {
        float *dst = grad_calibs + (size_t)v * 12 + j;
        *dst = accumulate ? *dst + s_sum[0] : s_sum[0];
    }
}

// Zero n floats with a kernel (any size, any 4-byte alignment): the rare empty-range call stays a kernel node inside captured graphs.
__global__ __launch_bounds__(256) void zero_floats_kernel(float *p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0.0f;
}
inline int zero_floats(float *p, size_t n, hipStream_t s)
{
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(zero_floats_kernel, dim3(blocks), dim3(256), 0, s, p, n);
    return (int)hipGetLastError();
}

inline int tiles_of(int cell_count) { return (cell_count + kTileCells - 1) / kTileCells; }

} // namespace

extern "C" {

size_t vfa_gather_backward_geometry_workspace_bytes(int n_views, int cell_count)
{
    if (n_views <= 0 || cell_count <= 0) return 0;
    const size_t bytes = (size_t)tiles_of(cell_count) * n_views * 12 * sizeof(float);
    return (bytes + 255) / 256 * 256;
}

int vfa_project_gather_backward_geometry_f32(const float *grad_vox, const float *integral, const float *calibs, const float *grid,
                                             const float *z_layers, const float *corner_off, float *grad_calibs, float *grad_grid,
                                             int n_views, int C, int Hf, int Wf, int nl, int n_cells, int cell_begin, int cell_count,
                                             int conv_kind, float img_w, float img_h, float cmin, float cmax, int flags, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    if (flags & ~VFA_BWD_ACCUMULATE) return VFA_ERR_BAD_ARGUMENT;
    if (n_views < 0 || C <= 0 || Hf <= 0 || Wf <= 0 || nl <= 0 || n_cells < 0 || cell_begin < 0 || cell_count < 0 ||
        cell_begin + cell_count > n_cells || conv_kind < 0 || conv_kind > 2)
        return VFA_ERR_BAD_ARGUMENT;
    if (!grad_calibs && !grad_grid) return 0;
    const int accumulate = flags & VFA_BWD_ACCUMULATE;
    hipStream_t s = (hipStream_t)stream;
    const bool boxes = n_views > 0 && cell_count > 0;
    if (!boxes) { // nothing to differentiate: the outputs are zero (or left as they are); a kernel, not a memset node (see zero_fill, vfa_geom.h)
        if (!accumulate && grad_calibs && n_views > 0) {
            const int e = zero_floats(grad_calibs, (size_t)n_views * 12, s);
            if (e) return e;
        }
        if (!accumulate && grad_grid && cell_count > 0) {
            const int e = zero_floats(grad_grid, (size_t)cell_count * 3, s);
            if (e) return e;
        }
        return 0;
    }
    if (!grad_vox || !integral || !calibs || !grid || !z_layers || !corner_off) return VFA_ERR_BAD_ARGUMENT;
    if ((long long)n_views * cell_count * nl * C >= (1ll << 40)) return VFA_ERR_BAD_ARGUMENT;
    if (grad_calibs && (!workspace || workspace_bytes < vfa_gather_backward_geometry_workspace_bytes(n_views, cell_count)))
        return VFA_ERR_BAD_ARGUMENT;
    BoxGeom g{calibs, grid, z_layers, corner_off, conv_kind, img_w, img_h, cmin, cmax};
    GeomGradDims d;
    d.n_views = n_views; d.C = C; d.Hf = Hf; d.Wf = Wf; d.nl = nl; d.cell_begin = cell_begin; d.cell_count = cell_count;
    d.tiles = tiles_of(cell_count); d.accumulate = accumulate;
    float *slots = grad_calibs ? reinterpret_cast<float *>(workspace) : nullptr;
    const unsigned blocks = (unsigned)((d.tiles + kWavesPerBlock - 1) / kWavesPerBlock);
    const bool vec4 = (C % 4) == 0 && ((reinterpret_cast<uintptr_t>(grad_vox) | reinterpret_cast<uintptr_t>(integral)) & 15) == 0;
    if (vec4)
        hipLaunchKernelGGL(geom_grad_kernel<4>, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, s, grad_vox, integral, g, d, grad_grid, slots);
    else
        hipLaunchKernelGGL(geom_grad_kernel<1>, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, s, grad_vox, integral, g, d, grad_grid, slots);
    int e = (int)hipGetLastError();
    if (e || !grad_calibs) return e;
    hipLaunchKernelGGL(geom_calib_reduce_kernel, dim3((unsigned)(n_views * 12)), dim3(kReduceThreads), 0, s, slots, grad_calibs, n_views,
                       d.tiles, accumulate);
    return (int)hipGetLastError();
}

} // extern "C"
