// vfa_heat.hip -- the dense heat-map target of a training step rendered from the packed object tensors: the reference's
// RotationGaussianKernel and GaussianKernel (vfa/data/GK.py), which its datasets compute once on the host and cache.  The rules and
// the per-element arithmetic: vfa_heat.h; the cell of an object: vfa_loss.h (the target encoder's).
//
//   vfa_heat_rgk_f32   a memset of the map and of n_clipped, then heat_rgk_kernel, ONE WORKGROUP PER (object slot, frame): the taps
//                      once into LDS, the rotated kernel into a second LDS plane, the workgroup's arg-max, the paste.  Objects meet in
//                      the map through an INTEGER max on the bit patterns (the values are >= 0: unsigned order is float order), the
//                      centre through a max with the bits of 1: the map does not depend on the order of the objects or of the
//                      workgroups.  No float atomics.
//   vfa_heat_gk_f32    a memset of the occupancy bytes (the workspace), heat_occupancy_kernel (one thread per object slot, plain
//                      idempotent stores: a duplicate counts once), heat_gk_kernel (one thread per cell, the table in LDS, float64 sum
//                      in raster order).
// Everything is stream-ordered (memset nodes and kernel nodes under capture); a frame of a batch has the bits of its single-frame call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"
#include "vfa_heat.h"
#include "vfa_loss.h"

namespace {

using namespace vfa_heat;

constexpr int kRgkThreads = 256, kGkThreads = 256, kOccThreads = 256;
static_assert(kMaxKernel == VFA_HEAT_MAX_KERNEL && kMaxRadius == VFA_HEAT_MAX_RADIUS, "include/vfa_hip.h and vfa_heat.h disagree");

struct HeatArgs {
    const float *location, *dimension, *table;
    const double *angle_deg;
    const int *count;
    int loc_width, K, L, W, kind, ratio, r;
    float world0, world1;
    double alpha;
    unsigned char *occ;  // (B, L, W)
    float *heat;         // (B, L, W)
    int *n_clipped;      // (B)
};

__device__ __forceinline__ int live_count(const HeatArgs &a, int b)
{
    const int n = a.count[b];
    return n < 0 ? 0 : (n > a.K ? a.K : n);
}

__device__ __forceinline__ int cell_of(const HeatArgs &a, int b, int i)
{
    const float *loc = a.location + ((size_t)b * a.K + i) * a.loc_width;
    return vfa_loss::assign_cell(loc[0], loc[1], a.world0, a.world1, a.L, a.W, a.kind).cell;
}

__global__ __launch_bounds__(kRgkThreads) void heat_rgk_kernel(const HeatArgs a)
{
    __shared__ float taps[kMaxKernel * kMaxKernel], rot[kMaxKernel * kMaxKernel];
    __shared__ unsigned long long wave_best[kRgkThreads / 64];

    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (i >= live_count(a, b)) return;  // (uniform over the workgroup, as every return below)
    const int cell = cell_of(a, b, i);
    if (cell < 0) return;               // dropped, as by the target encoder
    unsigned int *map = (unsigned int *)(a.heat + (size_t)b * a.L * a.W);
    const float *dim = a.dimension + ((size_t)b * a.K + i) * 3;  // (h, w, l)
    const Kernel g = kernel_of(dim[2], dim[1], a.alpha, a.ratio);
    const Turn t = turn_of(a.angle_deg[(size_t)b * a.K + i]);
    if (!g.ok || !t.ok) {
        if (tid == 0) {
            atomicMax(map + cell, kOneBits);
            atomicAdd(a.n_clipped + b, 1);
        }
        return;
    }
    const int n = g.n, cells = n * n;  // (n <= kMaxKernel)
    for (int e = tid; e < cells; e += kRgkThreads) {
        const int r = e / n;
        taps[e] = tap(g, r, e - r * n);
    }
    __syncthreads();
    unsigned long long best = 0;  // (below every key: index_of_key(0) is no index)
    for (int e = tid; e < cells; e += kRgkThreads) {
        const int r = e / n;
        const float v = rotated(taps, n, r, e - r * n, t);
        rot[e] = v;
        const unsigned long long key = rank_key(v, e);
        best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(best, o, 64);
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();  // (also: rot is complete)
    best = wave_best[0];
    for (int w = 1; w < kRgkThreads / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    const int at = index_of_key(best), g_t = at / n, g_l = at - g_t * n;
    const int row = cell / a.W, col = cell - row * a.W;
    for (int e = tid; e < cells; e += kRgkThreads) {
        const uint32_t bits = pasted(rot[e]);
        if (bits == 0) continue;
        const int r = e / n;
        const int to = paste_cell(row, col, g_t, g_l, r, e - r * n, a.L, a.W);
        if (to >= 0) atomicMax(map + to, bits);
    }
    if (tid == 0) atomicMax(map + cell, kOneBits);
}

__global__ __launch_bounds__(kOccThreads) void heat_occupancy_kernel(const HeatArgs a)
{
    const int i = blockIdx.x * kOccThreads + threadIdx.x, b = blockIdx.y;
    if (i >= live_count(a, b)) return;
    const int cell = cell_of(a, b, i);
    if (cell >= 0) a.occ[(size_t)b * a.L * a.W + cell] = 1;
}

__global__ __launch_bounds__(kGkThreads) void heat_gk_kernel(const HeatArgs a)
{
    __shared__ float table[(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1)];
    const int side = 2 * a.r + 1, b = blockIdx.y, n_cells = a.L * a.W;
    for (int e = threadIdx.x; e < side * side; e += kGkThreads) table[e] = a.table[e];
    __syncthreads();
    const int i = blockIdx.x * kGkThreads + threadIdx.x;
    if (i >= n_cells) return;
    const int y = i / a.W;
    a.heat[(size_t)b * n_cells + i] = gk_cell(a.occ + (size_t)b * n_cells, table, a.r, a.L, a.W, y, i - y * a.W);
}

// what both entry points check alike; 0: go on, *empty: nothing to do
int check_heat_shapes(const float *location, int loc_width, const int *count, int B, int K, int L, int W, float world0, float world1,
                      int kind, const float *heat, bool *empty)
{
    *empty = false;
    if (B < 0 || K < 0 || L < 0 || W < 0 || (loc_width != 2 && loc_width != 3) || kind < 0 || kind > 2) return VFA_ERR_BAD_ARGUMENT;
    if (!(world0 > 0.0f) || !(world1 > 0.0f)) return VFA_ERR_BAD_ARGUMENT;
    if (K > vfa_loss::kMaxObjects) return VFA_ERR_UNSUPPORTED;
    if (B == 0 || L == 0 || W == 0) {
        *empty = true;
        return 0;
    }
    if (B > 65535 || (long long)L * W > INT32_MAX - 1024) return VFA_ERR_UNSUPPORTED;  // (a thread's cell index stays an int)
    if (!count || !heat || (K > 0 && !location)) return VFA_ERR_BAD_ARGUMENT;
    return 0;
}

}  // namespace

extern "C" {

size_t vfa_heat_workspace_bytes(int B, int L, int W)
{
    if (B <= 0 || L <= 0 || W <= 0) return 0;
    return ((size_t)B * (size_t)L * (size_t)W + 7) / 8 * 8;  // one occupancy byte per cell
}

int vfa_heat_rgk_f32(const float *location, int loc_width, const int *count, const float *dimension, const double *angle_deg, int B,
                     int K, int L, int W, float world0, float world1, int kind, double alpha, int ratio, float *heat, int *n_clipped,
                     void *stream)
{
    bool empty;
    const int status = check_heat_shapes(location, loc_width, count, B, K, L, W, world0, world1, kind, heat, &empty);
    if (status != 0 || empty) return status;
    if (!n_clipped || (K > 0 && (!dimension || !angle_deg))) return VFA_ERR_BAD_ARGUMENT;
    if (!(alpha > 0.0) || ratio < 1 || ratio > 1024) return VFA_ERR_BAD_ARGUMENT;

    HeatArgs a = {};
    a.location = location;
    a.dimension = dimension;
    a.angle_deg = angle_deg;
    a.count = count;
    a.loc_width = loc_width;
    a.K = K;
    a.L = L;
    a.W = W;
    a.kind = kind;
    a.ratio = ratio;
    a.world0 = world0;
    a.world1 = world1;
    a.alpha = alpha;
    a.heat = heat;
    a.n_clipped = n_clipped;
    hipError_t err = hipMemsetAsync(heat, 0, (size_t)B * L * W * sizeof(float), (hipStream_t)stream);
    if (err == hipSuccess) err = hipMemsetAsync(n_clipped, 0, (size_t)B * sizeof(int), (hipStream_t)stream);
    if (err != hipSuccess) return (int)err;
    if (K > 0) hipLaunchKernelGGL(heat_rgk_kernel, dim3(K, B), dim3(kRgkThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int vfa_heat_gk_f32(const float *location, int loc_width, const int *count, const float *table, int r, int B, int K, int L, int W,
                    float world0, float world1, int kind, void *workspace, size_t workspace_bytes, float *heat, void *stream)
{
    bool empty;
    const int status = check_heat_shapes(location, loc_width, count, B, K, L, W, world0, world1, kind, heat, &empty);
    if (status != 0 || empty) return status;
    if (r < 0 || !table) return VFA_ERR_BAD_ARGUMENT;
    if (r > kMaxRadius) return VFA_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < vfa_heat_workspace_bytes(B, L, W)) return VFA_ERR_BAD_ARGUMENT;

    HeatArgs a = {};
    a.location = location;
    a.table = table;
    a.count = count;
    a.loc_width = loc_width;
    a.K = K;
    a.L = L;
    a.W = W;
    a.kind = kind;
    a.r = r;
    a.world0 = world0;
    a.world1 = world1;
    a.occ = (unsigned char *)workspace;
    a.heat = heat;
    const size_t n_cells = (size_t)L * W;
    const hipError_t err = hipMemsetAsync(workspace, 0, (size_t)B * n_cells, (hipStream_t)stream);
    if (err != hipSuccess) return (int)err;
    if (K > 0) hipLaunchKernelGGL(heat_occupancy_kernel, dim3((K + kOccThreads - 1) / kOccThreads, B), dim3(kOccThreads), 0, (hipStream_t)stream, a);
    const int groups = (int)((n_cells + kGkThreads - 1) / kGkThreads);
    hipLaunchKernelGGL(heat_gk_kernel, dim3(groups, B), dim3(kGkThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
