// vfa_det.hip -- hand-written HIP (gfx950 / CDNA4, wave64) kernels of the bit-reproducible training backward, behind the C ABI
// of include/vfa_hip.h: used when the caller asks for determinism (torch.use_deterministic_algorithms(True) on the Python side).
//
//   vfa_project_gather_backward_det_f32   d vox -> d integral without float atomics: "store, then sum per destination".
//       1. emit     every (view, cell, layer) box writes its 16 taps as (tap key, record index) + coefficient +-w/area into FIXED
//                   slots (record index = 16 box + tap); a masked box writes a sentinel key that sorts last;
//       2. sort     stable LSD radix sort of the 64-bit words (key << 32 | record) on the key: 8-bit digits, per-workgroup digit
//                   counts, an exclusive scan of the counts (digit-major), stable in-workgroup ranks from wave ballots;
//       3. merge    one wave per PIECE of kPiece sorted positions: lanes over channels, every record gathers its grad_vox row and
//                   the sum of a key runs in list order; a key whose list lies inside one piece is stored straight away;
//       4. fix-up   a key whose list crosses pieces left its first piece's sum in `tail` and the others in `head`: the wave of
//                   the piece where the list ends adds them in piece order and stores the result.
//   Every grid is a function of the shapes, every order a function of the data: the result does not depend on timing,
//   workgroup count or placement.
//
//   vfa_column_sum_f32   column sums in a fixed order (d bias without atomics).
//
// Compiled with -ffp-contract=off: an FMA appears only where fmaf() is written.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "vfa_hip.h"

#include "vfa_geom.h"

namespace {
using namespace vfa_dev;

constexpr int kSortRounds = 16;                   // rounds of 64 elements per sort workgroup (one wave)
constexpr int kSortTile = kWave * kSortRounds;    // elements per sort workgroup
constexpr int kScanTile = 256 * 16;               // counts per scan workgroup
constexpr int kPiece = 256;                       // sorted positions per merge wave
constexpr int kAhead = 8;                         // gradient rows a merge wave has in flight
constexpr unsigned long long kNoRec = 0ull;       // (a record index is never read past the end: see merge)

// ------------------------------------------------------------------------------------------------
// workspace layout (host): every region 256-byte aligned
// ------------------------------------------------------------------------------------------------
struct DetLayout {
    long long n_boxes, n_rec, sort_blocks, n_counts, scan_blocks, n_pieces;
    unsigned sentinel;
    int passes, cblocks;
    size_t keys_a, keys_b, coef, counts, sums, head, tail, total;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// false: shapes outside what the 32-bit keys and record indices hold (the callers chunk cells long before that)
inline bool det_layout(DetLayout &L, int n_views, int nl, int cell_count, int C, int Hf, int Wf)
{
    if (n_views < 0 || nl <= 0 || cell_count < 0 || C <= 0 || Hf <= 0 || Wf <= 0) return false;
    L.n_boxes = (long long)n_views * nl * cell_count;
    L.n_rec = 16 * L.n_boxes;
    const unsigned long long keys = (unsigned long long)n_views * (unsigned long long)(Hf + 2) * (unsigned long long)(Wf + 2);
    if (L.n_rec >= (1ll << 31) || keys >= 0xffffffffull) return false;
    L.sentinel = (unsigned)keys; // one past the last tap of the last view
    int bits = 1;
    while (bits < 32 && (L.sentinel >> bits) != 0u) ++bits;
    L.passes = (bits + 7) / 8;
    L.sort_blocks = (L.n_rec + kSortTile - 1) / kSortTile;
    L.n_counts = 256 * L.sort_blocks;
    L.scan_blocks = (L.n_counts + kScanTile - 1) / kScanTile;
    L.n_pieces = (L.n_rec + kPiece - 1) / kPiece;
    L.cblocks = C % 4 == 0 ? (C + 4 * kWave - 1) / (4 * kWave) : (C + kWave - 1) / kWave;
    size_t o = 0;
    L.keys_a = o; o = align256(o + (size_t)L.n_rec * 8);
    L.keys_b = o; o = align256(o + (size_t)L.n_rec * 8);
    L.coef = o;   o = align256(o + (size_t)L.n_rec * 4);
    L.counts = o; o = align256(o + (size_t)L.n_counts * 4);
    L.sums = o;   o = align256(o + (size_t)L.scan_blocks * 4);
    L.head = o;   o = align256(o + (size_t)L.n_pieces * C * 4);
    L.tail = o;   o = align256(o + (size_t)L.n_pieces * C * 4);
    L.total = o;
    return true;
}

// ------------------------------------------------------------------------------------------------
// 1. emit: one thread per box, box b = (view * cell_count + cell_local) * nl + layer = its row of the layer-major grad_vox
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void det_emit_kernel(BoxGeom g, int nl, int cell_begin, int cell_count, int Hf, int Wf,
                                                       long long n_boxes, unsigned sentinel, unsigned long long *__restrict__ keys,
                                                       float *__restrict__ coef)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_boxes) return;
    const int layer = (int)(b % nl);
    const long long vc = b / nl;
    const int cell = cell_begin + (int)(vc % cell_count), view = (int)(vc / cell_count);
    float l, t, r, bt;
    cube_box(g, g.calibs + (size_t)view * 12, cell, layer, l, t, r, bt); // the forward's box
    const float area = box_area(l, t, r, bt, Hf, Wf);
    const unsigned long long rec0 = (unsigned long long)(16 * b);
    unsigned long long *kb = keys + 16 * b;
    float *cb = coef + 16 * b;
    if (!box_visible(area, Hf, Wf)) { // masked voxels pass no gradient (and their grad_vox is never read)
#pragma unroll
        for (int i = 0; i < 16; ++i) { kb[i] = ((unsigned long long)sentinel << 32) | (rec0 + i); cb[i] = 0.0f; }
        return;
    }
    // taps and weights exactly as the pooling kernels form them (fill_record, vfa_kernels.hip): out-of-image taps land on the border
    const Axis xl = make_axis(l, Wf), xr = make_axis(r, Wf), yt = make_axis(t, Hf), yb = make_axis(bt, Hf);
    const int xs[4] = {xl.i0, xl.i0 + 1, xr.i0, xr.i0 + 1}, ys[4] = {yt.i0, yt.i0 + 1, yb.i0, yb.i0 + 1};
    unsigned col[4], row[4];
    const unsigned Wp = (unsigned)Wf + 2u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        col[k] = (unsigned)(min(max(xs[k], -1), Wf) + 1);
        row[k] = ((unsigned)view * ((unsigned)Hf + 2u) + (unsigned)(min(max(ys[k], -1), Hf) + 1)) * Wp;
    }
    float wlt[4], wrb[4], wrt[4], wlb[4];
    bilinear_weights(wlt, xl, yt);
    bilinear_weights(wrb, xr, yb);
    bilinear_weights(wrt, xr, yt);
    bilinear_weights(wlb, xl, yb);
    // (((lt + rb) - rt) - lb) / area: tap (row, col) of sample s gets +-w_s / area, in the order of the atomic kernels
    const int tr[16] = {0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2, 3, 3};
    const int tc[16] = {0, 1, 0, 1, 2, 3, 2, 3, 2, 3, 2, 3, 0, 1, 0, 1};
    const float w[16] = {wlt[0], wlt[1], wlt[2], wlt[3], wrb[0], wrb[1], wrb[2], wrb[3],
                         -wrt[0], -wrt[1], -wrt[2], -wrt[3], -wlb[0], -wlb[1], -wlb[2], -wlb[3]};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        kb[i] = ((unsigned long long)(row[tr[i]] + col[tc[i]]) << 32) | (rec0 + i);
        cb[i] = w[i] / area;
    }
}

// ------------------------------------------------------------------------------------------------
// 2. radix sort pass on key bits [shift, shift + 8): one wave per tile of kSortTile consecutive elements
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned digit_of(unsigned long long e, int shift) { return (unsigned)(e >> (32 + shift)) & 255u; }

__global__ __launch_bounds__(kWave) void det_hist_kernel(const unsigned long long *__restrict__ in, long long n, int shift,
                                                         long long n_blocks, unsigned *__restrict__ counts)
{
    __shared__ unsigned cnt[256];
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[lane + 64 * k] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const long long i = base + r * kWave + lane;
        if (i < n) atomicAdd(&cnt[digit_of(in[i], shift)], 1u); // (integer counts: the order of the adds does not matter)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) counts[(size_t)(lane + 64 * k) * n_blocks + blockIdx.x] = cnt[lane + 64 * k];
}

__global__ __launch_bounds__(kWave) void det_scatter_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                            long long n, int shift, long long n_blocks, const unsigned *__restrict__ offsets)
{
    __shared__ unsigned base[256], cnt[256];
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        base[lane + 64 * k] = offsets[(size_t)(lane + 64 * k) * n_blocks + blockIdx.x];
        cnt[lane + 64 * k] = 0u;
    }
    __syncthreads();
    const long long tile0 = (long long)blockIdx.x * kSortTile;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    for (int r = 0; r < kSortRounds; ++r) {
        const long long i = tile0 + r * kWave + lane;
        const bool valid = i < n;
        const unsigned long long e = valid ? in[i] : 0ull;
        const unsigned d = digit_of(e, shift);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long m = __ballot((d >> bit) & 1u);
            peers &= ((d >> bit) & 1u) ? m : ~m;
        }
        const unsigned before = cnt[d];
        __syncthreads();
        // stable: lanes of one digit in lane order, after every earlier round of the tile
        if (valid && (peers >> lane) == 1ull) cnt[d] = before + (unsigned)__popcll(peers); // the highest lane of its digit
        __syncthreads();
        const unsigned long long pos = (unsigned long long)base[d] + before + (unsigned)__popcll(peers & lt_mask);
        if (valid && pos < (unsigned long long)n) out[pos] = e;
    }
}

// Exclusive scan of n 32-bit counts in place: tile sums, a scan of the tile sums, the tiles again.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *red, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) red[wave] = x;
    __syncthreads();
    unsigned off = 0u, tot = 0u;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) off += red[w];
        tot += red[w];
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

__global__ __launch_bounds__(256) void det_scan_reduce_kernel(const unsigned *__restrict__ a, long long n, unsigned *__restrict__ sums)
{
    __shared__ unsigned red[4];
    const long long i0 = (long long)blockIdx.x * kScanTile + threadIdx.x * 16;
    unsigned s = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (i0 + k < n) s += a[i0 + k];
    unsigned total;
    block_exclusive_scan(s, red, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void det_scan_top_kernel(unsigned *__restrict__ sums, long long n)
{
    __shared__ unsigned red[16];
    unsigned carry = 0u;
    for (long long b = 0; b < n; b += 1024) {
        const long long i = b + threadIdx.x;
        const unsigned v = i < n ? sums[i] : 0u;
        unsigned total;
        const unsigned ex = block_exclusive_scan(v, red, total);
        if (i < n) sums[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void det_scan_down_kernel(unsigned *__restrict__ a, long long n, const unsigned *__restrict__ sums)
{
    __shared__ unsigned red[4];
    const long long i0 = (long long)blockIdx.x * kScanTile + threadIdx.x * 16;
    unsigned v[16], s = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v[k] = i0 + k < n ? a[i0 + k] : 0u;
        s += v[k];
    }
    unsigned total;
    unsigned run = sums[blockIdx.x] + block_exclusive_scan(s, red, total);
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (i0 + k < n) { a[i0 + k] = run; run += v[k]; }
}

// ------------------------------------------------------------------------------------------------
// 3. merge: wave = piece q (positions [q kPiece, (q + 1) kPiece) of the sorted array) x a block of 64 VEC channels
// ------------------------------------------------------------------------------------------------
template <int VEC> struct vecf;
template <> struct vecf<1> {
    typedef float type;
    static __device__ __forceinline__ float zero() { return 0.0f; }
};
template <> struct vecf<4> {
    typedef float4 type;
    static __device__ __forceinline__ float4 zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
};
__device__ __forceinline__ float vfmaf(float c, float g, float a) { return fmaf(c, g, a); }
__device__ __forceinline__ float4 vfmaf(float c, float4 g, float4 a)
{
    return make_float4(fmaf(c, g.x, a.x), fmaf(c, g.y, a.y), fmaf(c, g.z, a.z), fmaf(c, g.w, a.w));
}
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

struct MergeArgs {
    const unsigned long long *sorted;
    const float *coef, *grad_vox;
    float *head, *tail, *out;
    long long n_rec, n_pieces;
    unsigned sentinel;
    int C, accumulate;
};

__device__ __forceinline__ unsigned key_at(const MergeArgs &m, long long i) { return (unsigned)(m.sorted[i] >> 32); }

template <int VEC>
__device__ __forceinline__ void store_result(const MergeArgs &m, unsigned key, int c, typename vecf<VEC>::type s)
{
    using V = typename vecf<VEC>::type;
    V *p = reinterpret_cast<V *>(m.out + (size_t)key * m.C + c);
    *p = m.accumulate ? vadd(*p, s) : s; // accumulate: exactly one add per element
}

template <int VEC>
__global__ __launch_bounds__(kWave) void det_merge_kernel(MergeArgs m)
{
    using V = typename vecf<VEC>::type;
    const int lane = threadIdx.x;
    const long long q = blockIdx.x;
    const int c = (blockIdx.y * kWave + lane) * VEC;
    const bool active = c < m.C;
    const int cc = active ? c : 0; // (inactive lanes load channel 0 and store nothing)
    const long long a = q * kPiece, b = min(a + kPiece, m.n_rec);
    const unsigned key_prev = a > 0 ? key_at(m, a - 1) : 0xffffffffu;
    const unsigned key_next = b < m.n_rec ? key_at(m, b) : 0xffffffffu;
    unsigned cur = 0xffffffffu;
    long long start = a;
    V acc = vecf<VEC>::zero();
    auto flush = [&](long long end) {
        const bool before = start == a && key_prev == cur, after = end == b && key_next == cur;
        if (before) { if (active) *reinterpret_cast<V *>(m.head + (size_t)q * m.C + c) = acc; }
        else if (after) { if (active) *reinterpret_cast<V *>(m.tail + (size_t)q * m.C + c) = acc; }
        else if (active) store_result<VEC>(m, cur, c, acc);
    };
    for (long long j0 = a; j0 < b; j0 += kWave) {
        // lane k holds position j0 + k: its word and its coefficient; then the wave walks them with scalar reads
        const long long jl = j0 + lane;
        const unsigned long long e = jl < b ? m.sorted[jl] : ((unsigned long long)m.sentinel << 32) | kNoRec;
        const float cf = jl < b ? m.coef[min((unsigned)e, (unsigned)(m.n_rec - 1))] : 0.0f;
        const int cnt = (int)min((long long)kWave, b - j0);
        const int e_lo = (int)(unsigned)e, e_hi = (int)(unsigned)(e >> 32), cf_i = __float_as_int(cf);
        for (int k0 = 0; k0 < cnt; k0 += kAhead) {
            // the rows of the next kAhead positions first (independent loads in flight), then the sums in list order
            V g[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const unsigned rec = min((unsigned)__builtin_amdgcn_readlane(e_lo, min(k0 + u, cnt - 1)), (unsigned)(m.n_rec - 1));
                g[u] = *reinterpret_cast<const V *>(m.grad_vox + (size_t)(rec >> 4) * m.C + cc); // (in range by construction)
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int k = k0 + u;
                if (k >= cnt) break;
                const unsigned key = (unsigned)__builtin_amdgcn_readlane(e_hi, k);
                if (key >= m.sentinel) { // masked boxes sort last: nothing more in this piece
                    if (cur != 0xffffffffu) flush(j0 + k);
                    return;
                }
                if (key != cur) {
                    if (cur != 0xffffffffu) flush(j0 + k);
                    cur = key; start = j0 + k; acc = vecf<VEC>::zero();
                }
                acc = vfmaf(__int_as_float(__builtin_amdgcn_readlane(cf_i, k)), g[u], acc);
            }
        }
    }
    if (cur != 0xffffffffu) flush(b);
}

// 4. fix-up: the wave of the piece in which a multi-piece list ends adds the list's piece sums in piece order
template <int VEC>
__global__ __launch_bounds__(kWave) void det_fixup_kernel(MergeArgs m)
{
    using V = typename vecf<VEC>::type;
    const long long q = blockIdx.x;
    const int c = (blockIdx.y * kWave + threadIdx.x) * VEC;
    const long long a = q * kPiece;
    if (a == 0) return;
    const long long b = min(a + kPiece, m.n_rec);
    const unsigned kf = key_at(m, a);
    if (kf >= m.sentinel || key_at(m, a - 1) != kf) return;            // no list continues into this piece
    if (key_at(m, b - 1) == kf && b < m.n_rec && key_at(m, b) == kf) return; // ... or it goes on past it
    long long qa = q - 1;
    while (qa > 0 && key_at(m, qa * kPiece - 1) == kf) --qa;            // the piece where the list starts (its sum is in `tail`)
    if (c >= m.C) return;
    V s = *reinterpret_cast<const V *>(m.tail + (size_t)qa * m.C + c);
    for (long long j = qa + 1; j <= q; ++j) s = vadd(s, *reinterpret_cast<const V *>(m.head + (size_t)j * m.C + c));
    store_result<VEC>(m, kf, c, s);
}

// ------------------------------------------------------------------------------------------------
// column sums: a workgroup owns 64 columns (VEC4: 16 lanes x float4 = 256 contiguous bytes of a row; otherwise 64 lanes x float) and
// row slot k adds rows k, k + slots, ... in row order; then the slot sums are added pairwise in a fixed tree.  Tall narrow
// matrices run best as two calls (ops.column_sum): first over the (rows / B, B N) view, then over the (B, N) partial sums.
// ------------------------------------------------------------------------------------------------
constexpr int kColTile = 64, kColThreads = 1024;

template <bool VEC4>
__global__ __launch_bounds__(kColThreads) void column_sum_kernel(const float *__restrict__ x, float *__restrict__ out, long long rows,
                                                                 int N, int accumulate)
{
    constexpr int kLanes = VEC4 ? kColTile / 4 : kColTile, kSlots = kColThreads / kLanes;
    __shared__ float part[kSlots][kColTile];
    const int slot = threadIdx.x / kLanes, li = threadIdx.x % kLanes;
    const long long c = (long long)blockIdx.x * kColTile + li * (VEC4 ? 4 : 1);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c < N) {
        const float *p = x + c;
        auto add = [&](long long r) {
            if constexpr (VEC4) {
                const float4 v = *reinterpret_cast<const float4 *>(p + r * N);
                acc[0] = acc[0] + v.x; acc[1] = acc[1] + v.y; acc[2] = acc[2] + v.z; acc[3] = acc[3] + v.w;
            } else {
                acc[0] = acc[0] + p[r * N];
            }
        };
        long long r = slot;
        for (; r + 3 * kSlots < rows; r += 4 * kSlots) { // (the compiler keeps the four loads in flight; the adds stay in row order)
            add(r); add(r + kSlots); add(r + 2 * kSlots); add(r + 3 * kSlots);
        }
        for (; r < rows; r += kSlots) add(r);
    }
#pragma unroll
    for (int k = 0; k < (VEC4 ? 4 : 1); ++k) part[slot][li * (VEC4 ? 4 : 1) + k] = acc[k];
    __syncthreads();
    for (int s = kSlots / 2; s >= 1; s >>= 1) {
        for (int i = threadIdx.x; i < s * kColTile; i += kColThreads) {
            const int sl = i / kColTile, col = i % kColTile;
            part[sl][col] = part[sl][col] + part[sl + s][col];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < kColTile) {
        const long long col = (long long)blockIdx.x * kColTile + threadIdx.x;
        if (col < N) out[col] = accumulate ? out[col] + part[0][threadIdx.x] : part[0][threadIdx.x];
    }
}

inline int launch_status() { return (int)hipGetLastError(); }

} // namespace

extern "C" {

size_t vfa_gather_backward_det_workspace_bytes(int n_views, int nl, int cell_count, int C, int Hf, int Wf)
{
    DetLayout L;
    if (!det_layout(L, n_views, nl, cell_count, C, Hf, Wf)) return 0;
    return L.total;
}

int vfa_project_gather_backward_det_f32(const float *grad_vox, const float *calibs, const float *grid, const float *z_layers,
                                        const float *corner_off, float *grad_integral, int n_views, int C, int Hf, int Wf, int nl,
                                        int n_cells, int cell_begin, int cell_count, int grid_w, int conv_kind, float img_w,
                                        float img_h, float cmin, float cmax, int flags, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    // (VFA_FLAG_RESERVED_CUS is accepted and changes nothing: no kernel of this entry point is persistent, every grid follows
    // from the shapes)
    if (flags & ~(VFA_BWD_ACCUMULATE | VFA_FLAG_RESERVED_CUS(0xff))) return VFA_ERR_BAD_ARGUMENT;
    if (grid_w < 0 || (grid_w > 0 && n_cells % grid_w != 0)) return VFA_ERR_BAD_ARGUMENT;
    if (n_views < 0 || C <= 0 || Hf <= 0 || Wf <= 0 || nl <= 0 || n_cells < 0 || cell_begin < 0 || cell_count < 0 ||
        cell_begin + cell_count > n_cells || conv_kind < 0 || conv_kind > 2)
        return VFA_ERR_BAD_ARGUMENT;
    DetLayout L;
    if (!det_layout(L, n_views, nl, cell_count, C, Hf, Wf)) return VFA_ERR_BAD_ARGUMENT;
    if (workspace_bytes != L.total || (L.n_rec > 0 && !workspace)) return VFA_ERR_BAD_ARGUMENT;
    const int accumulate = flags & VFA_BWD_ACCUMULATE;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {
        const size_t bytes = (size_t)n_views * (Hf + 2) * (Wf + 2) * C * sizeof(float);
        if (bytes) {
            const hipError_t e = hipMemsetAsync(grad_integral, 0, bytes, s);
            if (e != hipSuccess) return (int)e;
        }
    }
    if (L.n_rec == 0) return 0;
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned long long *keys[2] = {reinterpret_cast<unsigned long long *>(ws + L.keys_a), reinterpret_cast<unsigned long long *>(ws + L.keys_b)};
    float *coef = reinterpret_cast<float *>(ws + L.coef);
    unsigned *counts = reinterpret_cast<unsigned *>(ws + L.counts), *sums = reinterpret_cast<unsigned *>(ws + L.sums);
    BoxGeom g{calibs, grid, z_layers, corner_off, conv_kind, img_w, img_h, cmin, cmax};
    hipLaunchKernelGGL(det_emit_kernel, dim3((unsigned)((L.n_boxes + 255) / 256)), dim3(256), 0, s, g, nl, cell_begin, cell_count, Hf, Wf,
                       L.n_boxes, L.sentinel, keys[0], coef);
    int st = launch_status();
    if (st) return st;
    for (int p = 0; p < L.passes; ++p) {
        const unsigned long long *in = keys[p & 1];
        unsigned long long *out = keys[(p + 1) & 1];
        hipLaunchKernelGGL(det_hist_kernel, dim3((unsigned)L.sort_blocks), dim3(kWave), 0, s, in, L.n_rec, 8 * p, L.sort_blocks, counts);
        hipLaunchKernelGGL(det_scan_reduce_kernel, dim3((unsigned)L.scan_blocks), dim3(256), 0, s, counts, L.n_counts, sums);
        hipLaunchKernelGGL(det_scan_top_kernel, dim3(1), dim3(1024), 0, s, sums, L.scan_blocks);
        hipLaunchKernelGGL(det_scan_down_kernel, dim3((unsigned)L.scan_blocks), dim3(256), 0, s, counts, L.n_counts, sums);
        hipLaunchKernelGGL(det_scatter_kernel, dim3((unsigned)L.sort_blocks), dim3(kWave), 0, s, in, out, L.n_rec, 8 * p, L.sort_blocks,
                           counts);
        if ((st = launch_status())) return st;
    }
    MergeArgs m;
    m.sorted = keys[L.passes & 1];
    m.coef = coef;
    m.grad_vox = grad_vox;
    m.head = reinterpret_cast<float *>(ws + L.head);
    m.tail = reinterpret_cast<float *>(ws + L.tail);
    m.out = grad_integral;
    m.n_rec = L.n_rec;
    m.n_pieces = L.n_pieces;
    m.sentinel = L.sentinel;
    m.C = C;
    m.accumulate = accumulate;
    const dim3 grid_m((unsigned)L.n_pieces, (unsigned)L.cblocks);
    if (C % 4 == 0) {
        hipLaunchKernelGGL(det_merge_kernel<4>, grid_m, dim3(kWave), 0, s, m);
        hipLaunchKernelGGL(det_fixup_kernel<4>, grid_m, dim3(kWave), 0, s, m);
    } else {
        hipLaunchKernelGGL(det_merge_kernel<1>, grid_m, dim3(kWave), 0, s, m);
        hipLaunchKernelGGL(det_fixup_kernel<1>, grid_m, dim3(kWave), 0, s, m);
    }
    return launch_status();
}

int vfa_column_sum_f32(const float *x, float *out, long long rows, int N, int accumulate, void *stream)
{
    if (rows < 0 || N <= 0) return VFA_ERR_BAD_ARGUMENT;
    const unsigned tiles = (unsigned)((N + kColTile - 1) / kColTile);
    if (N % 4 == 0)
        hipLaunchKernelGGL(column_sum_kernel<true>, dim3(tiles), dim3(kColThreads), 0, (hipStream_t)stream, x, out, rows, N, accumulate);
    else
        hipLaunchKernelGGL(column_sum_kernel<false>, dim3(tiles), dim3(kColThreads), 0, (hipStream_t)stream, x, out, rows, N, accumulate);
    return launch_status();
}

} // extern "C"
