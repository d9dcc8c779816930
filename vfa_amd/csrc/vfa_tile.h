// vfa_tile.h -- what the two frame kernels (vfa_fused.hip: single-layer grids, vfa_pipe.hip: any number of z-layers) share in
// front of their own record payloads: the 8 x 4-cell tile, the decoding of a half-wave into (view, tile, cell), the tap coordinates
// of a box and the window of the integral image that holds all taps of a tile's visible boxes.  The box itself is `cube_box`
// (vfa_geom.h).  The integer part of the window is plain host / device code: tests/native/tile_window_harness.cpp compiles it with
// g++ and checks it on the CPU (the pattern of vfa_pipe_seq.h).
#ifndef VFA_TILE_H
#define VFA_TILE_H

#if defined(__HIPCC__)
#define VFA_TILE_HD __host__ __device__ __forceinline__
#else
#define VFA_TILE_HD inline
#endif

namespace vfa_dev {

constexpr int kTileW = 8, kTileL = 4, kTileBoxes = kTileW * kTileL; // 32 cells = one 32-row MFMA block

// ------------------------------------------------------------------------------------------------
// the tap window of a tile, integer part
// ------------------------------------------------------------------------------------------------
// Taps of the visible boxes of a tile lie in columns [x0, x1], top rows [t0, t1] and bottom rows [b0, b1] (coordinates -1 .. size:
// the zero border included).  The window keeps `cwid` columns of `top_rows` rows from t0 and `bot_rows` rows from b0, row-major,
// the bottom band behind the top band: n_slots taps.  Bands that touch or overlap are one band (bot_rows = 0).
struct Window { int x0, t0, b0, cwid, top_rows, bot_rows, n_slots; };

VFA_TILE_HD Window make_window(bool any_vis, int x0, int x1, int t0, int t1, int b0, int b1)
{
    Window w = {x0, t0, b0, 0, 0, 0, 0};
    if (any_vis) {
        w.cwid = x1 - x0 + 1;
        if (b0 <= t1 + 1) { // the bands touch or overlap: one band [t0, max(t1, b1)]
            w.top_rows = (t1 > b1 ? t1 : b1) - t0 + 1;
            w.bot_rows = 0;
            w.b0 = t0 + w.top_rows; // rows >= b0 would start the (empty) second band
        } else {
            w.top_rows = t1 - t0 + 1;
            w.bot_rows = b1 - b0 + 1;
        }
        w.n_slots = w.cwid * (w.top_rows + w.bot_rows);
    }
    return w;
}
// window row of image row y (a row of one of the bands)
VFA_TILE_HD int slot_row(const Window &w, int y) { return y < w.t0 + w.top_rows ? y - w.t0 : w.top_rows + (y - w.b0); }
// floor(s / cwid) == (s * inv) >> 16 for s < 128 (the consumers turn a slot into its window row and column with it)
VFA_TILE_HD int window_inv(int cwid) { return cwid > 0 ? (65536 + cwid - 1) / cwid : 0; }

} // namespace vfa_dev

#if defined(__HIPCC__)
#include "vfa_geom.h"

namespace vfa_dev {

// ------------------------------------------------------------------------------------------------
// constants, types and helpers of both frame kernels
// ------------------------------------------------------------------------------------------------
constexpr int kC = 256;                         // channels in = channels out
constexpr int kMaxScales = 3;
constexpr int kSlotBytes = kC * 4;              // one tap in the integral image: 256 fp32
constexpr int kHdrBytes = 32;                   // tile header: two uint4 (tile_header0 / tile_header1)
constexpr int kChunks = 8192;                   // pieces of the work cuts (fine enough that a launch with any number of workgroups gets pieces within 3 % of each other)
constexpr int kMaxBlocks = 512;                 // workgroups of a persistent frame kernel
constexpr int kVis = 1;                         // record flag: the box is visible
constexpr int kTileLive = 1, kTileDirect = 2;   // tile header flags: a live box in the tile; pooled straight from the integral image

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct ScaleDims { int Hf, Wf; };
struct Frag { bf16x8 hi, lo; };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float4 mul4(float4 a, float w) { return make_float4(a.x * w, a.y * w, a.z * w, a.w * w); }
__device__ __forceinline__ float4 fma4(float4 a, float w, float4 c)
{
    return make_float4(fmaf(a.x, w, c.x), fmaf(a.y, w, c.y), fmaf(a.z, w, c.z), fmaf(a.w, w, c.w));
}
// bilinear sample from the four rounded weights, taps in the order nw, ne, sw, se: one product, three FMAs
__device__ __forceinline__ float4 sample4(float4 nw, float4 ne, float4 sw, float4 se, float w0, float w1, float w2, float w3)
{
    float4 v = mul4(nw, w0);
    v = fma4(ne, w1, v);
    v = fma4(sw, w2, v);
    v = fma4(se, w3, v);
    return v;
}

// ------------------------------------------------------------------------------------------------
// geometry of the frame: one half-wave (32 lanes) per (view, tile[, layer]), lane = cell of the tile (4 rows of 8)
// ------------------------------------------------------------------------------------------------
struct TileLane {
    int half, b;          // half-wave of the workgroup, lane of the half-wave
    int view, tile, layer;
    int cl, cw, cell;     // the lane's cell (cell = 0 where !valid)
    bool pair_ok, valid;  // the half-wave has a (view, tile); the lane has a cell of the grid
};
// Unit blockIdx.x * 2 + half = pair * nl + layer, pair = view * n_tiles + tile.
__device__ __forceinline__ TileLane tile_lane(int n_views, int n_tiles, int tiles_w, int L, int W, int nl = 1)
{
    TileLane q;
    const int lane = threadIdx.x;
    q.half = lane >> 5; q.b = lane & 31;
    const long long unit = (long long)blockIdx.x * 2 + q.half;
    const long long pair = unit / nl;
    q.layer = (int)(unit - pair * nl);
    q.pair_ok = pair < (long long)n_views * n_tiles;
    q.view = q.pair_ok ? (int)(pair / n_tiles) : 0; q.tile = q.pair_ok ? (int)(pair % n_tiles) : 0;
    const int tl = q.tile / tiles_w, tw = q.tile - tl * tiles_w;
    q.cl = tl * kTileL + (q.b >> 3); q.cw = tw * kTileW + (q.b & 7);
    q.valid = q.pair_ok && q.cl < L && q.cw < W;
    q.cell = q.valid ? q.cl * W + q.cw : 0;
    return q;
}

// The bilinear set-up of the four box edges on a feature map and the sixteen taps they touch: columns xs = {left, left + 1, right,
// right + 1}, rows ys alike, out-of-image taps redirected to the zero border (coordinate -1 or Hf / Wf)
struct BoxTaps { Axis xl, xr, yt, yb; int xs[4], ys[4]; };
__device__ __forceinline__ BoxTaps box_taps(float l, float t, float r, float bt, int Hf, int Wf)
{
    BoxTaps p;
    p.xl = make_axis(l, Wf); p.xr = make_axis(r, Wf); p.yt = make_axis(t, Hf); p.yb = make_axis(bt, Hf);
    p.xs[0] = clampi(p.xl.i0, -1, Wf); p.xs[1] = clampi(p.xl.i0 + 1, -1, Wf); p.xs[2] = clampi(p.xr.i0, -1, Wf); p.xs[3] = clampi(p.xr.i0 + 1, -1, Wf);
    p.ys[0] = clampi(p.yt.i0, -1, Hf); p.ys[1] = clampi(p.yt.i0 + 1, -1, Hf); p.ys[2] = clampi(p.yb.i0, -1, Hf); p.ys[3] = clampi(p.yb.i0 + 1, -1, Hf);
    return p;
}

// The window of a tile over its VISIBLE boxes (a half-wave reduction), the largest of their sliver shifts (vfa_geom.h: the binary
// places the fp16 split gives up for the tile's noisiest visible box; 0 for honest boxes) and whether the tile has a visible / a
// live box at all.  area, Hf, Wf: the lane's box on the feature map.  Every lane of the half-wave leaves with the same values.
struct TileWindow { Window w; int shift; bool any_vis, any_live; };
__device__ __forceinline__ TileWindow tile_window(const BoxTaps &p, bool vis, bool live_box, float area, int Hf, int Wf, int half)
{
    constexpr int kBig = 1 << 20;
    int x0 = vis ? min(p.xs[0], p.xs[2]) : kBig, x1 = vis ? max(p.xs[1], p.xs[3]) : -kBig;
    int t0 = vis ? p.ys[0] : kBig, t1 = vis ? p.ys[1] : -kBig, b0 = vis ? p.ys[2] : kBig, b1 = vis ? p.ys[3] : -kBig;
    int shift = vis ? sliver_shift(area, Hf, Wf) : 0;
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
        x0 = min(x0, __shfl_xor(x0, m, 32)); x1 = max(x1, __shfl_xor(x1, m, 32));
        t0 = min(t0, __shfl_xor(t0, m, 32)); t1 = max(t1, __shfl_xor(t1, m, 32));
        b0 = min(b0, __shfl_xor(b0, m, 32)); b1 = max(b1, __shfl_xor(b1, m, 32));
        shift = max(shift, __shfl_xor(shift, m, 32));
    }
    const unsigned long long vis_all = __ballot(vis), live_all = __ballot(live_box);
    TileWindow tw;
    tw.shift = shift;
    tw.any_vis = ((vis_all >> (32 * half)) & 0xffffffffull) != 0ull;
    tw.any_live = ((live_all >> (32 * half)) & 0xffffffffull) != 0ull;
    tw.w = make_window(tw.any_vis, x0, x1, t0, t1, b0, b1);
    return tw;
}

// Row and column parts of a box's taps in its record.  direct: pixel coordinates of the padded integral image (the box is pooled
// from L2); else the window slot of the row's first tap and the column inside the window.
__device__ __forceinline__ void tap_parts(const Window &w, const BoxTaps &p, bool direct, unsigned (&rows)[4], unsigned (&cols)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (direct) { rows[k] = (unsigned)(p.ys[k] + 1); cols[k] = (unsigned)(p.xs[k] + 1); }
        else { rows[k] = (unsigned)(slot_row(w, p.ys[k]) * w.cwid); cols[k] = (unsigned)(p.xs[k] - w.x0); }
    }
}

// The tile header (kHdrBytes).  Word 2 of the first half is the caller's: the window width, or the serial kernel's row slot.
__device__ __forceinline__ uint4 tile_header0(unsigned hflags, const Window &w, unsigned word2)
{
    return make_uint4(hflags, (unsigned)w.n_slots, word2, (unsigned)window_inv(w.cwid));
}
__device__ __forceinline__ uint4 tile_header1(const Window &w)
{
    return make_uint4((unsigned)w.x0, (unsigned)w.t0, (unsigned)w.top_rows, (unsigned)w.b0);
}

} // namespace vfa_dev
#endif // __HIPCC__
#endif // VFA_TILE_H
