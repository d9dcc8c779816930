// vfa_conv_grad.h -- the integer rules of the weight gradient of the dense 3x3 convolution (vfa_conv_grad.hip; host / device code;
// tests/native/conv_grad_harness.cpp checks them against a brute-force enumeration): how the cells of a map are cut into slabs, and
// where a partial sum lies in the workspace.  At the end, the rules of the two gradients of a stride-2 convolution.
//
// The cells are the K dimension of the product.  They are walked in the forward kernel's tiles (vfa_conv.h: kTileRows x kTileCols
// cells, row-major over the map), and a SLAB is a run of consecutive tiles.  The cut is a function of (L, W) alone: a map of n
// tiles has min(n, kMaxSlabs) slabs and slab s owns the tiles [n s / slabs, n (s + 1) / slabs) -- never empty, every tile in
// exactly one slab -- so what is summed where depends on neither the device nor the batch.  A workgroup owns one (frame, slab) and
// one tile of kTileO outputs x kTileC inputs x 9 taps of the result and writes it, unscaled, as one float32 partial; the merge
// kernel adds the partials of an element in ascending (frame, slab) order.
//
// The trunk's layers (vfa_trunk_conv_wgrad_f32) have up to 512 x 512 weights on small maps, where kMaxSlabs partials of 9 O C floats per
// frame are larger than the operands: slabs_for(L, W, O, C) is slabs(L, W) up to O C = 256^2 and shrinks in proportion past it (at
// least one), so a frame's partials never exceed those of a 256 x 256 layer on the same map -- a rule of the shape alone, too.  The
// forms that end in _of take the number of slabs; with slabs(L, W) they are the forms above.
#ifndef VFA_CONV_GRAD_H
#define VFA_CONV_GRAD_H
#include <stddef.h>

#include "vfa_conv.h"

namespace vfa_conv_grad {

constexpr int kTileO = 128;    // outputs of a workgroup's tile: one 32-row MFMA operand per wave
constexpr int kTileC = 32;     // inputs of a workgroup's tile: the chunk of vfa_conv.h
constexpr int kMaxSlabs = 16;  // slabs of a map
constexpr int kGHalves = kTileO + 8; // fp16 values per cell of the staged output gradient: 128 outputs + 8 of padding (272 bytes)

VFA_CONV_HD int tiles(int L, int W) { return vfa_conv::tiles_x(W) * vfa_conv::tiles_y(L); }
VFA_CONV_HD int slabs(int L, int W) { return tiles(L, W) < kMaxSlabs ? tiles(L, W) : kMaxSlabs; }
// first tile of slab s (s == slabs: one past the last tile)
VFA_CONV_HD int slab_begin(int s, int L, int W) { return (int)((long long)tiles(L, W) * s / slabs(L, W)); }

// floats of one (frame, slab) partial: laid out [tap][o][c], the whole (O, C) plane of every tap
VFA_CONV_HD size_t partial_floats(int O, int C) { return (size_t)vfa_conv::kTaps * (size_t)O * (size_t)C; }
// index of element (o, c, tap t) in the partial of (frame b, slab s)
VFA_CONV_HD size_t partial_index(int b, int s, int t, int o, int c, int O, int C, int L, int W)
{
    return ((size_t)b * slabs(L, W) + s) * partial_floats(O, C) + ((size_t)t * O + o) * C + c;
}

// slabs of the trunk's weight gradient: slabs(L, W) wherever O C <= kFullSlabsOC, never more partial floats per frame than there
constexpr long long kFullSlabsOC = 256LL * 256;
VFA_CONV_HD int slabs_for(int L, int W, int O, int C)
{
    const long long oc = (long long)O * C;
    if (oc <= kFullSlabsOC) return slabs(L, W);
    const long long n = (long long)slabs(L, W) * kFullSlabsOC / oc;
    return n < 1 ? 1 : (int)n;
}
// first tile of slab s of n_slabs (1 <= n_slabs <= tiles; s == n_slabs: one past the last tile)
VFA_CONV_HD int slab_begin_of(int s, int n_slabs, int L, int W) { return (int)((long long)tiles(L, W) * s / n_slabs); }
VFA_CONV_HD size_t partial_index_of(int b, int s, int n_slabs, int t, int o, int c, int O, int C)
{
    return ((size_t)b * n_slabs + s) * partial_floats(O, C) + ((size_t)t * O + o) * C + c;
}

// ---- stride 2: the gradients of y = conv(x, w, stride 2) with a 3 x 3 weight (padding 1) or a 1 x 1 weight (no padding), x (L, W),
// y and its gradient g (Lo, Wo) = (out_size(L, 2), out_size(W, 2)); tests/native/trunk_down_harness.cpp checks these rules ------------
//
// Weight gradient, dW[o, c, ty, tx] = sum g[b, o, i, j] x[b, c, 2 i + ty - 1, 2 j + tx - 1] (1 x 1: x[b, c, 2 i, 2 j]).  The cells of g are
// K.  Tiles and slabs are those above on (Lo, Wo); a tile is walked as kDownHalves K TILES of kDownRows x kTileCols cells, because the
// window of a whole tile (9 x 65 positions) does not fit the CU's LDS beside g.  A K tile's window of x is down_window_rows x
// down_window_cols positions from map position (2 y0 - 1, 2 x0 - 1) (1 x 1: the K tile's own cells at (2 y, 2 x)), and its location
// in LDS is vfa_conv.h's stride-2 rule -- the even window columns of a row first, the odd ones behind them -- so the 8 consecutive
// cells of a transposed read are 8 consecutive locations for every tap.
constexpr int kDownRows = 2;                                  // rows of a K tile
constexpr int kDownHalves = vfa_conv::kTileRows / kDownRows;  // K tiles of a tile
VFA_CONV_HD constexpr int down_window_rows(int taps) { return taps == 9 ? 2 * (kDownRows - 1) + 3 : kDownRows; }
VFA_CONV_HD constexpr int down_window_cols(int taps) { return vfa_conv::window_cols(taps, 2, 1); }
VFA_CONV_HD constexpr int down_window_locations(int taps) { return down_window_rows(taps) * down_window_cols(taps); }
// K tile `half` of tile `tile` of the (Lo, Wo) map -> its first cell
VFA_CONV_HD void down_origin(int tile, int half, int Wo, int &y0, int &x0)
{
    vfa_conv::tile_origin(tile, Wo, y0, x0);
    y0 += half * kDownRows;
}
// window position p (row-major over the window, the order it is loaded in) of the K tile at (y0, x0) -> position of x; false: outside
VFA_CONV_HD bool down_window_position(int p, int y0, int x0, int taps, int L, int W, int &y, int &x)
{
    return vfa_conv::window_position(p, y0, x0, taps, 2, 1, L, W, y, x);
}
// window position p -> location in LDS
VFA_CONV_HD int down_window_location(int p, int taps)
{
    const int wc = down_window_cols(taps);
    return vfa_conv::window_location(p / wc, p % wc, taps, 2, 1);
}
// location of tap t of the K tile's cell (ry, rx)
VFA_CONV_HD int down_tap_location(int ry, int rx, int t, int taps) { return vfa_conv::tap_location(ry, rx, t, taps, 2, 1); }
// the partials with `taps` planes: [frame][slab][tap][o][c]
VFA_CONV_HD size_t down_partial_floats(int O, int C, int taps) { return (size_t)taps * (size_t)O * (size_t)C; }
VFA_CONV_HD size_t down_partial_index(int b, int s, int n_slabs, int t, int o, int c, int O, int C, int taps)
{
    return ((size_t)b * n_slabs + s) * down_partial_floats(O, C, taps) + ((size_t)t * O + o) * C + c;
}

// Input gradient, dx[b, c, y, x] = sum_o sum g[b, o, i, j] w[o, c, ty, tx] over 2 i + ty - 1 = y, 2 j + tx - 1 = x.  Along an axis an even
// position 2 k is reached by tap 1 alone, from g[k]; an odd position 2 k + 1 by tap 2 from g[k] and by tap 0 from g[k + 1].  So dx
// falls into four CLASSES (py, px) = (y & 1, x & 1); class cell (k, l) is dx position (2 k + py, 2 l + px), and the class is a
// stride-1 convolution of g with the block of (1 + py) x (1 + px) taps of vfa_conv.h: its tap (dy, dx) reads g[k + dy, l + dx] (a
// zero past the map) against w's tap (ty, tx) = (py ? 2 - 2 dy : 1, px ? 2 - 2 dx : 1).  One packed weight holds the nine taps of
// the four classes behind one another -- class (0,0) | (1,0) | (0,1) | (1,1) -- as a nine-tap pack of the transposed weight whose tap
// t is w's tap down_source_tap(t).
VFA_CONV_HD int down_class_size(int n, int parity) { return parity ? n / 2 : (n + 1) / 2; }   // positions of that parity in 0 .. n - 1
VFA_CONV_HD constexpr int down_class_taps(int py, int px) { return 10 * (1 + py) + (1 + px); } // the block code of vfa_conv.h
VFA_CONV_HD constexpr int down_class_first(int taps) { return taps == 11 ? 0 : taps == 21 ? 1 : taps == 12 ? 3 : 5; } // its first packed tap
VFA_CONV_HD int down_source_tap(int t) { return (int)((0x026835174ULL >> (4 * t)) & 15); }    // 4 | 7 1 | 5 3 | 8 6 2 0

} // namespace vfa_conv_grad
#endif // VFA_CONV_GRAD_H
