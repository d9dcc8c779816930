// vfa_trunk.h -- the integer rules of the trunk convolution of vfa_trunk.hip (host / device code; tests/native/trunk_harness.cpp
// checks them against a brute-force enumeration): the dense kernel of vfa_conv.h generalised to a stride s of 1 or 2 and to 1 or 9
// taps.  Tiles, the 32-channel chunk, the 80-byte location rows and the slice layout of the packed weights are vfa_conv.h's.
//
// The output is (Lo, Wo) = (out_size(L, s), out_size(W, s)).  A tile is kTileRows x kTileCols OUTPUT cells and kTileOut outputs;
// the output cell (ry, rx) of the tile at (y0, x0) is output position (y0 + ry, x0 + rx).
//   taps 9 (3 x 3, zero padding 1): the window is (s (kTileRows - 1) + 3) x (s (kTileCols - 1) + 3) positions, window position
//       (wy, wx) being map position (s y0 - 1 + wy, s x0 - 1 + wx); tap t = 3 ty + tx of the cell (ry, rx) reads window position
//       (s ry + ty, s rx + tx).
//   taps 1 (1 x 1, no padding): the window is the tile itself, window position (wy, wx) being map position (s (y0 + wy), s (x0 + wx)).
// Where a window position lies in LDS is its LOCATION.  At stride 1 (and with one tap) location = wy cols + wx.  At stride 2 the even
// window columns of a row come first and the odd ones behind them: the 32 cells of an MFMA operand read tap tx at the columns
// 2 rx + tx, which are 32 CONSECUTIVE locations of one half (tx = 0: even rx; tx = 1: odd rx; tx = 2: even rx + 1), so their 80-byte
// rows fall on the banks as they do at stride 1 (16 lanes: 20 k mod 64 dwords, sixteen disjoint quads) instead of two-way onto eight.
//
// Packed weights: vfa_conv.h's slices with `taps` slices per (output tile, chunk) instead of nine.
#ifndef VFA_TRUNK_H
#define VFA_TRUNK_H
#include "vfa_conv.h"

namespace vfa_trunk {

using vfa_conv::kChunkC;
using vfa_conv::kLocHalves;
using vfa_conv::kPackHeaderBytes;
using vfa_conv::kSliceHalves;
using vfa_conv::kTileCols;
using vfa_conv::kTileOut;
using vfa_conv::kTileRows;
using vfa_conv::out_tiles;
using vfa_conv::tile_origin; // of the OUTPUT map: tile_origin(tile, Wo, y0, x0)
using vfa_conv::tiles_x;
using vfa_conv::tiles_y;

constexpr int kSplitC = 256; // more channels than this: two accumulator chains, one per half of the chunks (vfa_trunk.hip)

VFA_CONV_HD bool valid(int taps, int s) { return (taps == 1 || taps == 9) && (s == 1 || s == 2); }
VFA_CONV_HD int out_size(int n, int s) { return n < 1 ? 0 : (n - 1) / s + 1; }
VFA_CONV_HD constexpr int window_rows(int taps, int s) { return taps == 9 ? s * (kTileRows - 1) + 3 : kTileRows; }
VFA_CONV_HD constexpr int window_cols(int taps, int s) { return taps == 9 ? s * (kTileCols - 1) + 3 : kTileCols; }
VFA_CONV_HD constexpr int window_locations(int taps, int s) { return window_rows(taps, s) * window_cols(taps, s); }
// chunks of the first accumulator chain (all of them up to kSplitC channels)
VFA_CONV_HD int first_chunks(int C) { return C > kSplitC ? (C / kChunkC + 1) / 2 : C / kChunkC; }

// window position (wy, wx) -> location in LDS
VFA_CONV_HD int window_location(int wy, int wx, int taps, int s)
{
    const int wc = window_cols(taps, s);
    if (taps == 9 && s == 2) return wy * wc + (wx & 1) * ((wc + 1) / 2) + wx / 2;
    return wy * wc + wx;
}

// location of tap t of the tile's output cell (ry, rx)
VFA_CONV_HD int tap_location(int ry, int rx, int t, int taps, int s)
{
    if (taps == 1) return window_location(ry, rx, taps, s);
    return window_location(s * ry + t / 3, s * rx + t % 3, taps, s);
}

// window position p = wy cols + wx (the order the window is loaded in) of the tile at output (y0, x0) -> map position; false:
// outside the map (zero padding, or past the last strided position; no address is formed)
VFA_CONV_HD bool window_position(int p, int y0, int x0, int taps, int s, int L, int W, int &y, int &x)
{
    const int wc = window_cols(taps, s), wy = p / wc, wx = p % wc;
    if (taps == 9) {
        y = s * y0 - 1 + wy;
        x = s * x0 - 1 + wx;
    } else {
        y = s * (y0 + wy);
        x = s * (x0 + wx);
    }
    return y >= 0 && y < L && x >= 0 && x < W;
}

// fp16 values of both packed planes (without the header)
VFA_CONV_HD size_t packed_halves(int O, int C, int taps) { return (size_t)out_tiles(O) * (size_t)(C / kChunkC) * (size_t)taps * kSliceHalves; }

// index of weight (o, c, tap t) of piece 0 (hi) / 1 (lo) in the packed planes
VFA_CONV_HD size_t packed_index(int o, int c, int t, int piece, int C, int taps)
{
    const size_t slice = ((size_t)(o / kTileOut) * (size_t)(C / kChunkC) + (size_t)(c / kChunkC)) * (size_t)taps + (size_t)t;
    const int cc = c % kChunkC;
    return slice * kSliceHalves + (size_t)(((piece * 4 + cc / 8) * kTileOut + o % kTileOut) * 8 + cc % 8);
}

} // namespace vfa_trunk
#endif // VFA_TRUNK_H
