// vfa_stem.h -- the integer rules of the trunk's stem of vfa_stem.hip (host / device code; tests/native/stem_harness.cpp checks them
// against a brute-force enumeration): the 7 x 7 stride-2 convolution of three channels with zero padding 3, and the 3 x 3 stride-2
// max pooling with padding 1 behind it; at the end, the rules of the two backward kernels.
//
// Convolution.  The output is (Lo, Wo) = (conv_out(L), conv_out(W)).  A tile is kTileRows x kTileCols OUTPUT cells and all (at most
// kMaxOut) outputs; the cell (ry, rx) of the tile at (y0, x0) is output position (y0 + ry, x0 + rx).  Its window is the
// kWinRows x kWinCols positions of each of the three channels the tile's taps touch, window position (wy, wx) being image position
// (2 y0 - 3 + wy, 2 x0 - 3 + wx).  The sum runs over k = (c 7 + ky) 7 + kx, the order the weight (O, 3, 7, 7) lies in, ascending,
// padded with zero weights from kK = 147 to kKPad = 148 (the f32 MFMA takes two k at a time); tap k of the cell (ry, rx) reads window
// position (2 ry + ky, 2 rx + kx) of channel c.
// Where a window position lies in LDS is its LOCATION: rows of kWinPitch floats, the even window columns of a row first and the odd
// ones behind them, so that the 32 cells of an MFMA operand -- window columns 2 rx + kx -- read 32 CONSECUTIVE locations (the rule of
// vfa_conv.h at stride 2).  location = cell_base(ry, rx) + tap_offset(k): the second term is the same for every lane of an operand.
//
// Packed weight: kKPad rows of 64 floats, row k holding (output r, output 32 + r) pairs for r = 0 .. 31 -- the two A operands of a
// lane as one 8-byte read; outputs past O and the row k = 147 are zeros.
//
// Pooling.  Output (oy, ox) of an (L, W) map takes the maximum over rows pool_first(oy) .. pool_last(oy, L) and columns
// pool_first(ox) .. pool_last(ox, W): the taps 2 o - 1 .. 2 o + 1 that lie inside the map (the others are skipped, not zeros).
#ifndef VFA_STEM_H
#define VFA_STEM_H
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VFA_STEM_HD __host__ __device__ inline
#else
#define VFA_STEM_HD inline
#endif

namespace vfa_stem {

constexpr int kChannels = 3;
constexpr int kKernel = 7;   // 7 x 7 taps, zero padding 3, stride 2
constexpr int kPad = 3;
constexpr int kTileRows = 4;  // output rows of a tile: one wave and one 32-cell MFMA operand each
constexpr int kTileCols = 32; // output columns of a tile
constexpr int kMaxOut = 64;   // outputs of a tile: two 32-row MFMA blocks
constexpr int kK = kChannels * kKernel * kKernel; // 147
constexpr int kKPad = 148;
constexpr int kSteps = kKPad / 2; // v_mfma_f32_32x32x2_f32 instructions per output block
constexpr int kWinRows = 2 * (kTileRows - 1) + kKernel; // 13
constexpr int kWinCols = 2 * (kTileCols - 1) + kKernel; // 69
constexpr int kWinEven = (kWinCols + 1) / 2;            // 35 even columns, 34 odd ones behind them
constexpr int kWinPitch = 70;
constexpr int kWinValues = kChannels * kWinRows * kWinCols;     // 2691 positions to load
constexpr int kWinLocations = kChannels * kWinRows * kWinPitch; // 2730 floats of LDS
constexpr int kPackedFloats = kKPad * kMaxOut;                  // 9472

VFA_STEM_HD int conv_out(int n) { return n < 1 ? 0 : (n - 1) / 2 + 1; }
VFA_STEM_HD int pool_out(int n) { return n < 1 ? 0 : (n - 1) / 2 + 1; }
VFA_STEM_HD int tiles_x(int Wo) { return (Wo + kTileCols - 1) / kTileCols; }
VFA_STEM_HD int tiles_y(int Lo) { return (Lo + kTileRows - 1) / kTileRows; }

// tile index (0 .. tiles_x * tiles_y - 1) of the OUTPUT map -> the output position of its first cell
VFA_STEM_HD void tile_origin(int tile, int Wo, int &y0, int &x0)
{
    const int tx = tiles_x(Wo);
    y0 = (tile / tx) * kTileRows;
    x0 = (tile % tx) * kTileCols;
}

// window position p = (c kWinRows + wy) kWinCols + wx of the tile at output (y0, x0) -> channel and image position; false: outside
// the image (zero padding; no address is formed)
VFA_STEM_HD bool window_position(int p, int y0, int x0, int L, int W, int &c, int &y, int &x)
{
    c = p / (kWinRows * kWinCols);
    const int q = p % (kWinRows * kWinCols);
    y = 2 * y0 - kPad + q / kWinCols;
    x = 2 * x0 - kPad + q % kWinCols;
    return y >= 0 && y < L && x >= 0 && x < W;
}

// window position (wy, wx) of channel c -> location in LDS
VFA_STEM_HD constexpr int window_location(int c, int wy, int wx) { return (c * kWinRows + wy) * kWinPitch + (wx & 1) * kWinEven + wx / 2; }

// k -> (channel, ky, kx); k >= kK is the zero padding of the sum
VFA_STEM_HD constexpr int k_channel(int k) { return k / (kKernel * kKernel); }
VFA_STEM_HD constexpr int k_row(int k) { return k / kKernel % kKernel; }
VFA_STEM_HD constexpr int k_col(int k) { return k % kKernel; }

// location of tap k of the tile's cell (ry, rx) = cell_base(ry, rx) + tap_offset(k); a padded k reads the location of the last tap
// (any value: the kernel replaces it by a zero)
VFA_STEM_HD constexpr int cell_base(int ry, int rx) { return 2 * ry * kWinPitch + rx; }
VFA_STEM_HD constexpr int tap_offset(int k) { return k >= kK ? tap_offset(kK - 1) : window_location(k_channel(k), k_row(k), k_col(k)); }

// The two halves of a wave hold k = 2 s and k = 2 s + 1 of pair s: tap_offset(2 s + 1) - tap_offset(2 s) takes kPairDeltas values
// (the padded pair, an even column to the odd one behind it, an odd one to the next even one, the last column of a row to the first
// of the next row, and of a channel's last row to the next channel's first), so the upper half's address is one of as many per-lane
// bases plus the offset of the lower half's.
constexpr int kPairDeltas = 5;
VFA_STEM_HD constexpr int pair_delta(int slot)
{
    return slot == 0 ? 0 : slot == 1 ? kWinEven : slot == 2 ? 1 - kWinEven : slot == 3 ? kWinPitch - kPad : (kWinRows - kKernel + 1) * kWinPitch - kPad;
}
VFA_STEM_HD constexpr int pair_slot(int s)
{
    const int d = tap_offset(2 * s + 1) - tap_offset(2 * s);
    return d == pair_delta(0) ? 0 : d == pair_delta(1) ? 1 : d == pair_delta(2) ? 2 : d == pair_delta(3) ? 3 : d == pair_delta(4) ? 4 : -1;
}

// index of weight (o, k), o < kMaxOut and k < kKPad, in the packed weight
VFA_STEM_HD constexpr int packed_index(int o, int k) { return k * kMaxOut + 2 * (o % 32) + o / 32; }

// the pooling's taps of output o along an axis of n positions
VFA_STEM_HD int pool_first(int o) { return 2 * o - 1 < 0 ? 0 : 2 * o - 1; }
VFA_STEM_HD int pool_last(int o, int n) { return 2 * o + 1 > n - 1 ? n - 1 : 2 * o + 1; }

// ---- the backward rules (vfa_stem_pool_backward_f32, vfa_stem_conv_wgrad_f32; tests/native/stem_grad_harness.cpp checks them) ----------
//
// Pooling.  Along an axis position p lies in the windows pool_window_first(p) .. pool_window_last(p, n_out) of the n_out outputs:
// an even position in one, an odd one in two unless the second is past the last output.  A window's taps are scanned rows
// ascending, columns ascending inside a row, the taps outside the map skipped: pool_scan_rank is a tap's place in that order
// (0 .. pool_taps(oy, L) pool_taps(ox, W) - 1).  The WINNER of a window is kept as a code that does not depend on the map's size:
// pool_tap_code = 3 (ty - (2 oy - 1)) + (tx - (2 ox - 1)), 0 .. 8, kNoWinner for a window past the map.
VFA_STEM_HD int pool_window_first(int p) { return p / 2; }
VFA_STEM_HD int pool_window_last(int p, int n_out) { return (p + 1) / 2 > n_out - 1 ? n_out - 1 : (p + 1) / 2; }
VFA_STEM_HD int pool_taps(int o, int n) { return pool_last(o, n) - pool_first(o) + 1; }
VFA_STEM_HD int pool_scan_rank(int oy, int ox, int ty, int tx, int W) { return (ty - pool_first(oy)) * pool_taps(ox, W) + (tx - pool_first(ox)); }
VFA_STEM_HD int pool_tap_code(int oy, int ox, int ty, int tx) { return 3 * (ty - (2 * oy - 1)) + (tx - (2 * ox - 1)); }
constexpr int kNoWinner = 255;

// A workgroup of the pooling's backward owns a tile of kPoolTileRows x kPoolTileCols positions of u at an even origin (p0, q0).  The
// windows that contain them are kPoolWinRows x kPoolWinCols, from window (p0 / 2, q0 / 2); their taps are kPoolTapRows x kPoolTapCols
// positions from (p0 - 1, q0 - 1).
constexpr int kPoolTileRows = 32, kPoolTileCols = 64;
constexpr int kPoolWinRows = kPoolTileRows / 2 + 1, kPoolWinCols = kPoolTileCols / 2 + 1;
constexpr int kPoolTapRows = kPoolTileRows + 3, kPoolTapCols = kPoolTileCols + 3;
VFA_STEM_HD int pool_tiles_x(int W) { return (W + kPoolTileCols - 1) / kPoolTileCols; }
VFA_STEM_HD int pool_tiles_y(int L) { return (L + kPoolTileRows - 1) / kPoolTileRows; }

// Weight gradient.  The output cells are the K dimension of the product.  They are walked in the forward's tiles (tile_origin),
// row-major over the (Lo, Wo) map, and a SLAB is a run of consecutive tiles.  The cut is a function of (Lo, Wo) alone: a map of n
// tiles has min(n, kMaxSlabs) slabs and slab s owns the tiles [n s / slabs, n (s + 1) / slabs) -- never empty, every tile in exactly
// one slab -- so what is summed where depends on neither the device nor the batch (the rule of vfa_conv_grad.h).  One (image, slab)
// gives one float32 partial of O x kK floats, [image][slab][o][k].
constexpr int kMaxSlabs = 64;
constexpr int kNBlocks = (kK + 31) / 32;  // 32-column MFMA blocks of the taps: N = 147 padded to 160
VFA_STEM_HD int wgrad_tiles(int Lo, int Wo) { return tiles_x(Wo) * tiles_y(Lo); }
VFA_STEM_HD int wgrad_slabs(int Lo, int Wo) { return wgrad_tiles(Lo, Wo) < kMaxSlabs ? wgrad_tiles(Lo, Wo) : kMaxSlabs; }
// first tile of slab s (s == slabs: one past the last tile)
VFA_STEM_HD int wgrad_slab_begin(int s, int Lo, int Wo) { return (int)((long long)wgrad_tiles(Lo, Wo) * s / wgrad_slabs(Lo, Wo)); }
VFA_STEM_HD size_t wgrad_partial_floats(int O) { return (size_t)O * kK; }
VFA_STEM_HD size_t wgrad_partial_index(int b, int s, int n_slabs, int o, int k, int O) { return ((size_t)b * n_slabs + s) * wgrad_partial_floats(O) + (size_t)o * kK + k; }

} // namespace vfa_stem
#endif // VFA_STEM_H
