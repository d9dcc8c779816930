// vfa_conv.h -- the integer rules of the dense 3x3 convolution of vfa_conv.hip (host / device code; tests/native/conv_harness.cpp
// checks them against a brute-force enumeration): which cells a tile owns, where a (cell, tap) lies in the tile's staged window,
// which window locations are inside the map (the others are the zero padding), and where a weight sits in the packed planes.
//
// A tile is kTileRows x kTileCols cells of one frame and kTileOut outputs.  Its window is the tile grown by the dilation d on every
// side: (kTileRows + 2 d) x (kTileCols + 2 d) locations, location (wy, wx) being map position (y0 - d + wy, x0 - d + wx).  Tap
// t = 3 ty + tx of the cell (ry, rx) of the tile reads location (ry + ty d, rx + tx d): map position (y + (ty - 1) d, x + (tx - 1) d).
//
// Packed weights: two fp16 planes (hi, lo) in slices of one (output tile, chunk of 32 channels, tap): a slice is
// [piece][4 groups of 8 channels][kTileOut outputs][8 channels], 16 KiB, copied to LDS as it lies; outputs past O are zeros.
#ifndef VFA_CONV_H
#define VFA_CONV_H
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VFA_CONV_HD __host__ __device__ inline
#else
#define VFA_CONV_HD inline
#endif

namespace vfa_conv {

constexpr int kTaps = 9;
constexpr int kTileRows = 4;   // map rows of a tile: one 32-cell MFMA operand each
constexpr int kTileCols = 32;  // map columns of a tile
constexpr int kTileOut = 128;  // outputs of a tile
constexpr int kChunkC = 32;    // channels staged at a time (C % 32 == 0)
constexpr int kMaxDilation = 4;
constexpr int kLocHalves = 40; // fp16 values per window location in LDS: 32 channels + 8 of padding (80 bytes, 16-byte aligned)
constexpr int kSliceHalves = 2 * kChunkC * kTileOut; // one (output tile, chunk, tap) slice: both pieces
constexpr int kPackHeaderBytes = 64; // word 0: the bit pattern of the weight's absmax

VFA_CONV_HD int tiles_x(int W) { return (W + kTileCols - 1) / kTileCols; }
VFA_CONV_HD int tiles_y(int L) { return (L + kTileRows - 1) / kTileRows; }
VFA_CONV_HD int out_tiles(int O) { return (O + kTileOut - 1) / kTileOut; }
VFA_CONV_HD int window_rows(int d) { return kTileRows + 2 * d; }
VFA_CONV_HD int window_cols(int d) { return kTileCols + 2 * d; }
VFA_CONV_HD int window_locations(int d) { return window_rows(d) * window_cols(d); }

// tile index (0 .. tiles_x * tiles_y - 1) -> the map position of its first cell
VFA_CONV_HD void tile_origin(int tile, int W, int &y0, int &x0)
{
    const int tx = tiles_x(W);
    y0 = (tile / tx) * kTileRows;
    x0 = (tile % tx) * kTileCols;
}

// window location of tap t of the tile's cell (ry, rx)
VFA_CONV_HD int window_index(int ry, int rx, int t, int d) { return (ry + (t / 3) * d) * window_cols(d) + rx + (t % 3) * d; }

// window location -> map position; false: outside the map (zero padding, no address is formed)
VFA_CONV_HD bool window_position(int loc, int y0, int x0, int d, int L, int W, int &y, int &x)
{
    const int wc = window_cols(d);
    y = y0 - d + loc / wc;
    x = x0 - d + loc % wc;
    return y >= 0 && y < L && x >= 0 && x < W;
}

// fp16 values of both packed planes (without the header)
VFA_CONV_HD size_t packed_halves(int O, int C) { return (size_t)out_tiles(O) * (size_t)(C / kChunkC) * kTaps * kSliceHalves; }

// index of weight (o, c, tap t) of piece 0 (hi) / 1 (lo) in the packed planes
VFA_CONV_HD size_t packed_index(int o, int c, int t, int piece, int C)
{
    const size_t slice = ((size_t)(o / kTileOut) * (size_t)(C / kChunkC) + (size_t)(c / kChunkC)) * kTaps + (size_t)t;
    const int cc = c % kChunkC;
    return slice * kSliceHalves + (size_t)(((piece * 4 + cc / 8) * kTileOut + o % kTileOut) * 8 + cc % 8);
}

// host side, defined in vfa_conv.hip: per frame b the maximum of the bit patterns of the finite |x[b]| into absmax[b] (merged with an
// integer atomicMax: the caller zeroes absmax[0 .. B - 1] on the stream first) -- the operand's power-of-two scale of vfa_split.h.
// x (B, C, L, W) is read through its four element strides.  0, or the error of the entry points (an empty map launches nothing).
int frame_absmax(const float *x, const long long *stride, int B, int C, int L, int W, unsigned *absmax, void *stream);

} // namespace vfa_conv
#endif // VFA_CONV_H
