// vfa_conv.h -- the integer rules of the dense convolution kernel of vfa_dense.h (host / device code; tests/native/conv_harness.cpp and
// tests/native/trunk_harness.cpp check them against brute-force enumerations): which cells a tile owns, where a (cell, tap) lies in
// the tile's staged window, which window positions are inside the map (the others are the zero padding), and where a weight sits in
// the packed planes.  One rule in (taps, s, d): taps 9 (3 x 3, zero padding d) or 1 (1 x 1, no padding), stride s, dilation d;
// valid() names the combinations that exist -- the heads (vfa_conv.hip) are (9, 1, 1..4), the trunk (vfa_trunk.hip) (9 | 1, 1 | 2, 1).
// A third family, the BLOCKS 10 r + c (11, 12, 21, 22; stride 1, no padding): r x c taps that reach down and right, tap t = c dy + dx
// reading map position (y + dy, x + dx) -- the four parity classes of a stride-2 convolution's input gradient (vfa_conv_grad.h).
//
// The output is (Lo, Wo) = (out_size(L, s), out_size(W, s)).  A tile is kTileRows x kTileCols OUTPUT cells of one frame and kTileOut
// outputs; the output cell (ry, rx) of the tile at (y0, x0) is output position (y0 + ry, x0 + rx).
//   taps 9: the window is (s (kTileRows - 1) + 2 d + 1) x (s (kTileCols - 1) + 2 d + 1) positions, window position (wy, wx) being map
//       position (s y0 - d + wy, s x0 - d + wx); tap t = 3 ty + tx of the cell (ry, rx) reads window position (s ry + ty d, s rx + tx d):
//       map position (s y + (ty - 1) d, s x + (tx - 1) d).
//   taps 1: the window is the tile itself, window position (wy, wx) being map position (s (y0 + wy), s (x0 + wx)).
//   block r x c: the window is (kTileRows + r - 1) x (kTileCols + c - 1) positions from map position (y0, x0); tap t of the cell
//       (ry, rx) reads window position (ry + t / c, rx + t % c).
// Where a window position lies in LDS is its LOCATION.  At stride 1 (and with one tap) location = wy cols + wx.  At stride 2 the even
// window columns of a row come first and the odd ones behind them: the 32 cells of an MFMA operand read tap tx at the columns
// 2 rx + tx, which are 32 CONSECUTIVE locations of one half (tx = 0: even rx; tx = 1: odd rx; tx = 2: even rx + 1), so their 80-byte
// rows fall on the banks as they do at stride 1 (16 lanes: 20 k mod 64 dwords, sixteen disjoint quads) instead of two-way onto eight.
//
// Packed weights: two fp16 planes (hi, lo) in slices of one (output tile, chunk of 32 channels, tap), `taps` slices per (output tile,
// chunk): a slice is [piece][4 groups of 8 channels][kTileOut outputs][8 channels], 16 KiB, copied to LDS as it lies; outputs past O
// are zeros.
#ifndef VFA_CONV_H
#define VFA_CONV_H
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VFA_CONV_HD __host__ __device__ inline
#else
#define VFA_CONV_HD inline
#endif

namespace vfa_conv {

constexpr int kTaps = 9;
constexpr int kTileRows = 4;   // output rows of a tile: one 32-cell MFMA operand each
constexpr int kTileCols = 32;  // output columns of a tile
constexpr int kTileOut = 128;  // outputs of a tile
constexpr int kChunkC = 32;    // channels staged at a time (C % 32 == 0)
constexpr int kMaxDilation = 4;
constexpr int kLocHalves = 40; // fp16 values per window location in LDS: 32 channels + 8 of padding (80 bytes, 16-byte aligned)
constexpr int kSliceHalves = 2 * kChunkC * kTileOut; // one (output tile, chunk, tap) slice: both pieces
constexpr int kPackHeaderBytes = 64; // word 0: the bit pattern of the weight's absmax
constexpr int kSplitC = 256; // more channels than this: two accumulator chains, one per half of the chunks (the trunk's kernels)

VFA_CONV_HD bool valid(int taps, int s, int d)
{
    if (taps == 9) return s == 1 ? d >= 1 && d <= kMaxDilation : s == 2 && d == 1;
    return taps == 1 && (s == 1 || s == 2) && d == 1;
}
// the blocks of taps and how many taps a code has (9 and 1 are their own count)
VFA_CONV_HD constexpr bool is_block(int taps) { return taps == 11 || taps == 12 || taps == 21 || taps == 22; }
VFA_CONV_HD constexpr int tap_count(int taps) { return is_block(taps) ? (taps / 10) * (taps % 10) : taps; }
VFA_CONV_HD int out_size(int n, int s) { return n < 1 ? 0 : (n - 1) / s + 1; }
VFA_CONV_HD int tiles_x(int Wo) { return (Wo + kTileCols - 1) / kTileCols; }
VFA_CONV_HD int tiles_y(int Lo) { return (Lo + kTileRows - 1) / kTileRows; }
VFA_CONV_HD int out_tiles(int O) { return (O + kTileOut - 1) / kTileOut; }
VFA_CONV_HD constexpr int window_rows(int taps, int s, int d)
{
    return taps == 9 ? s * (kTileRows - 1) + 2 * d + 1 : is_block(taps) ? kTileRows + taps / 10 - 1 : kTileRows;
}
VFA_CONV_HD constexpr int window_cols(int taps, int s, int d)
{
    return taps == 9 ? s * (kTileCols - 1) + 2 * d + 1 : is_block(taps) ? kTileCols + taps % 10 - 1 : kTileCols;
}
VFA_CONV_HD constexpr int window_locations(int taps, int s, int d) { return window_rows(taps, s, d) * window_cols(taps, s, d); }
// chunks of the first accumulator chain (all of them up to kSplitC channels)
VFA_CONV_HD int first_chunks(int C) { return C > kSplitC ? (C / kChunkC + 1) / 2 : C / kChunkC; }

// tile index (0 .. tiles_x * tiles_y - 1) of the OUTPUT map -> the output position of its first cell
VFA_CONV_HD void tile_origin(int tile, int Wo, int &y0, int &x0)
{
    const int tx = tiles_x(Wo);
    y0 = (tile / tx) * kTileRows;
    x0 = (tile % tx) * kTileCols;
}

// window position (wy, wx) -> location in LDS
VFA_CONV_HD int window_location(int wy, int wx, int taps, int s, int d)
{
    const int wc = window_cols(taps, s, d);
    if (taps == 9 && s == 2) return wy * wc + (wx & 1) * ((wc + 1) / 2) + wx / 2;
    return wy * wc + wx;
}

// location of tap t of the tile's output cell (ry, rx)
VFA_CONV_HD int tap_location(int ry, int rx, int t, int taps, int s, int d)
{
    if (taps == 1) return window_location(ry, rx, taps, s, d);
    if (is_block(taps)) return window_location(ry + t / (taps % 10), rx + t % (taps % 10), taps, s, d);
    return window_location(s * ry + (t / 3) * d, s * rx + (t % 3) * d, taps, s, d);
}

// window position p = wy cols + wx (the order the window is loaded in) of the tile at output (y0, x0) -> map position; false:
// outside the map (zero padding, or past the last strided position; no address is formed)
VFA_CONV_HD bool window_position(int p, int y0, int x0, int taps, int s, int d, int L, int W, int &y, int &x)
{
    const int wc = window_cols(taps, s, d); // (wy, wx) = (p / wc, p % wc)
    if (taps == 9) {
        y = s * y0 - d + p / wc;
        x = s * x0 - d + p % wc;
    } else {
        y = s * (y0 + p / wc);
        x = s * (x0 + p % wc);
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

// the 3 x 3, stride-1 forms of the weight gradient (vfa_conv_grad.hip) and of tests/native/conv_harness.cpp, where location = window
// position
VFA_CONV_HD constexpr int window_locations(int d) { return window_locations(kTaps, 1, d); }
VFA_CONV_HD int window_index(int ry, int rx, int t, int d) { return tap_location(ry, rx, t, kTaps, 1, d); }
VFA_CONV_HD bool window_position(int loc, int y0, int x0, int d, int L, int W, int &y, int &x)
{
    return window_position(loc, y0, x0, kTaps, 1, d, L, W, y, x);
}
VFA_CONV_HD size_t packed_halves(int O, int C) { return packed_halves(O, C, kTaps); }
VFA_CONV_HD size_t packed_index(int o, int c, int t, int piece, int C) { return packed_index(o, c, t, piece, C, kTaps); }

// host side, defined in vfa_conv.hip: per frame b the maximum of the bit patterns of the finite |x[b]| into absmax[b] (merged with an
// integer atomicMax: the caller zeroes absmax[0 .. B - 1] on the stream first) -- the operand's power-of-two scale of vfa_split.h.
// x (B, C, L, W) is read through its four element strides.  0, or the error of the entry points (an empty map launches nothing).
int frame_absmax(const float *x, const long long *stride, int B, int C, int L, int W, unsigned *absmax, void *stream);
// ... of the values max(fmaf(a[b, c], x, b[b, c]), 0) behind the prologue of vfa_dense.h (a, b: (B, C) floats, or both nullptr: x itself)
int frame_absmax(const float *x, const long long *stride, const float *a, const float *b, int B, int C, int L, int W, unsigned *absmax, void *stream);

#if defined(__HIPCC__)
// host side: hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel ON A DEVICE, so a launcher keeps one of these per kernel
// instantiation (`static DynamicLds lds;`) and asks it before every launch: one flag per device (past kDevices the call is made
// every time).  Idempotent: a race only repeats the call.  0, or the HIP error.
struct DynamicLds {
    static constexpr int kDevices = 64;
    bool set[kDevices] = {};
    int allow(const void *kernel, int bytes)
    {
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return (int)e;
        if (device >= 0 && device < kDevices && set[device]) return 0;
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess && device >= 0 && device < kDevices) set[device] = true;
        return (int)e;
    }
};
#endif

} // namespace vfa_conv
#endif // VFA_CONV_H
