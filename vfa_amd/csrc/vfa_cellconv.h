// vfa_cellconv.h -- the integer logic of the 3x3 convolution at listed cells (vfa_cellconv.hip) as plain host / device code: which
// cells are rows at all, where the nine taps of a cell lie, which of them the zero border removes, and which (row, tap) pair writes
// a location of the input gradient.  The kernels run these functions from their threads; tests/native/cellconv_harness.cpp compiles
// this file with g++ and checks them against a brute-force enumeration of small grids.
//
// The problem: a map of L x W cells, a dilation d >= 1, zero padding d ("same").  A ROW is one entry of the cell list of a frame:
// a flat index l * W + w.  An entry outside [0, L * W) -- the decode writes -1 behind a frame's count -- is a SKIPPED row: nothing
// is read for it and no address is formed from it.  Tap t = 3 * ty + tx (the weight's last two axes) of a row lies at
// (l + (ty - 1) d, w + (tx - 1) d); a tap outside the map contributes nothing.
//
// The gradient's ownership rule.  The input gradient at a location (y, x) of a frame is the sum over the PAIRS (row, tap) of that
// frame whose tap lies on (y, x); a row has at most one such tap (`tap_landing_on`), since its nine taps lie on nine different
// locations.  Several rows can share a location: cells exactly d apart in a row, a column or a diagonal, and duplicate cells.  The
// location is written once, by the LOWEST pair that lies on it, i.e. by the lowest such row (`pair_owns`); that owner adds the
// pairs in ASCENDING (row, tap) order, its own first, and inside a pair the output channels in ascending order.  No location has
// two writers, so there is no atomic and every run gives the same bits.
#ifndef VFA_CELLCONV_H
#define VFA_CELLCONV_H

#if defined(__HIPCC__)
#define VFA_CELLCONV_HD __host__ __device__ __forceinline__
#else
#define VFA_CELLCONV_HD inline
#endif

namespace vfa_cellconv {

constexpr int kTaps = 9;
constexpr int kMaxRows = 1024; // rows of one frame the backward searches in LDS (the decode's VFA_BEV_DECODE_MAX_TOPK)

VFA_CELLCONV_HD bool cell_valid(long long cell, int L, int W) { return cell >= 0 && cell < (long long)L * (long long)W; }

// where tap t of a valid cell lies; false: outside the map (the zero border), y and x are then not written
VFA_CELLCONV_HD bool tap_location(int cell, int t, int L, int W, int dilation, int &y, int &x)
{
    const int l = cell / W, w = cell - l * W;
    const long long yy = (long long)l + (long long)(t / 3 - 1) * dilation, xx = (long long)w + (long long)(t % 3 - 1) * dilation;
    if (yy < 0 || yy >= L || xx < 0 || xx >= W) return false;
    y = (int)yy;
    x = (int)xx;
    return true;
}

// the tap of a valid cell that lies on location (y, x) of the map, -1: none
VFA_CELLCONV_HD int tap_landing_on(int cell, int y, int x, int W, int dilation)
{
    const int l = cell / W, w = cell - l * W;
    const long long ry = (long long)y - l, rx = (long long)x - w, d = dilation;
    const int ty = ry == -d ? 0 : ry == 0 ? 1 : ry == d ? 2 : -1;
    const int tx = rx == -d ? 0 : rx == 0 ? 1 : rx == d ? 2 : -1;
    return ty < 0 || tx < 0 ? -1 : 3 * ty + tx;
}

// `cells`: the k entries of one frame.  Does pair (row, tap) write its location?  False also for a skipped row and a tap outside.
VFA_CELLCONV_HD bool pair_owns(const int *cells, int row, int tap, int L, int W, int dilation)
{
    int y, x;
    if (!cell_valid(cells[row], L, W) || !tap_location(cells[row], tap, L, W, dilation, y, x)) return false;
    for (int j = 0; j < row; ++j)
        if (cell_valid(cells[j], L, W) && tap_landing_on(cells[j], y, x, W, dilation) >= 0) return false;
    return true;
}

} // namespace vfa_cellconv
#endif // VFA_CELLCONV_H
