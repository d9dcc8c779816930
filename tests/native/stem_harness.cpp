// The integer rules of the trunk's stem (vfa_amd/csrc/vfa_stem.h, shared host / device code) on the CPU, against a brute-force
// enumeration that shares nothing with them.
//
//   harness conv      images from 1 x 1 to 20 x 150 and 37 x 131: the output size is the number of 7-wide stride-2 windows of the
//                     image padded by 3; every output cell lies in exactly one tile; every window position of a tile is the channel
//                     and image position the definition gives, inside the image exactly when that position is.  Once, for every cell
//                     of a tile and every k: the locations of a window are distinct and inside [0, kWinLocations); k is (c, ky, kx) in
//                     the weight's own order; tap k of cell (ry, rx) reads the location that holds window position
//                     (2 ry + ky, 2 rx + kx) of channel c; the 32 cells of a tile row read 32 consecutive locations; the upper
//                     half-wave's tap of a k pair lies pair_delta(pair_slot) behind the lower one's.
//   harness weights   the packed-weight index is a bijection of (o < 64, k < 148) onto [0, kPackedFloats); a lane's two outputs r and
//                     32 + r are neighbours, and the rows of k are 64 floats apart.
//   harness pool      axes of 1 .. 300 positions: the output size is the number of 3-wide stride-2 windows of the axis padded by 1,
//                     and pool_first .. pool_last are exactly the window's taps inside the axis, at least one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_stem.h"

using namespace vfa_stem;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

static long long cells_checked, positions_checked, positions_outside, taps_checked, weights_checked, windows_checked;

// windows of `width` positions at stride 2 that fit the axis of n positions padded by `pad` on both sides
static int windows_of(int n, int width, int pad)
{
    int count = 0;
    for (int start = 0; start + width <= n + 2 * pad; start += 2) ++count;
    return count;
}

static void check_image(int L, int W)
{
    const int Lo = windows_of(L, 7, 3), Wo = windows_of(W, 7, 3);
    CHECK(conv_out(L) == Lo && conv_out(W) == Wo, "%d x %d: output %d x %d, want %d x %d", L, W, conv_out(L), conv_out(W), Lo, Wo);
    const int n_tiles = tiles_x(Wo) * tiles_y(Lo);
    std::vector<int> owner((size_t)Lo * Wo, -1);
    for (int tile = 0; tile < n_tiles; ++tile) {
        int y0 = -1, x0 = -1;
        tile_origin(tile, Wo, y0, x0);
        CHECK(y0 >= 0 && y0 < Lo && x0 >= 0 && x0 < Wo && y0 % kTileRows == 0 && x0 % kTileCols == 0, "tile %d: origin (%d, %d)", tile, y0, x0);
        for (int ry = 0; ry < kTileRows; ++ry)
            for (int rx = 0; rx < kTileCols; ++rx) {
                const int y = y0 + ry, x = x0 + rx;
                if (y >= Lo || x >= Wo) continue;
                CHECK(owner[(size_t)y * Wo + x] == -1, "cell (%d, %d) has two tiles", y, x);
                owner[(size_t)y * Wo + x] = tile;
                ++cells_checked;
            }
        int p = 0;
        for (int c = 0; c < 3; ++c)
            for (int wy = 0; wy < 13; ++wy)
                for (int wx = 0; wx < 69; ++wx, ++p) {
                    int gc = -9, gy = -99, gx = -99;
                    const bool got = window_position(p, y0, x0, L, W, gc, gy, gx);
                    // the first tap of the tile's first cell lies three positions in front of twice the cell's position
                    const int my = 2 * y0 - 3 + wy, mx = 2 * x0 - 3 + wx;
                    CHECK(gc == c && gy == my && gx == mx, "window %d: (%d, %d, %d), want (%d, %d, %d)", p, gc, gy, gx, c, my, mx);
                    const bool inside = my >= 0 && my < L && mx >= 0 && mx < W;
                    CHECK(got == inside, "window %d of tile %d, %d x %d", p, tile, L, W);
                    ++positions_checked;
                    if (!inside) ++positions_outside;
                }
        CHECK(p == kWinValues, "%d window positions", p);
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] >= 0, "cell %zu of %d x %d has no tile", i, Lo, Wo);
}

static void check_taps()
{
    CHECK(kWinRows == 13 && kWinCols == 69 && kK == 147 && kKPad == 148 && kSteps == 74 && kKPad % 2 == 0 && kKPad >= kK, "constants");
    std::vector<int> pos_c(kWinLocations, -1), pos_y(kWinLocations, -1), pos_x(kWinLocations, -1);
    for (int c = 0; c < 3; ++c)
        for (int wy = 0; wy < 13; ++wy)
            for (int wx = 0; wx < 69; ++wx) {
                const int loc = window_location(c, wy, wx);
                CHECK(loc >= 0 && loc < kWinLocations && pos_c[loc] == -1, "window (%d, %d, %d): location %d", c, wy, wx, loc);
                pos_c[loc] = c;
                pos_y[loc] = wy;
                pos_x[loc] = wx;
            }
    for (int ry = 0; ry < kTileRows; ++ry)
        for (int rx = 0; rx < kTileCols; ++rx) {
            int k = 0;
            for (int c = 0; c < 3; ++c) // the order the weight (O, 3, 7, 7) lies in
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx, ++k) {
                        CHECK(k_channel(k) == c && k_row(k) == ky && k_col(k) == kx, "k %d: (%d, %d, %d)", k, k_channel(k), k_row(k), k_col(k));
                        const int loc = cell_base(ry, rx) + tap_offset(k);
                        CHECK(loc >= 0 && loc < kWinLocations, "cell (%d, %d) k %d: location %d", ry, rx, k, loc);
                        CHECK(pos_c[loc] == c && pos_y[loc] == 2 * ry + ky && pos_x[loc] == 2 * rx + kx, "cell (%d, %d) k %d reads (%d, %d, %d)", ry, rx, k,
                              pos_c[loc], pos_y[loc], pos_x[loc]);
                        if (rx > 0) CHECK(loc == cell_base(ry, rx - 1) + tap_offset(k) + 1, "cell (%d, %d) k %d: the row's locations are not consecutive", ry, rx, k);
                        ++taps_checked;
                    }
            CHECK(k == kK, "%d taps", k);
            for (int kp = kK; kp < kKPad; ++kp) { // a padded k reads SOME location of the window (its value is replaced by a zero)
                const int loc = cell_base(ry, rx) + tap_offset(kp);
                CHECK(loc >= 0 && loc < kWinLocations, "cell (%d, %d) padded k %d: location %d", ry, rx, kp, loc);
            }
        }
    for (int s = 0; s < kSteps; ++s) {
        const int slot = pair_slot(s);
        CHECK(slot >= 0 && slot < kPairDeltas, "pair %d: slot %d", s, slot);
        CHECK(tap_offset(2 * s + 1) == tap_offset(2 * s) + pair_delta(slot), "pair %d: %d and %d, slot %d", s, tap_offset(2 * s), tap_offset(2 * s + 1), slot);
    }
    for (int a = 0; a < kPairDeltas; ++a)
        for (int b = a + 1; b < kPairDeltas; ++b) CHECK(pair_delta(a) != pair_delta(b), "pair deltas %d and %d are equal", a, b);
}

static void check_weights()
{
    std::vector<unsigned char> seen(kPackedFloats, 0);
    CHECK(kPackedFloats == 64 * 148 && kMaxOut == 64, "packed size %d", kPackedFloats);
    for (int o = 0; o < 64; ++o)
        for (int k = 0; k < 148; ++k) {
            const int at = packed_index(o, k);
            CHECK(at >= 0 && at < kPackedFloats && !seen[at], "(%d, %d): index %d", o, k, at);
            seen[at] = 1;
            CHECK(at / 64 == k, "(%d, %d): row %d", o, k, at / 64);
            if (o < 32) CHECK(packed_index(o + 32, k) == at + 1 && at % 2 == 0, "(%d, %d): the lane's second output is not its neighbour", o, k);
            if (o % 32 != 31) CHECK(packed_index(o + 1, k) == at + 2, "(%d, %d): the next lane's pair is not 8 bytes on", o, k);
            ++weights_checked;
        }
}

static void check_pool(int n)
{
    const int want = windows_of(n, 3, 1);
    CHECK(pool_out(n) == want, "axis %d: %d outputs, want %d", n, pool_out(n), want);
    for (int o = 0; o < want; ++o) {
        int first = -1, last = -1;
        for (int t = 2 * o - 1; t <= 2 * o + 1; ++t) // the window's taps, the axis padded by one
            if (t >= 0 && t < n) {
                if (first < 0) first = t;
                last = t;
            }
        CHECK(first >= 0, "axis %d output %d has no tap", n, o);
        CHECK(pool_first(o) == first && pool_last(o, n) == last, "axis %d output %d: taps %d .. %d, want %d .. %d", n, o, pool_first(o), pool_last(o, n), first,
              last);
        ++windows_checked;
    }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "conv")) {
        check_taps();
        for (int L = 1; L <= 20; ++L)
            for (int W = 1; W <= 150; ++W) check_image(L, W);
        check_image(37, 131);
        CHECK(conv_out(0) == 0 && conv_out(-3) == 0 && conv_out(720) == 360 && conv_out(1280) == 640, "conv_out");
        std::printf("ok %lld cells %lld positions %lld outside %lld taps\n", cells_checked, positions_checked, positions_outside, taps_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "weights")) {
        check_weights();
        std::printf("ok %lld weights\n", weights_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "pool")) {
        for (int n = 1; n <= 300; ++n) check_pool(n);
        CHECK(pool_out(0) == 0 && pool_out(360) == 180 && pool_out(640) == 320, "pool_out");
        std::printf("ok %lld windows\n", windows_checked);
        return 0;
    }
    std::printf("usage: harness conv | weights | pool\n");
    return 2;
}
