// The integer rules of the dense 3x3 convolution (vfa_amd/csrc/vfa_conv.h, shared host / device code) on the CPU, against a
// brute-force enumeration that shares nothing with them.
//
//   harness tiles     maps from 1 x 1 to 20 x 37 (and a few wider ones), dilations 1, 2 and 4, maps smaller than the dilation: every
//                     cell of the map lies in exactly one tile; every window location of a tile is the map position the definition
//                     gives, inside the map exactly when that position is; tap t of a cell reads the window location that holds
//                     position (y + (ty - 1) d, x + (tx - 1) d), inside the window's bounds.
//   harness weights   the packed-weight index is a bijection of (o, c, tap, piece) with o < the padded O onto [0, packed_halves),
//                     a slice is contiguous, and within a (piece, group of 8 channels) the outputs of a tile are 8 values apart.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_conv.h"

using namespace vfa_conv;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

static long long cells_checked, taps_checked, taps_outside, locations_checked, weights_checked;

static void check_map(int L, int W, int d)
{
    const int n_tiles = tiles_x(W) * tiles_y(L);
    std::vector<int> owner((size_t)L * W, -1);
    for (int tile = 0; tile < n_tiles; ++tile) {
        int y0 = -1, x0 = -1;
        tile_origin(tile, W, y0, x0);
        CHECK(y0 >= 0 && y0 < L && x0 >= 0 && x0 < W && y0 % kTileRows == 0 && x0 % kTileCols == 0, "tile %d of %d x %d: origin (%d, %d)", tile,
              L, W, y0, x0);
        // the window: every location against the definition
        std::vector<int> pos_y(window_locations(d)), pos_x(window_locations(d));
        for (int wy = 0; wy < kTileRows + 2 * d; ++wy)
            for (int wx = 0; wx < kTileCols + 2 * d; ++wx) {
                const int loc = wy * (kTileCols + 2 * d) + wx;
                CHECK(loc < window_locations(d), "location %d of %d", loc, window_locations(d));
                int y = -99, x = -99;
                const bool got = window_position(loc, y0, x0, d, L, W, y, x);
                const int my = y0 - d + wy, mx = x0 - d + wx;
                CHECK(y == my && x == mx, "location %d: (%d, %d), want (%d, %d)", loc, y, x, my, mx);
                CHECK(got == (my >= 0 && my < L && mx >= 0 && mx < W), "location %d of tile %d, %d x %d d %d", loc, tile, L, W, d);
                pos_y[loc] = my;
                pos_x[loc] = mx;
                ++locations_checked;
            }
        for (int ry = 0; ry < kTileRows; ++ry)
            for (int rx = 0; rx < kTileCols; ++rx) {
                const int y = y0 + ry, x = x0 + rx;
                if (y < L && x < W) {
                    CHECK(owner[(size_t)y * W + x] == -1, "cell (%d, %d) has two tiles", y, x);
                    owner[(size_t)y * W + x] = tile;
                    ++cells_checked;
                }
                for (int ty = 0; ty < 3; ++ty) // (cells past the map's edge compute too: their reads must stay inside the window)
                    for (int tx = 0; tx < 3; ++tx) {
                        const int loc = window_index(ry, rx, 3 * ty + tx, d);
                        CHECK(loc >= 0 && loc < window_locations(d), "cell (%d, %d) tap %d: location %d", ry, rx, 3 * ty + tx, loc);
                        const int wy = y + (ty - 1) * d, wx = x + (tx - 1) * d;
                        CHECK(pos_y[loc] == wy && pos_x[loc] == wx, "cell (%d, %d) tap %d reads (%d, %d), want (%d, %d)", y, x, 3 * ty + tx,
                              pos_y[loc], pos_x[loc], wy, wx);
                        ++taps_checked;
                        if (!(wy >= 0 && wy < L && wx >= 0 && wx < W)) ++taps_outside;
                    }
            }
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] >= 0, "cell %zu of %d x %d has no tile", i, L, W);
}

static void check_weights(int O, int C)
{
    const size_t n = packed_halves(O, C);
    const int o_pad = out_tiles(O) * kTileOut;
    CHECK(n == (size_t)o_pad * C * kTaps * 2, "packed_halves(%d, %d) = %zu", O, C, n);
    std::vector<unsigned char> seen(n, 0);
    for (int piece = 0; piece < 2; ++piece)
        for (int o = 0; o < o_pad; ++o)
            for (int c = 0; c < C; ++c)
                for (int t = 0; t < kTaps; ++t) {
                    const size_t at = packed_index(o, c, t, piece, C);
                    CHECK(at < n, "(%d, %d, %d, %d) -> %zu of %zu", o, c, t, piece, at, n);
                    CHECK(!seen[at], "(%d, %d, %d, %d): index %zu twice", o, c, t, piece, at);
                    seen[at] = 1;
                    const size_t slice = ((size_t)(o / kTileOut) * (C / kChunkC) + c / kChunkC) * kTaps + t;
                    CHECK(at / kSliceHalves == slice, "(%d, %d, %d, %d): slice %zu, want %zu", o, c, t, piece, at / kSliceHalves, slice);
                    if (c % 8 != 7) CHECK(packed_index(o, c + 1, t, piece, C) == at + 1, "8 channels are not contiguous");
                    if (o % kTileOut != kTileOut - 1) CHECK(packed_index(o + 1, c, t, piece, C) == at + 8, "outputs are not 8 values apart");
                    ++weights_checked;
                }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "tiles")) {
        const int ds[3] = {1, 2, 4};
        for (int d : ds) {
            for (int L = 1; L <= 20; ++L)
                for (int W = 1; W <= 37; ++W) check_map(L, W, d);
            check_map(3, 70, d);
            check_map(37, 70, d);
            check_map(9, 129, d);
        }
        check_map(2, 3, 3);
        std::printf("ok %lld cells %lld taps %lld outside %lld locations\n", cells_checked, taps_checked, taps_outside, locations_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "weights")) {
        check_weights(1, 32);
        check_weights(40, 64);
        check_weights(128, 32);
        check_weights(129, 32);
        check_weights(360, 256);
        std::printf("ok %lld weights\n", weights_checked);
        return 0;
    }
    std::printf("usage: harness tiles | weights\n");
    return 2;
}
