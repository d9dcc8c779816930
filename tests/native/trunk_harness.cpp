// The integer rules of the dense convolution kernel in (taps, stride, dilation) (vfa_amd/csrc/vfa_conv.h, shared host / device code)
// on the CPU, against a brute-force enumeration that shares nothing with them.
//
//   harness tiles     taps 1 and 9 with strides 1 and 2 (the trunk), and nine taps at stride 1 with dilations 2..4 (the heads), maps
//                     from 1 x 1 to 20 x 70: the output size is the number of strided positions; every output cell lies in exactly
//                     one tile; every window position of a tile is the map position the definition gives, inside the map exactly
//                     when that position is; the locations of a window are a bijection onto [0, window_locations); tap t of an
//                     output cell reads the location that holds map position (s y + (ty - 1) d, s x + (tx - 1) d) (one tap: (s y,
//                     s x)); the 32 cells of a tile row read 32 consecutive locations for every tap.  The stride-1 forms that take
//                     the dilation alone (the weight gradient's) agree with the general rule for every (ry, rx, t, d) and every
//                     window location.  valid() accepts these combinations and no other.
//   harness weights   the packed-weight index with `taps` slices per (output tile, chunk) is a bijection of (o, c, tap, piece) with
//                     o < the padded O onto [0, packed_halves); with one tap a slice is one chunk; with nine it is the five-argument
//                     form's.
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

static long long cells_checked, taps_checked, taps_outside, locations_checked, weights_checked, wrappers_checked;

static void check_map(int L, int W, int taps, int s, int d)
{
    const int pad = taps == 9 ? d : 0, k = taps == 9 ? 3 : 1;
    int Lo = 0, Wo = 0;
    for (int y = 0; y < L; y += s) ++Lo;
    for (int x = 0; x < W; x += s) ++Wo;
    CHECK(out_size(L, s) == Lo && out_size(W, s) == Wo, "%d x %d stride %d: output %d x %d, want %d x %d", L, W, s, out_size(L, s), out_size(W, s), Lo,
          Wo);
    const int rows = (kTileRows - 1) * s + (k - 1) * d + 1, cols = (kTileCols - 1) * s + (k - 1) * d + 1, n_loc = rows * cols; // the span of the tile's taps
    CHECK(window_rows(taps, s, d) == (taps == 9 ? rows : kTileRows) && window_cols(taps, s, d) == (taps == 9 ? cols : kTileCols), "window %d x %d",
          window_rows(taps, s, d), window_cols(taps, s, d));
    const int wr = window_rows(taps, s, d), wc = window_cols(taps, s, d);
    CHECK(window_locations(taps, s, d) == wr * wc && (taps == 1 || wr * wc == n_loc), "window of %d locations", window_locations(taps, s, d));
    const int n_tiles = tiles_x(Wo) * tiles_y(Lo);
    std::vector<int> owner((size_t)Lo * Wo, -1);
    for (int tile = 0; tile < n_tiles; ++tile) {
        int y0 = -1, x0 = -1;
        tile_origin(tile, Wo, y0, x0);
        CHECK(y0 >= 0 && y0 < Lo && x0 >= 0 && x0 < Wo && y0 % kTileRows == 0 && x0 % kTileCols == 0, "tile %d: origin (%d, %d)", tile, y0, x0);
        std::vector<int> pos_y(wr * wc, -99), pos_x(wr * wc, -99);
        std::vector<unsigned char> used(wr * wc, 0);
        for (int wy = 0; wy < wr; ++wy)
            for (int wx = 0; wx < wc; ++wx) {
                int y = -99, x = -99;
                const bool got = window_position(wy * wc + wx, y0, x0, taps, s, d, L, W, y, x);
                // nine taps: the window starts the padding in front of the tile's first tap centre; one tap: the strided positions alone
                const int my = taps == 9 ? s * y0 - pad + wy : s * (y0 + wy), mx = taps == 9 ? s * x0 - pad + wx : s * (x0 + wx);
                CHECK(y == my && x == mx, "window (%d, %d): (%d, %d), want (%d, %d)", wy, wx, y, x, my, mx);
                CHECK(got == (my >= 0 && my < L && mx >= 0 && mx < W), "window (%d, %d) of tile %d, %d x %d taps %d stride %d dilation %d", wy, wx, tile,
                      L, W, taps, s, d);
                const int loc = window_location(wy, wx, taps, s, d);
                CHECK(loc >= 0 && loc < wr * wc && !used[loc], "window (%d, %d): location %d of %d", wy, wx, loc, wr * wc);
                used[loc] = 1;
                pos_y[loc] = my;
                pos_x[loc] = mx;
                ++locations_checked;
                if (taps == 9 && s == 1) { // the dilation-only form: location = window position
                    int y1 = -99, x1 = -99;
                    const bool got1 = window_position(loc, y0, x0, d, L, W, y1, x1);
                    CHECK(loc == wy * wc + wx && got1 == got && y1 == y && x1 == x, "window (%d, %d) dilation %d: the dilation-only form gives (%d, %d)",
                          wy, wx, d, y1, x1);
                    ++wrappers_checked;
                }
            }
        for (int ry = 0; ry < kTileRows; ++ry)
            for (int rx = 0; rx < kTileCols; ++rx) {
                const int y = y0 + ry, x = x0 + rx;
                if (y < Lo && x < Wo) {
                    CHECK(owner[(size_t)y * Wo + x] == -1, "cell (%d, %d) has two tiles", y, x);
                    owner[(size_t)y * Wo + x] = tile;
                    ++cells_checked;
                }
                for (int t = 0; t < taps; ++t) { // (cells past the output's edge compute too: their reads must stay inside the window)
                    const int ty = t / k, tx = t % k;
                    const int loc = tap_location(ry, rx, t, taps, s, d);
                    CHECK(loc >= 0 && loc < wr * wc, "cell (%d, %d) tap %d: location %d", ry, rx, t, loc);
                    const int my = s * y - pad + ty * d, mx = s * x - pad + tx * d;
                    CHECK(pos_y[loc] == my && pos_x[loc] == mx, "cell (%d, %d) tap %d reads (%d, %d), want (%d, %d)", y, x, t, pos_y[loc], pos_x[loc], my,
                          mx);
                    if (rx > 0) CHECK(loc == tap_location(ry, rx - 1, t, taps, s, d) + 1, "cell (%d, %d) tap %d: the row's locations are not consecutive", ry, rx, t);
                    if (taps == 9 && s == 1) {
                        CHECK(window_index(ry, rx, t, d) == loc, "cell (%d, %d) tap %d dilation %d: the dilation-only form gives %d, want %d", ry, rx, t, d,
                              window_index(ry, rx, t, d), loc);
                        ++wrappers_checked;
                    }
                    ++taps_checked;
                    if (!(my >= 0 && my < L && mx >= 0 && mx < W)) ++taps_outside;
                }
            }
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] >= 0, "cell %zu of %d x %d has no tile", i, Lo, Wo);
}

static void check_maps(int taps, int s, int d)
{
    CHECK(valid(taps, s, d), "taps %d stride %d dilation %d", taps, s, d);
    for (int L = 1; L <= 20; ++L)
        for (int W = 1; W <= 70; ++W) check_map(L, W, taps, s, d);
    check_map(37, 131, taps, s, d);
}

static void check_weights(int O, int C, int taps)
{
    const size_t n = packed_halves(O, C, taps);
    const int o_pad = out_tiles(O) * kTileOut;
    CHECK(n == (size_t)o_pad * C * taps * 2, "packed_halves(%d, %d, %d) = %zu", O, C, taps, n);
    if (taps == 9) CHECK(n == packed_halves(O, C), "nine taps: not the two-argument packed_halves");
    std::vector<unsigned char> seen(n, 0);
    for (int piece = 0; piece < 2; ++piece)
        for (int o = 0; o < o_pad; ++o)
            for (int c = 0; c < C; ++c)
                for (int t = 0; t < taps; ++t) {
                    const size_t at = packed_index(o, c, t, piece, C, taps);
                    CHECK(at < n, "(%d, %d, %d, %d) -> %zu of %zu", o, c, t, piece, at, n);
                    CHECK(!seen[at], "(%d, %d, %d, %d): index %zu twice", o, c, t, piece, at);
                    seen[at] = 1;
                    const size_t slice = ((size_t)(o / kTileOut) * (C / kChunkC) + c / kChunkC) * taps + t;
                    CHECK(at / kSliceHalves == slice, "(%d, %d, %d, %d): slice %zu, want %zu", o, c, t, piece, at / kSliceHalves, slice);
                    if (taps == 1) CHECK(at / kSliceHalves == (size_t)(o / kTileOut) * (C / kChunkC) + c / kChunkC, "one tap: a slice is one chunk");
                    if (taps == 9) CHECK(at == packed_index(o, c, t, piece, C), "nine taps: not the five-argument packed_index");
                    if (c % 8 != 7) CHECK(packed_index(o, c + 1, t, piece, C, taps) == at + 1, "8 channels are not contiguous");
                    if (o % kTileOut != kTileOut - 1) CHECK(packed_index(o + 1, c, t, piece, C, taps) == at + 8, "outputs are not 8 values apart");
                    ++weights_checked;
                }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "tiles")) {
        for (int taps = 1; taps <= 9; taps += 8)
            for (int s = 1; s <= 2; ++s) check_maps(taps, s, 1);
        for (int d = 2; d <= kMaxDilation; ++d) check_maps(9, 1, d);
        CHECK(wrappers_checked > 0, "the dilation-only forms were not compared");
        CHECK(!valid(3, 1, 1) && !valid(9, 3, 1) && !valid(9, 0, 1) && !valid(0, 1, 1), "valid()");
        CHECK(!valid(9, 2, 2) && !valid(1, 1, 2) && !valid(9, 1, 5) && !valid(9, 1, 0) && !valid(1, 2, 0), "valid() and the dilation");
        CHECK(first_chunks(64) == 2 && first_chunks(256) == 8 && first_chunks(288) == 5 && first_chunks(512) == 8, "first_chunks");
        std::printf("ok %lld cells %lld taps %lld outside %lld locations\n", cells_checked, taps_checked, taps_outside, locations_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "weights")) {
        for (int taps = 1; taps <= 9; taps += 8) {
            check_weights(1, 32, taps);
            check_weights(40, 64, taps);
            check_weights(129, 32, taps);
            check_weights(160, 512, taps);
        }
        std::printf("ok %lld weights\n", weights_checked);
        return 0;
    }
    std::printf("usage: harness tiles | weights\n");
    return 2;
}
