// The integer rules of the gradients of a stride-2 convolution (vfa_amd/csrc/vfa_conv_grad.h and the blocks of taps of vfa_conv.h,
// shared host / device code) on the CPU, against brute-force enumerations, for L, W in 1 .. 9 and {31, 32, 33, 64, 65, 66}.
//
//   harness classes    the input gradient: every (y, x) of dx lies in exactly one parity class, and the (i, j, ty, tx) its class's block
//                      of taps reads -- through tile_origin, tap_location and window_position as the dense kernel uses them, and
//                      down_source_tap of the packed weight -- are the terms of the defining sum 2 i + ty - 1 = y, 2 j + tx - 1 = x.
//   harness wgrad      the weight gradient, 3 x 3 and 1 x 1: the slabs, tiles and K tiles visit every (cell of g, tap) exactly once;
//                      the tap's location is the location the window's loader gave the position 2 (i, j) + tap - 1 of x (or says it
//                      is outside the map); the locations of a window are distinct and inside the plane; the 32 cells of a row read
//                      32 consecutive locations for every tap; the partials with 9 and with 1 planes are bijections.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_conv_grad.h"

using namespace vfa_conv;
using namespace vfa_conv_grad;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

static const int kSizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 64, 65, 66};
static long long positions_checked, terms_checked, pairs_checked, indices_checked;
typedef std::array<int, 4> Term; // (i, j, ty, tx)

static void check_classes(int L, int W)
{
    const int Lo = out_size(L, 2), Wo = out_size(W, 2);
    std::vector<int> owner((size_t)L * W, 0);
    int launched = 0;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int taps = down_class_taps(py, px), Lc = down_class_size(L, py), Wc = down_class_size(W, px);
            CHECK(is_block(taps) && tap_count(taps) == (1 + py) * (1 + px), "class (%d, %d): block %d", py, px, taps);
            if (Lc == 0 || Wc == 0) continue; // not launched
            ++launched;
            for (int tile = 0; tile < tiles_x(Wc) * tiles_y(Lc); ++tile) {
                int y0, x0;
                tile_origin(tile, Wc, y0, x0);
                for (int ry = 0; ry < kTileRows; ++ry)
                    for (int rx = 0; rx < kTileCols; ++rx) {
                        const int k = y0 + ry, l = x0 + rx;
                        if (k >= Lc || l >= Wc) continue; // (the epilogue's bound)
                        const int y = 2 * k + py, x = 2 * l + px;
                        CHECK(y < L && x < W, "%d x %d: class (%d, %d) cell (%d, %d) is outside dx", L, W, py, px, k, l);
                        ++owner[(size_t)y * W + x];
                        std::vector<Term> got, want;
                        for (int t = 0; t < tap_count(taps); ++t) {
                            const int loc = tap_location(ry, rx, t, taps, 1, 1); // (a block's location is its window position)
                            CHECK(loc >= 0 && loc < window_locations(taps, 1, 1), "block %d: location %d", taps, loc);
                            int i, j;
                            if (!window_position(loc, y0, x0, taps, 1, 1, Lo, Wo, i, j)) continue; // a zero of g
                            const int s = down_source_tap(down_class_first(taps) + t);
                            CHECK(s >= 0 && s < kTaps, "source tap %d", s);
                            got.push_back({i, j, s / 3, s % 3});
                        }
                        for (int i = 0; i < Lo; ++i)
                            for (int j = 0; j < Wo; ++j)
                                for (int ty = 0; ty < 3; ++ty)
                                    for (int tx = 0; tx < 3; ++tx)
                                        if (2 * i + ty - 1 == y && 2 * j + tx - 1 == x) want.push_back({i, j, ty, tx});
                        std::sort(got.begin(), got.end());
                        std::sort(want.begin(), want.end());
                        CHECK(got == want, "%d x %d: dx (%d, %d) has %zu terms, the sum %zu", L, W, y, x, got.size(), want.size());
                        terms_checked += (long long)want.size();
                    }
            }
        }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] == 1, "%d x %d: position %zu lies in %d classes", L, W, i, owner[i]);
    CHECK(launched == (L > 1 ? 2 : 1) * (W > 1 ? 2 : 1), "%d x %d: %d classes", L, W, launched);
    positions_checked += (long long)L * W;
}

static void check_source_taps()
{
    int seen[kTaps] = {};
    for (int t = 0; t < kTaps; ++t) ++seen[down_source_tap(t)];
    for (int s = 0; s < kTaps; ++s) CHECK(seen[s] == 1, "w's tap %d is packed %d times", s, seen[s]);
    CHECK(down_class_first(11) == 0 && down_class_first(21) == 1 && down_class_first(12) == 3 && down_class_first(22) == 5, "the classes' first taps");
}

static void check_wgrad(int L, int W, int taps, int n_slabs)
{
    const int Lo = out_size(L, 2), Wo = out_size(W, 2), n_loc = down_window_locations(taps);
    std::vector<int> position_at((size_t)n_loc, -1); // location -> window position
    for (int p = 0; p < n_loc; ++p) {
        const int loc = down_window_location(p, taps);
        CHECK(loc >= 0 && loc < n_loc && position_at[(size_t)loc] == -1, "taps %d: window position %d -> location %d", taps, p, loc);
        position_at[(size_t)loc] = p;
    }
    std::vector<int> visits((size_t)Lo * Wo * taps, 0);
    CHECK(slab_begin_of(0, n_slabs, Lo, Wo) == 0 && slab_begin_of(n_slabs, n_slabs, Lo, Wo) == tiles(Lo, Wo), "%d x %d: %d slabs", Lo, Wo, n_slabs);
    for (int s = 0; s < n_slabs; ++s)
        for (int k = slab_begin_of(s, n_slabs, Lo, Wo) * kDownHalves; k < slab_begin_of(s + 1, n_slabs, Lo, Wo) * kDownHalves; ++k) {
            int y0, x0;
            down_origin(k / kDownHalves, k % kDownHalves, Wo, y0, x0);
            for (int ry = 0; ry < kDownRows; ++ry)
                for (int rx = 0; rx < kTileCols; ++rx)
                    for (int t = 0; t < taps; ++t) {
                        const int loc = down_tap_location(ry, rx, t, taps);
                        CHECK(loc >= 0 && loc < n_loc, "taps %d: cell (%d, %d) tap %d -> location %d", taps, ry, rx, t, loc);
                        if (rx > 0) CHECK(loc == down_tap_location(ry, rx - 1, t, taps) + 1, "taps %d tap %d: the row's locations are not consecutive", taps, t);
                        const int i = y0 + ry, j = x0 + rx;
                        if (i >= Lo || j >= Wo) continue; // a zero of g
                        int y, x;
                        const bool inside = down_window_position(position_at[(size_t)loc], y0, x0, taps, L, W, y, x);
                        const int wy = taps == 9 ? 2 * i + t / 3 - 1 : 2 * i, wx = taps == 9 ? 2 * j + t % 3 - 1 : 2 * j;
                        CHECK(y == wy && x == wx, "%d x %d taps %d: cell (%d, %d) tap %d reads (%d, %d), not (%d, %d)", L, W, taps, i, j, t, y, x, wy, wx);
                        CHECK(inside == (wy >= 0 && wy < L && wx >= 0 && wx < W), "%d x %d: (%d, %d) inside = %d", L, W, wy, wx, (int)inside);
                        ++visits[((size_t)i * Wo + j) * taps + t];
                        ++pairs_checked;
                    }
        }
    for (size_t i = 0; i < visits.size(); ++i) CHECK(visits[i] == 1, "%d x %d taps %d: (cell, tap) %zu visited %d times", L, W, taps, i, visits[i]);
}

static void check_partials(int B, int O, int C, int n_slabs, int taps)
{
    const size_t n = (size_t)B * n_slabs * down_partial_floats(O, C, taps);
    std::vector<unsigned char> seen(n, 0);
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < n_slabs; ++s)
            for (int t = 0; t < taps; ++t)
                for (int o = 0; o < O; ++o)
                    for (int c = 0; c < C; ++c) {
                        const size_t at = down_partial_index(b, s, n_slabs, t, o, c, O, C, taps);
                        CHECK(at < n && !seen[at], "(%d, %d, %d, %d, %d) -> %zu of %zu", b, s, t, o, c, at, n);
                        seen[at] = 1;
                        if (taps == kTaps) CHECK(at == partial_index_of(b, s, n_slabs, t, o, c, O, C), "(%d, %d): not partial_index_of", b, s);
                        ++indices_checked;
                    }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "classes")) {
        check_source_taps();
        for (int L : kSizes)
            for (int W : kSizes) check_classes(L, W);
        std::printf("ok %lld positions %lld terms\n", positions_checked, terms_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "wgrad")) {
        static_assert(down_window_rows(9) == 5 && down_window_cols(9) == 65 && down_window_locations(1) == 64 && kDownHalves == 2, "the K tile");
        for (int L : kSizes)
            for (int W : kSizes)
                for (int taps : {9, 1}) {
                    const int Lo = out_size(L, 2), Wo = out_size(W, 2);
                    int last = -1;
                    for (int oc : {64, 512}) { // slabs(Lo, Wo), and the fewer slabs of a 512 x 512 layer
                        const int n = slabs_for(Lo, Wo, oc, oc);
                        if (n != last) check_wgrad(L, W, taps, n);
                        last = n;
                    }
                }
        check_partials(2, 64, 32, 3, 9);
        check_partials(2, 64, 32, 3, 1);
        std::printf("ok %lld pairs %lld indices\n", pairs_checked, indices_checked);
        return 0;
    }
    std::printf("usage: harness classes | wgrad\n");
    return 2;
}
