// The integer rules of the stem's backward kernels (vfa_amd/csrc/vfa_stem.h, shared host / device code) on the CPU, against a
// brute-force enumeration that shares nothing with them.  Maps from 1 x 1 to 20 x 150 and 37 x 131.
//
//   harness windows   per axis of 1 .. 300 positions: pool_window_first .. pool_window_last of a position are exactly the outputs whose
//                     3-wide stride-2 window (the axis padded by 1) holds it, at least one and at most two.  Per map: every
//                     position of a pool-backward tile reads windows and taps inside the tile's staged ranges.
//   harness scan      per map and window: walking rows ascending and columns ascending over the taps inside the map visits ranks
//                     0, 1, 2 .. of pool_scan_rank without a gap, pool_taps(oy) pool_taps(ox) in all; pool_tap_code is
//                     3 (row in the window) + (column in the window), 0 .. 8, distinct per tap, and never kNoWinner.
//   harness slabs     per (Lo, Wo): every tile lies in exactly one slab, the slabs ascend and none is empty, their count is
//                     min(tiles, kMaxSlabs) -- a function of (Lo, Wo) alone, whatever the batch --, every cell lies in exactly one
//                     slab, and the partial index is a bijection of (image, slab, o, k) onto [0, B slabs O kK).
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

static long long positions_checked, taps_checked, cells_checked, slabs_checked;

static void check_axis(int n)
{
    const int n_out = pool_out(n);
    for (int p = 0; p < n; ++p) {
        int first = -1, last = -1, count = 0;
        for (int o = 0; o < n_out; ++o)
            if (p >= 2 * o - 1 && p <= 2 * o + 1) { // the window of output o on the axis padded by one
                if (first < 0) first = o;
                last = o;
                ++count;
            }
        CHECK(count >= 1 && count <= 2, "axis %d position %d lies in %d windows", n, p, count);
        CHECK(pool_window_first(p) == first && pool_window_last(p, n_out) == last, "axis %d position %d: windows %d .. %d, want %d .. %d", n, p,
              pool_window_first(p), pool_window_last(p, n_out), first, last);
        ++positions_checked;
    }
}

// what a workgroup of the pooling's backward stages covers what its positions read
static void check_tiles(int L, int W)
{
    const int Lo = pool_out(L), Wo = pool_out(W);
    std::vector<int> owner((size_t)L * W, 0);
    for (int tile = 0; tile < pool_tiles_x(W) * pool_tiles_y(L); ++tile) {
        const int p0 = tile / pool_tiles_x(W) * kPoolTileRows, q0 = tile % pool_tiles_x(W) * kPoolTileCols;
        CHECK(p0 % 2 == 0 && q0 % 2 == 0, "tile %d: origin (%d, %d)", tile, p0, q0);
        for (int p = p0; p < p0 + kPoolTileRows && p < L; ++p)
            for (int q = q0; q < q0 + kPoolTileCols && q < W; ++q) {
                ++owner[(size_t)p * W + q];
                for (int i = pool_window_first(p); i <= pool_window_last(p, Lo); ++i)
                    for (int j = pool_window_first(q); j <= pool_window_last(q, Wo); ++j) {
                        CHECK(i - p0 / 2 >= 0 && i - p0 / 2 < kPoolWinRows && j - q0 / 2 >= 0 && j - q0 / 2 < kPoolWinCols, "(%d, %d): window (%d, %d)", p, q, i, j);
                        for (int ty = pool_first(i); ty <= pool_last(i, L); ++ty)
                            for (int tx = pool_first(j); tx <= pool_last(j, W); ++tx)
                                CHECK(ty - p0 + 1 >= 0 && ty - p0 + 1 < kPoolTapRows && tx - q0 + 1 >= 0 && tx - q0 + 1 < kPoolTapCols && ty < L && tx < W,
                                      "(%d, %d): tap (%d, %d)", p, q, ty, tx);
                    }
            }
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] == 1, "position %zu of %d x %d has %d tiles", i, L, W, owner[i]);
}

static void check_scan(int L, int W)
{
    const int Lo = pool_out(L), Wo = pool_out(W);
    for (int oy = 0; oy < Lo; ++oy)
        for (int ox = 0; ox < Wo; ++ox) {
            int rank = 0;
            unsigned seen = 0;
            for (int wy = 0; wy < 3; ++wy) // the window on the map padded by one, rows then columns ascending
                for (int wx = 0; wx < 3; ++wx) {
                    const int ty = 2 * oy - 1 + wy, tx = 2 * ox - 1 + wx;
                    if (ty < 0 || ty >= L || tx < 0 || tx >= W) continue;
                    CHECK(ty >= pool_first(oy) && ty <= pool_last(oy, L) && tx >= pool_first(ox) && tx <= pool_last(ox, W), "window (%d, %d): tap (%d, %d)", oy, ox,
                          ty, tx);
                    CHECK(pool_scan_rank(oy, ox, ty, tx, W) == rank, "window (%d, %d) of %d x %d: tap (%d, %d) has rank %d, want %d", oy, ox, L, W, ty, tx,
                          pool_scan_rank(oy, ox, ty, tx, W), rank);
                    const int code = pool_tap_code(oy, ox, ty, tx);
                    CHECK(code == 3 * wy + wx && code != kNoWinner && !(seen >> code & 1), "window (%d, %d): tap (%d, %d) has code %d", oy, ox, ty, tx, code);
                    seen |= 1u << code;
                    ++rank;
                    ++taps_checked;
                }
            CHECK(rank >= 1 && rank == pool_taps(oy, L) * pool_taps(ox, W), "window (%d, %d) of %d x %d: %d taps", oy, ox, L, W, rank);
        }
}

static void check_slabs(int Lo, int Wo)
{
    const int n_tiles = tiles_x(Wo) * tiles_y(Lo), n_slabs = wgrad_slabs(Lo, Wo);
    CHECK(wgrad_tiles(Lo, Wo) == n_tiles && n_slabs == (n_tiles < kMaxSlabs ? n_tiles : kMaxSlabs) && n_slabs >= 1, "%d x %d: %d slabs of %d tiles", Lo, Wo,
          n_slabs, n_tiles);
    CHECK(wgrad_slab_begin(0, Lo, Wo) == 0 && wgrad_slab_begin(n_slabs, Lo, Wo) == n_tiles, "%d x %d: the slabs do not span the tiles", Lo, Wo);
    std::vector<int> cell_slab((size_t)Lo * Wo, -1);
    for (int s = 0; s < n_slabs; ++s) {
        const int begin = wgrad_slab_begin(s, Lo, Wo), end = wgrad_slab_begin(s + 1, Lo, Wo);
        CHECK(begin < end, "%d x %d: slab %d is empty", Lo, Wo, s); // ascending, and with the two ends above every tile in exactly one
        for (int tile = begin; tile < end; ++tile) {
            int y0, x0;
            tile_origin(tile, Wo, y0, x0);
            for (int ry = 0; ry < kTileRows; ++ry)
                for (int rx = 0; rx < kTileCols; ++rx) {
                    if (y0 + ry >= Lo || x0 + rx >= Wo) continue;
                    CHECK(cell_slab[(size_t)(y0 + ry) * Wo + x0 + rx] == -1, "cell (%d, %d) has two slabs", y0 + ry, x0 + rx);
                    cell_slab[(size_t)(y0 + ry) * Wo + x0 + rx] = s;
                    ++cells_checked;
                }
        }
        ++slabs_checked;
    }
    for (size_t i = 0; i < cell_slab.size(); ++i) CHECK(cell_slab[i] >= 0, "cell %zu of %d x %d has no slab", i, Lo, Wo);
}

static void check_partials()
{
    CHECK(kK == 147 && kNBlocks == 5 && kNBlocks * 32 >= kK && kMaxSlabs == 64, "constants");
    const int B = 3, n_slabs = 5, O = 7;
    std::vector<unsigned char> seen((size_t)B * n_slabs * O * kK, 0);
    CHECK(wgrad_partial_floats(O) == (size_t)O * kK, "partial floats");
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < n_slabs; ++s)
            for (int o = 0; o < O; ++o)
                for (int k = 0; k < kK; ++k) {
                    const size_t at = wgrad_partial_index(b, s, n_slabs, o, k, O);
                    CHECK(at < seen.size() && !seen[at], "(%d, %d, %d, %d): index %zu", b, s, o, k, at);
                    seen[at] = 1;
                    CHECK(at % wgrad_partial_floats(O) == (size_t)o * kK + k, "(%d, %d): not dw's own layout", o, k); // the merge adds partials elementwise
                    CHECK(at / wgrad_partial_floats(O) == (size_t)b * n_slabs + s, "(%d, %d): partials are not ascending (image, slab)", b, s);
                }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "windows")) {
        for (int n = 1; n <= 300; ++n) check_axis(n);
        for (int L = 1; L <= 20; ++L)
            for (int W = 1; W <= 150; ++W) check_tiles(L, W);
        check_tiles(37, 131);
        std::printf("ok %lld positions\n", positions_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "scan")) {
        for (int L = 1; L <= 20; ++L)
            for (int W = 1; W <= 150; ++W) check_scan(L, W);
        check_scan(37, 131);
        std::printf("ok %lld taps\n", taps_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "slabs")) {
        check_partials();
        for (int Lo = 1; Lo <= 20; ++Lo)
            for (int Wo = 1; Wo <= 150; ++Wo) check_slabs(Lo, Wo);
        check_slabs(37, 131);
        check_slabs(360, 640); // 1800 tiles: kMaxSlabs slabs of 28 or 29 tiles
        CHECK(wgrad_slabs(360, 640) == kMaxSlabs && wgrad_slabs(10, 71) == 9 && wgrad_slabs(36, 256) == 64 && wgrad_tiles(36, 256) == 72, "slab counts");
        std::printf("ok %lld slabs %lld cells\n", slabs_checked, cells_checked);
        return 0;
    }
    std::printf("usage: harness windows | scan | slabs\n");
    return 2;
}
