// The slab rule of the trunk's weight gradient (slabs_for and the _of forms of vfa_amd/csrc/vfa_conv_grad.h, shared host / device
// code) on the CPU, against a brute-force enumeration.
//
//   harness slabs      every map from 1 x 1 to 48 x 48 and the trunk's maps, at every pair of widths 64 .. 512: slabs_for is slabs(L, W)
//                      wherever O C <= 256^2, at least 1 and at most slabs(L, W) past it, with never more partial floats per frame than
//                      a 256 x 256 layer has on the map (unless one slab is all that is left); its slabs are non-empty runs of
//                      consecutive tiles, in order, and every cell of the map lies in a tile of exactly one slab; with slabs(L, W)
//                      slabs the _of forms are slab_begin.
//   harness partials   partial_index_of is a bijection of (frame, slab, tap, o, c) onto [0, B slabs_for partial_floats) and, with
//                      slabs(L, W) slabs, partial_index.
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

static long long cells_checked, rules_checked, fewer, indices_checked;
static const int kWidths[] = {32, 64, 128, 256, 512};

static void check_cover(int L, int W, int n_slabs)
{
    const int n_tiles = tiles(L, W);
    CHECK(n_slabs >= 1 && n_slabs <= n_tiles, "%d x %d: %d slabs of %d tiles", L, W, n_slabs, n_tiles);
    CHECK(slab_begin_of(0, n_slabs, L, W) == 0 && slab_begin_of(n_slabs, n_slabs, L, W) == n_tiles, "%d x %d: the slabs do not span the tiles", L, W);
    std::vector<int> owner((size_t)L * W, -1);
    for (int s = 0; s < n_slabs; ++s) {
        const int begin = slab_begin_of(s, n_slabs, L, W), end = slab_begin_of(s + 1, n_slabs, L, W);
        CHECK(begin < end && end <= n_tiles, "%d x %d: slab %d of %d is [%d, %d)", L, W, s, n_slabs, begin, end);
        for (int tile = begin; tile < end; ++tile) {
            int y0, x0;
            tile_origin(tile, W, y0, x0);
            for (int ry = 0; ry < kTileRows; ++ry)
                for (int rx = 0; rx < kTileCols; ++rx) {
                    const int y = y0 + ry, x = x0 + rx;
                    if (y >= L || x >= W) continue;
                    CHECK(owner[(size_t)y * W + x] == -1, "%d x %d: cell (%d, %d) in slabs %d and %d", L, W, y, x, owner[(size_t)y * W + x], s);
                    owner[(size_t)y * W + x] = s;
                    ++cells_checked;
                }
        }
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] >= 0, "cell %zu of %d x %d has no slab", i, L, W);
}

static void check_map(int L, int W)
{
    const int full = slabs(L, W);
    for (int s = 0; s <= full; ++s) CHECK(slab_begin_of(s, full, L, W) == slab_begin(s, L, W), "%d x %d: slab %d", L, W, s);
    int last = -1;
    for (int O : kWidths)
        for (int C : kWidths) {
            const int n = slabs_for(L, W, O, C);
            const long long oc = (long long)O * C;
            if (oc <= 256LL * 256) CHECK(n == full, "%d x %d, %d x %d: %d slabs, not %d", L, W, O, C, n, full);
            else {
                CHECK(n >= 1 && n <= full, "%d x %d, %d x %d: %d slabs", L, W, O, C, n);
                CHECK(n == 1 || (long long)n * oc <= (long long)full * 256 * 256, "%d x %d, %d x %d: %d slabs are too many floats", L, W, O, C, n);
                CHECK((long long)(n + 1) * oc > (long long)full * 256 * 256, "%d x %d, %d x %d: %d slabs are fewer than the rule allows", L, W, O, C, n);
                fewer += n < full;
            }
            CHECK(n == slabs_for(L, W, C, O), "%d x %d: the rule is not symmetric in (%d, %d)", L, W, O, C);
            if (n != last) check_cover(L, W, n); // (every distinct count of this map)
            last = n;
            ++rules_checked;
        }
}

static void check_partials(int B, int O, int C, int L, int W)
{
    const int n_slabs = slabs_for(L, W, O, C);
    const size_t n = (size_t)B * n_slabs * partial_floats(O, C);
    std::vector<unsigned char> seen(n, 0);
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < n_slabs; ++s)
            for (int t = 0; t < kTaps; ++t)
                for (int o = 0; o < O; ++o)
                    for (int c = 0; c < C; ++c) {
                        const size_t at = partial_index_of(b, s, n_slabs, t, o, c, O, C);
                        CHECK(at < n && !seen[at], "(%d, %d, %d, %d, %d) -> %zu of %zu", b, s, t, o, c, at, n);
                        seen[at] = 1;
                        if (n_slabs == slabs(L, W)) CHECK(at == partial_index(b, s, t, o, c, O, C, L, W), "(%d, %d): not partial_index", b, s);
                        ++indices_checked;
                    }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "slabs")) {
        for (int L = 1; L <= 48; ++L)
            for (int W = 1; W <= 48; ++W) check_map(L, W);
        const int trunk[][2] = {{180, 320}, {90, 160}, {45, 80}, {23, 40}, {5, 9}, {3, 5}};
        for (const auto &m : trunk) check_map(m[0], m[1]);
        CHECK(slabs_for(23, 40, 512, 512) == 3 && slabs(23, 40) == 12 && slabs_for(45, 80, 256, 256) == 16 && slabs_for(3, 5, 512, 512) == 1,
              "the trunk's layers: %d, %d", slabs_for(23, 40, 512, 512), slabs_for(3, 5, 512, 512));
        std::printf("ok %lld cells %lld rules %lld fewer\n", cells_checked, rules_checked, fewer);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "partials")) {
        check_partials(2, 64, 64, 9, 37);
        check_partials(2, 512, 512, 23, 40);
        check_partials(1, 512, 256, 20, 70);
        std::printf("ok %lld indices\n", indices_checked);
        return 0;
    }
    std::printf("usage: harness slabs | partials\n");
    return 2;
}
