// The integer rules of the dense 3x3 convolution's weight gradient (vfa_amd/csrc/vfa_conv_grad.h, shared host / device code) on the
// CPU, against a brute-force enumeration.
//
//   harness slabs      every map from 1 x 1 to 70 x 70: the slabs are min(tiles, kMaxSlabs) non-empty runs of consecutive tiles, in
//                      order, and every cell of the map lies in a tile of exactly one slab.
//   harness partials   the partial index is a bijection of (frame, slab, tap, o, c) onto [0, B slabs partial_floats), an (o, c) plane
//                      of a tap is contiguous with c fastest.
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

static long long cells_checked, slabs_checked, indices_checked;

static void check_slabs(int L, int W)
{
    const int n_tiles = tiles_x(W) * tiles_y(L), n_slabs = slabs(L, W);
    CHECK(tiles(L, W) == n_tiles && n_slabs == (n_tiles < kMaxSlabs ? n_tiles : kMaxSlabs) && n_slabs >= 1, "%d x %d: %d slabs", L, W, n_slabs);
    CHECK(slab_begin(0, L, W) == 0 && slab_begin(n_slabs, L, W) == n_tiles, "%d x %d: the slabs do not span the tiles", L, W);
    std::vector<int> owner((size_t)L * W, -1);
    for (int s = 0; s < n_slabs; ++s) {
        const int begin = slab_begin(s, L, W), end = slab_begin(s + 1, L, W);
        CHECK(begin < end && end <= n_tiles, "%d x %d: slab %d is [%d, %d)", L, W, s, begin, end);
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
        ++slabs_checked;
    }
    for (size_t i = 0; i < owner.size(); ++i) CHECK(owner[i] >= 0, "cell %zu of %d x %d has no slab", i, L, W);
}

static void check_partials(int B, int O, int C, int L, int W)
{
    const int n_slabs = slabs(L, W);
    const size_t n = (size_t)B * n_slabs * partial_floats(O, C);
    CHECK(partial_floats(O, C) == (size_t)9 * O * C, "partial_floats(%d, %d)", O, C);
    std::vector<unsigned char> seen(n, 0);
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < n_slabs; ++s)
            for (int t = 0; t < kTaps; ++t)
                for (int o = 0; o < O; ++o)
                    for (int c = 0; c < C; ++c) {
                        const size_t at = partial_index(b, s, t, o, c, O, C, L, W);
                        CHECK(at < n && !seen[at], "(%d, %d, %d, %d, %d) -> %zu of %zu", b, s, t, o, c, at, n);
                        seen[at] = 1;
                        CHECK(at / partial_floats(O, C) == (size_t)b * n_slabs + s, "(%d, %d): partial %zu", b, s, at / partial_floats(O, C));
                        if (c + 1 < C) CHECK(partial_index(b, s, t, o, c + 1, O, C, L, W) == at + 1, "c is not the fastest index");
                        ++indices_checked;
                    }
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "slabs")) {
        for (int L = 1; L <= 70; ++L)
            for (int W = 1; W <= 70; ++W) check_slabs(L, W);
        check_slabs(156, 156);
        check_slabs(200, 200);
        std::printf("ok %lld cells %lld slabs\n", cells_checked, slabs_checked);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "partials")) {
        check_partials(1, 32, 32, 3, 5);
        check_partials(2, 96, 64, 9, 37);
        check_partials(3, 32, 64, 70, 70);
        std::printf("ok %lld indices\n", indices_checked);
        return 0;
    }
    std::printf("usage: harness slabs | partials\n");
    return 2;
}
