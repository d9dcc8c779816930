// The integer logic of the convolution at listed cells (vfa_amd/csrc/vfa_cellconv.h, shared host / device code) on the CPU, against
// a brute-force enumeration that shares nothing with it: a dense map per frame on which every (row, tap) pair is painted in
// ascending order.
//
//   harness taps           every cell and tap of small grids (also grids lower than 2 d + 1, d up to 5): tap_location against the
//                          definition written out with divisions, tap_landing_on as its inverse over every location of the map.
//   harness owners SEED    the named cell lists (cells d apart in a row, a column, a diagonal; duplicates; ids outside the map) and
//                          300 random lists: a location is owned by exactly the first pair painted on it, the owner's walk over the
//                          later rows (what cellconv_grad_feat_kernel does) lists the location's pairs in painting order, and
//                          skipped rows own nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../vfa_amd/csrc/vfa_cellconv.h"

using namespace vfa_cellconv;

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

static long long taps_checked, taps_outside, shared_locations, pairs_checked;

static void check_taps(int L, int W, int d)
{
    for (int l = 0; l < L; ++l)
        for (int w = 0; w < W; ++w) {
            const int cell = l * W + w;
            CHECK(cell_valid(cell, L, W), "cell %d of %d x %d", cell, L, W);
            std::vector<int> hit((size_t)L * W, -1);
            for (int ty = 0; ty < 3; ++ty)
                for (int tx = 0; tx < 3; ++tx) {
                    const int t = 3 * ty + tx, wy = l + (ty - 1) * d, wx = w + (tx - 1) * d;
                    const bool inside = wy >= 0 && wy < L && wx >= 0 && wx < W;
                    int y = -7, x = -7;
                    const bool got = tap_location(cell, t, L, W, d, y, x);
                    CHECK(got == inside, "cell %d tap %d of %d x %d d %d", cell, t, L, W, d);
                    if (inside) {
                        CHECK(y == wy && x == wx, "cell %d tap %d: (%d, %d), want (%d, %d)", cell, t, y, x, wy, wx);
                        hit[(size_t)wy * W + wx] = t;
                    } else {
                        CHECK(y == -7 && x == -7, "an outside tap wrote its location");
                        ++taps_outside;
                    }
                    ++taps_checked;
                }
            for (int y = 0; y < L; ++y)
                for (int x = 0; x < W; ++x)
                    CHECK(tap_landing_on(cell, y, x, W, d) == hit[(size_t)y * W + x], "cell %d location (%d, %d) of %d x %d d %d", cell, y, x,
                          L, W, d);
        }
    CHECK(!cell_valid(-1, L, W) && !cell_valid(-7, L, W) && !cell_valid((long long)L * W, L, W) && !cell_valid(INT32_MIN, L, W) &&
              !cell_valid(INT32_MAX, L, W) && cell_valid((long long)L * W - 1, L, W),
          "cell_valid of %d x %d", L, W);
}

// one frame: paint the pairs in ascending (row, tap) order, then ask the header
static void check_owners(const std::vector<int> &cells, int L, int W, int d)
{
    const int k = (int)cells.size();
    std::vector<std::vector<std::pair<int, int>>> painted((size_t)L * W);
    for (int row = 0; row < k; ++row) {
        if (cells[row] < 0 || cells[row] >= L * W) continue;
        const int l = cells[row] / W, w = cells[row] % W;
        for (int t = 0; t < kTaps; ++t) {
            const int y = l + (t / 3 - 1) * d, x = w + (t % 3 - 1) * d;
            if (y >= 0 && y < L && x >= 0 && x < W) painted[(size_t)y * W + x].push_back({row, t});
        }
    }
    std::vector<int> owners((size_t)L * W, 0);
    for (int row = 0; row < k; ++row)
        for (int t = 0; t < kTaps; ++t) {
            const bool owns = pair_owns(cells.data(), row, t, L, W, d);
            int y, x;
            const bool lies = cell_valid(cells[row], L, W) && tap_location(cells[row], t, L, W, d, y, x);
            if (!lies) {
                CHECK(!owns, "row %d tap %d lies nowhere and owns", row, t);
                continue;
            }
            const auto &want = painted[(size_t)y * W + x];
            CHECK(!want.empty(), "row %d tap %d was not painted", row, t);
            CHECK(owns == (want[0] == std::make_pair(row, t)), "row %d tap %d at (%d, %d): owns %d, first pair (%d, %d)", row, t, y, x,
                  (int)owns, want[0].first, want[0].second);
            ++pairs_checked;
            if (!owns) continue;
            owners[(size_t)y * W + x] += 1;
            // the owner's walk: itself, then the later rows in ascending order, each with the one tap it has on the location
            std::vector<std::pair<int, int>> walk = {{row, t}};
            for (int j = row + 1; j < k; ++j) {
                if (!cell_valid(cells[j], L, W)) continue;
                const int t2 = tap_landing_on(cells[j], y, x, W, d);
                if (t2 >= 0) walk.push_back({j, t2});
            }
            CHECK(walk == want, "location (%d, %d): the walk of %zu pairs is not the painting of %zu", y, x, walk.size(), want.size());
            if (want.size() > 1) ++shared_locations;
        }
    for (size_t i = 0; i < owners.size(); ++i)
        CHECK(owners[i] == (painted[i].empty() ? 0 : 1), "location %zu has %d owners and %zu pairs", i, owners[i], painted[i].size());
}

int main(int argc, char **argv)
{
    const char *mode = argc > 1 ? argv[1] : "";
    if (mode[0] == 't') {
        const int sizes[][2] = {{1, 1}, {1, 9}, {3, 1}, {2, 3}, {7, 9}, {5, 5}, {12, 13}, {10, 10}};
        for (const auto &s : sizes)
            for (int d = 1; d <= 5; ++d) check_taps(s[0], s[1], d);
        CHECK(taps_outside > 1000, "too few outside taps: %lld", taps_outside);
        std::printf("ok taps: %lld taps, %lld outside\n", taps_checked, taps_outside);
        return 0;
    }
    if (mode[0] == 'o') {
        rng_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
        const int L = 12, W = 13, d = 4;
        const int c = 5 * W + 6;
        check_owners({c, c + d, c + d * W, c + d * W + d, c, -1, L * W, -7, c - d * W - d, 0, L * W - 1}, L, W, d);
        check_owners({-1, -1, -1}, L, W, d);
        check_owners({}, L, W, d);
        check_owners({3, 3, 3, 3}, 1, 9, 1);
        check_owners({0, 62, 31, -1, 8, 54}, 7, 9, 4);
        CHECK(shared_locations > 10, "the named lists share too few locations: %lld", shared_locations);
        for (int n = 0; n < 300; ++n) {
            const int l = 1 + rnd() % 12, w = 1 + rnd() % 13, dd = 1 + rnd() % 4, k = rnd() % 41;
            std::vector<int> cells(k);
            for (int &cell : cells) {
                const uint32_t r = rnd() % 10;
                cell = r == 0 ? -1 - (int)(rnd() % 9) : r == 1 ? l * w + (int)(rnd() % 9) : (int)(rnd() % (uint32_t)(l * w));
            }
            check_owners(cells, l, w, dd);
        }
        std::printf("ok owners: %lld pairs, %lld shared locations\n", pairs_checked, shared_locations);
        return 0;
    }
    std::printf("usage: harness taps | owners SEED\n");
    return 2;
}
