// CPU check of the integer part of vfa_amd/csrc/vfa_tile.h (the tap window of a tile of the frame kernels): for random tap bounds
// of the boxes of a tile, -1 <= coordinate <= size, `make_window` / `slot_row` are compared with a brute-force restatement -- mark
// every image row between the first and the last top tap row and between the first and the last bottom tap row; the marked rows are
// the window's rows, one run of them or two, and the window row of an image row is its rank among them.  `window_inv` is checked
// for every width and slot.  Built and run by tests/test_tile_window.py.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "../../vfa_amd/csrc/vfa_tile.h"

using namespace vfa_dev;

static unsigned seed = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s (seed %u)\n", __FILE__, __LINE__, #c, seed); return 1; } } while (0)

struct Box { bool vis; int xs[4], ys[4]; };

static int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

// taps of a box whose left / right edges fall into columns xl <= xr and whose top / bottom edges into rows yt <= yb (floor of the
// pixel coordinate, any integer): the device's box_taps
static Box make_box(bool vis, int xl, int xr, int yt, int yb, int Hf, int Wf)
{
    Box b;
    b.vis = vis;
    const int x[4] = {xl, xl + 1, xr, xr + 1}, y[4] = {yt, yt + 1, yb, yb + 1};
    for (int k = 0; k < 4; ++k) { b.xs[k] = clampi(x[k], -1, Wf); b.ys[k] = clampi(y[k], -1, Hf); }
    return b;
}

enum Kind { kNone, kOverlap, kTouch, kDisjoint };

// one tile; -> which case it was (through `kind`), 0 = all checks passed
static int check_tile(const std::vector<Box> &boxes, int Hf, int Wf, Kind &kind)
{
    // the half-wave reduction of tile_window, serially
    const int kBig = 1 << 20;
    int x0 = kBig, x1 = -kBig, t0 = kBig, t1 = -kBig, b0 = kBig, b1 = -kBig;
    bool any_vis = false;
    for (const Box &b : boxes) {
        if (!b.vis) continue;
        any_vis = true;
        x0 = std::min(x0, std::min(b.xs[0], b.xs[2])); x1 = std::max(x1, std::max(b.xs[1], b.xs[3]));
        t0 = std::min(t0, b.ys[0]); t1 = std::max(t1, b.ys[1]);
        b0 = std::min(b0, b.ys[2]); b1 = std::max(b1, b.ys[3]);
    }
    const Window w = make_window(any_vis, x0, x1, t0, t1, b0, b1);
    if (!any_vis) {
        kind = kNone;
        CHECK(w.cwid == 0 && w.top_rows == 0 && w.bot_rows == 0 && w.n_slots == 0);
        return 0;
    }
    // brute force: rows -1 .. Hf and columns -1 .. Wf as marks (index + 1)
    std::vector<char> row(Hf + 2, 0), col(Wf + 2, 0);
    int top_lo = kBig, top_hi = -kBig, bot_lo = kBig, bot_hi = -kBig, col_lo = kBig, col_hi = -kBig;
    for (const Box &b : boxes) {
        if (!b.vis) continue;
        for (int k = 0; k < 2; ++k) { top_lo = std::min(top_lo, b.ys[k]); top_hi = std::max(top_hi, b.ys[k]); }
        for (int k = 2; k < 4; ++k) { bot_lo = std::min(bot_lo, b.ys[k]); bot_hi = std::max(bot_hi, b.ys[k]); }
        for (int k = 0; k < 4; ++k) { col_lo = std::min(col_lo, b.xs[k]); col_hi = std::max(col_hi, b.xs[k]); }
    }
    for (int y = top_lo; y <= top_hi; ++y) row[y + 1] = 1;
    for (int y = bot_lo; y <= bot_hi; ++y) row[y + 1] = 1;
    for (int x = col_lo; x <= col_hi; ++x) col[x + 1] = 1;
    int n_rows = 0, n_cols = 0, runs = 0;
    std::vector<int> rank(Hf + 2, -1);
    for (int i = 0; i < Hf + 2; ++i)
        if (row[i]) { if (i == 0 || !row[i - 1]) ++runs; rank[i] = n_rows++; }
    for (int i = 0; i < Wf + 2; ++i) n_cols += col[i];
    CHECK(runs == 1 || runs == 2);
    kind = runs == 2 ? kDisjoint : (bot_lo == top_hi + 1 ? kTouch : kOverlap);
    CHECK(w.cwid == n_cols && w.x0 == col_lo);
    CHECK(w.top_rows + w.bot_rows == n_rows);
    CHECK((w.bot_rows == 0) == (runs == 1));
    CHECK(w.n_slots == n_cols * n_rows);
    CHECK(w.t0 == top_lo);
    if (runs == 2) CHECK(w.top_rows == top_hi - top_lo + 1 && w.bot_rows == bot_hi - bot_lo + 1 && w.b0 == bot_lo);
    // slot_row over the rows of the bands: the rank of the row among the marked rows -- injective, and dense in [0, rows)
    std::set<int> seen;
    for (int i = 0; i < Hf + 2; ++i) {
        if (!row[i]) continue;
        const int sr = slot_row(w, i - 1);
        CHECK(sr == rank[i]);
        CHECK(seen.insert(sr).second);
    }
    CHECK((int)seen.size() == n_rows);
    // every tap of every visible box lies in the window
    for (const Box &b : boxes) {
        if (!b.vis) continue;
        for (int k = 0; k < 4; ++k) {
            CHECK(row[b.ys[k] + 1] && col[b.xs[k] + 1]);
            const int slot = slot_row(w, b.ys[k]) * w.cwid + (b.xs[k] - w.x0);
            CHECK(slot >= 0 && slot < w.n_slots);
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int n_cases = argc > 2 ? std::atoi(argv[2]) : 2000;
    std::mt19937 rng(seed);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };

    // floor(s / cwid) == (s * inv) >> 16 for every slot s < 128 and every width cwid <= 128
    for (int cwid = 1; cwid <= 128; ++cwid)
        for (int s = 0; s < 128; ++s) CHECK(s / cwid == (s * window_inv(cwid)) >> 16);
    CHECK(window_inv(0) == 0);

    long long count[4] = {0, 0, 0, 0};
    Kind kind;
    // the four cases by construction (an 8 x 8 map): bands that overlap, touch, are disjoint; no visible box
    {
        std::vector<Box> t;
        auto expect = [&](Kind want) { // 0 = passed
            if (check_tile(t, 8, 8, kind)) return 1;
            CHECK(kind == want);
            ++count[kind];
            return 0;
        };
        t = {make_box(true, 2, 3, 3, 3, 8, 8)};                                   // rows {3, 4} and {3, 4}
        if (expect(kOverlap)) return 1;
        t = {make_box(true, 2, 3, 1, 3, 8, 8)};                                   // rows {1, 2} and {3, 4}: b0 == t1 + 1
        if (expect(kTouch)) return 1;
        t = {make_box(true, 2, 5, 0, 5, 8, 8), make_box(true, 1, 6, 1, 6, 8, 8)};  // rows [0, 2] and [5, 7]
        if (expect(kDisjoint)) return 1;
        t = {make_box(false, 2, 5, 0, 5, 8, 8), make_box(false, 1, 6, 1, 6, 8, 8)};
        if (expect(kNone)) return 1;
        t = {make_box(true, -4, 12, -4, 12, 8, 8)};                               // everything clamped to the border: rows {-1} and {8}
        if (expect(kDisjoint)) return 1;
    }
    for (int c = 0; c < n_cases; ++c) {
        const int Hf = uni(1, 40), Wf = uni(1, 40);
        const int n_boxes = uni(1, 32);
        const int mode = uni(0, 9);                    // 0: nothing visible; else neighbouring boxes of a common size
        const int cx = uni(-3, Wf + 2), cy = uni(-3, Hf + 2), spread = uni(0, 4), high = uni(0, mode < 5 ? 3 : Hf), wide = uni(0, Wf);
        std::vector<Box> t;
        for (int i = 0; i < n_boxes; ++i) {
            const int xl = cx + uni(-spread, spread), yt = cy + uni(-spread, spread);
            const bool vis = mode != 0 && uni(0, 3) != 0;
            t.push_back(make_box(vis, xl, xl + std::max(0, wide + uni(-1, 1)), yt, yt + std::max(0, high + uni(-1, 1)), Hf, Wf));
        }
        if (check_tile(t, Hf, Wf, kind)) return 1;
        ++count[kind];
    }
    CHECK(count[kNone] > 1 && count[kOverlap] > 1 && count[kTouch] > 1 && count[kDisjoint] > 1);
    std::printf("ok: %lld tiles without a visible box, %lld with overlapping, %lld with touching, %lld with disjoint bands\n", count[kNone],
                count[kOverlap], count[kTouch], count[kDisjoint]);
    return 0;
}
