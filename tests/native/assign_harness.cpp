// The CLEAR-MOD assignment solver (vfa_amd/csrc/vfa_assign.h, shared host / device code) on the CPU; the 64 lanes run as a loop.
//
//   harness brute SEED COUNT   every shape up to 7 x 7, COUNT matrices in all: thresholded distances, integer distances (ties),
//                              entries at exactly td, matrices made only of 1e6, and matrices that hold NaN / +inf.  Finite ones:
//                              no flag, every row assigned, a one-to-one table, and the optimal cost of a brute force over all
//                              injections.  NaN / +inf ones: the solver returns, and what it assigned is one-to-one and in range.
//   harness frames FILE        frames written by tests/test_clear_mod_cpu.py from tests/golden/clear_mod.npz (all doubles:
//                              n_frames, then per frame G, P, c, unique, cost_sum, td, G x 2 ground truths, P x 2 detections,
//                              G matches): solve_frame against scipy's per-frame record, and against itself with the sides swapped.
//   harness wide SEED          frames of the cap's size (both cost paths, both orientations): no flag, one-to-one, sides swapped.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_assign.h"

using namespace vfa_assign;

static State S; // (static: 50 KB)
static const double kTd = 30.0;

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static double uniform() { return rnd() / 2147483648.0; }

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

struct Matrix {
    const double *a;
    int cols;
    double operator()(int i, int j) const { return a[i * cols + j]; }
};

// what the tables must be whatever the costs were: in range, each the inverse of the other
static int check_tables(int rows, int cols)
{
    int assigned = 0;
    for (int i = 0; i < rows; ++i) {
        const int j = S.col4row[i];
        CHECK(j >= -1 && j < cols, "row %d -> column %d", i, j);
        if (j >= 0) { CHECK(S.row4col[j] == i, "row %d -> column %d -> row %d", i, j, (int)S.row4col[j]); ++assigned; }
    }
    int held = 0;
    for (int j = 0; j < cols; ++j) {
        const int i = S.row4col[j];
        CHECK(i >= -1 && i < rows, "column %d -> row %d", j, i);
        if (i >= 0) { CHECK(S.col4row[i] == j, "column %d -> row %d -> column %d", j, i, (int)S.col4row[i]); ++held; }
    }
    CHECK(held == assigned, "%d rows assigned, %d columns held", assigned, held);
    return assigned;
}

static double brute_best;
static void brute(const double *a, int rows, int cols, int i, unsigned used, double sum)
{
    if (i == rows) { if (sum < brute_best) brute_best = sum; return; }
    for (int j = 0; j < cols; ++j)
        if (!(used >> j & 1)) brute(a, rows, cols, i + 1, used | 1u << j, sum + a[i * cols + j]);
}

static int run_brute(uint64_t seed, int count)
{
    rng_state = seed * 0x9e3779b97f4a7c15ull + 1;
    double a[49];
    int finite_cases = 0, odd_cases = 0;
    for (int n = 0; n < count; ++n) {
        const int shape = n % 49, r = shape / 7 + 1, c = shape % 7 + 1;
        const int rows = r < c ? r : c, cols = r < c ? c : r;
        const int kind = (n / 49) % 8; // 0-2 distances, 3 integers, 4 entries at td, 5 only 1e6, 6 NaN, 7 +inf
        const double reach = kind == 1 ? 33.0 : kind == 2 ? 300.0 : 60.0; // share of pairs within td: most, a tenth, half
        bool finite = true;
        for (int q = 0; q < rows * cols; ++q) {
            double d = uniform() * reach;
            if (kind == 3) d = std::floor(uniform() * 36.0);
            if (kind == 4 && rnd() % 3 == 0) d = kTd;
            if (kind == 5) d = 1000.0;
            a[q] = pair_cost(d, kTd);
            if (kind == 6 && rnd() % 4 == 0) { a[q] = NAN; finite = false; }
            if (kind == 7 && rnd() % 4 == 0) { a[q] = INFINITY; finite = false; }
        }
        const Matrix m = {a, cols};
        const int flags = solve(S, rows, cols, m);
        const int assigned = check_tables(rows, cols);
        CHECK((flags & ~(kFlagNoColumn | kFlagBound | kFlagWalk)) == 0, "flags %d", flags);
        if (!finite) { // (a bound that is met is a flag, never a hang; nothing more is promised)
            CHECK((flags & (kFlagBound | kFlagWalk)) == 0, "case %d (%d x %d, kind %d): flags %d", n, rows, cols, kind, flags);
            ++odd_cases;
            continue;
        }
        CHECK(flags == 0, "case %d (%d x %d, kind %d): flags %d", n, rows, cols, kind, flags);
        CHECK(assigned == rows, "case %d: %d of %d rows assigned", n, assigned, rows);
        double got = 0.0;
        for (int i = 0; i < rows; ++i) got += a[i * cols + S.col4row[i]];
        brute_best = INFINITY;
        brute(a, rows, cols, 0, 0u, 0.0);
        // at most 7 costs of at most 1e6: one ulp of the largest sum is 9.3e-10; the duals are sums of a few dozen such terms, so an
        // assignment that is optimal for the rounded duals is within 1e-7 (100 ulp) of the optimum, and the two sums are added
        // in different orders
        CHECK(std::fabs(got - brute_best) <= 1e-7, "case %d (%d x %d, kind %d): cost %.17g, optimum %.17g", n, rows, cols, kind, got, brute_best);
        ++finite_cases;
    }
    std::printf("ok brute: %d finite matrices optimal, %d with NaN / inf returned\n", finite_cases, odd_cases);
    return 0;
}

struct FrameResult { FrameTotals t; std::vector<int> match; std::vector<double> dist; };

static FrameResult run_frame(const std::vector<double> &gt, const std::vector<double> &det, double td)
{
    const int G = (int)gt.size() / 2, P = (int)det.size() / 2;
    for (int o = 0; o < G; ++o) { S.gx[o] = gt[2 * o]; S.gy[o] = gt[2 * o + 1]; }
    for (int e = 0; e < P; ++e) { S.ex[e] = det[2 * e]; S.ey[e] = det[2 * e + 1]; }
    FrameResult r;
    r.match.assign(G + 1, -7);
    r.dist.assign(G + 1, -7.0);
    r.t = solve_frame(S, G, P, td, r.match.data(), r.dist.data());
    CHECK(r.match[G] == -7 && r.dist[G] == -7.0, "solve_frame wrote behind its rows");
    CHECK(r.t.flags == 0, "flags %d (G %d, P %d)", r.t.flags, G, P);
    check_tables(G <= P ? G : P, G <= P ? P : G);
    std::vector<int> taken(P, 0);
    long long c = 0;
    for (int o = 0; o < G; ++o) {
        const int e = r.match[o];
        CHECK(e >= -1 && e < P, "ground truth %d -> detection %d", o, e);
        if (e < 0) { CHECK(std::isinf(r.dist[o]) && r.dist[o] > 0, "unmatched distance %g", r.dist[o]); continue; }
        CHECK(++taken[e] == 1, "detection %d matched twice", e);
        const double d = pair_distance(gt[2 * o], gt[2 * o + 1], det[2 * e], det[2 * e + 1]);
        CHECK(d < td && std::memcmp(&d, &r.dist[o], 8) == 0, "pair (%d, %d): distance %.17g, table %.17g", o, e, d, r.dist[o]);
        ++c;
    }
    CHECK(c == r.t.matched, "%lld matches in the table, %lld counted", c, r.t.matched);
    CHECK(c + r.t.beyond <= (G < P ? G : P), "more pairs than the smaller side");
    return r;
}

// the frame with ground truths and detections swapped is the same problem
static void check_swapped(const std::vector<double> &gt, const std::vector<double> &det, double td, const FrameResult &r)
{
    const FrameResult s = run_frame(det, gt, td);
    CHECK(s.t.matched == r.t.matched && s.t.beyond == r.t.beyond, "swapped sides: c %lld / %lld, at 1e6 %lld / %lld", s.t.matched,
          r.t.matched, s.t.beyond, r.t.beyond);
    CHECK(std::fabs(s.t.cost - r.t.cost) <= 1e-9 * std::fabs(r.t.cost), "swapped sides: cost %.17g / %.17g", s.t.cost, r.t.cost);
}

static int run_frames(const char *path)
{
    std::FILE *fp = std::fopen(path, "rb");
    CHECK(fp, "cannot open %s", path);
    std::vector<double> all;
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, 8, 4096, fp)) > 0) all.insert(all.end(), buf, buf + got);
    std::fclose(fp);
    size_t at = 0;
    const int n_frames = (int)all.at(at++);
    int compared = 0, stored = 0, recomputed = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int G = (int)all.at(at), P = (int)all.at(at + 1), c = (int)all.at(at + 2), unique = (int)all.at(at + 3);
        const double cost_sum = all.at(at + 4), td = all.at(at + 5);
        at += 6;
        CHECK(at + 3 * (size_t)G + 2 * (size_t)P <= all.size(), "frame %d: the file is short", f);
        const std::vector<double> gt(all.begin() + at, all.begin() + at + 2 * G);
        at += 2 * G;
        const std::vector<double> det(all.begin() + at, all.begin() + at + 2 * P);
        at += 2 * P;
        const FrameResult r = run_frame(gt, det, td);
        CHECK(r.t.matched == c, "frame %d (G %d, P %d): c %lld, scipy's %d", f, G, P, r.t.matched, c);
        CHECK(std::fabs(r.t.cost - cost_sum) <= 1e-9 * std::fabs(cost_sum), "frame %d: cost %.17g, scipy's %.17g", f, r.t.cost, cost_sum);
        if (unique) {
            for (int o = 0; o < G; ++o) CHECK(r.match[o] == (int)all.at(at + o), "frame %d: ground truth %d -> %d, scipy's %d", f, o, r.match[o], (int)all.at(at + o));
            ++compared;
        }
        at += G;
        check_swapped(gt, det, td, r);
        (G * P <= kCostEntries ? stored : recomputed) += 1;
    }
    CHECK(at == all.size(), "the file is longer than its frames");
    std::printf("ok frames: %d frames (%d with stored costs, %d with recomputed ones), %d match tables compared\n", n_frames, stored, recomputed, compared);
    return 0;
}

static int run_wide(uint64_t seed)
{
    rng_state = seed * 0x9e3779b97f4a7c15ull + 7;
    const int sizes[][2] = {{kMaxSide, kMaxSide}, {300, kMaxSide}, {kMaxSide, 3}, {45, 46}};
    for (const auto &gp : sizes) {
        std::vector<double> gt(2 * gp[0]), det(2 * gp[1]);
        for (size_t k = 0; k < gt.size(); k += 2) { gt[k] = uniform() * 480; gt[k + 1] = uniform() * 1440; }
        for (size_t k = 0; k < det.size(); k += 2) { // most detections near a ground truth, the rest anywhere
            const size_t o = 2 * (rnd() % gp[0]);
            const bool near = rnd() % 4 != 0;
            det[k] = near ? gt[o] + (uniform() - .5) * 50 : uniform() * 480;
            det[k + 1] = near ? gt[o + 1] + (uniform() - .5) * 50 : uniform() * 1440;
        }
        const FrameResult r = run_frame(gt, det, kTd);
        CHECK(r.t.matched > 0, "%d x %d: nothing matched", gp[0], gp[1]);
        check_swapped(gt, det, kTd, r);
    }
    std::printf("ok wide\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "brute")) return run_brute(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 3 && !std::strcmp(argv[1], "frames")) return run_frames(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "wide")) return run_wide(std::strtoull(argv[2], nullptr, 10));
    std::printf("usage: harness brute SEED COUNT | frames FILE | wide SEED\n");
    return 2;
}
