// The rules of the heat-map targets (vfa_amd/csrc/vfa_heat.h, shared host / device code) on the CPU: the threads of heat_rgk_kernel
// and heat_gk_kernel run as loops.  Numbers go in and out as BIT PATTERNS (decimal): float32 as uint32, float64 as uint64.
//
//   harness cases SEED     random objects, the degenerate ones included (zero, negative, huge, infinite and NaN dimensions and
//                          angles, k above the limit): every tap and rotated value is in [0, 1], the key order of the arg-max against
//                          a brute-force scan, paste_cell against its definition on maps the window leaves on every side.
//   harness kernels ALPHA RATIO N  L0 W0 DEG0 ...
//                          per object one line "n g_t g_l" followed by n * n pairs "branch value_bits" (n = 0: no kernel, centre only)
//   harness paste L W KIND WORLD0 WORLD1 ALPHA RATIO N  X0 Y0 L0 W0 DEG0 ...
//                          per object one line "cell n g_t g_l count y0 y1 x0 x1": its cell (-1: dropped), kernel size and arg-max,
//                          the number of kernel cells that land in the map and the rows / columns they span (count 0: -1s)
//   harness gk L W KIND WORLD0 WORLD1 R SIGMA2 N  X0 Y0 ...
//                          one frame through the occupancy stores and gk_cell: L * W value_bits
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../vfa_amd/csrc/vfa_heat.h"
#include "../../vfa_amd/csrc/vfa_loss.h"

using namespace vfa_heat;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                              \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static float uniform() { return (float)(rnd() & 0xffffff) / 16777216.0f; }

static float f32_arg(const char *s) { return float_of((uint32_t)std::strtoull(s, nullptr, 10)); }
static double f64_arg(const char *s)
{
    const uint64_t u = std::strtoull(s, nullptr, 10);
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

// heat_rgk_kernel up to its arg-max with the threads as loops; false: centre only
struct Made { int n, g_t, g_l; std::vector<float> rot; std::vector<int> branch; };
static bool make_kernel(float l, float w, double deg, double alpha, int ratio, Made *m)
{
    const Kernel g = kernel_of(l, w, alpha, ratio);
    const Turn t = turn_of(deg);
    m->n = m->g_t = m->g_l = 0;
    m->rot.clear();
    m->branch.clear();
    if (!g.ok || !t.ok) return false;
    const int n = g.n;
    CHECK(n >= 3 && n <= kMaxKernel && g.k == n - 1 && g.lo == -((n) / 2), "n %d k %d lo %d", n, g.k, g.lo);
    std::vector<float> taps((size_t)n * n);
    for (int e = 0; e < n * n; ++e) taps[e] = tap(g, e / n, e % n);
    m->rot.resize((size_t)n * n);
    m->branch.resize((size_t)n * n);
    unsigned long long best = 0;
    for (int e = 0; e < n * n; ++e) {
        m->rot[e] = rotated(taps.data(), n, e / n, e % n, t);
        m->branch[e] = source_of(e / n, e % n, n, t).branch;
        const unsigned long long key = rank_key(m->rot[e], e);
        best = key > best ? key : best;
    }
    const int at = index_of_key(best);
    CHECK(at >= 0 && at < n * n, "arg-max %d of %d", at, n * n);
    m->n = n;
    m->g_t = at / n;
    m->g_l = at % n;
    return true;
}

static int cases(uint64_t seed)
{
    rng_state = seed * 2654435761ull + 99;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float odd_dims[] = {0.0f, -50.0f, 1e-30f, 1e30f, inf, -inf, nan, 640.0f, 641.0f, 900.0f, 1.0f, 100.0f};
    const double odd_deg[] = {0.0, 90.0, -90.0, 180.0, 360.0, 45.0, 1e9, 2e9, (double)inf, (double)nan, -1e-300, 720.5};
    int made = 0, centre_only = 0;
    Made m;
    for (int it = 0; it < 400; ++it) {
        float l = 50.0f + 600.0f * uniform(), w = 20.0f + 300.0f * uniform();
        double deg = -360.0 + 720.0 * (double)uniform();
        if (it % 5 == 0) l = odd_dims[rnd() % 12];
        if (it % 7 == 0) w = odd_dims[rnd() % 12];
        if (it % 3 == 0) deg = odd_deg[rnd() % 12];
        const int ratio = it % 11 == 0 ? 1 + (int)(rnd() % 12) : 8;
        if (!make_kernel(l, w, deg, 0.01, ratio, &m)) {
            // refused for a reason: a dimension that is not positive (or so small that its divisor is 0), an angle that is not
            // finite, a kernel above the limit or below three taps
            const double size = std::ceil((double)(l > w ? l : w) * 0.01) * ratio;
            CHECK(!(l > 1e-10f) || !(w > 1e-10f) || !(std::fabs(deg) <= 1e9) || !(size <= 64.0) || size < 2.0,
                  "l %g w %g deg %g ratio %d refused", (double)l, (double)w, deg, ratio);
            ++centre_only;
            continue;
        }
        ++made;
        const int n = m.n;
        int first = -1;
        float top = -1.0f;
        for (int e = 0; e < n * n; ++e) {
            CHECK(m.rot[e] >= 0.0f && m.rot[e] <= 1.0f, "value %g at %d", (double)m.rot[e], e);
            CHECK(m.branch[e] != kSkip || m.rot[e] == 0.0f, "a skipped cell holds %g", (double)m.rot[e]);
            CHECK(pasted(m.rot[e]) <= kBelowOneBits && (m.rot[e] < 1.0f ? pasted(m.rot[e]) == bits_of(m.rot[e]) : true), "pasted");
            if (m.rot[e] > top) {  // the first of the maxima
                top = m.rot[e];
                first = e;
            }
        }
        CHECK(first == m.g_t * n + m.g_l && top > 0.0f, "arg-max %d, brute force %d", m.g_t * n + m.g_l, first);
        // the paste on a small map the window leaves on every side
        const int L = 5 + (int)(rnd() % 30), W = 5 + (int)(rnd() % 30), row = (int)(rnd() % L), col = (int)(rnd() % W);
        for (int e = 0; e < n * n; ++e) {
            const int r = e / n, q = e % n, y = row - m.g_t + r, x = col - m.g_l + q;
            const int to = paste_cell(row, col, m.g_t, m.g_l, r, q, L, W);
            CHECK(to == ((y >= 0 && y < L && x >= 0 && x < W) ? y * W + x : -1), "paste_cell");
        }
        CHECK(paste_cell(row, col, m.g_t, m.g_l, m.g_t, m.g_l, L, W) == row * W + col, "the arg-max lands on the centre");
    }
    CHECK(made > 100 && centre_only > 20, "made %d, centre only %d", made, centre_only);
    // the key order: value descending, then index ascending
    CHECK(rank_key(0.5f, 3) > rank_key(0.25f, 0) && rank_key(0.5f, 3) > rank_key(0.5f, 4) && rank_key(0.0f, 0) > 0, "key order");
    std::printf("ok %d kernels, %d centre only\n", made, centre_only);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "cases")) return cases(std::strtoull(argv[2], nullptr, 10));
    if (argc >= 5 && !std::strcmp(argv[1], "kernels")) {
        const double alpha = f64_arg(argv[2]);
        const int ratio = std::atoi(argv[3]), N = std::atoi(argv[4]);
        CHECK(argc == 5 + 3 * N, "argument count");
        std::printf("ok %d\n", N);
        Made m;
        for (int i = 0; i < N; ++i) {
            make_kernel(f32_arg(argv[5 + 3 * i]), f32_arg(argv[6 + 3 * i]), f64_arg(argv[7 + 3 * i]), alpha, ratio, &m);
            std::printf("%d %d %d", m.n, m.g_t, m.g_l);
            for (int e = 0; e < m.n * m.n; ++e) std::printf(" %d %u", m.branch[e], bits_of(m.rot[e]));
            std::printf("\n");
        }
        return 0;
    }
    if (argc >= 10 && !std::strcmp(argv[1], "paste")) {
        const int L = std::atoi(argv[2]), W = std::atoi(argv[3]), kind = std::atoi(argv[4]);
        const float world0 = f32_arg(argv[5]), world1 = f32_arg(argv[6]);
        const double alpha = f64_arg(argv[7]);
        const int ratio = std::atoi(argv[8]), N = std::atoi(argv[9]);
        CHECK(argc == 10 + 5 * N, "argument count");
        std::printf("ok %d\n", N);
        Made m;
        for (int i = 0; i < N; ++i) {
            char **o = argv + 10 + 5 * i;
            const int cell = vfa_loss::assign_cell(f32_arg(o[0]), f32_arg(o[1]), world0, world1, L, W, kind).cell;
            make_kernel(f32_arg(o[2]), f32_arg(o[3]), f64_arg(o[4]), alpha, ratio, &m);
            int count = 0, y0 = -1, y1 = -1, x0 = -1, x1 = -1;
            if (cell >= 0)
                for (int e = 0; e < m.n * m.n; ++e) {
                    const int to = paste_cell(cell / W, cell % W, m.g_t, m.g_l, e / m.n, e % m.n, L, W);
                    if (to < 0) continue;
                    const int y = to / W, x = to % W;
                    y0 = count ? (y < y0 ? y : y0) : y;
                    y1 = count ? (y > y1 ? y : y1) : y;
                    x0 = count ? (x < x0 ? x : x0) : x;
                    x1 = count ? (x > x1 ? x : x1) : x;
                    ++count;
                }
            std::printf("%d %d %d %d %d %d %d %d %d\n", cell, m.n, m.g_t, m.g_l, count, y0, y1, x0, x1);
        }
        return 0;
    }
    if (argc >= 10 && !std::strcmp(argv[1], "gk")) {
        const int L = std::atoi(argv[2]), W = std::atoi(argv[3]), kind = std::atoi(argv[4]);
        const float world0 = f32_arg(argv[5]), world1 = f32_arg(argv[6]);
        const int r = std::atoi(argv[7]);
        const double sigma2 = f64_arg(argv[8]);
        const int N = std::atoi(argv[9]), side = 2 * r + 1;
        CHECK(argc == 10 + 2 * N && r >= 0 && r <= kMaxRadius, "arguments");
        std::vector<float> table((size_t)side * side);
        for (int i = 0; i < side; ++i)
            for (int j = 0; j < side; ++j)
                table[(size_t)i * side + j] = (float)std::exp(-((double)((j - r) * (j - r)) + (double)((i - r) * (i - r))) / (2.0 * sigma2));
        std::vector<unsigned char> occ((size_t)L * W, 0);
        for (int i = 0; i < N; ++i) {
            const int cell = vfa_loss::assign_cell(f32_arg(argv[10 + 2 * i]), f32_arg(argv[11 + 2 * i]), world0, world1, L, W, kind).cell;
            if (cell >= 0) occ[cell] = 1;
        }
        std::printf("ok\n");
        for (int y = 0; y < L; ++y)
            for (int x = 0; x < W; ++x) std::printf("%u ", bits_of(gk_cell(occ.data(), table.data(), r, L, W, y, x)));
        std::printf("\n");
        return 0;
    }
    std::printf("usage: harness cases SEED | kernels ... | paste ... | gk ...\n");
    return 2;
}
