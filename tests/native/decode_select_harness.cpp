// The selection of the fused BEV decode (vfa_amd/csrc/vfa_decode.h, shared host / device code) on the CPU: the threads of the
// workgroup run as loops.  `select_topk` below walks the frame the way bev_decode_kernel does -- digit passes, select_advance, the
// collect by threshold in a scrambled slot order, zero padding, the bitonic network -- and every case is checked against std::sort
// of all the candidates' keys.
//
//   harness cases SEED    the named cases (0 candidates, fewer than k, exactly k, all equal, ties that straddle the k-th place, k = 1,
//                         k = 1024 with 1025 candidates, a frame of 70 000 cells that counts three index digits) and 300 random
//                         frames: sizes 1 .. 3000, k 1 .. 1024, confidences drawn from 1 .. 40 distinct values or all distinct.
//   harness keys          the packing: order, round trip, the digits no pass counts.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_decode.h"

using namespace vfa_decode;

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

static uint32_t bits_of(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static long long passes_run, early_ends, selects_of[kPasses + 1]; // selects_of[p]: selects that ran p passes

// bev_decode_kernel's select / collect / order with the threads as loops; returns the selected keys in their final order
static std::vector<uint64_t> select_topk(const std::vector<float> &conf, float thresh, int k)
{
    const long long n_cells = (long long)conf.size();
    Select s = select_begin(k, n_cells);
    int ran = 0;
    for (int pass = 0; pass < kPasses; ++pass) {
        if (!pass_counts(pass, n_cells)) continue;
        unsigned hist[kBins] = {0};
        for (long long i = 0; i < n_cells; ++i) {
            if (!(conf[i] > thresh)) continue;
            const uint64_t key = pack_key(bits_of(conf[i]), (uint32_t)i);
            if (select_matches(s, key)) hist[key_digit(key, pass)] += 1;
        }
        select_advance(s, hist, pass);
        ++passes_run;
        ++ran;
        if (s.done) { ++early_ends; break; }
    }
    ++selects_of[ran];
    static uint64_t keys[kMaxTopk];
    std::vector<uint64_t> taken;
    for (long long i = 0; i < n_cells; ++i) {
        if (!(conf[i] > thresh)) continue;
        const uint64_t key = pack_key(bits_of(conf[i]), (uint32_t)i);
        if (select_takes(s, key)) taken.push_back(key);
    }
    CHECK((long long)taken.size() <= k, "%zu keys pass the threshold, k = %d", taken.size(), k);
    for (size_t i = taken.size(); i > 1; --i) std::swap(taken[i - 1], taken[rnd() % i]); // (the LDS counter hands out slots in any order)
    const int n = (int)taken.size(), padded = pow2_at_least(n);
    CHECK(padded >= n && padded <= kMaxTopk && (padded & (padded - 1)) == 0 && (n <= 1 || padded < 2 * n), "n %d padded %d", n, padded);
    for (int i = 0; i < padded; ++i) keys[i] = i < n ? taken[i] : 0;
    for (int size = 2; size <= padded; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1)
            for (int t = padded / 2 - 1; t >= 0; --t) bitonic_exchange(keys, t, size, stride); // (any order of t)
    return std::vector<uint64_t>(keys, keys + n);
}

static void check(const std::vector<float> &conf, float thresh, int k, const char *what)
{
    std::vector<uint64_t> want;
    for (size_t i = 0; i < conf.size(); ++i)
        if (conf[i] > thresh) want.push_back(pack_key(bits_of(conf[i]), (uint32_t)i));
    std::sort(want.begin(), want.end(), [](uint64_t a, uint64_t b) { return a > b; });
    if ((long long)want.size() > k) want.resize(k);
    const std::vector<uint64_t> got = select_topk(conf, thresh, k);
    CHECK(got.size() == want.size(), "%s: %zu selected, %zu wanted", what, got.size(), want.size());
    for (size_t r = 0; r < got.size(); ++r)
        CHECK(got[r] == want[r], "%s: rank %zu holds cell %u, wanted cell %u", what, r, key_cell(got[r]), key_cell(want[r]));
    // the order the interface promises, stated without the key: confidence descending, equal ones by ascending cell
    for (size_t r = 1; r < got.size(); ++r) {
        const float a = conf[key_cell(got[r - 1])], b = conf[key_cell(got[r])];
        CHECK(a > b || (a == b && key_cell(got[r - 1]) < key_cell(got[r])), "%s: ranks %zu, %zu out of order", what, r - 1, r);
    }
}

static std::vector<float> frame_of(size_t n, int distinct)
{
    std::vector<float> conf(n);
    for (auto &c : conf) {
        const uint32_t r = distinct > 0 ? rnd() % (uint32_t)distinct * 1000003u % 16777216u : rnd() % 16777216u;
        c = (float)(r + 1) / 16777217.0f * 0.999f; // in (0, 1)
        if (rnd() % 4 == 0) c = 0.0f;                // (what the NMS writes off the peaks)
    }
    return conf;
}

static int run_cases(uint64_t seed)
{
    rng_state = seed * 2654435761ull + 12345;
    check(std::vector<float>(500, 0.0f), 0.0f, 100, "0 candidates");
    check(std::vector<float>(500, 0.3f), 0.4f, 100, "0 candidates above the threshold");
    check(std::vector<float>(), 0.4f, 100, "no cells");
    {
        std::vector<float> c = frame_of(700, 0);
        int above = 0;
        for (float v : c) above += v > 0.9f;
        CHECK(above > 1 && above < 100, "%d", above);
        check(c, 0.9f, 100, "fewer than k candidates");
        check(c, 0.9f, above, "exactly k candidates");
        check(c, 0.9f, above - 1, "one candidate more than k");
        check(c, 0.0f, 1, "k = 1");
        check(c, 0.9f, 1, "k = 1 above a threshold");
    }
    check(std::vector<float>(2970, 0.5f), 0.4f, 100, "all candidates equal");
    check(std::vector<float>(70000, 0.5f), 0.0f, 1024, "all equal, three index digits");
    check(std::vector<float>(300, 0.5f), 0.4f, 1024, "all equal, fewer than k");
    {
        std::vector<float> c(1200, 0.0f); // 40 above the plateau, a plateau of 200 across the 100th place, 300 below it
        for (int i = 0; i < 40; ++i) c[29 * i + 3] = 0.9f + 0.001f * (float)(i % 7);
        for (int i = 0; i < 200; ++i) c[5 * i + 1] = 0.75f;
        for (int i = 0; i < 300; ++i) c[4 * i + 2] = c[4 * i + 2] == 0.0f ? 0.5f + 0.0001f * (float)(i % 50) : c[4 * i + 2];
        check(c, 0.4f, 100, "ties that straddle the k-th place");
        check(c, 0.4f, 41, "one of the plateau");
        check(c, 0.4f, 240, "the whole plateau");
        check(c, 0.4f, 239, "the plateau but its last cell");
        check(c, 0.75f, 100, "the plateau is at the threshold");
    }
    {
        std::vector<float> c = frame_of(1025, 0);
        for (auto &v : c) v = v == 0.0f ? 0.25f : v;
        check(c, 0.0f, 1024, "k = 1024 with 1025 candidates");
        c.assign(1025, 0.6f);
        check(c, 0.0f, 1024, "k = 1024 with 1025 equal candidates");
    }
    {
        std::vector<float> c = frame_of(70000, 3); // three index digits, long plateaus
        check(c, 0.1f, 1000, "70 000 cells, three values");
        check(frame_of(65536, 0), 0.0f, 512, "65 536 cells");
        check(frame_of(65537, 2), 0.0f, 512, "65 537 cells");
    }
    for (int round = 0; round < 300; ++round) {
        const size_t n = 1 + rnd() % 3000;
        const int k = (int)std::min<size_t>(n, 1 + rnd() % (round % 3 == 0 ? 1024 : 120));
        const int distinct = round % 2 ? 1 + (int)(rnd() % 40) : 0;
        const float thresh = (rnd() % 3) ? 0.4f : 0.0f;
        check(frame_of(n, distinct), thresh, k, "random");
    }
    long long deep = 0;
    for (int p = 5; p <= kPasses; ++p) deep += selects_of[p];
    CHECK(selects_of[1] > 0 && selects_of[3] + selects_of[4] > 0 && deep > 0, "%lld %lld %lld", selects_of[1], selects_of[4], deep);
    std::printf("ok cases: %lld passes, %lld selects ended early, %lld went into the index digits\n", passes_run, early_ends, deep);
    return 0;
}

static int run_keys()
{
    const float values[] = {1e-45f, 1e-30f, 0.4f, 0.5f, 0.50000006f, 0.99999994f, 1.0f};
    const uint32_t cells[] = {0, 1, 255, 256, 43199, 65535, 65536, 2147483646u};
    uint64_t last = ~0ull;
    for (int v = 6; v >= 0; --v)
        for (uint32_t cell : cells) { // confidence descending, then cell ascending: the keys must fall
            const uint64_t key = pack_key(bits_of(values[v]), cell);
            CHECK(key < last, "value %d cell %u", v, cell);
            CHECK(key_cell(key) == cell && key_conf_bits(key) == bits_of(values[v]), "round trip of cell %u", cell);
            last = key;
        }
    CHECK(last > 0, "a candidate's key is above the zero padding");
    const long long sizes[] = {1, 2, 256, 257, 65536, 65537, 16777216, 16777217, 2147483647};
    const int counted[] = {4, 5, 5, 6, 6, 7, 7, 8, 8};
    for (int i = 0; i < 9; ++i) {
        int passes = 0;
        for (int pass = 0; pass < kPasses; ++pass) passes += pass_counts(pass, sizes[i]);
        CHECK(passes == counted[i], "%lld cells: %d passes", sizes[i], passes);
        const Select s = select_begin(7, sizes[i]);
        CHECK(select_matches(s, pack_key(bits_of(0.5f), (uint32_t)(sizes[i] - 1))) && select_matches(s, pack_key(1, 0)), "%lld", sizes[i]);
        CHECK(s.need == 7 && !s.done && key_conf_bits(s.prefix) == 0, "%lld", sizes[i]);
    }
    std::printf("ok keys\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "cases")) return run_cases(std::strtoull(argv[2], nullptr, 10));
    if (argc >= 2 && !std::strcmp(argv[1], "keys")) return run_keys();
    std::printf("usage: harness cases SEED | keys\n");
    return 2;
}
