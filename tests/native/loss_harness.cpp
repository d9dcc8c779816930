// The rules of the target encoder (vfa_amd/csrc/vfa_loss.h, shared host / device code) on the CPU: the threads of
// det_targets_kernel run as loops.  `encode_frame` below walks a frame the way the kernel does -- assign_cell per object, live_key,
// rank_of, rows written at their rank -- and is checked against brute force: a dense map that the objects overwrite in order, read
// out in ascending cell order (what the reference's loops followed by pred[...][mask] amount to).
//
//   harness cases SEED          random frames on small maps of the three dataset kinds: objects inside, outside, on the last row and
//                               column, at negative, huge, infinite and NaN coordinates, many duplicates; the label rows for labels
//                               -180 .. 539 at R = 360 (and every label at R = 24, 2) against the reference's slicing rule restated.
//   harness encode L W KIND WORLD0 WORLD1 N  X0 Y0 A0  X1 Y1 A1 ...
//                               one frame given as float32 BIT PATTERNS (decimal); prints "ok N_POS" and per live object
//                               "cell offx_bits offy_bits label": the Python test compares them with the reference's records.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../vfa_amd/csrc/vfa_loss.h"

using namespace vfa_loss;

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static float uniform() { return (float)(rnd() & 0xffffff) / 16777216.0f; }

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
static float float_of(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

struct Row { int cell; float off_x, off_y; int label; };

// det_targets_kernel with the threads as loops
static std::vector<Row> encode_frame(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &angle, float world0,
                                     float world1, int L, int W, int kind)
{
    const int n = (int)x.size();
    std::vector<int> cell(n), key(n);
    std::vector<Assigned> as(n);
    for (int i = 0; i < n; ++i) {
        as[i] = assign_cell(x[i], y[i], world0, world1, L, W, kind);
        cell[i] = as[i].cell;
    }
    int live = 0;
    for (int i = 0; i < n; ++i) {
        key[i] = live_key(cell.data(), n, i);
        live += key[i] >= 0;
    }
    std::vector<Row> rows(live, Row{-2, 0.0f, 0.0f, 0});
    for (int i = 0; i < n; ++i) {
        if (key[i] < 0) continue;
        const int r = rank_of(key.data(), n, i);
        CHECK(r >= 0 && r < live, "rank %d of %d live", r, live);
        CHECK(rows[r].cell == -2, "row %d written twice", r);
        rows[r] = Row{key[i], as[i].off_x, as[i].off_y, angle_label(angle[i])};
    }
    return rows;
}

static float odd_coordinate(float extent)
{
    switch (rnd() % 50) {
    case 0: return -extent * uniform();
    case 1: return extent * (1.0f + uniform());
    case 2: return std::numeric_limits<float>::quiet_NaN();
    case 3: return std::numeric_limits<float>::infinity();
    case 4: return -std::numeric_limits<float>::infinity();
    case 5: return 3.0e38f;
    case 6: return -1.0e30f;
    case 7: return extent;                                  // exactly the far edge: outside
    case 8: return std::nextafterf(extent, 0.0f);           // the last cell, or rounded onto the edge
    default: return extent * uniform();
    }
}

static void check_frames(int n_frames)
{
    long long dropped = 0, duplicates = 0, lives = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int L = 1 + (int)(rnd() % 9), W = 1 + (int)(rnd() % 13), kind = (int)(rnd() % 3);
        const float world0 = 10.0f + 500.0f * uniform(), world1 = 10.0f + 900.0f * uniform();
        const int n = (int)(rnd() % 40);
        std::vector<float> x(n), y(n), angle(n);
        for (int i = 0; i < n; ++i) {
            // a coordinate scaled by L may index a column of W > L cells: draw it over the larger extent
            x[i] = odd_coordinate(world0 * (float)(W > L ? W : L) / (float)L);
            y[i] = odd_coordinate(world1 * (float)(W > L ? W : L) / (float)W);
            angle[i] = (uniform() - 0.3f) * 12.0f;
        }
        const std::vector<Row> got = encode_frame(x, y, angle, world0, world1, L, W, kind);

        // brute force: the dense maps the objects overwrite in order
        std::vector<int> owner((size_t)L * W, -1);
        for (int i = 0; i < n; ++i) {
            const float u = x[i] / world0 * (float)L, v = y[i] / world1 * (float)W;
            if (!std::isfinite(u) || !std::isfinite(v) || std::fabs(u) >= 2147483648.0f || std::fabs(v) >= 2147483648.0f) {
                dropped += 1;
                continue;
            }
            const long long cx = (long long)std::trunc((double)u), cy = (long long)std::trunc((double)v);
            const long long row = kind == 2 ? cx : cy, col = kind == 2 ? cy : cx;
            if (row < 0 || col < 0 || row >= L || col >= W) {
                dropped += 1;
                continue;
            }
            duplicates += owner[row * W + col] >= 0;
            owner[row * W + col] = i;
        }
        size_t r = 0;
        for (int c = 0; c < L * W; ++c) {
            if (owner[c] < 0) continue;
            const int i = owner[c];
            CHECK(r < got.size(), "frame %d: fewer rows (%zu) than live cells", f, got.size());
            const float u = x[i] / world0 * (float)L, v = y[i] / world1 * (float)W;
            CHECK(got[r].cell == c, "frame %d row %zu: cell %d, brute force %d", f, r, got[r].cell, c);
            CHECK(bits_of(got[r].off_x) == bits_of(u - std::trunc(u)) && bits_of(got[r].off_y) == bits_of(v - std::trunc(v)),
                  "frame %d row %zu: offsets of object %d", f, r, i);
            CHECK(got[r].label == (int)(angle[i] * 57.29577951308232f), "frame %d row %zu: label", f, r);
            r += 1;
        }
        CHECK(r == got.size(), "frame %d: %zu rows, %zu live cells", f, got.size(), r);
        lives += (long long)r;
    }
    CHECK(dropped > n_frames && duplicates > n_frames / 2 && lives > n_frames, "the frames do not reach the cases: %lld %lld %lld", dropped,
          duplicates, lives);
    std::printf("%d frames: %lld live, %lld dropped, %lld overwritten\n", n_frames, lives, dropped, duplicates);
}

// gaussian_label's row for `label`: concatenate(y[c - label:], y[:c - label]) with Python's slice rules, c = R / 2, as indices into y
static std::vector<int> sliced_row(int label, int R)
{
    long long start = R / 2 - label;
    if (start < 0) start += R;
    if (start < 0) start = 0;
    if (start > R) start = R;
    std::vector<int> row;
    for (long long i = start; i < R; ++i) row.push_back((int)i);
    for (long long i = 0; i < start; ++i) row.push_back((int)i);
    return row;
}

static void check_labels()
{
    const int sizes[3] = {360, 24, 2};
    for (int R : sizes) {
        for (int label = -R / 2; label < R + R / 2; ++label) {   // the labels for which the reference's slices make a full rotation
            const std::vector<int> want = sliced_row(label, R);
            CHECK((int)want.size() == R, "R %d label %d: the slicing rule gives %zu entries", R, label, want.size());
            const int shift = label_shift(label, R);
            CHECK(shift >= 0 && shift < R, "shift %d", shift);
            int peaks = 0;
            for (int j = 0; j < R; ++j) {
                const int idx = table_index(j, shift, R);
                CHECK(idx == want[j], "R %d label %d entry %d: table index %d, the slices give %d", R, label, j, idx, want[j]);
                if (idx == R / 2) {
                    peaks += 1;
                    CHECK(j == ((label % R) + R) % R, "R %d label %d: the peak sits at %d", R, label, j);
                }
            }
            CHECK(peaks == 1, "R %d label %d: %d peaks", R, label, peaks);
        }
        const int far[6] = {-100000, -R - 1, 4 * R + 3, 2147483647, -2147483647 - 1, 1 << 30};   // beyond: wraps, stays inside the table
        for (int label : far)
            for (int j = 0; j < R; ++j) {
                const int idx = table_index(j, label_shift(label, R), R);
                CHECK(idx >= 0 && idx < R, "R %d label %d entry %d: index %d", R, label, j, idx);
            }
    }
    CHECK(angle_label(std::numeric_limits<float>::quiet_NaN()) == 0 && angle_label(std::numeric_limits<float>::infinity()) == 0 &&
              angle_label(1.0e30f) == 0,
          "a non-finite or huge angle has label 0");
    CHECK(angle_label(-0.8f) == -45 && angle_label(3.5f) == 200, "truncation toward zero");
    std::printf("labels ok\n");
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "cases")) {
        rng_state = 0x9e3779b97f4a7c15ull * (uint64_t)(std::atoi(argv[2]) + 1);
        std::printf("ok\n");
        check_frames(2000);
        check_labels();
        return 0;
    }
    if (argc >= 8 && !std::strcmp(argv[1], "encode")) {
        const int L = std::atoi(argv[2]), W = std::atoi(argv[3]), kind = std::atoi(argv[4]);
        const float world0 = (float)std::atof(argv[5]), world1 = (float)std::atof(argv[6]);
        const int n = std::atoi(argv[7]);
        CHECK(argc == 8 + 3 * n, "encode: %d objects need %d numbers", n, 3 * n);
        std::vector<float> x(n), y(n), angle(n);
        for (int i = 0; i < n; ++i) {
            x[i] = float_of((uint32_t)std::strtoul(argv[8 + 3 * i], nullptr, 10));
            y[i] = float_of((uint32_t)std::strtoul(argv[9 + 3 * i], nullptr, 10));
            angle[i] = float_of((uint32_t)std::strtoul(argv[10 + 3 * i], nullptr, 10));
        }
        const std::vector<Row> rows = encode_frame(x, y, angle, world0, world1, L, W, kind);
        std::printf("ok %zu\n", rows.size());
        for (const Row &r : rows) std::printf("%d %u %u %d\n", r.cell, bits_of(r.off_x), bits_of(r.off_y), r.label);
        return 0;
    }
    std::printf("usage: harness cases SEED | harness encode L W KIND WORLD0 WORLD1 N X Y A ...\n");
    return 2;
}
