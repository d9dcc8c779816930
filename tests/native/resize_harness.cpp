// The rules of the image front end (vfa_amd/csrc/vfa_resize.h, shared host / device code) on the CPU: image_plan_kernel and the two
// passes of image_frames_kernel run as loops over a whole image.  Floats go in as BIT PATTERNS (decimal uint32); images travel as files
// of raw bytes.
//
//   harness cases SEED     random axes, the limits included: 1 <= n <= ksize <= kMaxTaps where the lengths allow it, the taps inside
//                          the source, bounds that grow with the index (what a tile's source window relies on) and span the run of
//                          indices within the bound the kernel sizes its LDS by, coefficients >= 0 that sum to 2^22 within the
//                          rounding of n taps, the identity on an axis that keeps its length, a pass on constant bytes gives them
//                          back, the table against its expression.
//   harness frame IN HIN WIN HOUT WOUT MEAN0 MEAN1 MEAN2 STD0 STD1 STD2 OUT_U8 OUT_F32
//                          IN: HIN * WIN * 3 bytes -> OUT_U8: the resized bytes (HOUT, WOUT, 3), OUT_F32: the tensor (3, HOUT, WOUT)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vfa_amd/csrc/vfa_resize.h"

using namespace vfa_resize;

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

static float f32_arg(const char *s)
{
    const uint32_t u = (uint32_t)std::strtoull(s, nullptr, 10);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// image_plan_kernel for one axis
struct AxisPlan { int ksize; std::vector<int> first, n, k; };
static AxisPlan plan_axis(int in, int out)
{
    const Axis a = axis_of(in, out);
    AxisPlan p;
    p.ksize = a.ksize;
    p.first.resize(out);
    p.n.resize(out);
    p.k.resize((size_t)out * a.ksize);
    for (int i = 0; i < out; ++i) p.n[i] = coefficients(a, i, &p.first[i], p.k.data() + (size_t)i * a.ksize);
    return p;
}

// one pass over an image of `lines` lines of `in` pixels of three bytes: `along` the distance of neighbouring pixels of the axis,
// `across` that of neighbouring lines, in pixels, for the source; the target is written densely the same way round
static void run_pass(const std::vector<uint8_t> &src, std::vector<uint8_t> *dst, const AxisPlan &p, int out, int lines, bool horizontal)
{
    const int in_len = (int)(src.size() / 3 / lines);
    dst->assign((size_t)out * lines * 3, 0);
    for (int line = 0; line < lines; ++line)
        for (int i = 0; i < out; ++i)
            for (int c = 0; c < 3; ++c) {
                const size_t from = horizontal ? ((size_t)line * in_len + p.first[i]) * 3 + c : ((size_t)p.first[i] * lines + line) * 3 + c;
                const size_t to = horizontal ? ((size_t)line * out + i) * 3 + c : ((size_t)i * lines + line) * 3 + c;
                (*dst)[to] = pass_pixel(src.data() + from, horizontal ? 3 : 3 * lines, p.k.data() + (size_t)i * p.ksize, p.n[i]);
            }
}

static void check_axis(int in, int out)
{
    const int ksize = ksize_of(in, out);
    CHECK(ksize >= 3 && ksize % 2 == 1, "%d -> %d ksize %d", in, out, ksize);
    if ((long long)in <= 8LL * out) CHECK(ksize <= kMaxTaps, "%d -> %d ksize %d", in, out, ksize);
    if (ksize > kMaxTaps) return;
    const AxisPlan p = plan_axis(in, out);
    for (int i = 0; i < out; ++i) {
        const int first = p.first[i], n = p.n[i];
        int also_first;
        CHECK(bounds(axis_of(in, out), i, &also_first) == n && also_first == first, "%d -> %d at %d", in, out, i);
        CHECK(n >= 1 && n <= ksize && first >= 0 && first + n <= in, "%d -> %d at %d: first %d n %d", in, out, i, first, n);
        if (i > 0) CHECK(first >= p.first[i - 1] && first + n >= p.first[i - 1] + p.n[i - 1], "%d -> %d at %d: bounds go back", in, out, i);
        long long sum = 0;
        for (int t = 0; t < ksize; ++t) {
            const int k = p.k[(size_t)i * ksize + t];
            CHECK(k >= 0 && (t < n || k == 0), "%d -> %d at %d tap %d: %d", in, out, i, t, k);
            sum += k;
        }
        CHECK(sum >= (1 << kPrecisionBits) - n && sum <= (1 << kPrecisionBits) + n, "%d -> %d at %d: sum %lld", in, out, i, sum);
        if (in == out) CHECK(first == i && p.k[(size_t)i * ksize] == 1 << kPrecisionBits, "%d at %d: not the identity", in, i);
        for (int v = 0; v < 256; v += 51) {
            uint8_t line[kMaxTaps];
            std::memset(line, v, sizeof line);
            CHECK(pass_pixel(line, 1, p.k.data() + (size_t)i * ksize, n) == v, "%d -> %d at %d: constant %d", in, out, i, v);
        }
    }
    // the bound image_frames_kernel sizes its LDS by, for runs of every length a tile can have
    for (int count = 1; count <= 128 && count <= out; count = count * 2 + (rnd() & 1)) {
        const long long bound = ((long long)(count - 1) * in) / out + ksize + 1;
        for (int i = 0; i + count <= out; i += 1 + (int)(rnd() % 7)) {
            const int last = i + count - 1;
            CHECK(p.first[last] + p.n[last] - p.first[i] <= bound, "%d -> %d run %d at %d", in, out, count, i);
        }
    }
}

static int run_cases(uint64_t seed)
{
    rng_state = seed * 0x9e3779b97f4a7c15ull + 1;
    const int fixed[][2] = {{1080, 720}, {1920, 1280}, {720, 720}, {1, 1}, {1, 40}, {40, 1}, {8, 1}, {9, 1}, {16384, 2048}, {16384, 2047},
                            {2048, 16384}, {5, 41}, {100, 13}, {100, 99}, {kMaxLength, kMaxLength}};
    for (const auto &f : fixed) check_axis(f[0], f[1]);
    for (int i = 0; i < 300; ++i) {
        const int in = 1 + (int)(rnd() % 700), out = 1 + (int)(rnd() % 700);
        check_axis(in, out);
    }
    CHECK(ksize_of(1080, 720) == 5 && ksize_of(720, 1080) == 3 && ksize_of(8, 1) == 17 && ksize_of(9, 1) == 19, "ksize");
    for (int b = 0; b < 256; ++b) {
        const float t = (float)b / 255.0f, want = (t - 0.485f) / 0.229f;
        CHECK(table_entry(b, 0.485f, 0.229f) == want && table_entry(b, 0.0f, 1.0f) == t, "table at %d", b);
    }
    CHECK(table_entry(255, 0.0f, 1.0f) == 1.0f && table_entry(0, 0.0f, 1.0f) == 0.0f, "table ends");
    std::printf("ok cases\n");
    return 0;
}

static std::vector<uint8_t> read_file(const char *path, size_t bytes)
{
    std::vector<uint8_t> data(bytes);
    FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr, "cannot open %s", path);
    CHECK(std::fread(data.data(), 1, bytes, f) == bytes, "%s is short", path);
    std::fclose(f);
    return data;
}

static void write_file(const char *path, const void *data, size_t bytes)
{
    FILE *f = std::fopen(path, "wb");
    CHECK(f != nullptr, "cannot open %s", path);
    CHECK(std::fwrite(data, 1, bytes, f) == bytes, "%s: short write", path);
    std::fclose(f);
}

static int run_frame(char **argv)
{
    const int Hin = std::atoi(argv[1]), Win = std::atoi(argv[2]), Hout = std::atoi(argv[3]), Wout = std::atoi(argv[4]);
    CHECK(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && ksize_of(Hin, Hout) <= kMaxTaps && ksize_of(Win, Wout) <= kMaxTaps, "sizes");
    float mean[3], std_[3];
    for (int c = 0; c < 3; ++c) {
        mean[c] = f32_arg(argv[5 + c]);
        std_[c] = f32_arg(argv[8 + c]);
    }
    std::vector<uint8_t> image = read_file(argv[0], (size_t)Hin * Win * 3), inter, out;
    if (Win != Wout) {
        run_pass(image, &inter, plan_axis(Win, Wout), Wout, Hin, true);
    } else {
        inter = image;
    }
    if (Hin != Hout) {
        run_pass(inter, &out, plan_axis(Hin, Hout), Hout, Wout, false);
    } else {
        out = inter;
    }
    std::vector<float> table(kTableEntries), tensor((size_t)3 * Hout * Wout);
    for (int i = 0; i < kTableEntries; ++i) table[i] = table_entry(i & 255, mean[i >> 8], std_[i >> 8]);
    for (int c = 0; c < 3; ++c)
        for (size_t i = 0; i < (size_t)Hout * Wout; ++i) tensor[(size_t)c * Hout * Wout + i] = table[256 * c + out[3 * i + c]];
    write_file(argv[11], out.data(), out.size());
    write_file(argv[12], tensor.data(), tensor.size() * sizeof(float));
    std::printf("ok frame %d x %d -> %d x %d\n", Hin, Win, Hout, Wout);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::strcmp(argv[1], "cases") == 0) return run_cases(std::strtoull(argv[2], nullptr, 10));
    if (argc == 15 && std::strcmp(argv[1], "frame") == 0) return run_frame(argv + 2);
    std::printf("usage: harness cases SEED | frame IN HIN WIN HOUT WOUT MEAN0 MEAN1 MEAN2 STD0 STD1 STD2 OUT_U8 OUT_F32\n");
    return 2;
}
