// vfa_image.hip -- the front of a frame: the cameras' 8-bit frames (N, Hin, Win, 3) as they come off the rig -> the float32
// (N, 3, Hout, Wout) tensor the trunk consumes.  Pillow's antialiased bilinear resize (the reference's transforms.Resize,
// vfa/data/dataset.py:63, train.py:209-214), ToTensor and the model's (x - mean) / std (vfanet.py:59) in one kernel, bit for bit the
// reference's chain.  The rules and the per-element arithmetic: vfa_resize.h.
//
//   vfa_image_plan           image_plan_kernel, one thread per output column, output row and table entry: both axes' bounds and
//                            integer coefficients (double arithmetic of the shared header, on the device) and the 3 x 256 float table
//                            into the caller's workspace.  Once per (sizes, mean, std); no copy from the host, no host wait.
//   vfa_image_frames_u8_f32  image_frames_kernel, ONE WORKGROUP PER (tile of kTileW x TH output pixels, image).  The tile's slice of
//                            the plan and the table go to LDS.  Stage 1, the horizontal pass: the tile's source rows, eight at a
//                            time, come in with aligned dword loads along the row (32 threads a row, every load of a group in
//                            flight at once, issued while the pass runs on the group before) into an LDS staging area; a thread owns
//                            one output column and makes the three bytes of its pixel in the byte intermediate in LDS.  Stage 2, the
//                            vertical pass: a thread owns four neighbouring columns of one output row (twelve intermediate bytes,
//                            three dwords), looks the twelve results up in the table and stores one 16-byte vector per colour plane: a wave
//                            writes two 512-byte runs per plane.  The rows a tile shares with its neighbours above and below are
//                            made again by each; no intermediate image exists in memory.  TH (<= 32) is the host's: the largest
//                            power of two whose rows fit the LDS budget at the vertical scale.
// Both are stream-ordered launches without allocation or global state, so they can be captured in a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vfa_hip.h"
#include "vfa_resize.h"

namespace {

using namespace vfa_resize;

constexpr int kThreads = 256, kTileW = 128, kTileBytes = 3 * kTileW, kMaxTileH = 32, kStageRows = 8, kPlanLoads = 8;
constexpr int kRowLoadsNarrow = 5, kRowLoadsWide = 26;  // dwords of a staged row a thread holds: rows up to 640 bytes (1.6x), and any row
constexpr size_t kLdsBudget = 48 * 1024;  // three workgroups of a compute unit at the strongest downscale, five at 1.5x (32 KB)
static_assert(kMaxTaps == VFA_IMAGE_MAX_TAPS && kMaxLength == VFA_IMAGE_MAX_LENGTH, "include/vfa_hip.h and vfa_resize.h disagree");
static_assert(kThreads == 2 * kTileW && kThreads == 32 * kStageRows && kTileW % 4 == 0, "the thread roles of image_frames_kernel");

// the workspace, in 4-byte words: table (3 x 256) | x bounds (Wout x 2) | x coefficients (Wout x ksx) | y bounds | y coefficients
struct Plan {
    int ksx, ksy;
    size_t xb, xk, yb, yk, words;
};

Plan plan_of(int Hin, int Win, int Hout, int Wout)
{
    Plan p;
    p.ksx = ksize_of(Win, Wout);
    p.ksy = ksize_of(Hin, Hout);
    p.xb = kTableEntries;
    p.xk = p.xb + 2 * (size_t)Wout;
    p.yb = p.xk + (size_t)Wout * p.ksx;
    p.yk = p.yb + 2 * (size_t)Hout;
    p.words = (p.yk + (size_t)Hout * p.ksy + 3) / 4 * 4;
    return p;
}

// the source rows (or columns) a run of `count` output indices can need: end(last) - begin(first) <= (count - 1) scale + 2 support + 1
int span_of(int in, int out, int count, int ksize)
{
    const long long reach = ((long long)(count - 1) * in) / out + ksize + 1;  // (floor of (count - 1) * scale)
    return (int)(reach < in ? reach : in);
}

struct PlanArgs {
    int Hin, Win, Hout, Wout;
    const float *mean, *std;
    int *xb, *xk, *yb, *yk;
    float *table;
};

__global__ __launch_bounds__(kThreads) void image_plan_kernel(const PlanArgs a)
{
    int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < a.Wout) {
        const Axis ax = axis_of(a.Win, a.Wout);
        int first;
        const int n = coefficients(ax, i, &first, a.xk + (size_t)i * ax.ksize);
        a.xb[2 * i] = first;
        a.xb[2 * i + 1] = n;
        return;
    }
    i -= a.Wout;
    if (i < a.Hout) {
        const Axis ax = axis_of(a.Hin, a.Hout);
        int first;
        const int n = coefficients(ax, i, &first, a.yk + (size_t)i * ax.ksize);
        a.yb[2 * i] = first;
        a.yb[2 * i + 1] = n;
        return;
    }
    i -= a.Hout;
    if (i < kTableEntries) a.table[i] = table_entry(i & 255, a.mean[i >> 8], a.std[i >> 8]);
}

struct FrameArgs {
    const uint8_t *src;
    long long image_stride, row_stride;
    int Hin, Win, Hout, Wout, ksx, ksy;
    int TH, rows, stage_bytes;  // tile height; rows of the intermediate and bytes of a staged source row the LDS holds
    int vec4;                   // float4 stores: 4 | Wout and an aligned dst
    const int *xb, *xk, *yb, *yk;
    const float *table;
    float *dst;
};

size_t lds_bytes(int TH, int ksx, int ksy, int rows, int stage_bytes)
{
    return 4 * ((size_t)kTableEntries + 2 * kTileW + 2 * TH + (size_t)kTileW * ksx + (size_t)TH * ksy) + (size_t)rows * kTileBytes
           + (size_t)kStageRows * stage_bytes;
}

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ int byte_of(uint32_t word, int i) { return (int)((word >> (8 * i)) & 255u); }

template <int kRowLoads>
__global__ __launch_bounds__(kThreads) void image_frames_kernel(const FrameArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    float *table = (float *)lds;
    int *xb = (int *)(table + kTableEntries);
    int *yb = xb + 2 * kTileW;
    int *xk = yb + 2 * a.TH;
    int *yk = xk + kTileW * a.ksx;
    uint8_t *inter = (uint8_t *)(yk + a.TH * a.ksy);   // (rows, kTileBytes)
    uint8_t *stage = inter + (size_t)a.rows * kTileBytes;  // (kStageRows, stage_bytes), both multiples of 4

    const int tid = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * a.TH, img = blockIdx.z;
    const int tw = a.Wout - x0 < kTileW ? a.Wout - x0 : kTileW, th = a.Hout - y0 < a.TH ? a.Hout - y0 : a.TH;

    // the tile's slice of the plan, kPlanLoads loads of a thread in flight: the kernel is bound by latencies, not by bytes
    const int at_yb = kTableEntries + 2 * kTileW, at_xk = at_yb + 2 * a.TH, at_yk = at_xk + kTileW * a.ksx, plan_words = at_yk + a.TH * a.ksy;
    auto plan_word = [&](int e) -> const uint32_t * {  // the workspace word behind word e of the slice in LDS; null: none (0 is stored)
        if (e < kTableEntries) return (const uint32_t *)a.table + e;
        if (e < at_yb) return e - kTableEntries < 2 * tw ? (const uint32_t *)a.xb + 2 * (size_t)x0 + (e - kTableEntries) : nullptr;
        if (e < at_xk) return e - at_yb < 2 * th ? (const uint32_t *)a.yb + 2 * (size_t)y0 + (e - at_yb) : nullptr;
        if (e < at_yk) return e - at_xk < tw * a.ksx ? (const uint32_t *)a.xk + (size_t)x0 * a.ksx + (e - at_xk) : nullptr;
        return e - at_yk < th * a.ksy ? (const uint32_t *)a.yk + (size_t)y0 * a.ksy + (e - at_yk) : nullptr;
    };
    for (int base = tid; base < plan_words; base += kThreads * kPlanLoads) {
        uint32_t v[kPlanLoads];
#pragma unroll
        for (int u = 0; u < kPlanLoads; ++u) {
            const int e = base + kThreads * u;
            const uint32_t *p = e < plan_words ? plan_word(e) : nullptr;
            v[u] = p ? *p : 0u;
        }
#pragma unroll
        for (int u = 0; u < kPlanLoads; ++u)
            if (base + kThreads * u < plan_words) ((uint32_t *)lds)[base + kThreads * u] = v[u];
    }
    __syncthreads();

    // the tile's source window: bounds grow with the index, so the first index has the first tap and the last index the last
    const int c0 = xb[0], r0 = yb[0];
    int width = xb[2 * (tw - 1)] + xb[2 * (tw - 1) + 1] - c0, rows = yb[2 * (th - 1)] + yb[2 * (th - 1) + 1] - r0;
    if (3 * width + 3 > a.stage_bytes) width = (a.stage_bytes - 3) / 3;  // (span_of bounds both: never taken)
    if (rows > a.rows) rows = a.rows;
    const uint8_t *window = a.src + (long long)img * a.image_stride + (long long)r0 * a.row_stride + 3LL * c0;

    // ---- stage 1: the horizontal pass, kStageRows source rows at a time.  32 threads bring a row in: the dwords that hold its bytes
    // (inside the pages the row is in, whatever the pointer's alignment), at most 32 * kRowLoads, through registers: loaded while
    // the pass runs on the group before
    const int px = tid & (kTileW - 1), slot = tid >> 7, lrow = tid >> 5, lcol = tid & 31;
    uint32_t held[kRowLoads];
    auto row_words = [&](int r, const uint32_t **from) {
        const uint8_t *p = window + (long long)r * a.row_stride;
        const int skew = (int)((uintptr_t)p & 3);
        *from = (const uint32_t *)(p - skew);
        return (skew + 3 * width + 3) >> 2;
    };
    auto fetch = [&](int g0) {
        if (g0 + lrow >= rows) return;
        const uint32_t *from;
        const int words = row_words(g0 + lrow, &from);
#pragma unroll
        for (int u = 0; u < kRowLoads; ++u) held[u] = lcol + 32 * u < words ? from[lcol + 32 * u] : 0u;
    };
    auto put = [&](int g0) {
        if (g0 + lrow >= rows) return;
        const uint32_t *from;
        const int words = row_words(g0 + lrow, &from);
        uint32_t *to = (uint32_t *)(stage + (size_t)lrow * a.stage_bytes);
#pragma unroll
        for (int u = 0; u < kRowLoads; ++u)
            if (lcol + 32 * u < words) to[lcol + 32 * u] = held[u];
    };
    fetch(0);
    for (int g0 = 0; g0 < rows; g0 += kStageRows) {  // (uniform over the workgroup)
        put(g0);
        __syncthreads();
        fetch(g0 + kStageRows);
        if (px < tw) {
            const int first = xb[2 * px], n = xb[2 * px + 1];
            const int *k = xk + px * a.ksx;
            for (int g = slot; g < kStageRows && g0 + g < rows; g += kThreads / kTileW) {
                const int skew = (int)((uintptr_t)(window + (long long)(g0 + g) * a.row_stride) & 3);
                const uint8_t *s = stage + (size_t)g * a.stage_bytes + skew + 3 * (first - c0);
                int acc0 = pass_begin(), acc1 = acc0, acc2 = acc0;
                for (int t = 0; t < n; ++t, s += 3) {
                    const int kk = k[t];
                    acc0 = pass_tap(acc0, s[0], kk);
                    acc1 = pass_tap(acc1, s[1], kk);
                    acc2 = pass_tap(acc2, s[2], kk);
                }
                uint8_t *o = inter + (size_t)(g0 + g) * kTileBytes + 3 * px;
                o[0] = (uint8_t)pass_end(acc0);
                o[1] = (uint8_t)pass_end(acc1);
                o[2] = (uint8_t)pass_end(acc2);
            }
        }
        __syncthreads();
    }

    // ---- stage 2: the vertical pass, the table, the stores.  Item: four columns of one output row
    const size_t plane = (size_t)a.Hout * a.Wout;
    for (int item = tid; item < th * (kTileW / 4); item += kThreads) {
        const int q = item & (kTileW / 4 - 1), yl = item / (kTileW / 4);
        if (4 * q >= tw) continue;
        const int first = yb[2 * yl], n = yb[2 * yl + 1];
        const int *k = yk + yl * a.ksy;
        const uint32_t *col = (const uint32_t *)(inter + (size_t)(first - r0) * kTileBytes) + 3 * q;
        int acc[12];
        for (int j = 0; j < 12; ++j) acc[j] = pass_begin();
        for (int t = 0; t < n; ++t) {
            const int kk = k[t];
            for (int w = 0; w < 3; ++w) {
                const uint32_t word = col[(size_t)t * (kTileBytes / 4) + w];
                for (int i = 0; i < 4; ++i) acc[4 * w + i] = pass_tap(acc[4 * w + i], byte_of(word, i), kk);
            }
        }
        const int x = x0 + 4 * q;
        for (int c = 0; c < 3; ++c) {  // byte 3 p + c of the twelve: pixel p, channel c
            float v[4];
            for (int p = 0; p < 4; ++p) v[p] = table[256 * c + pass_end(acc[3 * p + c])];
            float *d = a.dst + ((size_t)img * 3 + c) * plane + (size_t)(y0 + yl) * a.Wout + x;
            if (a.vec4 && x + 4 <= a.Wout) {
                *(f32x4 *)d = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                for (int p = 0; p < 4; ++p)
                    if (x + p < a.Wout) d[p] = v[p];
            }
        }
    }
}

// what the entry points check alike about the four lengths
int check_sizes(int Hin, int Win, int Hout, int Wout)
{
    if (Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return VFA_ERR_BAD_ARGUMENT;
    if (Hin > kMaxLength || Win > kMaxLength || Hout > kMaxLength || Wout > kMaxLength) return VFA_ERR_UNSUPPORTED;
    if (ksize_of(Win, Wout) > kMaxTaps || ksize_of(Hin, Hout) > kMaxTaps) return VFA_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" {

size_t vfa_image_workspace_bytes(int Hin, int Win, int Hout, int Wout)
{
    if (check_sizes(Hin, Win, Hout, Wout) != 0) return 0;
    return plan_of(Hin, Win, Hout, Wout).words * 4;
}

int vfa_image_plan(int Hin, int Win, int Hout, int Wout, const float *mean, const float *std, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    const int status = check_sizes(Hin, Win, Hout, Wout);
    if (status != 0) return status;
    if (!mean || !std || !workspace) return VFA_ERR_BAD_ARGUMENT;
    const Plan p = plan_of(Hin, Win, Hout, Wout);
    if (workspace_bytes < p.words * 4) return VFA_ERR_BAD_ARGUMENT;

    int *words = (int *)workspace;
    PlanArgs a = {Hin, Win, Hout, Wout, mean, std, words + p.xb, words + p.xk, words + p.yb, words + p.yk, (float *)workspace};
    const int groups = (Wout + Hout + kTableEntries + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(image_plan_kernel, dim3(groups), dim3(kThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int vfa_image_frames_u8_f32(const unsigned char *src, long long image_stride_bytes, long long row_stride_bytes, int N, int Hin, int Win,
                            const void *workspace, size_t workspace_bytes, float *dst, int Hout, int Wout, void *stream)
{
    if (N < 0) return VFA_ERR_BAD_ARGUMENT;
    const int status = check_sizes(Hin, Win, Hout, Wout);
    if (status != 0) return status;
    if (N == 0) return 0;
    if (!src || !workspace || !dst) return VFA_ERR_BAD_ARGUMENT;
    if (row_stride_bytes < 3LL * Win || image_stride_bytes < 0) return VFA_ERR_BAD_ARGUMENT;
    const Plan p = plan_of(Hin, Win, Hout, Wout);
    if (workspace_bytes < p.words * 4) return VFA_ERR_BAD_ARGUMENT;
    if (N > 65535) return VFA_ERR_UNSUPPORTED;

    FrameArgs a = {};
    a.src = src;
    a.image_stride = image_stride_bytes;
    a.row_stride = row_stride_bytes;
    a.Hin = Hin;
    a.Win = Win;
    a.Hout = Hout;
    a.Wout = Wout;
    a.ksx = p.ksx;
    a.ksy = p.ksy;
    a.stage_bytes = (3 * span_of(Win, Wout, Wout < kTileW ? Wout : kTileW, p.ksx) + 3 + 3) / 4 * 4;
    for (a.TH = kMaxTileH;; a.TH /= 2) {  // (TH = 1 fits: 18 rows at most)
        a.rows = span_of(Hin, Hout, Hout < a.TH ? Hout : a.TH, p.ksy);
        if (a.TH == 1 || lds_bytes(a.TH, p.ksx, p.ksy, a.rows, a.stage_bytes) <= kLdsBudget) break;
    }
    const size_t lds = lds_bytes(a.TH, p.ksx, p.ksy, a.rows, a.stage_bytes);
    if (lds > kLdsBudget) return VFA_ERR_UNSUPPORTED;
    a.vec4 = Wout % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const int *words = (const int *)workspace;
    a.table = (const float *)workspace;
    a.xb = words + p.xb;
    a.xk = words + p.xk;
    a.yb = words + p.yb;
    a.yk = words + p.yk;
    a.dst = dst;
    const dim3 grid((Wout + kTileW - 1) / kTileW, (Hout + a.TH - 1) / a.TH, N);
    if (a.stage_bytes <= 4 * 32 * kRowLoadsNarrow) {
        hipLaunchKernelGGL(image_frames_kernel<kRowLoadsNarrow>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
    } else if (a.stage_bytes <= 4 * 32 * kRowLoadsWide) {
        hipLaunchKernelGGL(image_frames_kernel<kRowLoadsWide>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
    } else {
        return VFA_ERR_UNSUPPORTED;  // (17 taps stage at most 3 * (127 * 8 + 18) + 6 bytes: not reached)
    }
    return (int)hipGetLastError();
}

}  // extern "C"
