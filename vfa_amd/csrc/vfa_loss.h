// vfa_loss.h -- the rules of the target encoder (reference vfa/data/encoder.py:152-217) and of the detection loss (vfa/model/loss.py)
// as plain host / device code: everything integer or rule-like, and the per-element float32 arithmetic, so that
// tests/native/loss_harness.cpp compiles this file with g++ and checks it on the CPU (the pattern of vfa_cellconv.h / vfa_assign.h).
//
// Cell of an object (encoder.py:152-165, 173-190), float32, one rounding per reference operation (no contraction):
//   u = loc0 / world0 * L, v = loc1 / world1 * W; coord_x = (int)u, coord_y = (int)v (toward zero); offset = u - coord_x, v - coord_y;
//   MultiviewC / MultiviewX: row coord_y, column coord_x; Wildtrack: row coord_x, column coord_y; flat cell = row * W + column.
//   DEVIATION: an object outside the map, or with a non-finite coordinate, has cell -1 and is dropped (the reference raises, or wraps
//   a negative index).
// Angle label (encoder.py:214): (int)(angle * 57.29577951308232f); the CSL row is row[j] = table[(j + R/2 - label) mod R] for the
//   table[i] = exp(-(i - R/2)^2 / (2 sigma^2)) the HOST makes (float64, rounded to float32): no exp on the device.  Labels outside
//   the reference's slicing range wrap modulo R (a deviation; inside -R/2 .. 3R/2 - 1 the rows are the reference's).
// Duplicates: the LATER object of a cell wins (the reference overwrites), a cell counts once, live objects come out in ascending cell
//   order (the order of pred[...][mask]).
#ifndef VFA_LOSS_H
#define VFA_LOSS_H

#include <math.h>

#if defined(__HIPCC__)
#define VFA_LOSS_HD __host__ __device__ __forceinline__
#else
#define VFA_LOSS_HD inline
#endif

namespace vfa_loss {

constexpr int kMaxObjects = 1024;  // K of the encoder, k of the loss (VFA_DET_MAX_OBJECTS of include/vfa_hip.h)
constexpr int kMaxRot = 1024;      // R (VFA_DET_MAX_ROT)
constexpr int kKindWildtrack = 2;  // _lib.CONV_KIND
constexpr float kDegPerRad = 57.29577951308232f;
constexpr float kProbLo = 1e-5f, kProbHi = 0.99999f;  // clamp(eps, 1 - eps) of loss.py:9 after the cast to float32

struct Assigned {
    int cell;            // row * W + column, or -1: dropped
    float off_x, off_y;  // channels 0 and 1 of the loc_offset target
};

// (int)t is defined: t is finite and strictly inside the int range (a NaN fails both comparisons)
VFA_LOSS_HD bool truncates(float t) { return t > -2147483648.0f && t < 2147483648.0f; }

VFA_LOSS_HD Assigned assign_cell(float loc0, float loc1, float world0, float world1, int L, int W, int kind)
{
    Assigned a = {-1, 0.0f, 0.0f};
    const float u = loc0 / world0 * (float)L;
    const float v = loc1 / world1 * (float)W;
    if (!truncates(u) || !truncates(v)) return a;
    const int coord_x = (int)u, coord_y = (int)v;
    const int row = kind == kKindWildtrack ? coord_x : coord_y, col = kind == kKindWildtrack ? coord_y : coord_x;
    if (row < 0 || col < 0 || row >= L || col >= W) return a;
    a.cell = row * W + col;
    a.off_x = u - (float)coord_x;
    a.off_y = v - (float)coord_y;
    return a;
}

VFA_LOSS_HD int angle_label(float angle)
{
    const float deg = angle * kDegPerRad;
    return truncates(deg) ? (int)deg : 0;
}

// row[j] = table[table_index(j, label_shift(label, R), R)]; shift in [0, R)
VFA_LOSS_HD int label_shift(int label, int R)
{
    const int s = (R / 2 - label % R) % R;  // in (-R, R)
    return s < 0 ? s + R : s;
}

VFA_LOSS_HD int table_index(int j, int shift, int R)
{
    const int i = j + shift;
    return i >= R ? i - R : i;
}

// the cell of object i if it is live -- inside the map and no later object of the frame in the same cell -- else -1
VFA_LOSS_HD int live_key(const int *cell, int n, int i)
{
    const int c = cell[i];
    if (c < 0) return -1;
    for (int j = i + 1; j < n; ++j)
        if (cell[j] == c) return -1;
    return c;
}

// output row of live object i: the number of live objects in a lower cell (live cells are distinct)
VFA_LOSS_HD int rank_of(const int *key, int n, int i)
{
    int r = 0;
    for (int j = 0; j < n; ++j) r += (key[j] >= 0 && key[j] < key[i]) ? 1 : 0;
    return r;
}

// ---- per-element float32 arithmetic, the reference's operation sequence (loss.py:9-18, SmoothL1 with beta = 1)
VFA_LOSS_HD float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
VFA_LOSS_HD float clamp_prob(float p) { return p < kProbLo ? kProbLo : (p > kProbHi ? kProbHi : p); }  // (a NaN stays a NaN)

VFA_LOSS_HD float focal_pos(float p)
{
    const float q = 1.0f - p;
    return -((q * q) * logf(p));
}

VFA_LOSS_HD float focal_neg(float p, float gt)
{
    const float g = 1.0f - gt, g2 = g * g;
    return -(((g2 * g2) * (p * p)) * logf(1.0f - p));
}

// d p_clamped / d x at the unclamped sigmoid s: s (1 - s) inside [eps, 1 - eps], 0 outside
VFA_LOSS_HD float prob_slope(float s) { return (s < kProbLo || s > kProbHi) ? 0.0f : s * (1.0f - s); }

VFA_LOSS_HD float focal_pos_slope(float p)
{
    const float q = 1.0f - p;
    return 2.0f * q * logf(p) - (q * q) / p;
}

VFA_LOSS_HD float focal_neg_slope(float p, float gt)
{
    const float g = 1.0f - gt, g2 = g * g, q = 1.0f - p;
    return (g2 * g2) * (-2.0f * p * logf(q) + (p * p) / q);
}

VFA_LOSS_HD float smooth_l1(float d)
{
    const float z = fabsf(d);
    return z < 1.0f ? 0.5f * z * z : z - 0.5f;
}

VFA_LOSS_HD float smooth_l1_slope(float d) { return fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f); }

// focal loss with reduction 'mean' and its special cases (loss.py:19-31); no entries at all: 0
VFA_LOSS_HD float focal_mean(float pos_sum, float neg_sum, int n_pos, int n_neg)
{
    if (n_pos == 0 && n_neg == 0) return 0.0f;
    if (n_pos == 0) return neg_sum / (float)n_neg;
    if (n_neg == 0) return pos_sum / (float)n_pos;
    return neg_sum / (float)n_neg + pos_sum / (float)n_pos;
}

}  // namespace vfa_loss

#endif  // VFA_LOSS_H
