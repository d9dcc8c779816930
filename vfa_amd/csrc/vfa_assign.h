// vfa_assign.h -- the per-frame assignment of the CLEAR-MOD metric (reference vfa/evaluation/pyeval/CLEAR_MOD_HUN.py:44-93) as
// plain host / device code: ONE WAVE (64 lanes) solves one frame.  The kernel (vfa_assign.hip) runs the lanes as a wave; a host
// compiler runs them as a loop over the lanes (the pattern of vfa_tile.h and vfa_pipe_seq.h), so that tests/native/
// assign_harness.cpp compiles this file with g++ and checks the solver on the CPU against brute force and against scipy's records.
//
// The problem: ground truths o and detections e of a frame at distance d(o, e); cost = d > td ? 1e6 : d (a non-finite distance:
// 1e6); the minimum-cost assignment of min(G, P) pairs (what scipy.optimize.linear_sum_assignment solves, CLEAR_MOD_HUN.py:72);
// a pair is a match when its assigned cost is < td (:73).  Kept quirk: a pair at exactly td keeps the cost td, competes in the
// assignment and is not a match.
//
// The solver: shortest augmenting paths with dual variables (Jonker-Volgenant; the form of Crouse, "On implementing 2D rectangular
// assignment algorithms", 2016).  The smaller side is the rows.  One augmentation per row; each step of an augmentation relaxes the
// slack of every column that is not yet in the tree from the row that entered last (the lanes share the columns), takes the
// smallest slack, THE LOWEST COLUMN INDEX ON A TIE (a wave reduction), and either ends at an unassigned column or goes on from the
// row that column holds.  Each step puts one more column into the tree, so an augmentation ends after at most
// (assigned columns + 1) <= cols steps; EVERY LOOP IS A `for` WITH THAT BOUND, whatever the costs are: a NaN cost never passes a
// `<`, a tree that finds no column ends the augmentation, and a logic error gives a wrong table and a flag, never a loop that
// does not end.  Duals, slacks, predecessors and both match arrays live in the State (LDS on the device).
#ifndef VFA_ASSIGN_H
#define VFA_ASSIGN_H

#include <math.h>

#if defined(__HIPCC__)
#define VFA_ASSIGN_HD __device__ __forceinline__
#else
#define VFA_ASSIGN_HD inline
#endif

// the lanes of the wave: on the device every lane runs the body once, on the host a loop runs it for lane 0 .. 63; a value a lane
// keeps across two such bodies lives in a per-lane slot (one slot on the device: a register)
#if defined(__HIP_DEVICE_COMPILE__)
#define VFA_ASSIGN_LANES(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define VFA_ASSIGN_SLOTS 1
#define VFA_ASSIGN_SLOT(lane) 0
#define VFA_ASSIGN_SYNC() __syncthreads() /* one wave per workgroup: orders the LDS traffic of the lanes */
#else
#define VFA_ASSIGN_LANES(lane) for (int lane = 0; lane < vfa_assign::kLanes; ++lane)
#define VFA_ASSIGN_SLOTS vfa_assign::kLanes
#define VFA_ASSIGN_SLOT(lane) (lane)
#define VFA_ASSIGN_SYNC() ((void)0)
#endif

namespace vfa_assign {

constexpr int kLanes = 64;
constexpr int kMaxSide = 512;       // the cap: frames up to max(P_f, G_f) <= kMaxSide (VFA_CLEAR_MOD_MAX_SIDE of include/vfa_hip.h)
constexpr int kCostEntries = 2048;  // a frame of rows * cols <= kCostEntries keeps its cost matrix in the State; a larger one recomputes
constexpr double kBeyond = 1e6;     // cost of a pair beyond td (CLEAR_MOD_HUN.py:69)

// flags of a solve; 0 = every augmentation ended at an unassigned column within its bound
constexpr int kFlagNoColumn = 1;    // a tree found no column to go to (only costs that are NaN or +inf do that)
constexpr int kFlagBound = 2;       // a loop ran into its bound (a logic error)
constexpr int kFlagWalk = 4;        // the walk back along the predecessors left the table (a logic error)

struct State {
    double gx[kMaxSide], gy[kMaxSide], ex[kMaxSide], ey[kMaxSide]; // the frame: ground truths and detections
    double u[kMaxSide], v[kMaxSide];                               // duals of the rows and of the columns
    double shortest[kMaxSide];                                     // slack of a column: cost of the shortest path into it
    double cost[kCostEntries];                                     // rows x cols, when the frame fits
    short path[kMaxSide];                                          // predecessor: the row the shortest path enters the column from
    short row4col[kMaxSide], col4row[kMaxSide];                    // both match arrays, -1 = unassigned
    unsigned char in_tree[kMaxSide];                               // the column is in the tree of this augmentation
    int walk_flags;
};

struct LaneMin { double val; int idx; };

// (val, idx) of `theirs` replaces `mine` when it is smaller, or equal at a lower index; idx < 0 = nothing yet
VFA_ASSIGN_HD void take_smaller(LaneMin &mine, double val, int idx)
{
    if (idx >= 0 && (mine.idx < 0 || val < mine.val || (val == mine.val && idx < mine.idx))) { mine.val = val; mine.idx = idx; }
}

// the smallest of the lanes' candidates, the lowest index among equal ones, in every lane
VFA_ASSIGN_HD LaneMin wave_min(const LaneMin *part)
{
    LaneMin m = part[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int step = kLanes / 2; step > 0; step >>= 1) {
        const double val = __shfl_xor(m.val, step, kLanes);
        const int idx = __shfl_xor(m.idx, step, kLanes);
        take_smaller(m, val, idx);
    }
#else
    for (int lane = 1; lane < kLanes; ++lane) take_smaller(m, part[lane].val, part[lane].idx);
#endif
    return m;
}

// d(o, e) of CLEAR_MOD_HUN.py:6-7 in float64, in this order, no contraction: the bits of numpy's sqrt on the same operands
VFA_ASSIGN_HD double pair_distance(double gx, double gy, double ex, double ey)
{
    const double dx = gx - ex, dy = gy - ey;
    const double xx = dx * dx, yy = dy * dy;
    return sqrt(xx + yy);
}
// :69; NaN and +inf fail `<=` and cost 1e6 (the reference lets scipy raise on them)
VFA_ASSIGN_HD double pair_cost(double d, double td) { return d <= td ? d : kBeyond; }

// The assignment of `rows` <= `cols` <= kMaxSide: S.col4row[i] = column of row i (every row gets one unless a flag is returned),
// S.row4col[j] = row of column j or -1.  cost(i, j) may be any double.  Returns the flags above.
template <class Cost>
VFA_ASSIGN_HD int solve(State &S, int rows, int cols, const Cost &cost)
{
    int flags = 0;
    VFA_ASSIGN_LANES(lane) {
        for (int j = lane; j < cols; j += kLanes) { S.v[j] = 0.0; S.row4col[j] = -1; }
        for (int i = lane; i < rows; i += kLanes) { S.u[i] = 0.0; S.col4row[i] = -1; }
        if (lane == 0) S.walk_flags = 0;
    }
    for (int cur = 0; cur < rows; ++cur) {
        VFA_ASSIGN_LANES(lane) {
            for (int j = lane; j < cols; j += kLanes) { S.shortest[j] = INFINITY; S.path[j] = -1; S.in_tree[j] = 0; }
        }
        VFA_ASSIGN_SYNC();
        double min_val = 0.0;
        int i = cur, sink = -1;
        bool ended = false;
        for (int step = 0; step < cols + 1; ++step) {
            const double ui = S.u[i];
            LaneMin part[VFA_ASSIGN_SLOTS];
            VFA_ASSIGN_LANES(lane) {
                LaneMin m = {INFINITY, -1};
                for (int j = lane; j < cols; j += kLanes) {
                    if (S.in_tree[j]) continue;
                    const double r = min_val + cost(i, j) - ui - S.v[j];
                    double s = S.shortest[j];
                    if (r < s) { S.shortest[j] = s = r; S.path[j] = (short)i; }
                    if (s < m.val) { m.val = s; m.idx = j; } // (ascending j: the lowest index of equal slacks stays)
                }
                part[VFA_ASSIGN_SLOT(lane)] = m;
            }
            const LaneMin best = wave_min(part);
            if (best.idx < 0) { flags |= kFlagNoColumn; ended = true; break; }
            min_val = best.val;
            VFA_ASSIGN_LANES(lane) { if (lane == 0) S.in_tree[best.idx] = 1; }
            VFA_ASSIGN_SYNC();
            const int held_by = S.row4col[best.idx];
            if (held_by < 0) { sink = best.idx; ended = true; break; }
            i = held_by;
        }
        if (!ended) flags |= kFlagBound;
        if (sink < 0) continue;
        // duals: every column of the tree but the sink holds a row of the tree
        VFA_ASSIGN_LANES(lane) {
            for (int j = lane; j < cols; j += kLanes) {
                const int held_by = S.row4col[j];
                if (!S.in_tree[j] || held_by < 0) continue;
                const double d = min_val - S.shortest[j];
                S.u[held_by] += d;
                S.v[j] -= d;
            }
            if (lane == 0) S.u[cur] += min_val;
        }
        VFA_ASSIGN_SYNC();
        // augment: walk back from the sink along the predecessors to `cur`, at most one column per step of the search
        VFA_ASSIGN_LANES(lane) {
            if (lane == 0) {
                int j = sink, walk = kFlagBound;
                for (int k = 0; k < cols + 1; ++k) {
                    const int from = S.path[j];
                    if (from < 0 || from >= rows) { walk = kFlagWalk; break; }
                    S.row4col[j] = (short)from;
                    const int before = S.col4row[from];
                    S.col4row[from] = (short)j;
                    if (from == cur) { walk = 0; break; }
                    if (before < 0 || before >= cols) { walk = kFlagWalk; break; }
                    j = before;
                }
                S.walk_flags |= walk;
            }
        }
        VFA_ASSIGN_SYNC();
    }
    VFA_ASSIGN_SYNC();
    return flags | S.walk_flags;
}

// cost of (row, column) of a frame whose coordinates are in the State: from the stored matrix, or computed again
struct FrameCost {
    const State *S;
    int cols;
    bool gt_rows, stored;
    double td;
    VFA_ASSIGN_HD double operator()(int i, int j) const
    {
        if (stored) return S->cost[i * cols + j];
        const int o = gt_rows ? i : j, e = gt_rows ? j : i;
        return pair_cost(pair_distance(S->gx[o], S->gy[o], S->ex[e], S->ey[e]), td);
    }
};

struct FrameTotals { long long matched, beyond; double cost; int flags; };

// One frame: G ground truths (S.gx, S.gy) and P detections (S.ex, S.ey), both <= kMaxSide.  Fills gt_match[o] (detection of the
// frame, or -1) and gt_dist[o] (its distance, +inf where unmatched) for o < G and returns, in every lane, the number of matches,
// the number of pairs assigned at 1e6 and the sum of the assigned costs below 1e6, added in ground-truth order.
VFA_ASSIGN_HD FrameTotals solve_frame(State &S, int G, int P, double td, int *gt_match, double *gt_dist)
{
    const bool gt_rows = G <= P;
    const int rows = gt_rows ? G : P, cols = gt_rows ? P : G;
    FrameCost cost = {&S, cols, gt_rows, rows * cols <= kCostEntries, td};
    VFA_ASSIGN_SYNC();
    if (cost.stored) {
        VFA_ASSIGN_LANES(lane) {
            for (int q = lane; q < rows * cols; q += kLanes) {
                const int i = q / cols, j = q - i * cols;
                const int o = gt_rows ? i : j, e = gt_rows ? j : i;
                S.cost[q] = pair_cost(pair_distance(S.gx[o], S.gy[o], S.ex[e], S.ey[e]), td);
            }
        }
        VFA_ASSIGN_SYNC();
    }
    FrameTotals t = {0, 0, 0.0, 0};
    t.flags = solve(S, rows, cols, cost);
    for (int o = 0; o < G; ++o) { // (every lane adds the same terms in the same order: the totals are the wave's)
        const int e = gt_rows ? S.col4row[o] : S.row4col[o];
        if (e < 0 || e >= P) continue;
        const double c = gt_rows ? cost(o, e) : cost(e, o);
        if (c < kBeyond) t.cost += c; else t.beyond += 1;
        if (c < td) t.matched += 1;
    }
    VFA_ASSIGN_LANES(lane) {
        for (int o = lane; o < G; o += kLanes) {
            const int e = gt_rows ? S.col4row[o] : S.row4col[o];
            const bool inside = e >= 0 && e < P;
            const double c = inside ? (gt_rows ? cost(o, e) : cost(e, o)) : kBeyond;
            const bool match = inside && c < td;
            gt_match[o] = match ? e : -1;
            gt_dist[o] = match ? c : INFINITY;
        }
    }
    return t;
}

} // namespace vfa_assign
#endif // VFA_ASSIGN_H
