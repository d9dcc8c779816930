#!/usr/bin/env python3
"""Generate ``clear_mod.npz`` by RUNNING THE REFERENCE's MODA / MODP evaluation on the CPU.

Runs only where a checkout of the reference is available; ``VFA_REFERENCE_ROOT`` names it.  Nothing of the reference is copied:
the script imports ``vfa.evaluation.pyeval.evaluateDetection`` and calls its own ``evaluateDetection_py`` (-> ``CLEAR_MOD_HUN``) on
text files.  Three sets, each stored as arrays in the text layout ``frame x y``:
  * ``demo1``: ``vfa/evaluation/test-demo.txt`` + ``gt-demo.txt``, ``demo2``: ``pyeval/all_res.txt`` + ``all_test_gt.txt`` -- data the
    reference's programs read, the ground truth cut to the frames that have detections (the only ones the reference reads);
  * ``syn``: seeded synthetic frames, see ``synthetic_set``.
Per set: ``four`` = what ``evaluateDetection_py`` returns (recall, precision, MODA, MODP); per-frame records from THIS script's
call to ``scipy.optimize.linear_sum_assignment`` on the reference's cost matrix (``d > td -> 1e6``): ``records`` (g, n_det, c, sum
of matched distances), ``cost_sum`` (sum of the assigned costs below 1e6, the pairs at exactly td included), ``gt_match``
(detection within the frame or -1, per ground truth row), ``unique`` (every matched pair belongs to EVERY optimal assignment: the
frame's match table may be compared), ``tied`` (built to have tied optima), ``totals`` (sums of c, fp, m, g over the frames the
reference walks).  ``near_td_*``: one ground truth and detections whose dx^2 + dy^2 lies within a few ulps of td^2.
The script ASSERTS what the tests rely on (see ``check_*``); a seed that misses an assertion is not used.

Usage:  VFA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_clear_mod.py     (writes the file next to this script)
"""
import os
import sys
import tempfile

import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
if not os.environ.get("VFA_REFERENCE_ROOT"):
    raise SystemExit("set VFA_REFERENCE_ROOT to a checkout of the reference")
ROOT = os.environ["VFA_REFERENCE_ROOT"]
sys.path.insert(0, ROOT)

from vfa.evaluation.pyeval.evaluateDetection import evaluateDetection_py  # noqa: E402  (the reference)

TD = 30.0
SEED = 20261018
SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 70), (70, 1), (64, 65), (65, 64), (130, 70), (70, 130), (12, 14)]


# --- the per-frame solve, restated with scipy ------------------------------------------------------------------------------------
def distances(gt_xy, det_xy):
    dx, dy = gt_xy[:, None, 0] - det_xy[None, :, 0], gt_xy[:, None, 1] - det_xy[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def solve(cost):
    """scipy on the reference's cost matrix -> (gt_match, c, sum of matched distances, sum of assigned costs below 1e6, total)."""
    rows, cols = linear_sum_assignment(cost)
    assigned = cost[rows, cols]
    hit = assigned < TD
    match = np.full(cost.shape[0], -1, np.int32)
    match[rows[hit]] = cols[hit]
    return match, int(hit.sum()), float(assigned[hit].sum()), float(assigned[assigned < 1e6].sum()), float(assigned.sum())


def frame_record(gt_xy, det_xy, rng):
    d = distances(gt_xy, det_xy)
    cost = np.where(d > TD, 1e6, d)
    match, c, match_sum, cost_sum, total = solve(cost)
    # the same frame under 6 permutations of its rows and columns
    stable = True
    for _ in range(6):
        pr, pc = rng.permutation(cost.shape[0]), rng.permutation(cost.shape[1])
        _, c2, match_sum2, cost_sum2, _ = solve(cost[pr][:, pc])
        stable &= c2 == c and abs(match_sum2 - match_sum) <= 1e-9 * max(1.0, match_sum) and abs(cost_sum2 - cost_sum) <= 1e-9 * max(1.0, cost_sum)
    # a matched pair belongs to every optimal assignment when forbidding it makes the optimum dearer
    unique = True
    for o in np.flatnonzero(match >= 0):
        without = cost.copy()
        without[o, match[o]] = 1e6
        unique &= solve(without)[4] > total + 1e-6
    return dict(g=len(gt_xy), n_det=len(det_xy), c=c, match_sum=match_sum, cost_sum=cost_sum, match=match, stable=stable, unique=bool(unique),
                at_td=int((d == TD).sum()), dist=d)


# --- the sets --------------------------------------------------------------------------------------------------------------------
def cluster_frame(rng, G, P, side=None, near=0.75):
    """Float coordinates inside the 480 x 1440 ground: ground truths in a square of 70-110 units, a detection near each of three
    quarters of the smaller side's ground truths (sigma 12), the rest anywhere in the square."""
    side = side or rng.uniform(70, 110)
    corner = np.array([rng.uniform(0, 480 - side), rng.uniform(0, 1440 - side)])
    gt = corner + rng.uniform(0, side, (G, 2))
    det = corner + rng.uniform(0, side, (P, 2))
    k = int(np.ceil(near * min(G, P)))
    det[:k] = gt[rng.permutation(G)[:k]] + rng.normal(0, 12, (k, 2))
    return gt, np.clip(det, 0, [480, 1440])[rng.permutation(P)]


def synthetic_set(rng):
    """-> list of (kind, gt_xy, det_xy), one per frame number 0, 1, ..."""
    frames = [("sized", *cluster_frame(rng, G, P)) for G, P in SIZES]
    # a wider square, a detection near half of the ground truths only: misses, false positives and pairs assigned at 1e6
    frames += [("sparse", *cluster_frame(rng, G, P, side=400.0, near=0.5)) for G, P in ((40, 45), (90, 66))]
    # every pair beyond td: ground truths in one corner of the ground, detections in the opposite one
    frames.append(("beyond", rng.uniform(0, 60, (6, 2)), np.array([420, 1380]) + rng.uniform(0, 60, (7, 2))))
    # integer coordinates with pairs at EXACTLY td (offsets (18, 24), (0, 30), (30, 0): 18^2 + 24^2 = 900) beside nearer ones
    gt = np.array([[100 + 40 * k, 200] for k in range(6)], np.float64)
    offs = np.array([[18, 24], [0, 30], [3, 4], [18, -24], [6, 8], [30, 0], [-24, 18]], np.float64)
    det = np.concatenate([gt + offs[:6], gt[2:3] + offs[6:]])
    frames.append(("at_td", gt, det))
    # duplicated detections: tied optima
    gt, det = cluster_frame(rng, 8, 8)
    frames.append(("tied", gt, np.concatenate([det, det[[1, 4, 6]]])))
    # after the last frame that has ground truth: detections only (the reference drops them)
    frames += [("trailing", np.zeros((0, 2)), rng.uniform(0, 480, (n, 2))) for n in (3, 4)]
    return frames


def as_rows(frame_ids, per_frame):
    rows = [np.column_stack([np.full(len(xy), f, np.float64), xy]) for f, xy in zip(frame_ids, per_frame)]
    return np.concatenate(rows) if rows else np.zeros((0, 3))


def reference_four(gt_rows, det_rows):
    with tempfile.TemporaryDirectory() as tmp:
        res, gtf = os.path.join(tmp, "res.txt"), os.path.join(tmp, "gt.txt")
        np.savetxt(res, det_rows, "%.17g")
        np.savetxt(gtf, gt_rows, "%.17g")
        assert np.array_equal(np.loadtxt(res, ndmin=2), det_rows) and np.array_equal(np.loadtxt(gtf, ndmin=2), gt_rows)
        return np.array(evaluateDetection_py(res, gtf, None), np.float64)


def describe(name, gt_rows, det_rows, frame_ids, tied, rng, out):
    """Records of the frames `frame_ids`, the reference's four numbers, and the totals of the frames the reference walks."""
    recs = [frame_record(gt_rows[gt_rows[:, 0] == f, 1:3], det_rows[det_rows[:, 0] == f, 1:3], rng) for f in frame_ids]
    four = reference_four(gt_rows, det_rows)
    # the reference's bookkeeping from the records: frames that have detections, up to the last one that has ground truth
    walked = [r for r in recs if r["n_det"] > 0]
    last = max(k for k, r in enumerate(walked) if r["g"] > 0)
    walked = walked[:last + 1]
    c, g, n_det = (sum(r[k] for r in walked) for k in ("c", "g", "n_det"))
    fp, m = n_det - c, g - c
    terms = [1 - r["dist"][o, e] / TD for r in walked for o, e in enumerate(r["match"]) if e >= 0]
    mine = np.array([c / g * 100, c / (fp + c) * 100, max((1 - (m + fp) / g) * 100, 0), sum(terms) / c * 100])
    assert np.allclose(mine, four, rtol=1e-12, atol=0), (name, mine, four)  # the restatement IS the reference's solve
    out.update({f"{name}_gt": gt_rows, f"{name}_det": det_rows, f"{name}_four": four, f"{name}_frame_ids": np.array(frame_ids, np.float64),
                f"{name}_totals": np.array([c, fp, m, g], np.int64),
                f"{name}_records": np.array([[r["g"], r["n_det"], r["c"], r["match_sum"]] for r in recs], np.float64),
                f"{name}_cost_sum": np.array([r["cost_sum"] for r in recs]),
                f"{name}_unique": np.array([r["unique"] for r in recs]), f"{name}_tied": np.array(tied),
                f"{name}_gt_match": np.concatenate([r["match"] for r in recs]).astype(np.int32)})
    return recs, four


def main():
    rng = np.random.default_rng(SEED)
    out = {}
    ev = os.path.join(ROOT, "vfa", "evaluation")
    for name, res, gtf, want in (("demo1", "test-demo.txt", "gt-demo.txt", (95.48319327731093, 94.09937888198758, 89.49579831932773, 83.27931600146269)),
                                 ("demo2", os.path.join("pyeval", "all_res.txt"), os.path.join("pyeval", "all_test_gt.txt"),
                                  (91.17647058823529, 92.34042553191489, 83.61344537815127, 83.650244164872))):
        det_rows, gt_rows = np.loadtxt(os.path.join(ev, res), ndmin=2)[:, :3], np.loadtxt(os.path.join(ev, gtf), ndmin=2)[:, :3]
        whole = np.array(evaluateDetection_py(os.path.join(ev, res), os.path.join(ev, gtf), None))
        frame_ids = np.unique(det_rows[:, 0]).tolist()
        gt_rows = gt_rows[np.isin(gt_rows[:, 0], frame_ids)]
        recs, four = describe(name, gt_rows, det_rows, frame_ids, [False] * len(frame_ids), rng, out)
        assert np.array_equal(four, whole) and np.allclose(four, want, rtol=1e-14, atol=0), (name, four, whole)  # the cut changes nothing
        check_demo(name, recs)
    frames = synthetic_set(rng)
    ids = list(range(len(frames)))
    recs, four = describe("syn", as_rows(ids, [f[1] for f in frames]), as_rows(ids, [f[2] for f in frames]), ids,
                          [f[0] == "tied" for f in frames], rng, out)
    check_synthetic(frames, recs, four)
    # dx^2 + dy^2 within a few ulps of 900: the neighbours of (18, 24) seen from the origin
    steps = [(k, m) for k in range(-2, 3) for m in range(-2, 3)]
    out["near_td_gt"] = np.array([[0.0, 0.0]])
    out["near_td_det"] = np.array([[18.0 + k * np.spacing(18.0), 24.0 + m * np.spacing(24.0)] for k, m in steps])
    d = out["near_td_det"] - out["near_td_gt"]
    sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    assert (np.abs(sq - 900.0) <= 16 * np.spacing(900.0)).all() and len(np.unique(sq)) >= 5 and (sq == 900.0).any()
    np.savez_compressed(os.path.join(HERE, "clear_mod.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})
    print("file size", os.path.getsize(os.path.join(HERE, "clear_mod.npz")))


# --- what the tests rely on ------------------------------------------------------------------------------------------------------
def check_demo(name, recs):
    assert all(r["stable"] for r in recs), name                         # no frame depends on the order of its rows and columns
    assert sum(r["at_td"] for r in recs) >= 2, name                     # the quirk at exactly td is live in real data
    assert max(max(r["g"], r["n_det"]) for r in recs) <= 64 and len(recs) == 40
    assert sum(r["unique"] for r in recs) >= 30, (name, sum(r["unique"] for r in recs))
    print(name, "frames", len(recs), "pairs at td", sum(r["at_td"] for r in recs), "unique tables", sum(r["unique"] for r in recs))


def check_synthetic(frames, recs, four):
    for (kind, gt, det), r in zip(frames, recs):
        d = r["dist"]
        assert r["stable"] or kind == "tied", kind                      # order independence of every frame that is not tied
        if kind in ("sized", "sparse", "tied", "beyond"):
            assert np.abs(d - TD).min(initial=np.inf) >= 1e-6, kind     # margin: no float distance near td
            assert ((gt >= 0) & (gt <= [480, 1440])).all() and ((det >= 0) & (det <= [480, 1440])).all()
        if kind == "sized":
            assert r["unique"], (kind, r["g"], r["n_det"])
            if d.size >= 60:
                assert 0.10 <= (d < TD).mean() <= 0.60, (r["g"], r["n_det"], (d < TD).mean())
            if min(r["g"], r["n_det"]) >= 12:
                assert 0 < r["c"]
        if kind == "sparse":
            assert r["unique"] and 0.25 * min(r["g"], r["n_det"]) < r["c"] < 0.8 * min(r["g"], r["n_det"])
        if kind == "beyond":
            assert r["c"] == 0 and (d > TD).all()
        if kind == "at_td":
            assert r["at_td"] >= 4 and 0 < r["c"] < r["g"] and r["stable"]
            assert r["cost_sum"] - r["match_sum"] >= TD                 # a pair at exactly td is assigned and is not a match
        if kind == "tied":
            assert not r["unique"] and r["c"] >= 4
    print("syn (g, n_det, c):", [(r["g"], r["n_det"], r["c"]) for r in recs])
    assert [(r["g"], r["n_det"]) for r in recs[:len(SIZES)]] == SIZES
    assert all(0 < v < 100 for v in four)


if __name__ == "__main__":
    main()
