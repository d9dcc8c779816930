#!/usr/bin/env python3
"""Time the CLEAR-MOD (MODA / MODP) match tables on one MI355X: one wave per frame, one launch per evaluation set.

    python tools/bench_clear_mod.py [--frames 2000] [--side 40] [--repeats 20] [--calls 50] [--sweep]

Two sets: the first 40-frame demo set of tests/golden/clear_mod.npz (what an evaluation run of the reference's scripts looks like:
at most 33 detections and 32 ground truths in a frame) and a seeded synthetic set of ``--frames`` frames of ``--side`` ground
truths and ``--side`` detections each.  For each it measures
  * the library call alone (offsets built beforehand) and ``eval_ops.match_frames_hungarian`` with ``n_frames`` given, between HIP
    events: per call from windows of ``--calls`` queued calls, medians over ``--repeats`` windows, minimum and maximum next to them;
  * ``eval_ops.clear_mod`` from host arrays to the four numbers: wall clock of the whole call, host work and copies included;
  * on this machine's host, the per-frame solve of the reference restated with scipy (distances in numpy, ``d > td -> 1e6``,
    ``scipy.optimize.linear_sum_assignment``, the matches below td): wall clock of the loop over the frames.  This is the solve of
    ``CLEAR_MOD_HUN.py:58-73`` as tests/golden/make_clear_mod.py restates it, NOT the reference's own function (whose Python loop
    over the pairs of a frame costs more); ``null`` where scipy is not installed.
Prints one JSON line.  Warm-up first."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TD = 30.0


def synthetic_set(frames, side, seed=0):
    """gt and det rows ``frame x y``: per frame `side` ground truths in a square sized so that a ground truth has a handful of
    others within td, a detection near three quarters of them (sigma 12), the rest clutter in the square."""
    rng = np.random.default_rng(seed)
    edge = 30.0 * np.sqrt(side)
    gt, det = [], []
    for f in range(frames):
        g = rng.uniform(0, edge, (side, 2))
        d = rng.uniform(0, edge, (side, 2))
        k = (3 * side) // 4
        d[:k] = g[rng.permutation(side)[:k]] + rng.normal(0, 12, (k, 2))
        gt.append(np.column_stack([np.full(side, float(f)), g]))
        det.append(np.column_stack([np.full(side, float(f)), d[rng.permutation(side)]]))
    return np.concatenate(gt), np.concatenate(det)


def timed(fn, repeats, calls=1, warmup=3):
    """Per-call milliseconds of fn() (the scheme of tools/bench_ap_aos.py): median wall clock, median HIP-event time and the
    (min, max) of the HIP-event time over `repeats` windows of `calls` queued calls, each window ended by a device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, gpu = [], []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / calls)
        gpu.append(start.elapsed_time(end) / calls)
    return statistics.median(wall), statistics.median(gpu), (round(min(gpu), 5), round(max(gpu), 5))


def host_solve(gt, det, repeats):
    """The scipy restatement over the frames that have detections -> (median wall ms, sum of c), or (None, None) without scipy."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return None, None
    frames = np.unique(det[:, 0])
    per_frame = [(gt[gt[:, 0] == f, 1:3], det[det[:, 0] == f, 1:3]) for f in frames]

    def run():
        c = 0
        for g, d in per_frame:
            dx, dy = g[:, None, 0] - d[None, :, 0], g[:, None, 1] - d[None, :, 1]
            cost = np.sqrt(dx * dx + dy * dy)
            cost[cost > TD] = 1e6
            rows, cols = linear_sum_assignment(cost)
            c += int((cost[rows, cols] < TD).sum())
        return c
    run()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        c = run()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), c


def measure(name, gt, det, args):
    from vfa_amd import _lib, eval_ops
    dev = torch.device("cuda:0")
    four = eval_ops.clear_mod(gt, det)
    c_total = eval_ops.clear_mod_totals(gt, det)[0]
    wall, _, _ = timed(lambda: eval_ops.clear_mod(gt, det), args.repeats)
    frames = np.unique(det[:, 0])
    gt = gt[np.isin(gt[:, 0], frames)]
    det_ctr, gt_ctr = np.searchsorted(frames, det[:, 0]), np.searchsorted(frames, gt[:, 0])
    do, go = np.argsort(det_ctr, kind="stable"), np.argsort(gt_ctr, kind="stable")
    n_frames = len(frames)
    det_xy, gt_xy = torch.from_numpy(det[do, 1:3].copy()).to(dev), torch.from_numpy(gt[go, 1:3].copy()).to(dev)
    det_f, gt_f = torch.from_numpy(det_ctr[do]).to(dev), torch.from_numpy(gt_ctr[go]).to(dev)
    _, wrapper, wrapper_span = timed(lambda: eval_ops.match_frames_hungarian(det_xy, det_f, gt_xy, gt_f, n_frames=n_frames, td=TD),
                                     args.repeats, args.calls)
    edges = torch.arange(n_frames + 1, device=dev)
    det_begin, gt_begin = torch.searchsorted(det_f, edges).int(), torch.searchsorted(gt_f, edges).int()
    t = eval_ops.match_frames_hungarian(det_xy, det_f, gt_xy, gt_f, n_frames=n_frames, td=TD)

    def call():
        _lib.call("vfa_clear_mod_frames_f64", _lib.ptr(det_xy), _lib.ptr(det_begin), _lib.ptr(gt_xy), _lib.ptr(gt_begin), n_frames,
                  det_xy.shape[0], gt_xy.shape[0], TD, None, 0, None, _lib.ptr(t.gt_match), _lib.ptr(t.gt_dist), _lib.ptr(t.frame_counts),
                  _lib.ptr(t.frame_cost), _lib.ptr(t.frame_status), _lib.current_stream_handle())
    _, kernel, kernel_span = timed(call, args.repeats, args.calls)

    def first_frame():  # one workgroup on an otherwise idle device: the length of one frame's dependent chain (+ the launch)
        _lib.call("vfa_clear_mod_frames_f64", _lib.ptr(det_xy), _lib.ptr(det_begin), _lib.ptr(gt_xy), _lib.ptr(gt_begin), 1,
                  det_xy.shape[0], gt_xy.shape[0], TD, None, 0, None, _lib.ptr(t.gt_match), _lib.ptr(t.gt_dist), _lib.ptr(t.frame_counts),
                  _lib.ptr(t.frame_cost), _lib.ptr(t.frame_status), _lib.current_stream_handle())
    _, one, one_span = timed(first_frame, args.repeats, args.calls)
    host_ms, host_c = host_solve(gt, det, max(3, args.repeats // 4))
    sizes = np.maximum(np.bincount(det_ctr, minlength=n_frames), np.bincount(gt_ctr, minlength=n_frames))
    return {"set": name, "frames": n_frames, "ground_truths": int(gt.shape[0]), "detections": int(det.shape[0]),
            "largest_frame_side": int(sizes.max()), "rows_solved": int(np.minimum(np.bincount(det_ctr, minlength=n_frames),
                                                                                   np.bincount(gt_ctr, minlength=n_frames)).sum()),
            "recall_precision_moda_modp": [round(float(v), 6) for v in four], "matches": int(c_total),
            "library_call_gpu_ms": round(kernel, 5), "library_call_gpu_ms_min_max": kernel_span,
            "library_call_us_per_frame": round(kernel * 1e3 / n_frames, 4),
            "first_frame_alone_gpu_ms": round(one, 5), "first_frame_alone_gpu_ms_min_max": one_span,
            "first_frame_sides": [int(np.bincount(gt_ctr, minlength=1)[0]), int(np.bincount(det_ctr, minlength=1)[0])],
            "match_frames_hungarian_gpu_ms": round(wrapper, 5), "match_frames_hungarian_gpu_ms_min_max": wrapper_span,
            "clear_mod_wall_ms": round(wall, 3),
            "host_scipy_restatement_wall_ms": None if host_ms is None else round(host_ms, 3),
            "host_scipy_matches_agree": None if host_c is None else bool(host_c == int(t.frame_counts[:, 2].sum()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--side", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window of the HIP-event measurements")
    ap.add_argument("--sweep", action="store_true", help="also 256 frames of sides 10 .. 128")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clear_mod needs the MI355X"
    d = np.load(os.path.join(REPO, "tests", "golden", "clear_mod.npz"))
    out = [measure("demo1 (40 frames)", d["demo1_gt"], d["demo1_det"], args),
           measure(f"synthetic {args.frames} x ({args.side} x {args.side})", *synthetic_set(args.frames, args.side), args)]
    if args.sweep:  # how the launch scales with the side of the frames: 256 frames, the library call and one frame alone
        for side in (10, 20, 40, 64, 80, 128):
            r = measure(f"synthetic 256 x ({side} x {side})", *synthetic_set(256, side, seed=side), args)
            out.append({k: r[k] for k in ("set", "frames", "rows_solved", "matches", "library_call_gpu_ms", "library_call_gpu_ms_min_max",
                                          "first_frame_alone_gpu_ms", "first_frame_alone_gpu_ms_min_max", "host_scipy_restatement_wall_ms")})
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "sets": out}))


if __name__ == "__main__":
    main()
