#!/usr/bin/env python3
"""Time the BEV decode on one MI355X: the fused call (``BEVDecoder.decode_fused``, one library call, fixed shapes, no host wait)
against the torch-op chain it stands beside (``BEVDecoder.decode_frames``: batched NMS kernel, then per frame meshgrid, sigmoids,
topk, gathers and the masked selections, each of which waits for the device).

    python tools/bench_decode.py [--repeats 20] [--calls 50] [--profile]

The shipped head shapes -- 156 x 156 with the 360-channel rotation head (MultiviewC, 3D), 120 x 360 (Wildtrack, 2D), 160 x 250
(MultiviewX, 2D) -- at B = 1 and B = 8, with seeded heads that hold about 40 and about 300 candidates per frame (top-k keeps 100).
For each case, after asserting that both paths give the same detections on the timed inputs:
  * ``decode_fused`` and ``decode_frames`` in one process, ALTERNATING, between HIP events: per call from windows of ``--calls``
    queued calls, the median over ``--repeats`` windows with the minimum and maximum next to it (``decode_frames`` waits for the
    device inside each call, so its event time holds those waits: that is what the path costs a caller);
  * wall clock per call of ``split(decode_fused(...))``, the fused path INCLUDING its one host wait, and of ``decode_frames``.
Prints one JSON line.  ``--profile``: a few calls of each path per case and nothing else, for a kernel table from
``rocprofv3 --kernel-trace --stats -- python tools/bench_decode.py --profile`` in a run of its own."""
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

THRESH = 0.4
SHAPES = [("MultiviewC", 156, 156, (3900, 3900), (25, 25, 32)), ("Wildtrack", 120, 360, (480, 1440), (4, 4, 4)),
          ("MultiviewX", 160, 250, (640, 1000), (4, 4, 8))]


def seeded_heads(base, B, L, W, candidates, seed, dev):
    """Heads in the layout ``VFANet`` returns (NCHW storage, ``permute(0, 2, 3, 1)`` views): a heat map far below the threshold with
    `candidates` peaks per frame on cells at least three apart (each its own 5 x 5 maximum), logits 0 .. 4, all distinct."""
    rng = np.random.default_rng(seed)
    heat = rng.uniform(-8.0, -4.0, (B, 1, L, W)).astype(np.float32)
    for b in range(B):
        cells = [(l, w) for l in range(1, L, 3) for w in range(1, W, 3)]
        pick = rng.permutation(len(cells))[:candidates]
        logits = rng.permutation(np.linspace(0.0, 4.0, candidates, dtype=np.float32))
        for p, v in zip(pick, logits):
            heat[(b, 0) + cells[p]] = v
    g = torch.Generator().manual_seed(seed)
    pred = {"heatmap": torch.from_numpy(heat).to(dev), "loc_offset": torch.randn(B, 2, L, W, generator=g).to(dev).permute(0, 2, 3, 1)}
    if base == "MultiviewC":
        pred["dim_offset"] = (torch.randn(B, 3, L, W, generator=g) * 0.3).to(dev).permute(0, 2, 3, 1)
        pred["rotation"] = torch.randn(B, 360, L, W, generator=g).to(dev).permute(0, 2, 3, 1)
    return pred


def same_detections(fused_frames, eager_frames):
    for f, e in zip(fused_frames, eager_frames):
        assert sorted(f) == sorted(e) and f["conf"].shape == e["conf"].shape, (sorted(f), f["conf"].shape, e["conf"].shape)
        of, oe = torch.argsort(f["conf"], descending=True), torch.argsort(e["conf"], descending=True)   # (distinct confidences)
        assert torch.equal(f["conf"][of], e["conf"][oe]), "confidences differ"
        for k in f:
            torch.testing.assert_close(f[k][of], e[k][oe], rtol=1e-5, atol=1e-5, msg=k)
    return sum(len(f["conf"]) for f in fused_frames)


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls, (time.perf_counter() - t0) * 1e3 / calls


def summary(values):
    return {"median": round(statistics.median(values), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def measure(base, L, W, world, cube, B, candidates, args, dev):
    from vfa_amd import eval_ops
    dec = eval_ops.BEVDecoder(base, world, cube, dimension_mean=np.array([140, 60, 230], np.float32), topk=100)
    pred = seeded_heads(base, B, L, W, candidates, seed=L + B + candidates, dev=dev)
    detections = same_detections(dec.split(dec.decode_fused(pred, THRESH)), dec.decode_frames(pred, THRESH))
    paths = {"decode_fused": lambda: dec.decode_fused(pred, THRESH), "split_decode_fused": lambda: dec.split(dec.decode_fused(pred, THRESH)),
             "decode_frames": lambda: dec.decode_frames(pred, THRESH)}
    if args.profile:
        for fn in paths.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return None
    for fn in paths.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    gpu, wall = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(args.repeats):
        for name, fn in paths.items():   # alternating: one window of each path per round
            g, w = window(fn, args.calls)
            gpu[name].append(g)
            wall[name].append(w)
    return {"base": base, "grid": [L, W], "B": B, "candidates_per_frame": candidates, "detections": detections,
            "decode_fused_gpu_ms": summary(gpu["decode_fused"]), "decode_frames_gpu_ms": summary(gpu["decode_frames"]),
            "split_decode_fused_wall_ms": summary(wall["split_decode_fused"]), "decode_frames_wall_ms": summary(wall["decode_frames"]),
            "decode_fused_window_wall_ms": summary(wall["decode_fused"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--profile", action="store_true", help="a few calls of each path per case, no timing (for rocprofv3)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode needs the MI355X"
    dev = torch.device("cuda:0")
    cases = []
    for base, L, W, world, cube in SHAPES:
        for B in (1, 8):
            for candidates in (40, 300):
                r = measure(base, L, W, world, cube, B, candidates, args, dev)
                if r is not None:
                    cases.append(r)
                    print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "cls_thresh": THRESH, "topk": 100, "cases": cases}))


if __name__ == "__main__":
    main()
