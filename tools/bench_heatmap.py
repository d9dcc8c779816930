#!/usr/bin/env python3
"""Time the render of the dense heat-map target from the packed object tensors (``TargetEncoder.heatmap`` on ``vfa_heat_rgk_f32`` /
``vfa_heat_gk_f32``) on one MI355X against what it replaces: (a) the copy of the precomputed ``(B, L, W)`` map from pinned host
memory to the device, which is what a dataset-side cache costs per step, and (b) the numpy restatement of the reference's rules
(tests/heatmap_common.py) on the host, which is what computing the map costs where there is no cache (the reference's own Python
loops are slower still).

    python tools/bench_heatmap.py [--repeats 10] [--calls 20]

Shapes: RGK on 156 x 156 (MultiviewC), GK on 120 x 360 (Wildtrack) and 160 x 250 (MultiviewX), 40 objects per frame, B = 1 and B = 4.
The two device legs in one process, ALTERNATING, between HIP events around windows of ``--calls`` calls: the median over
``--repeats`` windows with the minimum and maximum.  The host leg is wall-clock time of one call, the median of three.  Prints one
JSON line."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

CASES = [("MultiviewC", 156, 156, "RGK"), ("Wildtrack", 120, 360, "GK"), ("MultiviewX", 160, 250, "GK")]
OBJECTS, K = 40, 64
MEAN = np.array([140.0, 60.0, 230.0], np.float32)  # (h, w, l)


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def summary(values):
    return {"median": round(statistics.median(values), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def alternate(paths, args):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name, fn in paths.items():
            times[name].append(window(fn, args.calls))
    return {k: summary(v) for k, v in times.items()}


def measure(base, L, W, kind, B, args, dev):
    import heatmap_common as hc
    import vfa_amd
    world = (4.0 * L, 4.0 * W)
    wildtrack = base == "Wildtrack"
    rng = np.random.RandomState(L + 7 * B)
    location, dimension = np.zeros((B, K, 3), np.float32), np.ones((B, K, 3), np.float32)
    degrees, count = np.zeros((B, K), np.float64), np.full(B, OBJECTS, np.int32)
    for b in range(B):
        rows, cols = rng.uniform(0, L, OBJECTS), rng.uniform(0, W, OBJECTS)
        first, second = (rows, cols) if wildtrack else (cols, rows)     # (MultiviewC / MultiviewX: the column is x / world0 * L)
        location[b, :OBJECTS, 0], location[b, :OBJECTS, 1] = 4 * first, 4 * second
        dimension[b, :OBJECTS] = MEAN * np.exp(rng.randn(OBJECTS, 3) * 0.2)
        degrees[b, :OBJECTS] = rng.uniform(-180, 180, OBJECTS)
    enc = vfa_amd.TargetEncoder(base, world, (4, 4, 4), dimension_mean=MEAN, max_objects=K)
    enc.gk_table(dev)
    t = [torch.from_numpy(v).to(dev) for v in (location, count, dimension, degrees)]

    def render():
        return enc.heatmap(t[0], t[1], dimension=t[2], rotation_deg=t[3], heatmap_type=kind, grid_lw=(L, W))

    def host():
        code = hc.WILDTRACK if wildtrack else 0
        if kind == "RGK":
            return np.stack([hc.rgk_map(location[b, :OBJECTS], dimension[b, :OBJECTS], degrees[b, :OBJECTS], world, (L, W), code)[0] for b in range(B)])
        return np.stack([hc.gk_map(location[b, :OBJECTS], world, (L, W), code) for b in range(B)])

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    got = render().cpu().numpy()
    assert np.array_equal(got == 1, want == 1) and float(np.abs(got.astype(np.float64) - want).max()) < 1e-6
    pinned, on_device = torch.from_numpy(want).pin_memory(), torch.empty((B, L, W), dtype=torch.float32, device=dev)

    def copy():
        on_device.copy_(pinned, non_blocking=True)

    out = {"base": base, "grid": [L, W], "type": kind, "B": B, "objects_per_frame": OBJECTS, "cells_equal_to_one": int((got == 1).sum())}
    out["ms"] = alternate({"pinned_copy": copy, "render": render}, args)
    out["ms"]["host_restatement"] = summary(host_ms)
    out["ms"]["render_over_copy"] = round(out["ms"]["render"]["median"] / out["ms"]["pinned_copy"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heatmap needs the MI355X"
    dev = torch.device("cuda:0")
    cases = []
    for base, L, W, kind in CASES:
        for B in (1, 4):
            r = measure(base, L, W, kind, B, args, dev)
            cases.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
