#!/usr/bin/env python3
"""Max-over-cameras fusion against the sum: per workload, the inference frame and one training step (forward +
backward of ``ortho.sum()``) with ``view_reduce="sum"`` and ``"max"``, and the workaround a user has without the keyword -- the
reference's camera loop (vfanet.py:64-82) through the port's ``VFA.forward`` with ``torch.maximum`` where line 82 adds.
Prints one line per measurement and a JSON summary."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import vfa_amd  # noqa: E402
from vfa_amd import lazy  # noqa: E402
from vfa_amd.synthetic import make_workload  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--workloads", default="multiviewc_200x200x1,multiviewc_156x156x5")
p.add_argument("--steps", type=int, default=10)
p.add_argument("--warmup", type=int, default=3)
a = p.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.steps * 1e3


results = {}
for name in a.workloads.split(","):
    wl = make_workload(name, channels=256, seed=0)
    n = wl["n_cam"]
    torch.manual_seed(0)
    mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
    lats = [torch.cat([wl["features"][c][s] for c in range(n)]).to(dev) for s in range(3)]
    lats_g = [l.clone().requires_grad_(True) for l in lats]
    calibs, grid = wl["calibs"].to(dev), wl["grid"].to(dev)

    def infer(mode):
        with torch.no_grad():
            vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce=mode)

    def train(mode):
        vfa_amd.aggregate_views(*mods, *lats_g, calibs, grid, view_reduce=mode).sum().backward()

    def loop_infer():
        with torch.no_grad():
            ortho = None
            for cam in range(n):
                f = [lazy.materialize(m(l[cam:cam + 1], calibs[cam], grid)) for m, l in zip(mods, lats)]
                t = (f[0] + f[1]) + f[2]
                ortho = t if ortho is None else torch.maximum(ortho, t)

    def loop_train():
        ortho = None
        for cam in range(n):
            f = [m(l[cam:cam + 1], calibs[cam], grid) for m, l in zip(mods, lats_g)]
            t = (f[0] + f[1]) + f[2]
            ortho = t if ortho is None else torch.maximum(ortho, t)
        ortho.sum().backward()

    row = {}
    for key, fn in (("infer_sum", lambda: infer("sum")), ("infer_max", lambda: infer("max")), ("infer_loop_max", loop_infer),
                    ("train_sum", lambda: train("sum")), ("train_max", lambda: train("max")), ("train_loop_max", loop_train)):
        torch.cuda.reset_peak_memory_stats()
        row[key] = round(timed(fn), 3)
        row[key + "_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
        print(f"{name} {key}: {row[key]:.3f} ms/frame (peak {row[key + '_peak_gb']:.2f} GB)", flush=True)
    results[name] = row
print(json.dumps(results))
