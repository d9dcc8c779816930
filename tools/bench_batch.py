#!/usr/bin/env python3
"""Batched frames of a static rig (``vfa_op.pipe_frames``: one pipelined launch for B frames) against B single-frame calls
(``vfa_op.pipe_frame``), both from the lateral maps (integral images, geometry, frame kernel), on the bench frame and the shipped
configs.  Prints one table: frames/s and ms/frame of each way, the gain, and the bytes of the batched workspace (next to the
single-frame one).

    python tools/bench_batch.py [--steps K] [--warmup W] [--batches 1,2,4,8] [--configs a,b,...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import vfa_amd  # noqa: E402
from vfa_amd import ops, vfa_op  # noqa: E402
from vfa_amd.synthetic import make_workload  # noqa: E402

CONFIGS = ("multiviewc_200x200x1", "multiviewc_156x156x5", "multiviewx_160x250x8", "wildtrack_120x360x8")


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    print(f"{'config':<22} {'B':>2} {'single ms/fr':>12} {'batch ms/fr':>11} {'single fr/s':>11} {'batch fr/s':>10} {'gain':>6} "
          f"{'ws single MB':>12} {'ws batch MB':>11}")
    for name in args.configs.split(","):
        wl = make_workload(name, channels=256, seed=0)
        n = wl["n_cam"]
        torch.manual_seed(0)
        mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
        nl = mods[0].num_grid_layer
        calibs, grid = wl["calibs"].to(dev), wl["grid"].to(dev)
        L, W = grid.shape[1:3]
        one = [torch.cat([wl["features"][c][s] for c in range(n)]).to(dev) for s in range(3)]
        gen = torch.Generator().manual_seed(1)
        for B in batches:
            # B frames: the workload's maps, each frame scaled by a factor of its own (distinct data, the same statistics' spread)
            f = torch.rand(B, generator=gen) + 0.5
            lats = [torch.cat([l * float(f[b]) for b in range(B)]) for l in one]
            frames = [[l[b * n:(b + 1) * n] for l in lats] for b in range(B)]
            with torch.no_grad():
                t_single = _time(lambda: [vfa_op.pipe_frame(mods, fr, calibs, grid) for fr in frames], args.steps, args.warmup) / B
                t_batch = _time(lambda: vfa_op.pipe_frames(mods, lats, calibs, grid, B), args.steps, args.warmup) / B
            ws1 = ops.pipe_workspace_bytes(n, L, W, nl, 3) / 2 ** 20
            wsb = ops.pipe_batch_workspace_bytes(B, n, L, W, nl, 3) / 2 ** 20
            print(f"{name:<22} {B:>2} {t_single:>12.3f} {t_batch:>11.3f} {1e3 / t_single:>11.1f} {1e3 / t_batch:>10.1f} "
                  f"{t_single / t_batch:>5.2f}x {ws1:>12.1f} {wsb:>11.1f}", flush=True)
            del lats, frames
        del one, mods
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
