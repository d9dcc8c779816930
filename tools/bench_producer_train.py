"""Training cost of the producer: (producer + fused frame node) forward + backward with loss = (ortho * probe).sum(), from synthetic
trunk outputs, the HIP producer (``vfa_op._LateralIntegrals``) and the library producer (MIOpen conv + torch GroupNorm + ReLU, then
the frame node on the NCHW lateral maps) alternating in one process.  Device events, warmed shapes, windows of >= 100 ms; peak memory.

    python tools/bench_producer_train.py [--workloads bench,multiviewc_156x156x5,wildtrack_120x360x8] [--window-ms 100]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import vfa_amd  # noqa: E402
from vfa_amd import vfa_op  # noqa: E402
from vfa_amd.synthetic import make_workload  # noqa: E402

WORKLOADS = {"bench": ("multiviewc_200x200x1", 7), "multiviewc_156x156x5": ("multiviewc_156x156x5", 7),
             "wildtrack_120x360x8": ("wildtrack_120x360x8", 7)}


def setup(name, dev):
    wl_name, n_cam = WORKLOADS[name]
    wl = make_workload(wl_name, channels=256, seed=1, n_cam=n_cam)
    torch.manual_seed(0)
    mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
    hw = [tuple(wl["features"][0][s].shape[-2:]) for s in range(3)]
    feats = [torch.relu(torch.randn(n_cam, K, h, w, device=dev)).requires_grad_(True) for K, (h, w) in zip((128, 256, 512), hw)]
    convs = [nn.Conv2d(K, 256, 1).to(dev) for K in (128, 256, 512)]
    norms = [nn.GroupNorm(16, 256).to(dev) for _ in range(3)]
    calibs, grid = wl["calibs"].to(dev), wl["grid"].to(dev)
    probe = torch.randn(1, 256, grid.shape[1], grid.shape[2], device=dev)
    return mods, feats, convs, norms, calibs, grid, probe, hw


def step(kind, mods, feats, convs, norms, calibs, grid, probe):
    if kind == "hip":
        integrals = vfa_op.lateral_integrals_train(feats, convs, norms)
        ortho = vfa_amd.aggregate_views(*mods, None, None, None, calibs, grid, integrals=integrals)
    else:
        lats = [F.relu(g(c(f))) for f, c, g in zip(feats, convs, norms)]
        ortho = vfa_amd.aggregate_views(*mods, *lats, calibs, grid)
    (ortho * probe).sum().backward()


def timed(kind, args, window_ms):
    n, ms = 1, 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step(kind, *args)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window_ms:
            return ms / n
        n = max(n * 2, int(n * window_ms / max(ms, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bench,multiviewc_156x156x5,wildtrack_120x360x8")
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.workloads.split(","):
        mods, feats, convs, norms, calibs, grid, probe, hw = setup(name, dev)
        args = (mods, feats, convs, norms, calibs, grid, probe)
        res = {"hip": [], "library": []}
        peak = {}
        for kind in res:  # warm the shapes, then the peak of one step
            step(kind, *args)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            step(kind, *args)
            torch.cuda.synchronize()
            peak[kind] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        for _ in range(a.rounds):  # alternating windows
            for kind in res:
                res[kind].append(timed(kind, args, a.window_ms))
        out = {"workload": name, "cameras": feats[0].shape[0], "maps": hw,
               **{f"{k}_ms": round(min(v), 3) for k, v in res.items()}, **{f"{k}_ms_all": [round(x, 3) for x in v] for k, v in res.items()},
               **{f"{k}_peak_mib": round(v, 1) for k, v in peak.items()}}
        out["speedup"] = round(out["library_ms"] / out["hip_ms"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
