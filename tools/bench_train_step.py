#!/usr/bin/env python3
"""Forward + backward of the aggregate on one workload, both training paths: fused forward + recomputing backward
(`vfa_op.FUSED_TRAIN`, the default) and the unfused kernels with vox / lin saved by autograd.  ``--deterministic`` adds the
bit-reproducible backward (torch.use_deterministic_algorithms(True)), with torch's fill of uninitialised memory on and off.
``--geometry-grad`` adds a step with calibs and grid requiring grad (vfa_project_gather_backward_geometry_f32 per scale and chunk)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import vfa_amd  # noqa: E402
from vfa_amd import ops  # noqa: E402
from vfa_amd.synthetic import make_workload  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--workload", default="multiviewc_200x200x1")
p.add_argument("--steps", type=int, default=5)
p.add_argument("--deterministic", action="store_true", help="also time the deterministic mode (fill of torch.empty on and off)")
p.add_argument("--geometry-grad", action="store_true", help="also time a step with calibs and grid requiring grad")
a = p.parse_args()
dev = torch.device("cuda:0")
wl = make_workload(a.workload, channels=256, seed=0)
n = wl["n_cam"]
torch.manual_seed(0)
mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
lats = [torch.cat([wl["features"][c][s] for c in range(n)]).to(dev).requires_grad_(True) for s in range(3)]
calibs, grid = wl["calibs"].to(dev), wl["grid"].to(dev)


def step():
    out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid)
    out.sum().backward()


from vfa_amd import vfa_op  # noqa: E402

import torch.utils.deterministic  # noqa: E402

MODES = [("default", False, None, False)]
if a.deterministic:
    MODES += [("deterministic", True, True, False), ("deterministic, no fill", True, False, False)]
if a.geometry_grad:
    MODES += [("geometry grad", False, None, True)]
fill0 = torch.utils.deterministic.fill_uninitialized_memory
for fused in (True, False):
    for mode, det, fill, geo in MODES:
        vfa_op.FUSED_TRAIN = fused
        calibs.requires_grad_(geo)
        grid.requires_grad_(geo)
        torch.use_deterministic_algorithms(det)
        if fill is not None:
            torch.utils.deterministic.fill_uninitialized_memory = fill
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        peak = torch.cuda.max_memory_allocated() / 1e9
        with ops.KernelTimer() as kt:
            step()
            torch.cuda.synchronize()
        torch.use_deterministic_algorithms(False)
        torch.utils.deterministic.fill_uninitialized_memory = fill0
        print(f"{a.workload} {'fused forward + recomputing backward' if fused else 'unfused (vox, lin saved)'} [{mode}]: "
              f"forward+backward {dt * 1e3:.2f} ms/step, peak memory {peak:.2f} GB")
        for k, v in kt.summary().items():
            print(f"  {k}: {v['launches']} launches/step, {v['ms']:.3f} ms/step")
            if k in ("vfa_project_gather_backward_det_f32", "vfa_column_sum_f32", "vfa_project_gather_backward_geometry_f32"):
                for tag, t in v["by_tag"].items():
                    print(f"    {tag}: {t['ms'] * 1e3 / t['launches']:.0f} us per call")
