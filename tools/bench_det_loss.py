#!/usr/bin/env python3
"""Time the tail of a training step -- object lists -> targets -> loss -> gradients of the head outputs -- through the sparse target
encoder and the fused detection loss (``pack_objects`` + ``TargetEncoder.encode`` + ``detection_loss`` + backward) against the
reference's chain restated with torch operations and driven the way its trainer drives it, on one MI355X.

    python tools/bench_det_loss.py [--repeats 10] [--calls 10]

The reference leg, per frame (the reference trains at a batch of one, so B frames are B passes): the object list to a device tensor,
three per-object loops that read ``int(loc[0])`` back from the device (one host wait per object and loop) and write the dense
``mask`` / ``loc_offset`` / ``dim_offset`` / ``(1, 360, L, W)`` CSL target entry by entry, the loss as elementwise and reduction
operators over the dense maps, ``pred['rotation'][mask]`` on the dense orientation output, backward, and five ``.item()`` waits.
The new leg does all frames at once and never waits; its orientation logits are the ``(B, k, 360)`` rows ``VFANet(rotation_at=...)``
returns.  Both legs start from the same Python object lists and end with gradients on the head outputs.

Shapes: 156 x 156 with 40 objects in 3D, 120 x 360 and 160 x 250 with 40 objects in 2D, B = 1 and B = 4.  Both legs in one process,
ALTERNATING, between HIP events around windows of ``--calls`` steps (the reference leg's waits are inside its window): the median over
``--repeats`` windows with the minimum and maximum.  Per leg also the work of one step: the library's kernel launches
(``ops.KernelTimer``) and the aten operators dispatched (each at least one launch or copy).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = [("MultiviewC", 156, 156, True), ("Wildtrack", 120, 360, False), ("MultiviewX", 160, 250, False)]
OBJECTS, R, SIGMA = 40, 360, 6
MEAN = np.array([140.0, 60.0, 230.0], np.float32)


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


class _CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def work_of(fn):
    from vfa_amd import ops
    with ops.KernelTimer() as kt, _CountOps() as counter:
        fn()
    torch.cuda.synchronize()
    return {"library_launches": sum(v["launches"] for v in kt.summary().values()), "aten_operators": counter.n}


# ---- the reference's chain in this project's words -----------------------------------------------------------------------------------

def _focal(x, gt):
    p = torch.sigmoid(x).clamp(1e-5, 1 - 1e-5)
    pos = gt == 1
    neg = ~pos
    n_pos, n_neg = pos.sum(), neg.sum()
    pos_loss = torch.sum(-(((1 - p) ** 2) * torch.log(p)) * pos.float()) / n_pos
    neg_loss = torch.sum(-(((1 - gt) ** 4) * (p ** 2) * torch.log(1 - p)) * neg.float()) / n_neg
    if n_pos == 0:       # (a host wait, as in the reference)
        return neg_loss
    if n_neg == 0:
        return pos_loss
    return neg_loss + pos_loss


def reference_frame(objs, pred, gt_heatmap, world, L, W, wildtrack, three_d, table):
    dev = gt_heatmap.device
    location = torch.tensor([o.location for o in objs], dtype=torch.float32, device=dev)[:, :2]
    scaled = location / torch.tensor(world, dtype=torch.float32, device=dev).view(-1, 2) * torch.tensor([[L, W]], dtype=torch.float32, device=dev)
    mask = torch.zeros(1, L, W, device=dev)
    loc_t = torch.zeros(1, 2, L, W, device=dev)
    index = []
    for loc in scaled:
        cx, cy = int(loc[0]), int(loc[1])
        if wildtrack:
            mask[:, cx, cy] = 1.0
        else:
            mask[:, cy, cx] = 1.0
        index.append((cx, cy))
    for loc in scaled:
        cx, cy = int(loc[0]), int(loc[1])
        r, c = (cx, cy) if wildtrack else (cy, cx)
        loc_t[:, 0, r, c] = loc[0] - cx
        loc_t[:, 1, r, c] = loc[1] - cy
    mask = mask.unsqueeze(0)
    cell_mask = mask.squeeze(0).unsqueeze(-1)
    n = torch.maximum(mask.sum(), torch.ones((), device=dev))
    smooth = torch.nn.SmoothL1Loss(reduction="none")
    loss_pos = torch.sum(smooth(torch.sigmoid(pred["loc_offset"]), loc_t.permute(0, 2, 3, 1)) * cell_mask / n)
    loss_hm = _focal(pred["heatmap"], gt_heatmap[None, None])
    if not three_d:
        loss = loss_pos + loss_hm
        loss.backward()
        return loss.item(), loss_hm.item(), loss_pos.item()
    dimension = torch.tensor([o.dimension for o in objs], dtype=torch.float32, device=dev)
    rotation = torch.tensor([o.rotation for o in objs], dtype=torch.float32, device=dev)
    mean = torch.tensor(MEAN, device=dev)
    dim_t = torch.zeros(1, 3, L, W, device=dev)
    for dim, (cx, cy) in zip(dimension, index):
        off = torch.log(dim / mean)
        dim_t[:, 0, cy, cx], dim_t[:, 1, cy, cx], dim_t[:, 2, cy, cx] = off[0], off[1], off[2]
    rot_t = torch.zeros(1, L, W, R, device=dev)
    for angle, (cx, cy) in zip(rotation, index):
        label = int(torch.rad2deg(angle).item())
        rot_t[:, cy, cx, :] = torch.tensor(np.roll(table, label - R // 2))[None, :].to(dev)
    loss_hwl = torch.sum(smooth(pred["dim_offset"], dim_t.permute(0, 2, 3, 1)) * cell_mask / n)
    fg = mask.squeeze(0) == 1
    loss_ang = _focal(pred["rotation"][fg], rot_t[fg])
    loss = loss_pos + loss_hwl + loss_hm + loss_ang
    loss.backward()
    return loss.item(), loss_hm.item(), loss_pos.item(), loss_hwl.item(), loss_ang.item()


def measure(base, L, W, three_d, B, args, dev):
    import vfa_amd
    from vfa_amd.loss import label_table
    world = (4.0 * L, 4.0 * W)
    wildtrack = base == "Wildtrack"
    rng = np.random.RandomState(L + 7 * B)
    g = torch.Generator().manual_seed(L * 3 + B)
    frames = []
    for _ in range(B):
        rows, cols = rng.uniform(0, L, OBJECTS), rng.uniform(0, W, OBJECTS)
        first, second = (rows, cols) if wildtrack else (cols, rows)
        frames.append([SimpleNamespace(location=[float(4 * first[i]), float(4 * second[i]), 0.0],
                                       **(dict(dimension=[float(v) for v in MEAN * np.exp(rng.randn(3) * 0.2)],
                                               rotation=float(rng.uniform(0, 6.2))) if three_d else {})) for i in range(OBJECTS)])
    enc = vfa_amd.TargetEncoder(base, world, (4, 4, 4), dimension_mean=MEAN, angle_range=R, angle_radius=SIGMA, max_objects=64)
    enc.table(dev)
    table = label_table(R, SIGMA).numpy()
    heads = {"heatmap": torch.randn(B, 1, L, W, generator=g) * 2 - 2, "loc_offset": torch.randn(B, L, W, 2, generator=g)}
    if three_d:
        heads["dim_offset"] = torch.randn(B, L, W, 3, generator=g) * 0.3
        heads["rotation"] = torch.randn(B, L, W, R, generator=g)
    heads = {k: v.to(dev).requires_grad_(True) for k, v in heads.items()}
    with torch.no_grad():
        probe = enc.encode(*vfa_amd.pack_objects(frames, dev, max_objects=64)[:2], grid_lw=(L, W))
        gt_heatmap = torch.rand(B, L * W + 1, generator=g).to(dev) * 0.9
        gt_heatmap.scatter_(1, torch.where(probe.cells < 0, L * W, probe.cells).long(), 1.0)
        gt_heatmap = gt_heatmap[:, :L * W].reshape(B, L, W).contiguous()

    def clear():
        for v in heads.values():
            v.grad = None

    def new_leg():
        clear()
        packed = vfa_amd.pack_objects(frames, dev, max_objects=64)
        targets = enc.encode(packed.location, packed.count, packed.dimension, packed.rotation, grid_lw=(L, W))
        pred = {k: v for k, v in heads.items() if k != "rotation"}
        if three_d:     # the rows VFANet(rotation_at=targets.cells) returns, here gathered from the same dense logits
            at = targets.cells.long().clamp(min=0)
            pred["rotation_at"] = torch.gather(heads["rotation"].reshape(B, L * W, R), 1, at.unsqueeze(-1).expand(-1, -1, R)).detach().requires_grad_(True)
        out = vfa_amd.detection_loss(pred, targets, gt_heatmap)
        out["loss"].sum().backward()
        return out

    def reference_leg():
        clear()
        return [reference_frame(frames[b], {k: v[b:b + 1] for k, v in heads.items()}, gt_heatmap[b], world, L, W, wildtrack, three_d, table)
                for b in range(B)]

    got, want = new_leg()["loss"].tolist(), [r[0] for r in reference_leg()]
    assert np.allclose(got, want, rtol=1e-5), (got, want)
    out = {"base": base, "grid": [L, W], "B": B, "objects_per_frame": OBJECTS, "positives": probe.n_pos.tolist(), "loss": [round(v, 6) for v in got]}
    out["step_tail_ms"] = alternate({"reference_chain": reference_leg, "fused": new_leg}, args)
    out["step_tail_ms"]["reference_over_fused"] = round(out["step_tail_ms"]["reference_chain"]["median"] / out["step_tail_ms"]["fused"]["median"], 2)
    out["work_per_step"] = {"reference_chain": work_of(reference_leg), "fused": work_of(new_leg)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10, help="steps per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_det_loss needs the MI355X"
    dev = torch.device("cuda:0")
    cases = []
    for base, L, W, three_d in CASES:
        for B in (1, 4):
            r = measure(base, L, W, three_d, B, args, dev)
            cases.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"steps_per_window": args.calls, "windows": args.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
