#!/usr/bin/env python3
"""Time a training step of the ResNet trunk's stem on the HIP kernels (``VFANet.trunk_stem_train = "hip"``: ``ops.stem_train`` --
``vfa_stem_pool_backward_f32``, ``vfa_group_norm_backward_f32`` and ``vfa_stem_conv_wgrad_f32`` behind the inference kernels) on one
MI355X, the sibling of tools/bench_trunk_proj_train.py.

    python tools/bench_stem_train.py [--repeats 5] [--calls 3] [--images 7 28]

A seeded ``VFANet`` (resnet18, 3D) in training mode on 7 and on 28 seeded images of 720 x 1280.  Per case, every setting in one
process, ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over ``--repeats`` windows
with the minimum and maximum next to it, library / hip:
  * the stem alone, forward + backward from a fixed cotangent (the gradients of ``conv1.weight``, ``bn1.weight`` and ``bn1.bias``), and
    ``torch.cuda.max_memory_allocated`` of one such step above what was allocated before it;
  * the three backward kernels alone through ``ops.KernelTimer``, each with its floor: the elementwise kernels by their bytes at
    6.29 TB/s, the weight gradient by the larger of its bytes and its multiply-adds (N padded to 160) at the 155 TF of the f32 MFMA;
  * the trunk, forward + backward from a scalar loss over the three maps, with ``trunk_convs_train = trunk_proj_train = "hip"`` and the
    stem's switch off and on, and the peak memory of a step in each setting.
The library side is the unchanged default path.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_trunk_proj_train import alternate  # noqa: E402
from bench_trunk_train import IMAGE, make_net, peak_mib  # noqa: E402

HBM_BYTES_PER_MS = 6.29e9       # 6.29 TB/s
F32_MFMA_FLOP_PER_MS = 155e9    # the rate the project measured for v_mfma_f32_32x32x2_f32
KERNELS = ("vfa_stem_pool_backward_f32", "vfa_group_norm_backward_f32", "vfa_stem_conv_wgrad_f32")


def floors(n):
    """The floor of each backward kernel in ms on n images: bytes every kernel must move, and the product's multiply-adds."""
    L, W = (IMAGE[0] - 1) // 2 + 1, (IMAGE[1] - 1) // 2 + 1
    raw, pooled, image = n * 64 * L * W * 4, n * 64 * ((L - 1) // 2 + 1) * ((W - 1) // 2 + 1) * 4, n * 3 * IMAGE[0] * IMAGE[1] * 4
    return {"vfa_stem_pool_backward_f32": (raw + pooled + raw) / HBM_BYTES_PER_MS,              # reads y and gout, writes u
            "vfa_group_norm_backward_f32": (2 * (raw + raw) + raw) / HBM_BYTES_PER_MS,          # two passes over (u, y), writes dy
            "vfa_stem_conv_wgrad_f32": max((raw + image) / HBM_BYTES_PER_MS, 2.0 * n * L * W * 64 * 160 / F32_MFMA_FLOP_PER_MS)}


def kernels(trunk, x, g, args):
    from vfa_amd import ops
    params = (trunk.conv1.weight, trunk.bn1.weight, trunk.bn1.bias)

    def step():
        torch.autograd.grad(trunk.stem_train_hip(x), params, g)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    per = {k: [] for k in KERNELS}
    for _ in range(args.repeats):
        with ops.KernelTimer(only=KERNELS) as kt:
            step()
        torch.cuda.synchronize()
        for k, v in kt.summary().items():
            per[k].append(v["ms"] / v["launches"])
    floor = floors(x.shape[0])
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "floor_ms": round(floor[k], 5),
                "over_floor": round(statistics.median(v) / floor[k], 2)} for k, v in per.items()}


def measure(net, n, args, dev):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 3, *IMAGE, generator=gen).to(dev)
    trunk = net.base
    params = (trunk.conv1.weight, trunk.bn1.weight, trunk.bn1.bias)
    with torch.no_grad():
        g = torch.randn(trunk.stem(x).shape, generator=gen).to(dev)
    stem = {"library": lambda: torch.autograd.grad(trunk.stem(x), params, g), "hip": lambda: torch.autograd.grad(trunk.stem_train_hip(x), params, g)}
    out = {"images": n, "stem_step_ms": alternate(stem, args), "stem_peak_mib": {k: peak_mib(fn) for k, fn in stem.items()}}
    out["kernels_ms"] = kernels(trunk, x, g, args)
    coef = None

    def step(setting):
        nonlocal coef
        net.trunk_convs_train = net.trunk_proj_train = "hip"
        net.trunk_stem_train = setting
        net.zero_grad(set_to_none=True)
        maps = net.trunk(x)
        if coef is None:
            coef = [torch.randn(m.shape, generator=gen).to(dev) for m in maps]
        sum((m * c).sum() for m, c in zip(maps, coef)).backward()
    settings = ("library", "hip")
    out["trunk_step_ms"] = alternate({k: (lambda k=k: step(k)) for k in settings}, args)
    out["trunk_peak_mib"] = {k: peak_mib(lambda k=k: step(k)) for k in settings}
    net.trunk_convs_train = net.trunk_proj_train = net.trunk_stem_train = "library"
    net.zero_grad(set_to_none=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--images", type=int, nargs="+", default=[7, 28])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stem_train needs the MI355X"
    dev = torch.device("cuda:0")
    net = make_net(dev)
    cases = []
    for n in args.images:
        r = measure(net, n, args, dev)
        cases.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
