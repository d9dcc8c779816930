#!/usr/bin/env python3
"""Time a training step of the ResNet trunk with its identity residual blocks on the HIP kernels (``VFANet.trunk_convs_train =
"hip"``: ``ops.residual_block_train`` -- ``vfa_trunk_conv_f32`` forward and input gradient, ``vfa_trunk_conv_wgrad_f32``,
``vfa_group_norm_stats_f32``, ``vfa_group_norm_backward_f32``) against the library path they stand beside, on one MI355X.

    python tools/bench_trunk_train.py [--repeats 5] [--calls 3] [--images 7 28]

A seeded ``VFANet`` (resnet18, 3D) in training mode on 7 and on 28 seeded images of 720 x 1280.  Per case, both settings in one
process, ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over ``--repeats`` windows
with the minimum and maximum next to it:
  * the trunk: ``VFANet.trunk`` forward + backward from a scalar loss over the three maps;
  * per stage one identity block alone on a map of the stage's shape: forward with a graph, backward (``torch.autograd.grad`` on the
    retained graph: input and all six parameters), and the two GroupNorm backwards of the block (``ops.group_norm_backward`` with
    the join's mask and with the prologue's mask / autograd of ``F.relu(F.group_norm(y))`` twice);
  * ``torch.cuda.max_memory_allocated`` of one trunk step above what was allocated before it, and per stage the bytes of the
    largest transient workspace of a block's step (the weight gradient's partials) and of its GroupNorm backward.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

IMAGE = (720, 1280)
STAGES = (("layer1", 64, 4), ("layer2", 128, 8), ("layer3", 256, 16), ("layer4", 512, 32))   # name, channels, stride of the map


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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name, fn in paths.items():
            times[name].append(window(fn, args.calls))
    out = {k: summary(v) for k, v in times.items()}
    a, b = (v["median"] for v in out.values())
    out["library_over_hip"] = round(a / b, 3)
    return out


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 2)


def make_net(dev):
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(0)
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=IMAGE), base="resnet18", mode="3D").train().to(dev)


def stage(net, name, C, stride, n, args, dev):
    """The last block of a stage (an identity block) alone on a seeded non-negative map of the stage's shape."""
    from vfa_amd import _lib, ops
    block = getattr(net.base, name)[-1]
    assert block.is_identity
    L, W = (IMAGE[0] - 1) // stride + 1, (IMAGE[1] - 1) // stride + 1
    gen = torch.Generator().manual_seed(C + n)
    x = torch.randn(n, C, L, W, generator=gen).abs().to(dev).requires_grad_()
    g = torch.randn(n, C, L, W, generator=gen).to(dev)
    params = list(block.parameters())
    forward = {"library": lambda: block(x), "hip": lambda: block.forward_train_hip(x)}
    out = {"stage": name, "map": [n, C, L, W], "forward_ms": alternate(forward, args)}
    kept = {k: fn() for k, fn in forward.items()}
    out["backward_ms"] = alternate({k: (lambda o=o: torch.autograd.grad(o, (x, *params), g, retain_graph=True)) for k, o in kept.items()}, args)
    del kept
    with torch.no_grad():
        y = ops.trunk_conv(x.detach(), block.conv1.weight)
        a, b, stats = ops.group_norm_stats(y, 16, block.bn1.weight, block.bn1.bias, block.bn1.eps)
        joined = ops.residual_join(y, (a, b), x.detach())
    yl = y.clone().requires_grad_()
    zl = F.relu(F.group_norm(yl, 16, block.bn1.weight, block.bn1.bias, block.bn1.eps))
    gn_params = (block.bn1.weight, block.bn1.bias)

    def hip_gn():
        ops.group_norm_backward(g, y, a, b, block.bn1.weight, stats, 16, mask_out=joined)
        ops.group_norm_backward(g, y, a, b, block.bn1.weight, stats, 16)

    def library_gn():
        torch.autograd.grad(zl, (yl, *gn_params), g, retain_graph=True)
        torch.autograd.grad(zl, (yl, *gn_params), g, retain_graph=True)
    out["group_norm_backward_x2_ms"] = alternate({"library": library_gn, "hip": hip_gn}, args)
    out["workspace_bytes"] = {"weight_grad_partials": ops.residual_block_workspace_bytes(n, C, L, W),
                              "group_norm_backward": int(_lib.lib().vfa_group_norm_backward_workspace_bytes(n, C))}
    return out


def measure(net, n, args, dev):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 3, *IMAGE, generator=gen).to(dev)
    coef = None

    def step(setting):
        nonlocal coef
        net.trunk_convs_train = setting
        net.zero_grad(set_to_none=True)
        maps = net.trunk(x)
        if coef is None:
            coef = [torch.randn(m.shape, generator=gen).to(dev) for m in maps]
        sum((m * c).sum() for m, c in zip(maps, coef)).backward()
    out = {"images": n}
    out["trunk_step_ms"] = alternate({"library": lambda: step("library"), "hip": lambda: step("hip")}, args)
    out["peak_mib"] = {"library": peak_mib(lambda: step("library")), "hip": peak_mib(lambda: step("hip"))}
    net.trunk_convs_train = "library"
    net.zero_grad(set_to_none=True)
    out["stages"] = [stage(net, name, C, stride, n, args, dev) for name, C, stride in STAGES]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--images", type=int, nargs="+", default=[7, 28])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trunk_train needs the MI355X"
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
