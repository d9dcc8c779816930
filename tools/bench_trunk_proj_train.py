#!/usr/bin/env python3
"""Time a training step of the ResNet trunk with its projection blocks on the HIP kernels too (``VFANet.trunk_proj_train = "hip"``:
``ops.projection_block_train`` -- the kernels of ``ops.residual_block_train`` and the two gradients of a stride-2 convolution,
``vfa_trunk_down_wgrad_f32`` and ``vfa_trunk_down_dgrad_f32``) on one MI355X, the sibling of tools/bench_trunk_train.py.

    python tools/bench_trunk_proj_train.py [--repeats 5] [--calls 3] [--images 7 28]

A seeded ``VFANet`` (resnet18, 3D) in training mode on 7 and on 28 seeded images of 720 x 1280.  Per case, every setting in one
process, ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over ``--repeats`` windows
with the minimum and maximum next to it:
  * the trunk, three settings -- ``library``, ``convs`` (``trunk_convs_train = "hip"`` alone) and ``both`` switches: ``VFANet.trunk``
    forward + backward from a scalar loss over the three maps, and ``torch.cuda.max_memory_allocated`` of one step above what was
    allocated before it;
  * each projection block alone on a map of its input's shape, ``library`` and ``hip``: forward with a graph, backward
    (``torch.autograd.grad`` on the retained graph: input and all nine parameters), and the peak memory of one forward + backward;
  * the new kernels on the block's shapes against autograd of ``F.conv2d(..., stride=2)``: the weight gradient 3 x 3 and 1 x 1, the
    input gradient 3 x 3, and the projection's term added to it;
  * ``ops.group_norm_backward`` on the projection's map with the join's mask (which writes dz) and with the prologue's mask (which
    does not): the difference is the most an entry point without the second dz could save.
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_trunk_train import IMAGE, make_net, peak_mib, summary, window  # noqa: E402

BLOCKS = (("layer2", 64, 128, 4), ("layer3", 128, 256, 8), ("layer4", 256, 512, 16))   # name, C, O, stride of the input map


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
    first = next(iter(out.values()))["median"]
    out["first_over"] = {k: round(first / v["median"], 3) for k, v in out.items() if k != next(iter(paths))}
    return out


def block(net, name, C, O, stride, n, args, dev):
    """The first block of a stage (a projection block) alone on a seeded non-negative map of its input's shape."""
    from vfa_amd import ops
    blk = getattr(net.base, name)[0]
    assert blk.is_projection
    L, W = (IMAGE[0] - 1) // stride + 1, (IMAGE[1] - 1) // stride + 1
    Lo, Wo = (L - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = torch.Generator().manual_seed(C + n)
    x = torch.randn(n, C, L, W, generator=gen).abs().to(dev).requires_grad_()
    g = torch.randn(n, O, Lo, Wo, generator=gen).to(dev)
    params = list(blk.parameters())
    forward = {"library": lambda: blk(x), "hip": lambda: blk.forward_train_hip(x)}
    out = {"block": name + ".0", "map": [n, C, L, W], "forward_ms": alternate(forward, args)}
    kept = {k: fn() for k, fn in forward.items()}
    out["backward_ms"] = alternate({k: (lambda o=o: torch.autograd.grad(o, (x, *params), g, retain_graph=True)) for k, o in kept.items()}, args)
    del kept
    out["peak_mib"] = {k: peak_mib(lambda fn=fn: torch.autograd.grad(fn(), (x, *params), g)) for k, fn in forward.items()}
    w1, wd = blk.conv1.weight, blk.downsample[0].weight
    xd = x.detach()
    y1 = F.conv2d(x, w1, stride=2, padding=1)
    yd = F.conv2d(x, wd, stride=2)
    base = torch.zeros_like(xd)
    out["weight_grad_3x3_ms"] = alternate({"library": lambda: torch.autograd.grad(y1, w1, g, retain_graph=True),
                                           "hip": lambda: ops.trunk_down_weight_grad(g, xd, 3)}, args)
    out["weight_grad_1x1_ms"] = alternate({"library": lambda: torch.autograd.grad(yd, wd, g, retain_graph=True),
                                           "hip": lambda: ops.trunk_down_weight_grad(g, xd, 1)}, args)
    out["input_grad_3x3_ms"] = alternate({"library": lambda: torch.autograd.grad(y1, x, g, retain_graph=True),
                                          "hip": lambda: ops.trunk_down_input_grad(g, w1, (L, W))}, args)
    out["input_grad_1x1_added_ms"] = alternate({"library": lambda: base.add_(torch.autograd.grad(yd, x, g, retain_graph=True)[0]),
                                                "hip": lambda: ops.trunk_down_input_grad(g, wd, (L, W), add_to=base)}, args)
    del y1
    with torch.no_grad():
        ydd = yd.detach()
        a, b, stats = ops.group_norm_stats(ydd, 16, blk.bn2.weight, blk.bn2.bias, blk.bn2.eps)
        joined = ops.residual_join(ydd, (a, b), g)
    out["group_norm_backward_ms"] = alternate({"join_mask_writes_dz": lambda: ops.group_norm_backward(g, ydd, a, b, blk.bn2.weight, stats, 16, mask_out=joined),
                                               "prologue_mask_no_dz": lambda: ops.group_norm_backward(g, ydd, a, b, blk.bn2.weight, stats, 16)}, args)
    return out


def measure(net, n, args, dev):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 3, *IMAGE, generator=gen).to(dev)
    coef = None
    settings = {"library": ("library", "library"), "convs": ("hip", "library"), "both": ("hip", "hip")}

    def step(setting):
        nonlocal coef
        net.trunk_convs_train, net.trunk_proj_train = settings[setting]
        net.zero_grad(set_to_none=True)
        maps = net.trunk(x)
        if coef is None:
            coef = [torch.randn(m.shape, generator=gen).to(dev) for m in maps]
        sum((m * c).sum() for m, c in zip(maps, coef)).backward()
    out = {"images": n}
    out["trunk_step_ms"] = alternate({k: (lambda k=k: step(k)) for k in settings}, args)
    out["peak_mib"] = {k: peak_mib(lambda k=k: step(k)) for k in settings}
    net.trunk_convs_train = net.trunk_proj_train = "library"
    net.zero_grad(set_to_none=True)
    out["blocks"] = [block(net, name, C, O, stride, n, args, dev) for name, C, O, stride in BLOCKS]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--images", type=int, nargs="+", default=[7, 28])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trunk_proj_train needs the MI355X"
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
