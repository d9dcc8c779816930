#!/usr/bin/env python3
"""Time a training step of the BEV heads with their four 256 -> 256 convolutions on the HIP kernels (``VFANet.head_convs_train =
"hip"``: ``ops.conv3x3_train`` -- ``vfa_conv3x3_f32`` forward and input gradient, ``vfa_conv3x3_wgrad_f32``) against the library path
they stand beside, on one MI355X.

    python tools/bench_head_train.py [--repeats 10] [--calls 10]

The head shapes 156 x 156 and 200 x 200 at B = 1 and B = 4, a seeded ``VFANet`` (resnet18, 3D) in training mode on a seeded BEV map
that requires a gradient.  Per case, both settings in one process, ALTERNATING, between HIP events: per call from windows of
``--calls`` queued calls, the median over ``--repeats`` windows with the minimum and maximum next to it:
  * the whole step: ``heads`` forward + backward from a scalar loss over all outputs;
  * one 256 -> 256 layer (dilation 1) alone, each launch sequence by itself: forward (``ops.conv3x3`` / ``F.conv2d``), input gradient
    (``ops.conv3x3_input_grad`` with its transposed pack / ``aten.convolution_backward`` for the input alone), weight and bias
    gradient (``ops.conv3x3_weight_grad``: two absmax passes, the matrix kernel, the merge, the bias sums / ``aten.convolution_backward``
    for weight and bias alone);
  * the weight gradient's fraction of its flop floor: 3 products x 2 B L W 256 256 9 flops at the dense 16-bit peak of 2.5e15 / s;
  * peak device memory of one step above what was allocated before it.
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

SHAPES = [(156, 156), (200, 200)]
PEAK_16BIT = 2.5e15


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
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").train().to(dev)


def layer(net, topdown, args):
    """One 256 -> 256 layer alone, launch sequence by launch sequence."""
    from vfa_amd import ops
    conv = net.tytx_pred[0]
    w, bias, x = conv.weight.detach(), conv.bias.detach(), topdown.detach()
    g = torch.randn(x.shape[0], 256, *x.shape[2:], generator=torch.Generator().manual_seed(2)).to(x.device)
    aten = torch.ops.aten.convolution_backward

    def backward(mask):
        return lambda: aten(g, x, w, [256], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
    with torch.no_grad():
        return {"forward_ms": alternate({"library": lambda: F.conv2d(x, w, bias, padding=1), "hip": lambda: ops.conv3x3(x, w, 1, shift=bias)}, args),
                "input_grad_ms": alternate({"library": backward([True, False, False]), "hip": lambda: ops.conv3x3_input_grad(g, w, 1)}, args),
                "weight_grad_ms": alternate({"library": backward([False, True, True]),
                                             "hip": lambda: ops.conv3x3_weight_grad(g, x, 1, want_bias=True)}, args)}


def measure(net, L, W, B, args, dev):
    gen = torch.Generator().manual_seed(L + B)
    topdown = torch.randn(B, 256, L, W, generator=gen).to(dev).requires_grad_()
    coef = {k: torch.randn(s, generator=gen).to(dev) for k, s in
            (("heatmap", (B, 1, L, W)), ("loc_offset", (B, L, W, 2)), ("dim_offset", (B, L, W, 3)), ("rotation", (B, L, W, 360)))}

    def step(setting):
        net.head_convs_train = setting
        net.zero_grad(set_to_none=True)
        topdown.grad = None
        out = net.heads(topdown)
        sum((out[k] * coef[k]).sum() for k in sorted(out)).backward()
    out = {"grid": [L, W], "B": B}
    out["step_ms"] = alternate({"library": lambda: step("library"), "hip": lambda: step("hip")}, args)
    out["peak_mib"] = {"library": peak_mib(lambda: step("library")), "hip": peak_mib(lambda: step("hip"))}
    net.head_convs_train = "library"
    net.zero_grad(set_to_none=True)
    out["layer"] = layer(net, topdown, args)
    floor_ms = 3 * 2.0 * B * L * W * 256 * 256 * 9 / PEAK_16BIT * 1e3
    out["weight_grad_floor_ms"] = round(floor_ms, 5)
    out["weight_grad_of_floor"] = round(floor_ms / out["layer"]["weight_grad_ms"]["hip"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_head_train needs the MI355X"
    dev = torch.device("cuda:0")
    net = make_net(dev)
    cases = []
    for L, W in SHAPES:
        for B in (1, 4):
            r = measure(net, L, W, B, args, dev)
            cases.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
