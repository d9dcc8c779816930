#!/usr/bin/env python3
"""Time the BEV heads with their dense 3x3 convolutions on the HIP kernels (``VFANet.head_convs = "hip"``: ``vfa_conv3x3_f32``,
``vfa_conv3x3_few_f32``, ``vfa_group_norm_affine_f32``) against the library path they stand beside, on one MI355X.

    python tools/bench_heads.py [--repeats 10] [--calls 20] [--profile]

The head shapes 156 x 156 and 200 x 200 at B = 1 and B = 4, a seeded ``VFANet`` (resnet18) in eval mode with perturbed BatchNorm
statistics on a seeded BEV map.  Per case, both settings in one process, ALTERNATING, between HIP events: per call from windows of
``--calls`` queued calls, the median over ``--repeats`` windows with the minimum and maximum next to it:
  * 3D: ``heads(rotation_at="detections")`` + ``decode_fused``; 2D: ``heads`` alone;
  * each of the four dense layers alone -- ``ops.conv3x3`` with its epilogue against ``F.conv2d`` (+ the eval-mode BatchNorm and ReLU
    behind it for the two ``fuse`` layers: what the kernel's epilogue replaces);
  * the (N) figures of both settings against the float64 modules on the CPU (B = 1 cases only: the float64 heads take seconds);
  * peak device memory of one call above what was allocated before it.
Prints one JSON line.  ``--profile``: no timing -- ten calls of the hip setting per shape, for a ``rocprofv3 --kernel-trace --stats``
run of its own, which gives the kernels' own times."""
import argparse
import copy
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(156, 156), (200, 200)]
POSITIVES = 40


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


def make_net(mode, dev):
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(0)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode=mode).eval()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for bn in (net.fuse[1], net.fuse[4]):
            bn.running_mean.copy_(torch.randn(256, generator=gen) * 0.2)
            bn.running_var.copy_(torch.rand(256, generator=gen) * 1.5 + 0.25)
    return net.to(dev)


def normwise(net, topdown):
    """(N): both settings against the float64 modules on the CPU, with the float32 modules on the CPU as the yardstick."""
    with torch.no_grad():
        cpu = copy.deepcopy(net).cpu()
        want64 = copy.deepcopy(cpu).double().heads(topdown.double().cpu())
        yard = cpu.heads(topdown.cpu())
        got = {s: net.heads(topdown, convs=s) for s in ("library", "hip")}

    def err(y, k):
        return float((y[k].double().cpu() - want64[k]).norm() / want64[k].norm())
    return {k: {"cpu_float32": err(yard, k), "library": err(got["library"], k), "hip": err(got["hip"], k),
                "hip_over_cpu_float32": round(err(got["hip"], k) / err(yard, k), 2)} for k in want64}


def layers(net, topdown, args):
    from vfa_amd import ops
    out = {}
    with torch.no_grad():
        fused0 = net.fuse[2](net.fuse[1](net.fuse[0](topdown)))
        for name, conv, bn, x in (("fuse0", net.fuse[0], net.fuse[1], topdown), ("fuse3", net.fuse[3], net.fuse[4], fused0),
                                  ("tytx0", net.tytx_pred[0], None, topdown), ("thtwtl0", net.thtwtl_pred[0], None, topdown)):
            d = conv.dilation[0]
            if bn is None:
                scale, shift, relu = None, conv.bias, False

                def library(conv=conv, x=x):
                    with torch.no_grad():
                        return conv(x)
            else:
                scale, shift = ops.bn_fold(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, conv.bias)
                relu = True

                def library(conv=conv, bn=bn, x=x):
                    with torch.no_grad():
                        return F.relu(bn(conv(x)))

            def hip(conv=conv, x=x, d=d, scale=scale, shift=shift, relu=relu):
                with torch.no_grad():
                    return ops.conv3x3(x, conv.weight, d, scale=scale, shift=shift, relu=relu)
            out[name] = alternate({"library": library, "hip": hip}, args)
    return out


def measure(nets, L, W, B, args, dev):
    from vfa_amd import eval_ops
    dec = eval_ops.BEVDecoder("MultiviewC", (L * 25, W * 25), (25, 25, 32), dimension_mean=np.array([140, 60, 230], np.float32), topk=100)
    topdown = torch.randn(B, 256, L, W, generator=torch.Generator().manual_seed(L + B)).to(dev)
    net3, net2 = nets["3D"], nets["2D"]
    with torch.no_grad():
        conf = eval_ops.bev_nms_batch(net3.heads(topdown, rotation_at="detections")["heatmap"]).reshape(B, -1)
        thresh = float(conf.topk(POSITIVES + 1, dim=1).values[:, -1].max())

    def infer3(setting):
        with torch.no_grad():
            return dec.decode_fused(net3.heads(topdown, rotation_at="detections", convs=setting), thresh)

    def infer2(setting):
        with torch.no_grad():
            return net2.heads(topdown, convs=setting)
    if args.profile:
        for _ in range(10):
            infer3("hip")
        torch.cuda.synchronize()
        return {"grid": [L, W], "B": B, "profiled_calls": 10}
    out = {"grid": [L, W], "B": B}
    out["heads_decode_3d_ms"] = alternate({"library": lambda: infer3("library"), "hip": lambda: infer3("hip")}, args)
    out["heads_2d_ms"] = alternate({"library": lambda: infer2("library"), "hip": lambda: infer2("hip")}, args)
    out["layer_ms"] = layers(net3, topdown, args)
    out["peak_mib"] = {"3d_library": peak_mib(lambda: infer3("library")), "3d_hip": peak_mib(lambda: infer3("hip")),
                       "2d_library": peak_mib(lambda: infer2("library")), "2d_hip": peak_mib(lambda: infer2("hip"))}
    if B == 1:
        out["normwise"] = normwise(net3, topdown)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--profile", action="store_true", help="ten calls of the hip setting per case and no timing (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heads needs the MI355X"
    dev = torch.device("cuda:0")
    nets = {mode: make_net(mode, dev) for mode in ("3D", "2D")}
    cases = []
    for L, W in SHAPES:
        for B in (1, 4):
            r = measure(nets, L, W, B, args, dev)
            cases.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
