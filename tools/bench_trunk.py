#!/usr/bin/env python3
"""Time the residual stages of the ResNet trunk on the HIP kernels (``VFANet.trunk_convs = "hip"``: ``vfa_trunk_conv_f32``,
``vfa_residual_join_f32``, ``vfa_group_norm_affine_f32``) against the library path they stand beside, on one MI355X.

    python tools/bench_trunk.py [--repeats 7] [--calls 5] [--base resnet18] [--profile]

A seeded ``VFANet`` in eval mode on seeded 7 x 3 x 720 x 1280 images (one frame of seven cameras) and on 28 images (B = 4 frames).
Both settings in one process, ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over
``--repeats`` windows with the minimum and maximum next to it:
  * the whole trunk (``VFANet.trunk``: the stem is the library's in both settings), and the stem alone;
  * each stage ``layer1`` .. ``layer4`` alone on the library trunk's own input of that stage, with the stage's multiply-adds and
    the flop floor at the 16-bit matrix peak -- three 16-bit products per multiply-add in the hip setting, one as the plain floor;
  * 7 images only: ``VFANet.detect`` end to end with ``trunk_convs`` / ``head_convs`` on "library" / "hip" in the four combinations;
  * the (N) figure of the hip trunk against the library trunk on the device (normwise difference of f8 / f16 / f32).
Prints one JSON line.  ``--profile``: no timing -- three calls of the hip trunk per case, for a ``rocprofv3 --kernel-trace --stats``
run of its own, which gives the kernels' own times."""
import argparse
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

PEAK_F16_TFLOPS = 2500.0    # MI355X, dense 16-bit matrix peak (about 2.5 PFLOP/s, specification): the floor's denominator


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


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
    if "library" in out and "hip" in out:
        out["library_over_hip"] = round(out["library"]["median"] / out["hip"]["median"], 3)
    return out


def stage_macs(layer, x):
    """Multiply-adds of one stage on the input x, from the shapes."""
    def macs(conv, L, W):
        """-> (multiply-adds of conv on an (L, W) map, its output size)"""
        s = conv.stride[0]
        Lo, Wo = (L - 1) // s + 1, (W - 1) // s + 1
        return B * conv.out_channels * conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1] * Lo * Wo, (Lo, Wo)
    total, (B, _, L, W) = 0, x.shape
    for block in layer:
        first, (Lo, Wo) = macs(block.conv1, L, W)                    # conv1 and the projection read the block's input ...
        total += first + macs(block.conv2, Lo, Wo)[0]                # ... conv2 reads conv1's output
        if block.downsample is not None:
            total += macs(block.downsample[0], L, W)[0]
        L, W = Lo, Wo
    return total


def measure(net, images, args, detect=None):
    n = images.shape[0]
    out = {"images": n}
    with torch.no_grad():
        x = net.normalized(images)
        stem = F.max_pool2d(F.relu(net.base.bn1(net.base.conv1(x))), 3, stride=2, padding=1)

    def trunk(setting):
        net.trunk_convs = setting
        with torch.no_grad():
            return net.trunk(x)
    if args.profile:
        for _ in range(3):
            trunk("hip")
        torch.cuda.synchronize()
        net.trunk_convs = "library"
        return {"images": n, "profiled_calls": 3}
    got, want = trunk("hip"), trunk("library")
    out["hip_against_library_normwise"] = {k: float((a.double() - b.double()).norm() / b.double().norm()) for k, a, b in zip(("f8", "f16", "f32"), got, want)}
    del got, want
    out["trunk_ms"] = alternate({"library": lambda: trunk("library"), "hip": lambda: trunk("hip")}, args)

    def stem_only():
        with torch.no_grad():
            return F.max_pool2d(F.relu(net.base.bn1(net.base.conv1(x)), inplace=True), 3, stride=2, padding=1)
    out["stem_ms"] = alternate({"library": stem_only}, args)["library"]
    stages, inp = {}, stem
    for i in (1, 2, 3, 4):
        layer = getattr(net.base, f"layer{i}")

        def library(layer=layer, inp=inp):
            with torch.no_grad():
                return layer(inp)

        def hip(layer=layer, inp=inp):
            with torch.no_grad():
                y = inp
                for block in layer:
                    y = block.forward_hip(y)
                return y
        r = alternate({"library": library, "hip": hip}, args)
        macs = stage_macs(layer, inp)
        r["input"] = list(inp.shape)
        r["gmacs"] = round(macs / 1e9, 2)
        r["floor_ms_one_product"] = round(2 * macs / (PEAK_F16_TFLOPS * 1e12) * 1e3, 4)
        r["floor_ms_three_products"] = round(6 * macs / (PEAK_F16_TFLOPS * 1e12) * 1e3, 4)
        stages[f"layer{i}"] = r
        inp = library()
    out["stage_ms"] = stages
    if detect is not None:
        calibs, grid, dec = detect
        paths = {}
        for t in ("library", "hip"):
            for h in ("library", "hip"):
                def run(t=t, h=h):
                    net.trunk_convs, net.head_convs = t, h
                    return net.detect(images, calibs, grid, dec, 0.5)
                paths[f"trunk_{t}_heads_{h}"] = run
        out["detect_ms"] = alternate(paths, args)
    net.trunk_convs = net.head_convs = "library"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--base", default="resnet18")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4], help="frames of seven cameras per case")
    ap.add_argument("--profile", action="store_true", help="three calls of the hip trunk per case and no timing (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trunk needs the MI355X"
    dev = torch.device("cuda:0")
    from vfa_amd import eval_ops
    from vfa_amd.synthetic import make_workload
    from vfa_amd.vfanet import VFANet
    wl = make_workload("multiviewc_200x200x1", channels=256, seed=0, device=dev, cameras=())     # (calibrations and grid; no feature maps)
    torch.manual_seed(0)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base=args.base, grid_height=wl["grid_height"],
                 cube_size=wl["cube_size"], angle_range=360).to(dev).eval()
    dec = eval_ops.BEVDecoder("MultiviewC", (3750, 3750), tuple(wl["cube_size"]), dimension_mean=np.array([140, 60, 230], np.float32), topk=100)
    cases = []
    for frames in args.frames:
        images = torch.rand(7 * frames, 3, 720, 1280, generator=torch.Generator().manual_seed(frames)).to(dev)
        r = measure(net, images, args, detect=(wl["calibs"], wl["grid"], dec) if frames == 1 else None)
        cases.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del images
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "base": args.base, "calls_per_window": args.calls, "windows": args.repeats,
                      "peak_f16_tflops": PEAK_F16_TFLOPS, "cases": cases}))


if __name__ == "__main__":
    main()
