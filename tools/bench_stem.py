#!/usr/bin/env python3
"""Time the stem of the ResNet trunk on the HIP kernels (``VFANet.trunk_stem = "hip"``: ``vfa_stem_conv_f32``,
``vfa_group_norm_affine_f32``, ``vfa_stem_pool_f32``) against the library path it stands beside, on one MI355X.

    python tools/bench_stem.py [--repeats 7] [--calls 5] [--base resnet18] [--profile]

A seeded ``VFANet`` in eval mode on seeded 7 x 3 x 720 x 1280 images (one frame of seven cameras) and on 28 images (B = 4 frames).
All settings in one process, ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over
``--repeats`` windows with the minimum and maximum next to it:
  * the stem alone, library against hip, with the hip stem's three kernels apart (``KernelTimer``: HIP events around each launch) and
    each kernel's distance from its floor -- the convolution's multiply-adds at the measured f32 matrix rate, the bytes of the
    statistics and of the pooling at the streaming rate;
  * the whole trunk (``VFANet.trunk``) in the four combinations of ``trunk_stem`` and ``trunk_convs``;
  * 7 images only: ``VFANet.detect`` end to end with everything on "library" and everything on "hip";
  * the (N) figure of the hip stem against the library stem on the device (normwise difference).
Prints one JSON line.  ``--profile``: no timing -- three calls of the hip stem per case, for a ``rocprofv3 --kernel-trace --stats``
run of its own, which gives the kernels' own times."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F32_MATRIX_TFLOPS = 155.0   # MI355X, the exact f32 MFMA as measured (157.3 by specification)
STREAM_TBPS = 6.29          # MI355X, a float4 copy as measured (8.0 by specification)
KERNELS = ("vfa_stem_conv_f32", "vfa_group_norm_affine_f32", "vfa_stem_pool_f32")


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


def floors_ms(n, L, W, O=64):
    """The least each kernel of the hip stem could take, from the shapes: -> (per kernel, the bytes moved in all)."""
    Lo, Wo = (L - 1) // 2 + 1, (W - 1) // 2 + 1
    Lp, Wp = (Lo - 1) // 2 + 1, (Wo - 1) // 2 + 1
    image, raw, pooled = 4 * n * 3 * L * W, 4 * n * O * Lo * Wo, 4 * n * O * Lp * Wp
    macs = n * O * Lo * Wo * 147
    rate = STREAM_TBPS * 1e12
    floors = {"vfa_stem_conv_f32": max(2 * macs / (F32_MATRIX_TFLOPS * 1e12), (image + raw) / rate) * 1e3,
              "vfa_group_norm_affine_f32": raw / rate * 1e3, "vfa_stem_pool_f32": (raw + pooled) / rate * 1e3}
    return floors, {"gmacs": round(macs / 1e9, 2), "image_mb": round(image / 1e6, 1), "raw_mb": round(raw / 1e6, 1), "pooled_mb": round(pooled / 1e6, 1),
                    "moved_mb": round((image + 3 * raw + pooled) / 1e6, 1)}


def measure(net, images, args, detect=None):
    from vfa_amd import ops
    n = images.shape[0]
    out = {"images": n}
    with torch.no_grad():
        x = net.normalized(images)

    def stem(setting):
        with torch.no_grad():
            return net.base.stem_hip(x) if setting == "hip" else net.base.stem(x)
    if args.profile:
        for _ in range(3):
            stem("hip")
        torch.cuda.synchronize()
        return {"images": n, "profiled_calls": 3}
    got, want = stem("hip"), stem("library")
    out["hip_against_library_normwise"] = float((got.double() - want.double()).norm() / want.double().norm())
    del got, want
    out["stem_ms"] = alternate({"library": lambda: stem("library"), "hip": lambda: stem("hip")}, args)
    per_kernel = {k: [] for k in KERNELS}
    for _ in range(args.repeats):
        with ops.KernelTimer(only=KERNELS) as kt:
            stem("hip")
        torch.cuda.synchronize()
        for k, v in kt.summary().items():
            per_kernel[k].append(v["ms"])
    floors, traffic = floors_ms(n, x.shape[2], x.shape[3])
    out["traffic"] = traffic
    out["kernel_ms"] = {k: dict(summary(v), floor=round(floors[k], 4), over_floor=round(statistics.median(v) / floors[k], 2)) for k, v in per_kernel.items()}

    def trunk(stem_setting, convs):
        net.trunk_stem, net.trunk_convs = stem_setting, convs
        with torch.no_grad():
            return net.trunk(x)
    out["trunk_ms"] = alternate({f"stem_{s}_stages_{c}": (lambda s=s, c=c: trunk(s, c)) for s in ("library", "hip") for c in ("library", "hip")}, args)
    if detect is not None:
        calibs, grid, dec = detect

        def run(setting):
            net.trunk_stem = net.trunk_convs = net.head_convs = setting
            return net.detect(images, calibs, grid, dec, 0.5)
        out["detect_ms"] = alternate({"library": lambda: run("library"), "hip": lambda: run("hip")}, args)
    net.trunk_stem = net.trunk_convs = net.head_convs = "library"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--base", default="resnet18")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4], help="frames of seven cameras per case")
    ap.add_argument("--profile", action="store_true", help="three calls of the hip stem per case and no timing (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stem needs the MI355X"
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
    print(json.dumps({"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "base": args.base,
                      "calls_per_window": args.calls, "windows": args.repeats, "f32_matrix_tflops": F32_MATRIX_TFLOPS, "stream_tbps": STREAM_TBPS,
                      "cases": cases}))


if __name__ == "__main__":
    main()
