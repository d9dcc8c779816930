#!/usr/bin/env python3
"""Time the front of a frame -- the cameras' uint8 frames to the normalised float32 tensor of the trunk -- on one MI355X:

  (a) ``ops.image_frontend`` (``vfa_image_frames_u8_f32``): Pillow's resize, ``ToTensor`` and the normalisation in one kernel;
  (b) the torch-op chain on the device: ``F.interpolate(float, mode="bilinear", antialias=True)``, the division by 255 and
      ``(x - mean) / std``.  NOT Pillow's pixels: its worst difference from (a) is printed next to its time, in byte levels;
  (c) where Pillow imports, the reference's host path: ``Image.resize`` + ``ToTensor`` per camera and the upload of the float32
      tensor (the normalisation stays on the device and is not in this leg).  Otherwise the leg reports itself as absent.

    python tools/bench_frontend.py [--repeats 10] [--calls 20]

Two cases, a rig of 7 cameras each: 1080 x 1920 -> 720 x 1280 (Wildtrack, MultiviewX) and 720 x 1280 without a resize.  (a) and (b)
in one process, ALTERNATING, between HIP events around windows of ``--calls`` calls: the median over ``--repeats`` windows with the
minimum and maximum.  Every call of a window works on another of ``--ring`` source / target pairs, so that what a call reads and
writes has left the 256 MiB Infinity Cache when its turn comes again.  ``floor_us`` is the bytes the call must move (the frames read
once, the tensor written once) over 6.3 TB/s, the HBM rate a streaming kernel reaches on this part; ``share_of_hbm_rate`` is that
floor over the measured time.  The host leg is wall-clock time of one frame, the median of three.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CAMERAS = 7
CASES = [("resize", (1080, 1920), (720, 1280)), ("no_resize", (720, 1280), (720, 1280))]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_BYTES_PER_S = 6.3e12


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def summary(values):
    return {"median": round(statistics.median(values), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def host_leg(frames, size, dev):
    """The reference's path for one frame of the rig -> (milliseconds, the uploaded tensor), or None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        planes = []
        for cam in frames:
            pic = Image.fromarray(cam)
            if pic.size != (size[1], size[0]):
                pic = pic.resize((size[1], size[0]), Image.BILINEAR)
            planes.append(torch.from_numpy(np.asarray(pic).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255))
        up = torch.stack(planes).to(dev)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return summary(times), up


def measure(name, in_hw, out_hw, args, dev):
    from vfa_amd import ops
    rng = np.random.default_rng(5)
    size = None if in_hw == out_hw else out_hw
    host = [rng.integers(0, 256, (CAMERAS, *in_hw, 3), dtype=np.uint8) for _ in range(args.ring)]
    src = [torch.from_numpy(h).to(dev) for h in host]
    dst = [torch.empty(CAMERAS, 3, *out_hw, device=dev) for _ in range(args.ring)]
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)

    def ours(i):
        return ops.image_frontend(src[i % args.ring], size=size, mean=mean, std=std, out=dst[i % args.ring])

    def chain(i):
        x = src[i % args.ring].permute(0, 3, 1, 2).float()
        if size is not None:
            x = F.interpolate(x, size=out_hw, mode="bilinear", antialias=True, align_corners=False)
        x = x / 255
        return (x - mean.view(3, 1, 1)) / std.view(3, 1, 1)

    for fn in (ours, chain):
        for i in range(args.ring):
            fn(i)
    torch.cuda.synchronize()
    times = {"image_frontend": [], "torch_chain": []}
    for _ in range(args.repeats):
        times["image_frontend"].append(window(ours, args.calls))
        times["torch_chain"].append(window(chain, args.calls))
    out = {"case": name, "cameras": CAMERAS, "in": list(in_hw), "out": list(out_hw), "ms": {k: summary(v) for k, v in times.items()}}
    # what the chain computes instead of Pillow's pixels, in byte levels
    ours_plain = ops.image_frontend(src[0], size=size)
    x = src[0].permute(0, 3, 1, 2).float()
    chain_plain = (F.interpolate(x, size=out_hw, mode="bilinear", antialias=True, align_corners=False) if size is not None else x) / 255
    out["torch_chain_worst_difference_in_byte_levels"] = round(float((chain_plain - ours_plain).abs().max()) * 255, 4)
    out["torch_chain_equal_bits"] = bool(torch.equal(chain(0), ours(0)))
    moved = CAMERAS * (in_hw[0] * in_hw[1] * 3 + 3 * out_hw[0] * out_hw[1] * 4)
    out["bytes_moved"] = moved
    out["floor_us"] = round(moved / HBM_BYTES_PER_S * 1e6, 2)
    out["share_of_hbm_rate"] = round(moved / HBM_BYTES_PER_S * 1e3 / out["ms"]["image_frontend"]["median"], 3)
    out["chain_over_frontend"] = round(out["ms"]["torch_chain"]["median"] / out["ms"]["image_frontend"]["median"], 2)
    leg = host_leg(host[0], out_hw, dev)
    if leg is None:
        out["ms"]["host_pillow_and_upload"] = "absent: Pillow is not installed"
    else:
        out["ms"]["host_pillow_and_upload"] = leg[0]
        out["host_path_equal_bits"] = bool(torch.equal(leg[1], ours_plain))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--ring", type=int, default=4, help="source / target pairs a window walks through")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frontend needs the MI355X"
    dev = torch.device("cuda:0")
    cases = []
    for name, in_hw, out_hw in CASES:
        r = measure(name, in_hw, out_hw, args, dev)
        cases.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "ring": args.ring, "cases": cases}))


if __name__ == "__main__":
    main()
