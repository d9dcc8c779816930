#!/usr/bin/env python3
"""Time the orientation head evaluated where it is read (``VFANet.heads(..., rotation_at=...)`` on ``vfa_conv3x3_at_cells_f32``)
against the dense head it stands beside (``orient_pred`` as a 256 -> 360 dilated convolution over the whole grid), on one MI355X.

    python tools/bench_sparse_rotation.py [--repeats 10] [--calls 20]

The head shapes 156 x 156 and 200 x 200 at B = 1 and B = 4, a seeded ``VFANet`` (resnet18, 3D) in eval mode on a seeded fused BEV map,
the threshold set so that about 40 cells per frame are detections (top-k keeps 100).  Per case, both sides in one process,
ALTERNATING, between HIP events: per call from windows of ``--calls`` queued calls, the median over ``--repeats`` windows with the
minimum and maximum next to it:
  * inference: ``heads`` + ``decode_fused``, dense against ``rotation_at="detections"`` (after asserting that every output but the
    rotation is the same bits), and the two layers alone: the dense ``orient_pred`` against the kernel at the decode's 100 cells;
  * training: forward + backward of the head from the fused map on 40 positive cells per frame, ``ops.conv3x3_at_cells`` against the
    dense ``orient_pred`` + ``[mask]``, gradients into the map and the weight;
  * peak device memory of one call of each above what was allocated before it.
Prints one JSON line."""
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
    return {k: summary(v) for k, v in times.items()}


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 2)


def measure(net, L, W, B, args, dev):
    from vfa_amd import eval_ops, ops
    dec = eval_ops.BEVDecoder("MultiviewC", (L * 25, W * 25), (25, 25, 32), dimension_mean=np.array([140, 60, 230], np.float32), topk=100)
    topdown = torch.randn(B, 256, L, W, generator=torch.Generator().manual_seed(L + B)).to(dev)
    conv = net.orient_pred[0]
    with torch.no_grad():
        lazy = net.heads(topdown, rotation_at="detections")
        fused = lazy["rotation_head"][0]
        dense_pred = {k: v for k, v in lazy.items() if k != "rotation_head"}      # the same heads, so the same bits to decode
        dense_pred["rotation"] = conv(fused).permute(0, 2, 3, 1)
        conf = eval_ops.bev_nms_batch(dense_pred["heatmap"]).reshape(B, -1)
        thresh = float(conf.topk(POSITIVES + 1, dim=1).values[:, -1].max())     # at most 40 detections per frame
        want, got = dec.decode_fused(dense_pred, thresh), dec.decode_fused(lazy, thresh)
        for k in ("count", "conf", "cell", "location", "dimension"):
            assert torch.equal(want[k], got[k]), k
        same_rotation = float((want["rotation"] == got["rotation"]).float().mean())
        cells100 = got["cell"]

    def infer(rotation_at):
        with torch.no_grad():
            return dec.decode_fused(net.heads(topdown, rotation_at=rotation_at), thresh)

    def layer_dense():
        with torch.no_grad():
            return conv(fused)

    def layer_cells():
        return ops.conv3x3_at_cells_forward(fused, conv.weight, cells100, 4, want_logits=False, want_rotation=True)

    # training: 40 positive cells per frame, ascending (the order of boolean indexing)
    rng = np.random.default_rng(L * 7 + B)
    cells = torch.tensor(np.stack([np.sort(rng.permutation(L * W)[:POSITIVES]) for _ in range(B)]), dtype=torch.int32, device=dev)
    mask = torch.zeros(B, L * W, dtype=torch.bool, device=dev)
    mask.scatter_(1, cells.long(), True)
    mask = mask.reshape(B, L, W)
    G = torch.randn(B * POSITIVES, 360, device=dev)
    x = fused.clone().requires_grad_()

    def train_dense():
        x.grad = conv.weight.grad = None
        (conv(x).permute(0, 2, 3, 1)[mask] * G).sum().backward()

    def train_cells():
        x.grad = conv.weight.grad = None
        (ops.conv3x3_at_cells(x, conv.weight, cells, dilation=4).reshape(B * POSITIVES, 360) * G).sum().backward()
    train_dense()
    gx, gw = x.grad.clone(), conv.weight.grad.clone()
    train_cells()
    torch.testing.assert_close(x.grad, gx, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(conv.weight.grad, gw, rtol=1e-4, atol=1e-5)

    out = {"grid": [L, W], "B": B, "detections": want["count"].tolist(), "rotations_equal_to_dense": same_rotation}
    out["inference_ms"] = alternate({"dense": lambda: infer(None), "at_detections": lambda: infer("detections")}, args)
    out["layer_ms"] = alternate({"dense_orient_pred": layer_dense, "at_100_cells": layer_cells}, args)
    out["train_head_ms"] = alternate({"dense_and_mask": train_dense, "at_40_cells": train_cells}, args)
    out["peak_mib"] = {"inference_dense": peak_mib(lambda: infer(None)), "inference_at_detections": peak_mib(lambda: infer("detections")),
                       "train_dense_and_mask": peak_mib(train_dense), "train_at_40_cells": peak_mib(train_cells)}
    for group in ("inference_ms", "layer_ms", "train_head_ms"):
        a, b = (v["median"] for v in out[group].values())
        out[group]["dense_over_cells"] = round(a / b, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sparse_rotation needs the MI355X"
    dev = torch.device("cuda:0")
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(0)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").to(dev).eval()
    cases = []
    for L, W in SHAPES:
        for B in (1, 4):
            r = measure(net, L, W, B, args, dev)
            cases.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"calls_per_window": args.calls, "windows": args.repeats, "topk": 100, "positives_per_frame": POSITIVES, "cases": cases}))


if __name__ == "__main__":
    main()
