#!/usr/bin/env python3
"""Time the AP/AOS metric on one MI355X: the fused HIP path against what the library offered before it.

    python tools/bench_ap_aos.py [--frames 200] [--cows 15] [--dets 100] [--repeats 20] [--pairwise 300]

On a seeded synthetic set of the size of a MultiviewC validation run (hundreds of frames, ~15 cows and up to 100 detections per
frame) it measures
  (a) ``eval_ops.ap_aos``: every IoU of the set and the best match of every detection in ONE launch, three thresholds from it
      (wall clock of the whole call, host work and copies included; ``match_frames`` and the library call alone between HIP events);
  (b) the same pairs through the reference's steps written as BATCHED torch ops over all pairs at once (``torch_iou3d`` below, this
      tool's own code) with ``eval_ops.sort_v`` in the middle -- the best one could compose from the library before the fused
      kernels existed -- plus the per-detection argmax (HIP events and wall clock);
  (c) that composition called PAIR BY PAIR the way the reference's ``cal_frame_TPFP_iou`` does (two 7-number host tensors per
      pair, copied to the device, ~60 small launches, a Python comparison of the result = one host synchronisation), on a subset
      of the pairs, wall clock, EXTRAPOLATED to the whole set times three thresholds and labelled as such.
Prints one JSON line.  Warm-up first; the HIP-event figures are per call from windows of ``--calls`` queued calls, medians over
``--repeats`` windows with their minimum and maximum next to them; (b) includes the two gathers that form the pairs."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_iou3d(box1, box2, sort_v):
    """The steps of the reference's IoU3D as batched torch ops: box1, box2 (n, 7) -> (iou3d, iou_bev, overlap), each (n).  The one
    step torch cannot express, the vertex ordering, is ``sort_v`` (vertices (1, n, 24, 2), mask, num_valid -> (1, n, 9))."""
    dev = box1.device
    sx = torch.tensor([.5, -.5, -.5, .5], device=dev)
    sy = torch.tensor([.5, .5, -.5, -.5], device=dev)

    def corners(b):
        tx, ty = sx * b[:, 3:4], sy * b[:, 4:5]
        c, s = torch.cos(b[:, 6:7]), torch.sin(b[:, 6:7])
        return torch.stack([b[:, 0:1] + (tx * c - ty * s), b[:, 1:2] + (tx * s + ty * c)], dim=-1)      # (n, 4, 2)

    def inside(p, q):  # corners of p inside rectangle q
        a, ab, ad = q[:, 0:1], q[:, 1:2] - q[:, 0:1], q[:, 3:4] - q[:, 0:1]
        am = p - a
        r_ab, r_ad = (am * ab).sum(-1) / (ab * ab).sum(-1), (am * ad).sum(-1) / (ad * ad).sum(-1)
        return (r_ab > -1e-6) & (r_ab < 1 + 1e-6) & (r_ad > -1e-6) & (r_ad < 1 + 1e-6)

    c1, c2 = corners(box1), corners(box2)
    n = c1.shape[0]
    e1 = torch.cat([c1, c1[:, [1, 2, 3, 0]]], dim=-1)[:, :, None, :].expand(n, 4, 4, 4)
    e2 = torch.cat([c2, c2[:, [1, 2, 3, 0]]], dim=-1)[:, None, :, :].expand(n, 4, 4, 4)
    x1, y1, x2, y2 = e1.unbind(-1)
    x3, y3, x4, y4 = e2.unbind(-1)
    den = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    mol_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)
    mol_u = (x2 - x1) * (y1 - y3) - (y2 - y1) * (x1 - x3)
    t, u = mol_t / den, mol_u / den
    hit = (t > 0) & (t < 1) & (u > 0) & (u < 1)
    t = mol_t / (den + 1e-8)
    inters = torch.stack([x1 + t * (x2 - x1), y1 + t * (y2 - y1)], dim=-1) * hit[..., None].float()
    vertices = torch.cat([c1, c2, inters.reshape(n, 16, 2)], dim=1)                                     # (n, 24, 2)
    masks = torch.cat([inside(c1, c2), inside(c2, c1), hit.reshape(n, 16)], dim=1)
    num_valid = masks.sum(-1).int()
    mean = (vertices * masks[..., None]).sum(1, keepdim=True) / num_valid[:, None, None]
    idx = sort_v((vertices - mean)[None].contiguous(), masks[None].contiguous(), num_valid[None].contiguous())[0].long()
    sel = torch.gather(vertices, 1, idx[..., None].expand(-1, -1, 2))
    overlap = (sel[:, :-1, 0] * sel[:, 1:, 1] - sel[:, :-1, 1] * sel[:, 1:, 0]).sum(1).abs() / 2
    union = box1[:, 3] * box1[:, 4] + box2[:, 3] * box2[:, 4] - overlap
    bev = overlap / union
    z_overlap = (torch.min(box1[:, 2] + 0.5 * box1[:, 5], box2[:, 2] + 0.5 * box2[:, 5])
                 - torch.max(box1[:, 2] - 0.5 * box1[:, 5], box2[:, 2] - 0.5 * box2[:, 5]))
    inter = bev * union * z_overlap
    return inter / (box1[:, 3] * box1[:, 4] * box1[:, 5] + box2[:, 3] * box2[:, 4] * box2[:, 5] - inter), bev, overlap


def synthetic_set(frames, cows, dets, seed=0):
    """gt (frames * cows, 8) and det (frames * dets, 9) in the text-file column layout: about 0.8 * cows true detections of
    graded quality per frame, the rest clutter."""
    rng = np.random.default_rng(seed)
    gt, det = [], []
    for f in range(frames):
        h = rng.uniform(120, 160, cows)
        g = np.stack([np.full(cows, f), rng.uniform(300, 3600, cows), rng.uniform(300, 3600, cows), h / 2, rng.uniform(180, 260, cows),
                      rng.uniform(60, 110, cows), h, rng.uniform(-np.pi, np.pi, cows)], axis=1)
        gt.append(g)
        hit = g[rng.uniform(size=cows) < 0.8]
        sigma = rng.choice([5.0, 15.0, 30.0, 60.0], size=len(hit))
        d = hit.copy()
        d[:, 1] += rng.normal(0, sigma)
        d[:, 2] += rng.normal(0, sigma)
        d[:, 7] += rng.normal(0, sigma / 100)
        n_fp = dets - len(d)
        hf = rng.uniform(120, 160, n_fp)
        fp = np.stack([np.full(n_fp, f), rng.uniform(300, 3600, n_fp), rng.uniform(300, 3600, n_fp), hf / 2, rng.uniform(180, 260, n_fp),
                       rng.uniform(60, 110, n_fp), hf, rng.uniform(-np.pi, np.pi, n_fp)], axis=1)
        det.append(np.concatenate([np.concatenate([d, fp]), rng.uniform(0.3, 1.0, (dets, 1))], axis=1))
    return np.concatenate(gt), np.concatenate(det)


def timed(fn, repeats, calls=1, warmup=3):
    """Per-call milliseconds of fn(): every timed window enqueues `calls` calls between two HIP events and ends in a device
    synchronise (one 0.1 ms launch per window would measure the events and the scheduler as much as the kernel).  Returns the
    median wall clock, the median HIP-event time and the (min, max) of the HIP-event time over the `repeats` windows."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, gpu = [], []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / calls)
        gpu.append(start.elapsed_time(end) / calls)
    return statistics.median(wall), statistics.median(gpu), (round(min(gpu), 4), round(max(gpu), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--cows", type=int, default=15)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window of the HIP-event measurements")
    ap.add_argument("--pairwise", type=int, default=300, help="pairs of the subset that is run one pair at a time")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ap_aos needs the MI355X"
    from vfa_amd import eval_ops
    dev = torch.device("cuda:0")
    gt, det = synthetic_set(args.frames, args.cows, args.dets)
    n_pairs = args.frames * args.cows * args.dets

    # (a) the fused path
    result = eval_ops.ap_aos(gt, det)
    a_wall, _, _ = timed(lambda: eval_ops.ap_aos(gt, det), args.repeats)
    det_b, gt_b = torch.from_numpy(det[:, 1:8]).float().to(dev), torch.from_numpy(gt[:, 1:8]).float().to(dev)
    det_f, gt_f = torch.from_numpy(det[:, 0]).long().to(dev), torch.from_numpy(gt[:, 0]).long().to(dev)
    _, a_launch, a_launch_span = timed(lambda: eval_ops.match_frames(det_b, det_f, gt_b, gt_f, n_frames=args.frames), args.repeats,
                                        args.calls)
    best_idx, best_iou = eval_ops.match_frames(det_b, det_f, gt_b, gt_f, n_frames=args.frames)
    # ... and the library call alone (offsets built beforehand): the fused best-match kernel, and the pair kernel that writes the matrix
    edges = torch.arange(args.frames + 1, device=dev)
    det_begin, gt_begin = torch.searchsorted(det_f, edges).int(), torch.searchsorted(gt_f, edges).int()
    pair_begin = (torch.arange(args.frames + 1, device=dev) * (args.cows * args.dets)).long()
    _, a_kernel, a_kernel_span = timed(lambda: eval_ops._frames_call(det_b, det_begin, gt_b, gt_begin, args.frames, None, 0, False, True),
                                        args.repeats, args.calls)
    _, a_matrix, a_matrix_span = timed(lambda: eval_ops._frames_call(det_b, det_begin, gt_b, gt_begin, args.frames, pair_begin, n_pairs,
                                                                     True, True), args.repeats, args.calls)

    # (b) batched torch ops + sort_v over the same pairs (every frame has `cows` ground truths: the rows form a (P, cows) matrix)
    di = torch.arange(det_b.shape[0], device=dev).repeat_interleave(args.cows)
    gi = (det_f * args.cows).repeat_interleave(args.cows) + torch.arange(args.cows, device=dev).repeat(det_b.shape[0])

    def batched():  # (forming the pairs -- the two gathers -- is part of this path and of its time)
        iou, _, _ = torch_iou3d(det_b[di], gt_b[gi], eval_ops.sort_v)
        m = iou.reshape(-1, args.cows)
        m = torch.where(torch.isnan(m), torch.full_like(m, -2.0), m)
        return m.max(dim=1)
    b_wall, _, _ = timed(batched, args.repeats)
    _, b_gpu, b_gpu_span = timed(batched, args.repeats, args.calls)
    b_val, b_idx = batched()
    agree = float((b_idx.int() == best_idx).float().mean())
    max_diff = float((b_val - best_iou).abs().max())

    # (c) the same composition pair by pair, the way the reference's evaluation loop calls it
    rng = np.random.default_rng(1)
    subset = rng.choice(n_pairs, size=min(args.pairwise, n_pairs), replace=False)
    di_h, gi_h = di.cpu().numpy(), gi.cpu().numpy()

    def pair_by_pair():
        hits = 0
        for k in subset:
            p = torch.Tensor(det[di_h[k], 1:8].tolist()).unsqueeze(0).to(dev)
            g = torch.Tensor(gt[gi_h[k], 1:8].tolist()).unsqueeze(0).to(dev)
            iou, _, _ = torch_iou3d(p, g, eval_ops.sort_v)
            if iou >= 0.5:  # (a host synchronisation per pair, like evaluateAPAOS.py:84)
                hits += 1
        return hits
    pair_by_pair()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pair_by_pair()
    torch.cuda.synchronize()
    c_subset = (time.perf_counter() - t0) * 1e3
    c_per_pair = c_subset / len(subset)

    print(json.dumps({
        "frames": args.frames, "ground_truths": int(gt.shape[0]), "detections": int(det.shape[0]), "pairs": n_pairs,
        "ap_aos": [[round(v, 6) for v in r] for r in result],
        "a_ap_aos_wall_ms": round(a_wall, 3), "a_match_frames_gpu_ms": round(a_launch, 4),
        "a_match_frames_gpu_ms_min_max": a_launch_span,
        "a_best_match_call_gpu_ms": round(a_kernel, 4), "a_best_match_call_gpu_ms_min_max": a_kernel_span,
        "a_matrix_and_best_match_call_gpu_ms": round(a_matrix, 4), "a_matrix_and_best_match_call_gpu_ms_min_max": a_matrix_span,
        "calls_per_window": args.calls, "windows": args.repeats,
        "b_batched_torch_sort_v_wall_ms": round(b_wall, 3), "b_batched_torch_sort_v_gpu_ms": round(b_gpu, 3), "b_batched_torch_sort_v_gpu_ms_min_max": b_gpu_span,
        "b_same_best_index": agree, "b_max_abs_best_iou_diff": max_diff,
        "c_pair_by_pair_subset_pairs": int(len(subset)), "c_pair_by_pair_ms_per_pair": round(c_per_pair, 4),
        "c_extrapolated_three_thresholds_s": round(c_per_pair * n_pairs * 3 / 1e3, 1),
        "ratio_b_gpu_over_a_match_frames_gpu": round(b_gpu / a_launch, 1), "ratio_b_wall_over_a_wall": round(b_wall / a_wall, 2),
        "ratio_c_extrapolated_over_a_wall": round(c_per_pair * n_pairs * 3 / a_wall, 0)}))


if __name__ == "__main__":
    main()
