"""Consumers of the path on the GPU: BEV decode and the AP/AOS metric's vertex sorter.

* ``sort_vertices`` / ``sort_v``  -- drop-in for the reference's CUDA op (``vfa/evaluation/pyeval/cuda_op/cuda_ext.py:6-17``,
  kernel ``sort_vert_kernel.cu:42-134``): same arguments, same ``(b, n, 9)`` int32 result, on the HIP kernel
  ``vfa_sort_vertices_f32``.  ``evaluateAPAOS.py:79-83`` hard-codes ``device('cuda')``, which IS the MI355X under PyTorch-ROCm.
* ``BEVDecoder``  -- ``ObjectEncoder.nms / decode3d / decode2d`` (``vfa/data/encoder.py:230-305``) with the dataset constants
  passed explicitly: sigmoid + 5x5 max-pool NMS in one HIP kernel (``vfa_bev_nms_f32``), then top-k and the gathers (torch ops on
  the device: a few hundred numbers).  ``BEVDecoder.decode_fused`` does the whole decode of a batch of frames in one call
  (``vfa_bev_decode_f32``) with outputs of a fixed shape and no host wait; ``split`` and ``flat_detections`` hand them on.
* ``iou3d`` / ``iou_bev`` / ``iou3d_matrix`` / ``match_frames``  -- the reference's rotated-box ``IoU3D`` (``vfa/evaluation/pyeval/
  IoU.py:206-225``) with one GPU lane per box pair (``vfa_iou3d_f32``, ``vfa_iou3d_frames_f32``): any batch shape, a whole
  evaluation set per launch, the best ground truth of every detection without a host round trip per pair.
* ``ap_aos_from_matches`` / ``ap_aos`` / ``evaluate_ap_aos``  -- the AP / AOS metric built on them (``evaluateAPAOS.py``);
  ``evaluate_ap_aos`` has the signature and the 9-tuple of the reference's ``evaluateDetectionAPAOS``.
* ``match_frames_hungarian`` / ``clear_mod`` / ``evaluate_detection``  -- the MODA / MODP metric of the 2D sets (``CLEAR_MOD_HUN.py``,
  ``evaluateDetection.py``): distances and the Hungarian assignment of every frame of an evaluation set in one launch, one wave per
  frame (``vfa_clear_mod_frames_f64``); ``evaluate_detection`` has the signature and the 4-tuple of ``evaluateDetection_py``.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, ops


def sort_vertices(vertices, mask, num_valid):
    """vertices (b,n,m,2) f32, mask (b,n,m) bool, num_valid (b,n) int32 -> idx (b,n,9) int32 (reference ``sort_v``)."""
    _lib.require_device(vertices, mask, num_valid)
    assert vertices.dtype == torch.float32 and mask.dtype == torch.bool and num_valid.dtype == torch.int32
    vertices, mask, num_valid = vertices.contiguous(), mask.contiguous(), num_valid.contiguous()
    b, n, m, _ = vertices.shape
    idx = torch.zeros((b, n, 9), dtype=torch.int32, device=vertices.device)
    _lib.call("vfa_sort_vertices_f32", _lib.ptr(vertices), _lib.ptr(mask.view(torch.uint8)), _lib.ptr(num_valid), _lib.ptr(idx),
              b, n, m, _lib.current_stream_handle())
    return idx


sort_v = sort_vertices  # the name the reference imports (IoU.py:3)


def bev_nms(heatmap):
    """heatmap (1,1,L,W) logits -> (1,1,L,W): sigmoid where it is the 5x5 maximum, else 0 (encoder.py:230-232, :238)."""
    _lib.require_device(heatmap)
    h = heatmap.to(torch.float32).contiguous()
    L, W = h.shape[-2:]
    assert h.numel() == L * W, "batch 1, one class, like the reference (a batch: bev_nms_batch)"
    conf = torch.empty_like(h)
    _lib.call("vfa_bev_nms_f32", _lib.ptr(h), _lib.ptr(conf), L, W, _lib.current_stream_handle())
    return conf


def bev_nms_batch(heatmap):
    """heatmap (B,1,L,W) logits -> (B,1,L,W): ``bev_nms`` of every frame in one launch (``vfa_bev_nms_batch_f32``); the 5x5 window
    stops at each frame's edges."""
    _lib.require_device(heatmap)
    h = heatmap.to(torch.float32).contiguous()
    if h.dim() != 4 or h.shape[1] != 1:
        raise ValueError(f"bev_nms_batch: heatmap must be (B, 1, L, W), got {tuple(h.shape)}")
    B, _, L, W = h.shape
    conf = torch.empty_like(h)
    _lib.call("vfa_bev_nms_batch_f32", _lib.ptr(h), _lib.ptr(conf), B, L, W, _lib.current_stream_handle())
    return conf


def _pair_ious(box1, box2, want_bev):
    _lib.require_device(box1, box2)
    if box1.shape != box2.shape or box1.dim() < 1 or box1.shape[-1] != 7:
        raise ValueError(f"two box tensors of one shape (..., 7) are needed, got {tuple(box1.shape)} and {tuple(box2.shape)}")
    lead = box1.shape[:-1]
    a, b = (t.to(torch.float32).reshape(-1, 7).contiguous() for t in (box1, box2))
    vol = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    bev = torch.empty_like(vol) if want_bev else None
    _lib.call("vfa_iou3d_f32", _lib.ptr(a), _lib.ptr(b), _lib.ptr(vol), _lib.ptr(bev), a.shape[0], _lib.current_stream_handle())
    return vol.reshape(lead), (bev.reshape(lead) if want_bev else None)


def iou3d(box3d1, box3d2):
    """The reference's ``IoU3D`` (IoU.py:206-225): boxes ``x y z l w h alpha``, ``(B, N, 7)`` like the reference's or any equal
    leading shape (the reference itself only works on a single pair, IoU.py:27-28) -> IoUs of that leading shape.  Boxes apart in z
    give a negative value like the reference's (its z overlap is not clamped)."""
    return _pair_ious(box3d1, box3d2, False)[0]


def iou_bev(box1, box2):
    """Rotated-rectangle IoU, the first result of the reference's ``IoUs2D`` (IoU.py:178-204): boxes ``x y w h alpha``,
    ``(..., 5)`` -> ``(...)``."""
    _lib.require_device(box1, box2)
    if box1.shape != box2.shape or box1.dim() < 1 or box1.shape[-1] != 5:
        raise ValueError(f"two box tensors of one shape (..., 5) are needed, got {tuple(box1.shape)} and {tuple(box2.shape)}")

    def lift(b):  # a unit-height box at z = 0 over the rectangle
        b = b.to(torch.float32)
        return torch.stack([b[..., 0], b[..., 1], torch.zeros_like(b[..., 0]), b[..., 2], b[..., 3], torch.ones_like(b[..., 0]),
                            b[..., 4]], dim=-1)
    return _pair_ious(lift(box1), lift(box2), True)[1]


def _frames_call(det, det_begin, gt, gt_begin, n_frames, pair_begin, n_pairs, want_matrix, want_best):
    dev = det.device
    iou = torch.empty(n_pairs, dtype=torch.float32, device=dev) if want_matrix else None
    best_idx = torch.full((det.shape[0],), -1, dtype=torch.int32, device=dev) if want_best else None
    best_iou = torch.full((det.shape[0],), -1.0, dtype=torch.float32, device=dev) if want_best else None
    _lib.call("vfa_iou3d_frames_f32", _lib.ptr(det), _lib.ptr(det_begin), _lib.ptr(gt), _lib.ptr(gt_begin), n_frames, det.shape[0],
              gt.shape[0], _lib.ptr(pair_begin), n_pairs, _lib.ptr(iou), _lib.ptr(best_idx), _lib.ptr(best_iou),
              _lib.current_stream_handle())
    return iou, best_idx, best_iou


def _frame_tables(who, det_frame, gt_frame, n_det, n_gt, n_frames, with_matrix, row="box"):
    """The offset tables ``match_frames`` and ``match_frames_hungarian`` (``who``) hand to their kernels, from the sorted frame
    counters -> ``(n_frames, det_begin, gt_begin, pair_begin, n_pairs)``: the begins int32, ``n_frames + 1`` long; ``pair_begin``
    int64 (``None`` and 0 pairs without a matrix).  Plain torch on the device the counters live on.  The host waits are the two the
    callers document: ``n_frames is None`` reads the largest counter (and the order), ``with_matrix`` the number of pairs."""
    det_frame, gt_frame = det_frame.to(torch.int64).contiguous(), gt_frame.to(torch.int64).contiguous()
    if det_frame.shape != (n_det,) or gt_frame.shape != (n_gt,):
        raise ValueError(f"one frame counter per {row} is needed")
    dev = det_frame.device
    if n_frames is None:
        both = torch.cat([det_frame, gt_frame])
        if both.numel() == 0:
            n_frames = 0
        else:
            ordered = torch.stack([(det_frame[1:] >= det_frame[:-1]).all(), (gt_frame[1:] >= gt_frame[:-1]).all(), both.min() >= 0])
            hi, ok = int(both.max()), bool(ordered.all())
            if not ok:
                raise ValueError(f"{who}: frame counters must be non-negative and sorted (non-decreasing)")
            n_frames = hi + 1
    edges = torch.arange(n_frames + 1, dtype=torch.int64, device=dev)
    det_begin64, gt_begin64 = torch.searchsorted(det_frame, edges), torch.searchsorted(gt_frame, edges)
    det_begin, gt_begin = det_begin64.to(torch.int32), gt_begin64.to(torch.int32)
    if not with_matrix:
        return n_frames, det_begin, gt_begin, None, 0
    pair_begin = torch.zeros(n_frames + 1, dtype=torch.int64, device=dev)
    pair_begin[1:] = torch.cumsum((det_begin64[1:] - det_begin64[:-1]) * (gt_begin64[1:] - gt_begin64[:-1]), 0)
    return n_frames, det_begin, gt_begin, pair_begin, int(pair_begin[-1])


def _box_rows(t, name):
    if t.dim() != 2 or t.shape[1] != 7:
        raise ValueError(f"{name} must be (n, 7) boxes x y z l w h alpha, got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def iou3d_matrix(det, gt):
    """``det (P, 7)``, ``gt (G, 7)`` -> the ``(P, G)`` matrix of 3D IoUs, one lane per pair in one launch."""
    _lib.require_device(det, gt)
    det, gt = _box_rows(det, "det"), _box_rows(gt, "gt")
    P, G = det.shape[0], gt.shape[0]
    det_begin = torch.tensor([0, P], dtype=torch.int32, device=det.device)
    gt_begin = torch.tensor([0, G], dtype=torch.int32, device=det.device)
    pair_begin = torch.tensor([0, P * G], dtype=torch.int64, device=det.device)
    iou, _, _ = _frames_call(det, det_begin, gt, gt_begin, 1, pair_begin, P * G, True, False)
    return iou.reshape(P, G)


def match_frames(det, det_frame, gt, gt_frame, n_frames=None, with_matrix=False):
    """The best ground truth of every detection of an evaluation set, in one launch (``vfa_iou3d_frames_f32``).

    ``det (P, 7)``, ``gt (G, 7)`` boxes; ``det_frame (P)``, ``gt_frame (G)`` integer frame counters ``0 .. n_frames - 1``, each
    NON-DECREASING (rows sorted by frame).  ``n_frames``: given by the caller, nothing here waits for the device; ``None``: taken
    from the largest counter, which costs one host synchronisation (and checks the order while it is at it).  With ``n_frames`` given
    the counters are NOT checked: unsorted or out-of-range ones stay within the arrays but give meaningless matches.
    Returns ``best_idx (P)`` int32 -- index of the ground truth WITHIN ITS FRAME with the largest IoU, the lowest index on a tie,
    -1 when the frame has no ground truth (or only NaN IoUs) -- and ``best_iou (P)`` (-1 there).  A threshold ``t > 0`` of the
    metric is then ``best_iou >= t`` (see include/vfa_hip.h for why that equals the reference's scan).
    ``with_matrix=True`` also fills the frames' IoU matrices and returns ``(best_idx, best_iou, iou, pair_begin)``: frame ``f``'s
    ``(P_f, G_f)`` matrix is ``iou[pair_begin[f]:pair_begin[f + 1]]``, detection-major (one more synchronisation, for its size)."""
    _lib.require_device(det, det_frame, gt, gt_frame)
    det, gt = _box_rows(det, "det"), _box_rows(gt, "gt")
    n_frames, det_begin, gt_begin, pair_begin, n_pairs = _frame_tables("match_frames", det_frame, gt_frame, det.shape[0], gt.shape[0],
                                                                       n_frames, with_matrix)
    iou, best_idx, best_iou = _frames_call(det, det_begin, gt, gt_begin, n_frames, pair_begin, n_pairs, with_matrix, True)
    return (best_idx, best_iou, iou, pair_begin) if with_matrix else (best_idx, best_iou)


def ap_aos_from_matches(conf, matched, delta_rot, n_gt):
    """The tail of the reference's ``CLEAR_MOD_HUN2`` (evaluateAPAOS.py:21-65) from the match table.

    ``conf (N)`` confidences, ``matched (N)`` true where the detection has a ground truth (TP), ``delta_rot (N)`` its angle
    difference in radians (read only where matched), ``n_gt`` the number of ground truths (``all_P``).  Detections in descending
    confidence; precision ``TP / (TP + FP)``, recall ``TP / n_gt`` and the running orientation similarity
    ``cumsum(tp (1 + cos delta) / 2) / (i + 1)`` as prefix sums (the reference's is a quadratic loop); then the 11 recall points
    ``arange(0, 1.1, 0.1)``: the maximum of the tail that starts at the first detection whose recall reaches the point, 0 when none
    does.  float64 like the reference's numpy, plain torch ops on the device the inputs live on.  Returns ``(AP, AOS)`` as fractions.
    Equal confidences: the order among them is unspecified, here as in the reference (whose reversed argsort is not stable)."""
    if n_gt <= 0:
        raise ValueError("ap_aos_from_matches: n_gt must be positive (recall is TP / n_gt)")
    conf = torch.as_tensor(conf).to(torch.float64)
    dev = conf.device
    n = conf.numel()
    if n == 0:
        return 0.0, 0.0
    order = torch.argsort(conf, descending=True)
    tp = torch.as_tensor(matched, device=dev).to(torch.bool)[order]
    delta = torch.as_tensor(delta_rot, device=dev).to(torch.float64)[order]
    rank = torch.arange(1, n + 1, dtype=torch.float64, device=dev)
    ctp = torch.cumsum(tp.to(torch.float64), 0)
    precision, recall = ctp / rank, ctp / float(n_gt)
    sim = torch.where(tp, (1 + torch.cos(delta)) / 2, torch.zeros_like(delta))
    aos = torch.cumsum(sim, 0) / rank
    points = torch.as_tensor(np.arange(0, 1.1, 0.1), dtype=torch.float64, device=dev)
    first = torch.searchsorted(recall.contiguous(), points)          # recall never decreases: the first index that reaches the point
    reached, first = first < n, first.clamp(max=n - 1)

    def eleven_point(curve):
        tail_max = torch.flip(torch.cummax(torch.flip(curve, [0]), 0).values, [0])
        return float(torch.where(reached, tail_max[first], torch.zeros_like(points)).sum() / 11)
    return eleven_point(precision), eleven_point(aos)


def _table(a, width, name):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    a = a.reshape(-1, width) if a.size == 0 else np.atleast_2d(a)
    if a.shape[1] != width:
        raise ValueError(f"{name}: {width} columns are needed, got {a.shape[1]}")
    return a


def _evaluation_set(gt, det):
    """The reference's bookkeeping of an evaluation set, for both metrics: ``gt`` and ``det`` rows whose column 0 is the frame
    number, ``det`` not empty -> ``(frames, det, det_ctr, gt, gt_ctr, n_frames)``, the rows kept and stably sorted by their frame
    counter ``0 .. n_frames - 1``, ``frames[counter]`` the frame number."""
    frames = np.unique(det[:, 0])               # the frames are those that HAVE detections (evaluateAPAOS.py:111, :123;
    det_ctr = np.searchsorted(frames, det[:, 0])                                          # evaluateDetection.py:30, :41-42)
    det = det[np.argsort(det_ctr, kind="stable")]
    det_ctr = np.sort(det_ctr)
    gt = gt[np.isin(gt[:, 0], frames)]          # ... so the ground truth of other frames does not count
    if gt.shape[0] == 0:                        # (the reference fails there on ``max`` of an empty array)
        raise ValueError("no ground truth in the frames that have detections")
    gt_ctr = np.searchsorted(frames, gt[:, 0])
    gt = gt[np.argsort(gt_ctr, kind="stable")]
    gt_ctr = np.sort(gt_ctr)
    n_frames = int(gt_ctr.max()) + 1            # the counters run to the last frame that has ground truth (evaluateAPAOS.py:10-12,
    det, det_ctr = det[det_ctr < n_frames], det_ctr[det_ctr < n_frames]     # CLEAR_MOD_HUN.py:29): later detections are dropped
    return frames, det, det_ctr, gt, gt_ctr, n_frames


def ap_aos(gt, det, thresholds=(0.75, 0.5, 0.25), device="cuda"):
    """AP and AOS of a detection set at each IoU threshold -> ``[(AP, AOS), ...]`` as fractions, one launch for all the IoUs.

    Arrays in the reference's text-file layout (evaluateAPAOS.py:121-122): ``gt`` rows ``frame x y z l w h rotation``, ``det`` rows
    ``frame x y z l w h rotation conf``.  The bookkeeping is the reference's: the frames are those that HAVE detections
    (:111, :123), ground truth of other frames does not count; several detections may match one ground truth; a detection is a
    true positive when its best IoU reaches the threshold.  Kept quirk: ``CLEAR_MOD_HUN2`` walks the frame counters up to the
    last frame that has ground truth (:10-12), so detections of later frames are dropped while frames in between that have
    detections and no ground truth count as false positives.  One deviation: the reference calls a detection a true positive when
    its row holds no -1 (:98), which also rejects a matched detection whose confidence or angle difference is exactly -1.0; here
    "has a match" decides."""
    thresholds = [float(t) for t in thresholds]
    if not thresholds or min(thresholds) <= 0 or any(t != t for t in thresholds):
        raise ValueError("ap_aos: IoU thresholds must be > 0 (one best match per detection serves every positive threshold only)")
    gt, det = _table(gt, 8, "gt"), _table(det, 9, "det")
    if det.shape[0] == 0:
        raise ValueError("detection is empty")
    _, det, det_ctr, gt, gt_ctr, n_frames = _evaluation_set(gt, det)
    dev = torch.device(device)
    best_idx, best_iou = match_frames(torch.from_numpy(det[:, 1:8]).to(dev), torch.from_numpy(det_ctr).to(dev),
                                      torch.from_numpy(gt[:, 1:8]).to(dev), torch.from_numpy(gt_ctr).to(dev), n_frames=n_frames)
    best_idx, best_iou = best_idx.cpu().numpy(), best_iou.cpu().numpy()
    gt_first = np.searchsorted(gt_ctr, det_ctr)                       # row of the frame's first ground truth
    gt_rot = gt[np.clip(gt_first + best_idx, 0, gt.shape[0] - 1), 7]
    out = []
    for t in thresholds:
        matched = (best_idx >= 0) & (best_iou >= np.float32(t))
        delta = np.where(matched, det[:, 7] - gt_rot, 0.0)
        out.append(ap_aos_from_matches(torch.from_numpy(det[:, 8].copy()), torch.from_numpy(matched), torch.from_numpy(delta),
                                       gt.shape[0]))
    return out


def evaluate_ap_aos(res_fpath, gt_fpath):
    """The reference's ``evaluateDetectionAPAOS(res_fpath, gt_fpath)`` (evaluateAPAOS.py:107-170): two text files ->
    ``(AP_75, AOS_75, OS_75, AP_50, AOS_50, OS_50, AP_25, AOS_25, OS_25)``, AP and AOS in per cent, OS = AOS / AP (NaN when AP is 0)."""
    gt_raw, det_raw = np.loadtxt(gt_fpath, ndmin=2), np.loadtxt(res_fpath, ndmin=2)
    assert det_raw.shape[0] != 0, "detection is empty"
    out = []
    for ap, aos in ap_aos(gt_raw, det_raw, (0.75, 0.5, 0.25)):
        out += [ap * 100, aos * 100, aos / ap if ap else float("nan")]
    return tuple(out)


HungarianTables = collections.namedtuple("HungarianTables", "gt_match gt_dist frame_counts frame_cost frame_status dist pair_begin")
CLEAR_MOD_MAX_SIDE = 512  # VFA_CLEAR_MOD_MAX_SIDE (include/vfa_hip.h)


def _xy_rows(t, name):
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{name} must be (n, 2) ground positions x y, got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def match_frames_hungarian(det_xy, det_frame, gt_xy, gt_frame, n_frames=None, td=30.0, with_matrix=False):
    """The match tables of the CLEAR-MOD metric for a whole evaluation set in one launch (``vfa_clear_mod_frames_f64``): per frame
    the distances, the reference's cost ``d > td -> 1e6`` and the minimum-cost assignment ``scipy.optimize.linear_sum_assignment``
    solves (``CLEAR_MOD_HUN.py:58-73``), one wave per frame.

    ``det_xy (P, 2)``, ``gt_xy (G, 2)`` ground positions (converted to float64, the reference's precision); ``det_frame (P)``,
    ``gt_frame (G)`` integer frame counters ``0 .. n_frames - 1``, each NON-DECREASING, with the conventions of ``match_frames``:
    ``n_frames`` given, nothing here waits for the device and the counters are not checked; ``None``, it is taken from the largest
    counter, which costs one host synchronisation that also checks the order.
    Returns ``HungarianTables``: ``gt_match (G)`` int32 -- index of the matched detection WITHIN ITS FRAME, -1 when unmatched;
    ``gt_dist (G)`` float64 -- its distance, +inf when unmatched (the reference's ``distances``); ``frame_counts (n_frames, 4)``
    int64 -- ground truths, detections, matches ``c``, pairs assigned at 1e6; ``frame_cost (n_frames)`` float64 -- sum of the
    assigned costs below 1e6; ``frame_status (n_frames)`` int32 -- 0, or 1 for a frame with more than ``CLEAR_MOD_MAX_SIDE``
    ground truths or detections (its rows are -1 / +inf, its counts 0).  A pair is a match when its assigned cost is ``< td``; a
    pair at exactly ``td`` competes in the assignment and is not a match (the reference's).  ``with_matrix=True`` also fills
    ``dist`` and ``pair_begin``: frame ``f``'s ``(G_f, P_f)`` matrix of distances is ``dist[pair_begin[f]:pair_begin[f + 1]]``,
    ground-truth-major like the reference's ``dist[o, e]`` (one more synchronisation, for its size)."""
    _lib.require_device(det_xy, det_frame, gt_xy, gt_frame)
    det_xy, gt_xy = _xy_rows(det_xy, "det_xy"), _xy_rows(gt_xy, "gt_xy")
    n_frames, det_begin, gt_begin, pair_begin, n_pairs = _frame_tables("match_frames_hungarian", det_frame, gt_frame, det_xy.shape[0],
                                                                       gt_xy.shape[0], n_frames, with_matrix, row="position")
    dev, G = det_xy.device, gt_xy.shape[0]
    gt_match = torch.full((G,), -1, dtype=torch.int32, device=dev)
    gt_dist = torch.full((G,), float("inf"), dtype=torch.float64, device=dev)
    frame_counts = torch.zeros((n_frames, 4), dtype=torch.int64, device=dev)
    frame_cost = torch.zeros(n_frames, dtype=torch.float64, device=dev)
    frame_status = torch.zeros(n_frames, dtype=torch.int32, device=dev)
    dist = torch.full((n_pairs,), float("nan"), dtype=torch.float64, device=dev) if with_matrix else None
    _lib.call("vfa_clear_mod_frames_f64", _lib.ptr(det_xy), _lib.ptr(det_begin), _lib.ptr(gt_xy), _lib.ptr(gt_begin), n_frames,
              det_xy.shape[0], G, float(td), _lib.ptr(pair_begin), n_pairs, _lib.ptr(dist), _lib.ptr(gt_match), _lib.ptr(gt_dist),
              _lib.ptr(frame_counts), _lib.ptr(frame_cost), _lib.ptr(frame_status), _lib.current_stream_handle())
    return HungarianTables(gt_match, gt_dist, frame_counts, frame_cost, frame_status, dist, pair_begin)


def clear_mod_totals(gt, det, td=30.0, device="cuda"):
    """The sums behind ``clear_mod`` -> ``(c, fp, m, g, distances)``: matches, false positives, misses and ground truths summed
    over the frames the reference walks, and the matched distances in (frame, ground truth) order.  Raises what ``clear_mod`` raises;
    ``det`` must not be empty."""
    gt, det = _table(gt, 3, "gt"), _table(det, 3, "det")
    if det.shape[0] == 0:
        raise ValueError("detection is empty")
    if not (np.isfinite(gt).all() and np.isfinite(det).all()):
        raise ValueError("clear_mod: frame numbers and coordinates must be finite")
    frames, det, det_ctr, gt, gt_ctr, n_frames = _evaluation_set(gt, det)
    sizes = np.maximum(np.bincount(det_ctr, minlength=n_frames), np.bincount(gt_ctr, minlength=n_frames))
    if sizes.max() > CLEAR_MOD_MAX_SIDE:
        worst = int(np.argmax(sizes))
        raise ValueError(f"clear_mod: frame {frames[worst]:g} has {sizes[worst]} ground truths or detections, more than the "
                         f"{CLEAR_MOD_MAX_SIDE} one wave solves")
    dev = torch.device(device)
    t = match_frames_hungarian(torch.from_numpy(det[:, 1:3]).to(dev), torch.from_numpy(det_ctr).to(dev),
                               torch.from_numpy(gt[:, 1:3]).to(dev), torch.from_numpy(gt_ctr).to(dev), n_frames=n_frames, td=td)
    counts, status, distances = t.frame_counts.cpu().numpy(), t.frame_status.cpu().numpy(), t.gt_dist.cpu().numpy()
    if status.any():
        raise _lib.VFAHipError(f"vfa_clear_mod_frames_f64: status {status.max()} in frame {frames[int(np.argmax(status))]:g}")
    g, n_det, c = (int(v) for v in counts[:, :3].sum(axis=0))
    return c, n_det - c, g - c, g, distances


def clear_mod(gt, det, td=30.0, device="cuda"):
    """The reference's ``CLEAR_MOD_HUN`` behind ``evaluateDetection_py`` -> ``(recall, precision, MODA, MODP)`` in per cent; the
    distances and the Hungarian assignment of every frame in one launch (``match_frames_hungarian``).

    ``gt`` and ``det``: arrays in the reference's text layout, rows ``frame x y``.  The bookkeeping is the reference's, quirks kept:
    * the frames are those that HAVE detections; ground truth of other frames does not count (``evaluateDetection.py:30, 41-42``);
    * the frame counters run to the last frame that has ground truth (``CLEAR_MOD_HUN.py:29``): detections of later frames are
      dropped, frames in between that have detections and no ground truth count as false positives;
    * per frame ``fp = n_det - c`` and ``m = g - c`` (``:92-93``); a pair at exactly ``td`` competes in the assignment and is not a
      match (``:69, :73``);
    * MODP is ``sum(1 - d / td)`` over the matched pairs, added in (frame, ground truth) order like the reference's builtin ``sum``,
      over ``sum(c)``, times 100 (``:94``); MODA ``(1 - (sum(m) + sum(fp)) / sum(g)) * 100``; recall ``sum(c) / sum(g) * 100``;
      precision ``sum(c) / (sum(fp) + sum(c)) * 100``;
    * every metric that is not ``> 0`` becomes 0 (``:94-99``), the 0 / 0 of a set without matches included (no numpy warning here).
    No detections: ``(0, 0, 0, 0)`` (``evaluateDetection.py:37-39``).  ``ValueError``: no ground truth in the frames that have
    detections (the reference fails there on ``max`` of an empty array), non-finite input, a frame with more than
    ``CLEAR_MOD_MAX_SIDE`` ground truths or detections (named in the message)."""
    if _table(det, 3, "det").shape[0] == 0:
        return 0, 0, 0, 0
    c, fp, m, g, distances = clear_mod_totals(gt, det, td, device)
    td = float(td)

    def positive(v):
        return v if v > 0 else 0
    modp = sum(1 - distances[distances < td] / td) / c * 100 if c else 0
    return positive(c / g * 100), positive(c / (fp + c) * 100), positive((1 - (m + fp) / g) * 100), positive(modp)


def evaluate_detection(res_fpath, gt_fpath, dataset_name=None):
    """The reference's ``evaluateDetection_py(res_fpath, gt_fpath, dataset_name)`` (``evaluateDetection.py:6-72``): two text files
    of rows ``frame x y`` -> ``(recall, precision, MODA, MODP)`` in per cent.  ``dataset_name`` is ignored, as the reference
    ignores it."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (loadtxt's "input contained no data" for an empty result file)
        gt_raw, det_raw = np.loadtxt(gt_fpath, ndmin=2), np.loadtxt(res_fpath, ndmin=2)
    if det_raw.shape[0] == 0 or det_raw.size == 0:
        return 0, 0, 0, 0
    return clear_mod(gt_raw[:, :3], det_raw[:, :3])


DECODE_MAX_TOPK = 1024  # VFA_BEV_DECODE_MAX_TOPK (include/vfa_hip.h)


def flat_detections(fused):
    """``BEVDecoder.decode_fused``'s result -> ``(rows, frame_index, n_frames)`` for ``match_frames`` /
    ``match_frames_hungarian`` with ``n_frames`` given: a batch goes from heads to match tables without the host seeing a count.

    The ``B * k`` rows are compacted on the device, shapes fixed: a stable sort by frame counter brings the detections to the front
    in (frame, rank) order; the unused rows follow with the counter ``n_frames = B``, which puts them behind the last frame's end
    in the offset tables both functions build, so neither reads them (``match_frames`` returns -1 / -1 for them).  ``rows``:
    ``conf (B k)``, ``location (B k, 3)``, ``cell (B k)``, ``xy (B k, 2)`` -- the ground positions ``match_frames_hungarian``
    takes -- and in 3D ``dimension``, ``rotation`` and ``box (B k, 7)`` = ``x y z l w h alpha``, the rows ``match_frames`` takes
    (the dimension reversed, as the reference writes its result file, evaluate.py:95-102)."""
    count, conf = fused["count"], fused["conf"]
    B, k = conf.shape
    rank = torch.arange(k, device=conf.device)
    frame = torch.arange(B, device=conf.device)[:, None].expand(B, k)
    frame_index = torch.where(rank[None, :] < count[:, None], frame, torch.full_like(frame, B)).reshape(-1)
    frame_index, order = torch.sort(frame_index, stable=True)
    rows = {name: fused[name].reshape(B * k, *fused[name].shape[2:])[order] for name in ("conf", "location", "cell", "dimension", "rotation")
            if name in fused}
    rows["xy"] = rows["location"][:, :2]
    if "dimension" in rows:
        rows["box"] = torch.cat([rows["location"], rows["dimension"].flip(-1), rows["rotation"][:, None]], dim=1)
    return rows, frame_index, B


class BEVDecoder:
    """``ObjectEncoder``'s decode half (encoder.py:230-305).  ``base`` is the dataset class name, ``world_size`` / ``cube_LWH``
    as in the dataset configs, ``dimension_mean`` = ``classAverage.get_mean(...)`` (3D only)."""

    def __init__(self, base, world_size, cube_LWH, dimension_mean=None, topk=100):
        self.base, self.topk = base, topk
        self.world_size = np.array(world_size)
        self.grid_size = self.world_size / np.array(cube_LWH)[:2]
        self.dimension_mean = dimension_mean

    def nms(self, heatmap):
        return bev_nms(heatmap)

    def _peaks(self, pred, conf=None):
        """``conf``: the NMS of the heatmap where the caller has it already (``decode_frames``); ``None``: ``self.nms(heatmap)``."""
        heatmap, tytx = pred["heatmap"], pred["loc_offset"]
        device, dtype = heatmap.device, heatmap.dtype
        conf = (self.nms(heatmap) if conf is None else conf).flatten(start_dim=2).transpose(1, 2)     # (1, L*W, 1)
        conf, _ = torch.max(conf, dim=-1)
        L, W = heatmap.shape[2:]
        grid_y, grid_x = torch.meshgrid(torch.arange(L, dtype=dtype, device=device), torch.arange(W, dtype=dtype, device=device),
                                        indexing="ij")
        tytx = torch.sigmoid(tytx)
        cy = (grid_y[None, ...] + tytx[..., 0]).flatten(start_dim=1) / self.grid_size[0] * self.world_size[0]
        cx = (grid_x[None, ...] + tytx[..., 1]).flatten(start_dim=1) / self.grid_size[1] * self.world_size[1]
        _, topk_index = torch.topk(conf, k=min(self.topk, conf.shape[1]), dim=1)
        return conf, cy, cx, topk_index

    def decode3d(self, pred, cls_thresh, *, conf=None):
        conf, cy, cx, topk_index = self._peaks(pred, conf)
        thtwtl, orient = pred["dim_offset"], pred["rotation"]
        mean = self.dimension_mean
        dims = [torch.exp(thtwtl[..., k]).flatten(start_dim=1) * mean[k] for k in range(3)]
        _, orient_idx = torch.max(torch.sigmoid(orient), dim=-1)
        orient_idx = orient_idx.flatten(start_dim=1)
        out = [torch.gather(x, dim=1, index=topk_index) for x in [conf, cy, cx, *dims, orient_idx]]
        mask = out[0] > cls_thresh
        return {"conf": out[0][mask],
                "location": torch.stack([out[2][mask], out[1][mask], torch.zeros_like(out[1][mask])], dim=-1),
                "dimension": torch.stack([out[3][mask], out[4][mask], out[5][mask]], dim=-1),
                "rotation": torch.deg2rad(out[6][mask].to(torch.float32))}

    def decode2d(self, pred, cls_thresh, *, conf=None):
        conf, cy, cx, topk_index = self._peaks(pred, conf)
        out = [torch.gather(x, dim=1, index=topk_index) for x in [conf, cy, cx]]
        mask = out[0] > cls_thresh
        first, second = (out[1], out[2]) if self.base == "Wildtrack" else (out[2], out[1])
        return {"conf": out[0][mask],
                "location": torch.stack([first[mask], second[mask], torch.zeros_like(out[1][mask])], dim=-1)}

    def batch_decode(self, pred, cls_thresh, *, conf=None):
        decode = self.decode3d if self.base in ("MultiviewC", "MVM3D") else self.decode2d
        return decode(pred, cls_thresh, conf=conf)

    def decode_frames(self, pred, cls_thresh):
        """A batch of B frames (every head (B, ...)) -> a list of B per-frame results, each what ``batch_decode`` gives for that
        frame alone; the NMS of all frames runs as one launch (``bev_nms_batch``)."""
        B = pred["heatmap"].shape[0]
        conf = bev_nms_batch(pred["heatmap"])
        return [self.batch_decode({k: v[b:b + 1] for k, v in pred.items()}, cls_thresh, conf=conf[b:b + 1]) for b in range(B)]

    def decode_fused(self, pred, cls_thresh):
        """A batch of B >= 1 frames (every head ``(B, ...)``) -> detections in tensors of a FIXED shape, in one library call
        (``vfa_bev_decode_f32``): nothing here waits for the device or reads a value back, so the call can be captured by
        ``torch.cuda.graph`` and its result handed on (``flat_detections``) without the host seeing a count.

        ``pred``: ``heatmap (B, 1, L, W)``, ``loc_offset (B, L, W, 2)`` and, for the 3D bases, ``dim_offset (B, L, W, 3)`` and
        ``rotation (B, L, W, R)``, float32; the three heads are read through their strides, so ``VFANet``'s ``permute(0, 2, 3, 1)``
        views and contiguous tensors are taken alike and never copied.  Returns, with ``k = min(topk, L * W)``: ``count (B)`` int32;
        ``conf (B, k)``; ``location (B, k, 3)``; ``cell (B, k)`` int32, the flat index ``l * W + w``; in 3D ``dimension (B, k, 3)``
        and ``rotation (B, k)``.  Frame ``b``'s detections are rows ``0 .. count[b] - 1``: those ``batch_decode`` gives for it (cells
        with ``conf > cls_thresh`` among the top k), by confidence descending, EQUAL confidences by ascending cell (``torch.topk``
        leaves that order open); the rows behind them are zeros with ``cell`` -1.  In place of ``rotation``, ``pred`` may carry
        ``rotation_head = (feature (B, C, L, W), weight (R, C, 3, 3), dilation)`` (``VFANet.heads(..., rotation_at="detections")``):
        the orientation head is then evaluated at the selected cells only (``vfa_conv3x3_at_cells_f32``, the same arg-max rule),
        still without a host wait or an allocation that depends on a value; every other output is unchanged.
        ``ValueError``: ``cls_thresh < 0`` (the equivalence with top-k-then-threshold needs it), ``topk`` outside 1 .. 1024, a 3D base
        without ``dimension_mean``."""
        three_d = self.base in ("MultiviewC", "MVM3D")
        if not float(cls_thresh) >= 0:
            raise ValueError(f"decode_fused: cls_thresh must be >= 0, got {cls_thresh}")
        if not 1 <= int(self.topk) <= DECODE_MAX_TOPK:
            raise ValueError(f"decode_fused: topk must be in 1 .. {DECODE_MAX_TOPK}, got {self.topk}")
        if three_d and self.dimension_mean is None:
            raise ValueError(f"decode_fused: base {self.base} decodes 3D boxes and needs dimension_mean")
        at_cells = three_d and "rotation_head" in pred and "rotation" not in pred
        names = ("heatmap", "loc_offset") + ((("dim_offset",) if at_cells else ("dim_offset", "rotation")) if three_d else ())
        _lib.require_device(*(pred[n] for n in names))
        heat = pred["heatmap"].to(torch.float32).contiguous()
        if heat.dim() != 4 or heat.shape[1] != 1:
            raise ValueError(f"decode_fused: heatmap must be (B, 1, L, W), got {tuple(heat.shape)}")
        B, _, L, W = heat.shape
        dev = heat.device

        def head(name, channels):
            t = pred[name]
            if t.dtype != torch.float32 or t.dim() != 4 or tuple(t.shape[:3]) != (B, L, W) or (channels and t.shape[3] != channels):
                raise ValueError(f"decode_fused: {name} must be float32 (B, L, W, {channels or 'R'}) = ({B}, {L}, {W}, ...), got "
                                 f"{t.dtype} {tuple(t.shape)}")
            return t, (ctypes.c_longlong * 4)(*t.stride())
        loc, loc_stride = head("loc_offset", 2)
        dim = rot = dim_stride = rot_stride = mean = None
        n_rot = 0
        if three_d:
            dim, dim_stride = head("dim_offset", 3)
            if at_cells:  # the library call decodes one zero logit read through zero strides; the rotation is written below
                rot, rot_stride, n_rot = torch.zeros(1, dtype=torch.float32, device=dev), (ctypes.c_longlong * 4)(0, 0, 0, 0), 1
            else:
                rot, rot_stride = head("rotation", 0)
                n_rot = rot.shape[3]
            if n_rot < 1:
                raise ValueError("decode_fused: rotation needs at least one channel")
            mean = (ctypes.c_float * 3)(*[float(m) for m in self.dimension_mean])
        k = min(int(self.topk), L * W)
        empty = B * L * W == 0
        out = {"count": torch.zeros(B, dtype=torch.int32, device=dev) if empty else torch.empty(B, dtype=torch.int32, device=dev),
               "conf": torch.empty((B, k), dtype=torch.float32, device=dev),
               "location": torch.empty((B, k, 3), dtype=torch.float32, device=dev),
               "cell": torch.empty((B, k), dtype=torch.int32, device=dev)}
        if three_d:
            out["dimension"] = torch.empty((B, k, 3), dtype=torch.float32, device=dev)
            out["rotation"] = torch.empty((B, k), dtype=torch.float32, device=dev)
        ws_bytes = _lib.lib().vfa_bev_decode_workspace_bytes(B, L, W, int(self.topk))
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        _lib.call("vfa_bev_decode_f32", _lib.ptr(heat), _lib.ptr(loc), loc_stride, _lib.ptr(dim), dim_stride, _lib.ptr(rot), rot_stride,
                  B, L, W, n_rot, int(self.topk), float(cls_thresh), float(self.grid_size[0]), float(self.grid_size[1]),
                  float(self.world_size[0]), float(self.world_size[1]), mean, int(self.base == "Wildtrack" and not three_d),
                  _lib.ptr(ws), ws_bytes, _lib.ptr(out["count"]), _lib.ptr(out["conf"]), _lib.ptr(out["location"]),
                  _lib.ptr(out["cell"]), _lib.ptr(out.get("dimension")), _lib.ptr(out.get("rotation")), _lib.current_stream_handle())
        if at_cells and not empty:
            feat, weight, dilation = pred["rotation_head"]
            if feat.dim() != 4 or (feat.shape[0], feat.shape[2], feat.shape[3]) != (B, L, W):
                raise ValueError(f"decode_fused: rotation_head's feature must be (B, C, L, W) = ({B}, C, {L}, {W}), got {tuple(feat.shape)}")
            out["rotation"] = ops.conv3x3_at_cells_forward(feat, weight, out["cell"], dilation, want_logits=False, want_rotation=True)[1]
        return out

    @staticmethod
    def split(fused):
        """``decode_fused``'s result -> a list of B per-frame dicts in ``batch_decode``'s format and dtypes (``conf (n)``,
        ``location (n, 3)``, in 3D ``dimension (n, 3)`` and ``rotation (n)``).  Reading the counts is the one host wait of the
        fused path."""
        keys = [k for k in ("conf", "location", "dimension", "rotation") if k in fused]
        return [{k: fused[k][b, :n] for k in keys} for b, n in enumerate(fused["count"].tolist())]
