"""The AP/AOS metric on the MI355X (-m gpu): the fused rotated-box IoU kernels against float64 truths and the reference's recorded
numbers (tests/golden/iou3d_pairs.npz, tests/golden/ap_aos_mc.npz; generated from the reference by tests/golden/make_ap_aos.py).

Bound on an IoU, a derivation and not a measurement: the project allows the overlap area of the reference pipeline an error of
1e-4 x the larger box area (tests/test_eval_ops.py::_check_overlaps); d iou / d overlap = (a1 + a2) / union^2 <= 2 / max(a1, a2),
so the IoU may be off by 2e-4.  The 3D IoU is the BEV overlap times a z term that is exact to fp32 rounding over a union that
is at least the larger volume: the same derivation with volumes for areas."""
import numpy as np
import pytest
import torch

from conftest import golden_path

pytestmark = pytest.mark.gpu

IOU_BOUND = 2e-4
THRESHOLDS = (0.75, 0.5, 0.25)


def _dev():
    return torch.device("cuda:0")


def _pairs():
    d = np.load(golden_path("iou3d_pairs.npz"))
    return d, torch.from_numpy(d["box1"]).to(_dev()), torch.from_numpy(d["box2"]).to(_dev())


def _set():
    d = np.load(golden_path("ap_aos_mc.npz"))
    dev = _dev()
    det_frame = np.repeat(np.arange(len(d["det_begin"]) - 1), np.diff(d["det_begin"]))
    gt_frame = np.repeat(np.arange(len(d["gt_begin"]) - 1), np.diff(d["gt_begin"]))
    return (d, torch.from_numpy(d["det_boxes"]).to(dev), torch.from_numpy(det_frame).to(dev), torch.from_numpy(d["gt_boxes"]).to(dev),
            torch.from_numpy(gt_frame).to(dev))


def test_iou3d_meets_the_float64_truth():
    from vfa_amd import eval_ops
    d, b1, b2 = _pairs()
    got = eval_ops.iou3d(b1.view(1, -1, 7), b2.view(1, -1, 7))
    assert got.shape == (1, len(d["kind"])) and got.dtype == torch.float32
    got = got[0].cpu().numpy().astype(np.float64)
    bev = eval_ops.iou_bev(b1[:, [0, 1, 3, 4, 6]], b2[:, [0, 1, 3, 4, 6]]).cpu().numpy().astype(np.float64)
    kind = d["kind"]
    for k in dict.fromkeys(kind.tolist()):
        sel = kind == k
        print(f"{k:13s}: max |BEV - truth| {np.abs(bev - d['iou_bev'])[sel].max():.2e}, max |3D - truth| {np.abs(got - d['iou3d'])[sel].max():.2e}, "
              f"max |3D - reference's fp32| {np.abs(got - d['ref_iou3d'])[sel].max():.2e}")
    assert not np.isnan(got).any() and not np.isnan(bev).any()
    assert (np.abs(bev - d["iou_bev"]) <= IOU_BOUND).all()
    up = d["z_overlap"] > 0
    assert up.sum() > 150 and (np.abs(got - d["iou3d"])[up] <= IOU_BOUND).all()
    assert (got[kind == "disjoint"] == 0.0).all() and (bev[kind == "disjoint"] == 0.0).all()
    assert (np.abs(got[kind == "identical"] - 1) <= IOU_BOUND).all() and (np.abs(bev[kind == "identical"] - 1) <= IOU_BOUND).all()
    apart = kind == "z_apart"
    assert (got[apart] < 0).all() and (d["ref_iou3d"][apart] < 0).all()
    assert (np.abs(got - d["iou3d"])[apart] <= IOU_BOUND).all()  # (the reference's sign and size there, not only its sign)


def test_iou3d_batches_are_the_pairs_one_at_a_time():
    from vfa_amd import eval_ops
    d, b1, b2 = _pairs()
    n = len(d["kind"])
    assert n % 64 != 0 and n == 6 * 36  # (blocks of 64 lanes: a ragged last block)
    batch = eval_ops.iou3d(b1.view(6, 36, 7), b2.view(6, 36, 7))
    assert batch.shape == (6, 36)
    single = torch.stack([eval_ops.iou3d(b1[k].view(1, 1, 7), b2[k].view(1, 1, 7)).reshape(()) for k in range(n)])
    assert torch.equal(batch.reshape(-1).view(torch.int32), single.view(torch.int32))
    flat = eval_ops.iou3d(b1, b2)
    assert flat.shape == (n,) and torch.equal(flat.view(torch.int32), single.view(torch.int32))
    # more than one block with a ragged tail; the tail lanes of the last block write nothing
    reps = torch.cat([b1] * 3)[:600], torch.cat([b2] * 3)[:600]
    many = eval_ops.iou3d(*reps)
    assert torch.equal(many.view(torch.int32), torch.cat([single] * 3)[:600].view(torch.int32))
    bev_batch = eval_ops.iou_bev(b1[:, [0, 1, 3, 4, 6]].view(6, 36, 5), b2[:, [0, 1, 3, 4, 6]].view(6, 36, 5))
    assert bev_batch.shape == (6, 36)
    # empty input
    empty = torch.zeros(0, 4, 7, device=_dev())
    assert eval_ops.iou3d(empty, empty).shape == (0, 4)
    assert eval_ops.iou3d_matrix(empty[:, 0], b2).shape == (0, n) and eval_ops.iou3d_matrix(b1, empty[:, 0]).shape == (n, 0)
    with pytest.raises(ValueError):
        eval_ops.iou3d(b1, b2[:5])


def _torch_iou3d(box1, box2, sort_v):
    """TEST CODE: the steps of the reference's IoU3D as batched torch ops, box1, box2 (n, 7) -> (iou3d, iou_bev, overlap), with the
    stand-alone ``sort_v`` kernel for the vertex ordering (vertices (1, n, 24, 2), mask, num_valid -> (1, n, 9))."""
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


def test_fused_ordering_is_the_ordering_of_sort_v():
    """The shared device code was not mis-compiled when inlined into the larger kernel: the 24 candidates built with torch ops on
    the device (``_torch_iou3d`` above, test code), ordered by the
    stand-alone ``sort_v`` kernel, shoelace in torch -- against the overlap of the fused kernel (iou_bev x union)."""
    from vfa_amd import eval_ops
    d, b1, b2 = _pairs()
    want_vol, want_bev, want_overlap = (t.cpu().numpy().astype(np.float64) for t in _torch_iou3d(b1, b2, eval_ops.sort_v))
    bev = eval_ops.iou_bev(b1[:, [0, 1, 3, 4, 6]], b2[:, [0, 1, 3, 4, 6]]).cpu().numpy().astype(np.float64)
    vol = eval_ops.iou3d(b1, b2).cpu().numpy().astype(np.float64)
    a1, a2 = d["box1"][:, 3].astype(np.float64) * d["box1"][:, 4], d["box2"][:, 3].astype(np.float64) * d["box2"][:, 4]
    overlap = bev * (a1 + a2) / (1 + bev)  # iou = overlap / (a1 + a2 - overlap)
    print(f"max |overlap - sort_v composition| / larger area {(np.abs(overlap - want_overlap) / np.maximum(a1, a2)).max():.2e}, "
          f"max |BEV IoU diff| {np.abs(bev - want_bev).max():.2e}, max |3D IoU diff| {np.abs(vol - want_vol).max():.2e}")
    sure = np.isin(d["kind"], ["identical", "contained", "cows_cm", "z_equal", "z_partial", "z_apart"])
    assert (want_overlap[sure] > 0).all() and (want_overlap > 0).sum() > 150  # the composition itself saw polygons
    assert (np.abs(overlap - want_overlap) <= 1e-4 * np.maximum(a1, a2)).all()
    assert (np.abs(bev - want_bev) <= IOU_BOUND).all() and (np.abs(vol - want_vol) <= IOU_BOUND).all()


def test_matrices_and_best_matches_are_the_references():
    from vfa_amd import eval_ops
    d, det, det_frame, gt, gt_frame = _set()
    det_begin, gt_begin, pair_begin = d["det_begin"], d["gt_begin"], d["pair_begin"]
    n_frames = len(det_begin) - 1
    best_idx, best_iou, iou, pb = eval_ops.match_frames(det, det_frame, gt, gt_frame, with_matrix=True)
    assert np.array_equal(pb.cpu().numpy(), pair_begin)
    iou = iou.cpu().numpy()
    print(f"max |IoU - reference's| over {len(iou)} pairs: {np.abs(iou - d['iou']).max():.2e}")
    assert iou.shape == d["iou"].shape and (np.abs(iou - d["iou"]) <= IOU_BOUND).all()
    for f in range(n_frames):  # the per-frame matrix entry point gives the same numbers
        m = eval_ops.iou3d_matrix(det[det_begin[f]:det_begin[f + 1]], gt[gt_begin[f]:gt_begin[f + 1]])
        assert m.shape == (det_begin[f + 1] - det_begin[f], gt_begin[f + 1] - gt_begin[f])
        assert np.array_equal(m.cpu().numpy().reshape(-1), iou[pair_begin[f]:pair_begin[f + 1]])
    best_idx, best_iou = best_idx.cpu().numpy(), best_iou.cpu().numpy()
    assert best_idx.dtype == np.int32 and best_idx.shape == (det_begin[-1],)
    for t, key in zip(THRESHOLDS, ("rows_75", "rows_50", "rows_25")):
        rows = d[key]
        mine = np.where(best_iou >= np.float32(t), best_idx, -1)
        assert np.array_equal(mine, rows[:, 1].astype(np.int64)), t
        hit = mine >= 0
        assert (np.abs(best_iou[hit] - rows[hit, 2]) <= IOU_BOUND).all()
    empty = [f for f in range(n_frames) if gt_begin[f + 1] == gt_begin[f] and det_begin[f + 1] > det_begin[f]]
    assert empty
    for f in empty:  # a frame without ground truth
        assert (best_idx[det_begin[f]:det_begin[f + 1]] == -1).all() and (best_iou[det_begin[f]:det_begin[f + 1]] == -1).all()

    # NaN: a detection with a NaN field has a NaN row and no match; a NaN ground truth never wins; other rows are unaffected
    f = next(f for f in range(n_frames) if gt_begin[f + 1] - gt_begin[f] >= 3 and det_begin[f + 1] - det_begin[f] >= 3)
    bad_det, bad_gt = det.clone(), gt.clone()
    row = int(det_begin[f]) + 1
    bad_det[row, 3] = float("nan")
    col = int(best_idx[det_begin[f]])  # the ground truth the frame's first detection is matched to ...
    other = [p for p in range(det_begin[f], det_begin[f + 1]) if p != row]
    bi, bv, m, _ = eval_ops.match_frames(bad_det, det_frame, gt, gt_frame, n_frames=n_frames, with_matrix=True)
    bi, bv, m = bi.cpu().numpy(), bv.cpu().numpy(), m.cpu().numpy()
    G = gt_begin[f + 1] - gt_begin[f]
    nan_row = slice(pair_begin[f] + (row - det_begin[f]) * G, pair_begin[f] + (row - det_begin[f] + 1) * G)
    assert np.isnan(m[nan_row]).all() and bi[row] == -1 and bv[row] == -1
    keep = np.ones(len(m), bool)
    keep[nan_row] = False
    assert np.array_equal(m[keep], iou[keep]) and np.array_equal(np.delete(bi, row), np.delete(best_idx, row))
    bad_gt[int(gt_begin[f]) + col, 6] = float("nan")  # ... becomes NaN: the detection falls back to its next best, or to none
    bi2, bv2 = (t.cpu().numpy() for t in eval_ops.match_frames(det, det_frame, bad_gt, gt_frame, n_frames=n_frames))
    first = int(det_begin[f])
    rest = np.delete(iou[pair_begin[f]:pair_begin[f] + G], col)
    assert bi2[first] != col and not np.isnan(bv2[first]) and bv2[first] == rest.max()
    assert bi2[first] == int(np.flatnonzero(iou[pair_begin[f]:pair_begin[f] + G] == rest.max())[0])
    outside = np.ones(len(bi2), bool)
    outside[det_begin[f]:det_begin[f + 1]] = False
    assert np.array_equal(bi2[outside], best_idx[outside]) and np.array_equal(bv2[outside], best_iou[outside])
    assert other


def test_ap_aos_returns_the_reference_numbers(tmp_path):
    from vfa_amd import eval_ops
    d = np.load(golden_path("ap_aos_mc.npz"))
    nine = d["nine"]
    got = eval_ops.ap_aos(d["gt"], d["det"])
    flat = [v for ap, aos in got for v in (ap * 100, aos * 100, aos / ap)]
    np.savetxt(tmp_path / "gt.txt", d["gt"])
    np.savetxt(tmp_path / "det.txt", d["det"])
    from_files = eval_ops.evaluate_ap_aos(str(tmp_path / "det.txt"), str(tmp_path / "gt.txt"))
    assert isinstance(from_files, tuple) and len(from_files) == 9
    for name, mine in (("ap_aos", flat), ("evaluate_ap_aos", from_files)):
        print(name, [f"{v:.10f}" for v in mine], "reference", [f"{v:.10f}" for v in nine])
        assert (np.abs(np.array(mine) - nine) <= 1e-9 * np.abs(nine)).all(), name
    # rows in another order in the files: the metric sorts by frame itself, and keeps the order within a frame
    order = np.argsort(-d["det"][:, 0], kind="stable")
    shuffled = eval_ops.ap_aos(d["gt"][::-1], d["det"][order])
    for (ap, aos), k in zip(shuffled, range(3)):
        # (reversed ground truths renumber the matches, not the metric; sums may run in another order)
        assert abs(ap * 100 - nine[3 * k]) <= 1e-9 * nine[3 * k] and abs(aos * 100 - nine[3 * k + 1]) <= 1e-9 * nine[3 * k + 1]
    one = eval_ops.ap_aos(torch.from_numpy(d["gt"]), torch.from_numpy(d["det"]), thresholds=(0.5,))
    assert len(one) == 1 and one[0] == got[1]


def test_fused_best_match_equals_the_matrix_form_bit_for_bit():
    from vfa_amd import eval_ops
    d, det, det_frame, gt, gt_frame = _set()
    n_frames = len(d["det_begin"]) - 1
    fused_idx, fused_iou = eval_ops.match_frames(det, det_frame, gt, gt_frame, n_frames=n_frames)
    idx, val, iou, _ = eval_ops.match_frames(det, det_frame, gt, gt_frame, n_frames=n_frames, with_matrix=True)
    assert torch.equal(fused_idx, idx) and torch.equal(fused_iou.view(torch.int32), val.view(torch.int32))
    # ... and derived from the matrix on the host: the lowest-index maximum of every row
    m, want_idx, want_val = iou.cpu().numpy(), [], []
    for f in range(n_frames):
        P, G = d["det_begin"][f + 1] - d["det_begin"][f], d["gt_begin"][f + 1] - d["gt_begin"][f]
        rows = m[d["pair_begin"][f]:d["pair_begin"][f + 1]].reshape(P, G)
        want_idx += [int(np.argmax(r)) if G else -1 for r in rows] if G else [-1] * P
        want_val += [r.max() for r in rows] if G else [np.float32(-1)] * P
    assert np.array_equal(fused_idx.cpu().numpy(), np.array(want_idx, np.int32))
    assert np.array_equal(fused_iou.cpu().numpy().view(np.int32), np.array(want_val, np.float32).view(np.int32))
    again_idx, again_iou = eval_ops.match_frames(det, det_frame, gt, gt_frame)  # (n_frames from the counters: the same table)
    assert torch.equal(again_idx, fused_idx) and torch.equal(again_iou.view(torch.int32), fused_iou.view(torch.int32))
    with pytest.raises(ValueError):
        eval_ops.match_frames(det, det_frame.flip(0), gt, gt_frame)


def test_one_launch_serves_the_set(monkeypatch):
    """``match_frames`` issues the same number of library calls for one frame as for the whole set, repeated four times over."""
    from vfa_amd import _lib, eval_ops
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    d, det, det_frame, gt, gt_frame = _set()
    n_frames = len(d["det_begin"]) - 1
    counts = []
    one_det, one_gt = int(d["det_begin"][1]), int(d["gt_begin"][1])
    eval_ops.match_frames(det[:one_det], det_frame[:one_det], gt[:one_gt], gt_frame[:one_gt], n_frames=1)
    counts.append(len(calls))
    eval_ops.match_frames(det, det_frame, gt, gt_frame, n_frames=n_frames)
    counts.append(len(calls) - sum(counts))
    big = [torch.cat([t + k * n_frames if t.dtype == torch.int64 else t for k in range(4)]) for t in (det, det_frame, gt, gt_frame)]
    best_idx, _ = eval_ops.match_frames(*big, n_frames=4 * n_frames)
    counts.append(len(calls) - sum(counts))
    assert counts == [1, 1, 1] and set(calls) == {"vfa_iou3d_frames_f32"}
    single, _ = eval_ops.match_frames(det, det_frame, gt, gt_frame, n_frames=n_frames)
    assert torch.equal(best_idx, torch.cat([single] * 4))
    calls.clear()
    eval_ops.ap_aos(d["gt"], d["det"])  # three thresholds, one launch
    assert calls == ["vfa_iou3d_frames_f32"]
