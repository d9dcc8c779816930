"""The fused BEV decode on the GPU (``BEVDecoder.decode_fused`` / ``split`` / ``flat_detections`` on ``vfa_bev_decode_f32``) against
the reference's recorded outputs, against ``batch_decode`` on the same device, and -- for the synthetic cases -- against the numpy
restatement of tests/decode_common.py, which tests/test_decode_fused_cpu.py pins to the reference's records.  Shapes are the smallest
that reach each way the kernel can go: fewer / more candidates than k, k = L * W, one / two / three counted index digits, a width that
is no multiple of the NMS tile, ties across the k-th place, a threshold at a cell's confidence, saturated rotation logits."""
import numpy as np
import pytest
import torch

import decode_common as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS_3D = ("conf", "location", "dimension", "rotation")


def _pred_of(d, three_d, device=DEV):
    pred = {"heatmap": torch.from_numpy(d["heatmap"]).to(device), "loc_offset": torch.from_numpy(d["loc_offset"]).to(device)}
    if three_d:
        pred["dim_offset"] = torch.from_numpy(d["dim_offset"]).to(device)
        pred["rotation"] = torch.from_numpy(d["rotation_logits"]).to(device)
    return pred


def _heads(seed, B, L, W, n_rot=0):
    """Seeded heads: a heat map of -20 (no candidate) for the test to put peaks into, random offsets."""
    g = torch.Generator().manual_seed(seed)
    pred = {"heatmap": torch.full((B, 1, L, W), -20.0), "loc_offset": torch.randn(B, L, W, 2, generator=g)}
    if n_rot:
        pred["dim_offset"] = torch.randn(B, L, W, 3, generator=g) * 0.3
        pred["rotation"] = torch.randn(B, L, W, n_rot, generator=g)      # (unsaturated: the top two sigmoids are far apart)
    return pred


def _decoder(L, W, three_d=False, topk=100, base=None):
    from vfa_amd import eval_ops
    base = base or ("MultiviewC" if three_d else "MultiviewX")
    return eval_ops.BEVDecoder(base, (L * 4, W * 4), (4, 4, 4), dimension_mean=np.array([140, 60, 230], np.float32), topk=topk)


def _check_against_restatement(dec, pred, thresh):
    """decode_fused on the device against the restatement fed with the device's own NMS: counts, cells and their order exactly, the
    confidences bit for bit those of ``bev_nms_batch``, the boxes at the tolerance of the fixture comparison."""
    from vfa_amd import eval_ops
    dpred = {k: v.to(DEV) for k, v in pred.items()}
    out = {k: v.cpu().numpy() for k, v in dec.decode_fused(dpred, thresh).items()}
    conf_maps = eval_ops.bev_nms_batch(dpred["heatmap"]).cpu().numpy()[:, 0]
    B, _, L, W = pred["heatmap"].shape
    three_d = "rotation" in out
    k = min(dec.topk, L * W)
    assert out["conf"].shape == (B, k) and out["location"].shape == (B, k, 3) and out["cell"].shape == (B, k)
    assert out["count"].dtype == np.int32 and out["cell"].dtype == np.int32 and out["conf"].dtype == np.float32
    wants = []
    for b in range(B):
        want = dc.restate(conf_maps[b], pred["loc_offset"][b].numpy(), thresh, dec.topk, dec.grid_size, dec.world_size,
                          yx_first=dec.base == "Wildtrack" and not three_d, dim=pred["dim_offset"][b].numpy() if three_d else None,
                          rot=pred["rotation"][b].numpy() if three_d else None, mean=dec.dimension_mean)
        n = len(want["cell"])
        assert out["count"][b] == n, (b, out["count"][b], n)
        assert np.array_equal(out["cell"][b, :n], want["cell"]), b
        assert np.array_equal(out["conf"][b, :n].view(np.uint32), conf_maps[b].ravel()[want["cell"]].view(np.uint32)), b
        for key in ("location",) + (("dimension", "rotation") if three_d else ()):
            np.testing.assert_allclose(out[key][b, :n], want[key], rtol=1e-5, atol=1e-5, err_msg=f"{key} of frame {b}")
            assert not out[key][b, n:].any(), f"{key}: rows behind frame {b}'s count are not zero"
        assert not out["conf"][b, n:].any() and (out["cell"][b, n:] == -1).all()
        wants.append(want)
    return out, wants


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.FIXTURES)
def test_fixture_through_decode_fused_and_split(name):
    from vfa_amd import eval_ops
    d, three_d = dc.load(name)
    dec = dc.decoder_of(d)
    pred = _pred_of(d, three_d)
    fused = dec.decode_fused(pred, dc.THRESH)
    frames = dec.split(fused)
    eager = dec.batch_decode(pred, dc.THRESH)
    assert len(frames) == 1 and int(fused["count"][0]) == len(d["out_conf"]) == (36 if three_d else 100)
    got = {k: v.cpu().numpy() for k, v in frames[0].items()}
    keys = KEYS_3D if three_d else KEYS_3D[:2]
    assert tuple(got) == keys
    order_got = dc.by_conf_x_y(got["conf"], got["location"])
    order_ref = dc.by_conf_x_y(d["out_conf"], d["out_location"])
    e = {k: v.cpu().numpy() for k, v in eager.items()}
    order_eager = dc.by_conf_x_y(e["conf"], e["location"])
    for k in keys:
        assert got[k].shape == d["out_" + k].shape == e[k].shape and got[k].dtype == e[k].dtype == np.float32, k
        np.testing.assert_allclose(got[k][order_got], d["out_" + k][order_ref], rtol=1e-5, atol=1e-5, err_msg=k + " (recorded)")
        np.testing.assert_allclose(got[k][order_got], e[k][order_eager], rtol=1e-5, atol=1e-5, err_msg=k + " (batch_decode)")
    # the confidences are bev_nms's, bit for bit, at the cells the call names; the order is the promised one
    nms = eval_ops.bev_nms(pred["heatmap"]).cpu().numpy().ravel()
    n = len(got["conf"])
    cell = fused["cell"][0, :n].cpu().numpy()
    assert np.array_equal(got["conf"].view(np.uint32), nms[cell].view(np.uint32))
    want = dc.restate_fixture(d, conf_map=nms.reshape(d["nms"].shape[2:]))
    assert np.array_equal(cell, want["cell"])
    if three_d:
        assert np.array_equal(np.round(np.rad2deg(got["rotation"])).astype(np.int64), want["rot_index"])


# ---- 2. layouts -------------------------------------------------------------------------------------------------------------------

def test_permuted_nchw_views_give_the_bits_of_contiguous_heads_and_are_not_copied(monkeypatch):
    from vfa_amd import _lib
    d, _ = dc.load("decode_mc.npz")
    dec = dc.decoder_of(d)
    pred = _pred_of(d, True)
    views = dict(pred)
    for k in ("loc_offset", "dim_offset", "rotation"):
        views[k] = pred[k].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)      # NCHW storage, the view VFANet returns
        assert not views[k].is_contiguous() and views[k].stride(3) == 24 * 30
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (seen.append((name, args)), real(name, *args))[1])
    a, b = dec.decode_fused(pred, dc.THRESH), dec.decode_fused(views, dc.THRESH)
    assert [name for name, _ in seen] == ["vfa_bev_decode_f32"] * 2                   # one library call each
    assert seen[0][1][5].value == pred["rotation"].data_ptr() and seen[1][1][5].value == views["rotation"].data_ptr()
    assert sorted(a) == sorted(b) == ["cell", "conf", "count", "dimension", "location", "rotation"]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["count"][0]) == 36


# ---- 3. batch ---------------------------------------------------------------------------------------------------------------------

def test_batch_of_three_frames_each_equals_its_single_frame_decode():
    d, _ = dc.load("decode_mc.npz")
    dec = dc.decoder_of(d)
    L, W = 24, 30
    pred = _heads(5, 3, L, W, n_rot=360)
    for k, src in (("heatmap", "heatmap"), ("loc_offset", "loc_offset"), ("dim_offset", "dim_offset"), ("rotation", "rotation_logits")):
        pred[k][0] = torch.from_numpy(d[src][0])
    pred["heatmap"][2] = 0.0                                                            # constant: every cell a candidate at 0.5
    out, _ = _check_against_restatement(dec, pred, dc.THRESH)
    assert out["count"].tolist() == [36, 0, 100]
    assert np.array_equal(out["cell"][2], np.arange(100)) and (out["conf"][2] == 0.5).all()
    assert (out["cell"][1] == -1).all() and not out["conf"][1].any() and not out["location"][1].any()
    assert not out["dimension"][1].any() and not out["rotation"][1].any()
    singles = [dec.decode_fused({k: v[b:b + 1].to(DEV) for k, v in pred.items()}, dc.THRESH) for b in range(3)]
    for b in range(3):
        for k in out:
            assert np.array_equal(out[k][b], singles[b][k][0].cpu().numpy()), (b, k)
    # a peak in the last rows of frame 0 (and of frame 1) changes neither frame 1 nor frame 2
    pred["heatmap"][0, 0, L - 1, W - 1] = 9.0
    pred["heatmap"][0, 0, L - 2, W - 4] = 8.0
    pred["heatmap"][1, 0, L - 1, 0] = 7.0
    again = {k: v.cpu().numpy() for k, v in dec.decode_fused({k: v.to(DEV) for k, v in pred.items()}, dc.THRESH).items()}
    assert again["count"][1:].tolist() == [1, 100] and L * W - 1 in again["cell"][0] and again["cell"][1, 0] == (L - 1) * W
    for k in out:
        assert np.array_equal(again[k][2], out[k][2]), k
        if k != "count":
            assert np.array_equal(again[k][1, 1:], out[k][1, 1:]), k


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------

def _scatter_peaks(heat, rng, step=3):
    """Distinct logits on a lattice `step` apart (each its own 5 x 5 maximum only where it beats its neighbours), random elsewhere."""
    L, W = heat.shape
    heat[:] = torch.from_numpy(rng.uniform(-3.0, 3.0, (L, W)).astype(np.float32))
    return heat


@pytest.mark.parametrize("L,W,topk,three_d", [(3, 5, 100, True), (9, 33, 100, False), (9, 33, 1, True), (9, 33, 7, False),
                                              (40, 63, 100, True)])
def test_small_and_odd_grids_against_the_restatement(L, W, topk, three_d):
    """3 x 5 with topk = 100: k = 15 = every cell; 9 x 33: a width that is no multiple of the 32-wide NMS tile; topk = 1; random
    maps, both above and below k candidates (thresholds 0 and 0.4), a Wildtrack decoder for the swapped location."""
    rng = np.random.default_rng(L * 1000 + W + topk)
    pred = _heads(L + W + topk, 2, L, W, n_rot=360 if three_d else 0)
    for b in range(2):
        _scatter_peaks(pred["heatmap"][b, 0], rng)
    for thresh in (0.0, 0.4, 0.9):
        out, _ = _check_against_restatement(_decoder(L, W, three_d, topk), pred, thresh)
        assert (out["count"] <= min(topk, L * W)).all()
    if not three_d:
        _check_against_restatement(_decoder(L, W, False, topk, base="Wildtrack"), pred, 0.4)
    pred["heatmap"][0] = 1.5                                                            # constant: count = k, cells 0 .. k - 1
    out, _ = _check_against_restatement(_decoder(L, W, three_d, topk), pred, 0.4)
    k = min(topk, L * W)
    assert out["count"][0] == k and np.array_equal(out["cell"][0], np.arange(k))


def test_three_index_digits_and_the_full_sort():
    """260 x 260 = 67 600 cells (a third counted index digit) with topk = 1024 (the whole bitonic network): a constant map selects
    cells 0 .. 1023; a random map goes against the restatement."""
    L = W = 260
    pred = _heads(11, 2, L, W)
    pred["heatmap"][0] = 0.25
    _scatter_peaks(pred["heatmap"][1, 0], np.random.default_rng(12))
    out, _ = _check_against_restatement(_decoder(L, W, False, 1024), pred, 0.5)
    assert out["count"].tolist() == [1024, 1024] and np.array_equal(out["cell"][0], np.arange(1024))


def _lattice_map(L, W, logits, cells):
    heat = torch.full((1, 1, L, W), -20.0)
    for (l, w), v in zip(cells, logits):
        heat[0, 0, l, w] = v
    return heat


def test_equal_confidences_across_the_kth_place_follow_the_stable_order():
    L, W = 9, 33
    cells = [(1, 2), (1, 27), (4, 7), (4, 20), (7, 2), (7, 14), (7, 30)]
    logits = [2.0, 1.0, 3.0, 2.5, 1.0, 0.5, 1.0]            # 3.0 > 2.5 > 2.0 > a plateau of three at 1.0 > 0.5
    pred = _heads(21, 1, L, W)
    pred["heatmap"] = _lattice_map(L, W, logits, cells)
    plateau = [1 * W + 27, 7 * W + 2, 7 * W + 30]           # ascending cell index
    for topk, want_tail in ((4, plateau[:1]), (5, plateau[:2]), (6, plateau), (3, [])):
        out, _ = _check_against_restatement(_decoder(L, W, False, topk), pred, 0.4)
        assert out["count"][0] == topk
        assert out["cell"][0].tolist() == [4 * W + 7, 4 * W + 20, 1 * W + 2] + want_tail


def test_threshold_at_a_cells_confidence_excludes_it():
    from vfa_amd import eval_ops
    L, W = 9, 33
    cells = [(1, 2), (1, 27), (4, 7), (4, 20), (7, 2)]
    pred = _heads(22, 1, L, W)
    pred["heatmap"] = _lattice_map(L, W, [2.0, 1.0, 3.0, 0.3, -0.2], cells)
    conf = eval_ops.bev_nms_batch(pred["heatmap"].to(DEV)).cpu().numpy()[0, 0]
    at = float(conf[1, 27])                                   # the float32 value itself, as a Python float
    assert np.float32(at) == conf[1, 27] and 0.7 < at < 0.74
    out, _ = _check_against_restatement(_decoder(L, W), pred, at)
    assert out["count"][0] == 2 and out["cell"][0, :2].tolist() == [4 * W + 7, 1 * W + 2]
    out, _ = _check_against_restatement(_decoder(L, W), pred, float(np.nextafter(np.float32(at), np.float32(0))))
    assert out["count"][0] == 3 and out["cell"][0, 2] == 1 * W + 27


def test_saturated_rotation_logits_tie_at_the_first_index():
    L, W = 9, 33
    cells = [(1, 2), (4, 7), (7, 20)]
    pred = _heads(23, 1, L, W, n_rot=360)
    pred["heatmap"] = _lattice_map(L, W, [3.0, 2.0, 1.0], cells)
    pred["rotation"][0, 1, 2, [250, 100, 17, 359]] = 30.0     # sigmoid = 1.0f at four angles: the first wins
    pred["rotation"][0, 4, 7, :] = 40.0                       # every angle saturated: index 0
    pred["rotation"][0, 7, 20, :] = -5.0
    pred["rotation"][0, 7, 20, 359] = 29.0                    # the last angle alone
    out, wants = _check_against_restatement(_decoder(L, W, True), pred, 0.4)
    assert wants[0]["rot_index"].tolist() == [17, 0, 359]
    assert np.array_equal(out["rotation"][0, :3], wants[0]["rotation"]) and abs(out["rotation"][0, 2] - np.deg2rad(359.0)) < 1e-5


def test_nan_and_infinite_logits_end_and_stay_inside_the_frame():
    """Not-a-number heat is no candidate, +Inf is confidence 1, -Inf is 0; a cell whose rotation logits are all NaN gets index 0."""
    L, W = 9, 33
    pred = _heads(24, 2, L, W, n_rot=360)
    _scatter_peaks(pred["heatmap"][1, 0], np.random.default_rng(3))
    pred["heatmap"][0, 0, 4, 7] = float("inf")
    pred["heatmap"][0, 0, 4, 20] = float("nan")
    pred["heatmap"][0, 0, 1, 2] = float("-inf")
    pred["heatmap"][0, 0, 7, 2] = 2.0
    pred["rotation"][0, 4, 7, :] = float("nan")
    dec = _decoder(L, W, True)
    out = {k: v.cpu().numpy() for k, v in dec.decode_fused({k: v.to(DEV) for k, v in pred.items()}, 0.4).items()}
    assert out["count"][0] == 2 and out["cell"][0, :2].tolist() == [4 * W + 7, 7 * W + 2] and out["conf"][0, 0] == 1.0
    assert out["rotation"][0, 0] == 0.0 and (out["cell"][0, 2:] == -1).all()
    single = dec.decode_fused({k: v[1:2].to(DEV) for k, v in pred.items()}, 0.4)
    for k in out:
        assert np.array_equal(out[k][1], single[k][0].cpu().numpy()), k


# ---- 5. graph ---------------------------------------------------------------------------------------------------------------------

def test_decode_fused_is_captured_and_replayed_on_new_heads():
    d, _ = dc.load("decode_mc.npz")
    dec = dc.decoder_of(d)
    static = _pred_of(d, True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            dec.decode_fused(static, dc.THRESH)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        captured = dec.decode_fused(static, dc.THRESH)
    graph.replay()
    first = {k: v.clone() for k, v in captured.items()}
    eager = dec.decode_fused(static, dc.THRESH)
    for k in eager:
        assert torch.equal(first[k], eager[k]), k
    assert int(first["count"][0]) == 36
    second = _heads(31, 1, 24, 30, n_rot=360)
    _scatter_peaks(second["heatmap"][0, 0], np.random.default_rng(32))
    for k in static:
        static[k].copy_(second[k].to(DEV))
    graph.replay()
    eager = dec.decode_fused({k: v.to(DEV) for k, v in second.items()}, dc.THRESH)
    for k in eager:
        assert torch.equal(captured[k], eager[k]), k
    assert 0 < int(captured["count"][0]) <= 100 and not torch.equal(captured["cell"], first["cell"])


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from vfa_amd._lib import VFAHipError
    d, _ = dc.load("decode_mc.npz")
    pred = _pred_of(d, True)
    with pytest.raises(ValueError):
        dc.decoder_of(d).decode_fused(pred, -0.01)
    with pytest.raises(ValueError):
        dc.decoder_of(d, topk=1025).decode_fused(pred, 0.4)
    with pytest.raises(ValueError):
        dc.decoder_of(d, with_mean=False).decode_fused(pred, 0.4)
    with pytest.raises(VFAHipError):
        dc.decoder_of(d).decode_fused(_pred_of(d, True, device="cpu"), 0.4)
    with pytest.raises(VFAHipError):
        dc.decoder_of(d).decode_fused(dict(pred, rotation=pred["rotation"].cpu()), 0.4)
    assert int(dc.decoder_of(d, topk=1024).decode_fused(pred, 0.4)["count"][0]) == 36     # the largest topk is taken


# ---- heads to match tables without the host seeing a count --------------------------------------------------------------------

def test_flat_detections_feed_the_match_tables():
    from vfa_amd import eval_ops
    d, _ = dc.load("decode_wt.npz")
    dec = dc.decoder_of(d)
    one = _pred_of(d, False)
    pred = {k: torch.cat([v, torch.full_like(v, -20.0), v]) for k, v in one.items()}
    pred["heatmap"][2, 0, :15] = -20.0                                                   # frame 2: the lower half only
    fused = dec.decode_fused(pred, dc.THRESH)
    rows, frame_index, n_frames = eval_ops.flat_detections(fused)
    frames = dec.split(fused)
    counts = [len(f["conf"]) for f in frames]
    assert counts[0] == 100 and counts[1] == 0 and 0 < counts[2] <= 100 and n_frames == 3
    gt_xy = torch.cat([f["location"][:, :2] + 1.0 for f in frames])
    gt_frame = torch.cat([torch.full((n,), b, dtype=torch.int64, device=DEV) for b, n in enumerate(counts)])
    t = eval_ops.match_frames_hungarian(rows["xy"], frame_index, gt_xy, gt_frame, n_frames=n_frames)
    assert t.frame_counts[:, :3].tolist() == [[n, n, n] for n in counts] and not t.frame_status.any()
    assert t.gt_match.tolist() == list(range(counts[0])) + list(range(counts[2]))
    np.testing.assert_allclose(t.gt_dist.cpu().numpy(), np.sqrt(2.0), rtol=1e-3)
    # 3D: every box against a copy of itself moved by 5 (identical rectangles are the reference IoU's degenerate case)
    d, _ = dc.load("decode_mc.npz")
    dec = dc.decoder_of(d)
    one = _pred_of(d, True)
    pred = {k: torch.cat([torch.full_like(v, -20.0), v]) for k, v in one.items()}
    fused = dec.decode_fused(pred, dc.THRESH)
    rows, frame_index, n_frames = eval_ops.flat_detections(fused)
    gt = rows["box"][:36].clone()
    gt[:, :2] += 5.0
    best_idx, best_iou = eval_ops.match_frames(rows["box"], frame_index, gt, torch.ones(36, dtype=torch.int64, device=DEV),
                                               n_frames=n_frames)
    assert best_idx[:36].tolist() == list(range(36)) and (best_idx[36:] == -1).all() and (best_iou[36:] == -1).all()
    assert (best_iou[:36] > 0.6).all() and (best_iou[:36] < 1.0).all()
