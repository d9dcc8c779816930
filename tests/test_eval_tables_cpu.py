"""The host side of the evaluation path without a GPU (vfa_amd/eval_ops.py): the frame tables both match functions build from the
frame counters, on CPU tensors against literals; the reference's set bookkeeping as both metrics hand it to their match function,
recorded through stubs; ``BEVDecoder.decode_frames`` frame by frame against ``batch_decode`` with the NMS restated in torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vfa_amd import eval_ops


# ---- 1. the frame tables -----------------------------------------------------------------------------------------------------------

def _tables(det_frame, gt_frame, n_frames, with_matrix, who="match_frames", device="cpu"):
    det_frame, gt_frame = (torch.tensor(v, dtype=torch.int64, device=device) for v in (det_frame, gt_frame))
    return eval_ops._frame_tables(who, det_frame, gt_frame, det_frame.shape[0], gt_frame.shape[0], n_frames, with_matrix)


def _check(got, n_frames, det_begin, gt_begin, pair_begin, n_pairs):
    assert got[0] == n_frames and type(got[0]) is int
    assert got[1].dtype == torch.int32 and got[1].tolist() == det_begin
    assert got[2].dtype == torch.int32 and got[2].tolist() == gt_begin
    if pair_begin is None:
        assert got[3] is None
    else:
        assert got[3].dtype == torch.int64 and got[3].tolist() == pair_begin
    assert got[4] == n_pairs and type(got[4]) is int


def test_tables_of_the_empty_set():
    _check(_tables([], [], None, False), 0, [0], [0], None, 0)
    _check(_tables([], [], None, True), 0, [0], [0], [0], 0)


def test_tables_with_one_sided_frames():
    """Frame 1 has detections and no ground truth, frame 2 the converse; the frame count comes from the largest counter."""
    det, gt = [0, 0, 1, 1, 1, 3], [0, 2, 2, 3, 3]
    _check(_tables(det, gt, None, True), 4, [0, 2, 5, 5, 6], [0, 1, 1, 3, 5], [0, 2, 2, 2, 4], 4)
    _check(_tables(det, gt, None, False), 4, [0, 2, 5, 5, 6], [0, 1, 1, 3, 5], None, 0)
    _check(_tables(det[:5], gt[:3], None, True), 3, [0, 2, 5, 5], [0, 1, 1, 3], [0, 2, 2, 2], 2)
    _check(_tables([], [0, 1], None, True), 2, [0, 0, 0], [0, 1, 2], [0, 0, 0], 0)


def test_tables_with_a_leading_and_a_trailing_empty_frame():
    _check(_tables([1, 1, 2], [1, 2, 2], 4, True), 4, [0, 0, 2, 3, 3], [0, 0, 1, 3, 3], [0, 0, 2, 4, 4], 4)
    _check(_tables([1, 1, 2], [1, 2, 2], 4, False), 4, [0, 0, 2, 3, 3], [0, 0, 1, 3, 3], None, 0)


def test_counters_of_another_integer_type_are_taken():
    got = eval_ops._frame_tables("match_frames", torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1], dtype=torch.int16), 2, 1,
                                 None, True)
    _check(got, 2, [0, 1, 2], [0, 0, 1], [0, 0, 1], 1)


BAD_COUNTERS = [([1, 0], [0, 1]), ([0, 1], [2, 1]), ([-1, 0], [0]), ([0], [-2, 0])]


@pytest.mark.parametrize("det,gt", BAD_COUNTERS)
@pytest.mark.parametrize("who", ["match_frames", "match_frames_hungarian"])
def test_bad_counters_are_refused_in_the_callers_name_when_the_count_is_derived(det, gt, who):
    with pytest.raises(ValueError) as e:
        _tables(det, gt, None, False, who=who)
    assert str(e.value) == f"{who}: frame counters must be non-negative and sorted (non-decreasing)"


@pytest.mark.parametrize("det,gt", BAD_COUNTERS)
def test_given_frame_count_checks_nothing_and_reads_nothing_back(det, gt):
    """With ``n_frames`` given the counters are not checked, and no value leaves the device: tensors on the ``meta`` device hold
    no values, so an ``.item()`` / ``int()`` on that path would raise."""
    got = _tables(det, gt, 2, False)
    assert got[0] == 2 and got[1].shape == got[2].shape == (3,) and got[3] is None and got[4] == 0
    got = _tables(det, gt, 2, False, device="meta")
    assert got[0] == 2 and got[3] is None and got[4] == 0
    for begin in got[1:3]:
        assert begin.device.type == "meta" and begin.shape == (3,) and begin.dtype == torch.int32


def test_one_counter_per_row_is_needed():
    with pytest.raises(ValueError) as e:
        eval_ops._frame_tables("match_frames", torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 3, 1, 1, False)
    assert str(e.value) == "one frame counter per box is needed"
    with pytest.raises(ValueError) as e:
        eval_ops._frame_tables("match_frames_hungarian", torch.zeros(2, dtype=torch.int64), torch.zeros((1, 1), dtype=torch.int64),
                               2, 1, 1, False, row="position")
    assert str(e.value) == "one frame counter per position is needed"


# ---- 2. the set bookkeeping, as both metrics hand it on ----------------------------------------------------------------------------

DET = np.array([[7, 1, 1], [2.5, 2, 2], [11, 3, 3], [4, 4, 4], [2.5, 5, 5], [7, 6, 6]], dtype=np.float64)
GT = np.array([[9, 1, 0], [7, 2, 0], [2.5, 3, 0], [7, 4, 0], [1, 9, 9]], dtype=np.float64)
# recorded at the commit before the bookkeeping was stated once, by this stub: what both metrics handed on
WANT_DET_XY, WANT_DET_CTR = [[2, 2], [5, 5], [4, 4], [1, 1], [6, 6]], [0, 0, 1, 2, 2]
WANT_GT_XY, WANT_GT_CTR, WANT_N_FRAMES = [[3, 0], [2, 0], [4, 0]], [0, 2, 2], 3


def _record_calls(monkeypatch):
    calls = {}

    def match_frames(det, det_frame, gt, gt_frame, n_frames=None, with_matrix=False):
        calls["ap_aos"] = (det, det_frame, gt, gt_frame, n_frames, with_matrix)
        return torch.full((det.shape[0],), -1, dtype=torch.int32), torch.full((det.shape[0],), -1.0)

    def match_frames_hungarian(det_xy, det_frame, gt_xy, gt_frame, n_frames=None, td=30.0, with_matrix=False):
        calls["clear_mod"] = (det_xy, det_frame, gt_xy, gt_frame, n_frames, with_matrix)
        G = gt_xy.shape[0]
        return eval_ops.HungarianTables(torch.full((G,), -1, dtype=torch.int32), torch.full((G,), float("inf"), dtype=torch.float64),
                                        torch.zeros((n_frames, 4), dtype=torch.int64), torch.zeros(n_frames, dtype=torch.float64),
                                        torch.zeros(n_frames, dtype=torch.int32), None, None)
    monkeypatch.setattr(eval_ops, "match_frames", match_frames)
    monkeypatch.setattr(eval_ops, "match_frames_hungarian", match_frames_hungarian)
    return calls


def test_both_metrics_hand_on_the_same_frames_rows_and_counters(monkeypatch):
    """Unsorted rows, a non-integer frame number, ground truth in frames without detections (9 and 1), a frame with detections
    and no ground truth between frames that have both (4), a detection behind the last frame that has ground truth (11)."""
    calls = _record_calls(monkeypatch)
    det9 = np.column_stack([DET, np.full((len(DET), 5), 0.5), np.linspace(0.9, 0.4, len(DET))])   # frame x y | z l w h rotation | conf
    gt8 = np.column_stack([GT, np.full((len(GT), 5), 0.5)])
    assert eval_ops.ap_aos(gt8, det9, device="cpu") == [(0.0, 0.0)] * 3
    assert eval_ops.clear_mod_totals(GT, DET, device="cpu")[:4] == (0, 0, 0, 0)
    for name, width in (("ap_aos", 7), ("clear_mod", 2)):
        det, det_ctr, gt, gt_ctr, n_frames, with_matrix = calls[name]
        assert det.shape == (5, width) and gt.shape == (3, width) and det.dtype == gt.dtype == torch.float64, name
        assert det[:, :2].tolist() == WANT_DET_XY and det_ctr.tolist() == WANT_DET_CTR, name
        assert gt[:, :2].tolist() == WANT_GT_XY and gt_ctr.tolist() == WANT_GT_CTR, name
        assert det_ctr.dtype == gt_ctr.dtype == torch.int64 and n_frames == WANT_N_FRAMES and type(n_frames) is int, name
        assert with_matrix is False, name
        xy = det[:, :2].tolist()
        assert [3.0, 3.0] not in xy                                     # the detection of frame 11 is dropped
        assert [1.0, 0.0] not in gt[:, :2].tolist() and [9.0, 9.0] not in gt[:, :2].tolist()   # so is the ground truth of frames 9 and 1
        assert xy[det_ctr.tolist().index(1)] == [4.0, 4.0] and 1 not in gt_ctr.tolist()        # frame 4: its detection, no ground truth


def test_no_ground_truth_in_the_frames_that_have_detections(monkeypatch):
    _record_calls(monkeypatch)
    gt8 = np.column_stack([GT[[0, 4]], np.full((2, 5), 0.5)])
    det9 = np.column_stack([DET, np.full((len(DET), 6), 0.5)])
    for call in (lambda: eval_ops.ap_aos(gt8, det9, device="cpu"), lambda: eval_ops.clear_mod_totals(GT[[0, 4]], DET, device="cpu")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "no ground truth in the frames that have detections"


# ---- 3. decode_frames ---------------------------------------------------------------------------------------------------------------

def _torch_nms(heatmap):
    conf = torch.sigmoid(heatmap.to(torch.float32))
    return torch.where(conf == F.max_pool2d(conf, 5, stride=1, padding=2), conf, torch.zeros_like(conf))


def _heads(seed, three_d, B=3, L=6, W=7):
    g = torch.Generator().manual_seed(seed)
    pred = {"heatmap": torch.randn(B, 1, L, W, generator=g) * 2, "loc_offset": torch.randn(B, L, W, 2, generator=g)}
    if three_d:
        pred["dim_offset"] = torch.randn(B, L, W, 3, generator=g) * 0.1
        pred["rotation"] = torch.randn(B, L, W, 8, generator=g)
    return pred


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("base", ["MultiviewC", "Wildtrack", "MultiviewX"])
def test_decode_frames_is_batch_decode_of_every_frame_and_keeps_no_state(monkeypatch, base):
    three_d = base == "MultiviewC"
    dec = eval_ops.BEVDecoder(base, (39, 39), (0.5, 0.5, 1.0), dimension_mean=[1.5, 0.8, 2.0] if three_d else None, topk=10)
    pred, other = _heads(1, three_d), _heads(2, three_d)
    monkeypatch.setattr(eval_ops, "bev_nms", _torch_nms)
    monkeypatch.setattr(eval_ops, "bev_nms_batch", _torch_nms)
    alone = [dec.batch_decode({k: v[b:b + 1] for k, v in pred.items()}, 0.4) for b in range(3)]
    assert sum(len(f["conf"]) for f in alone) >= 6 and all(len(f["conf"]) < 10 for f in alone)  # the threshold cuts, not the top-k alone
    frames = dec.decode_frames(pred, 0.4)
    assert len(frames) == 3
    for got, want in zip(frames, alone):
        _same(got, want)
    assert not hasattr(dec, "_conf") and not hasattr(eval_ops.BEVDecoder, "_conf")

    # a second decode_frames on the same decoder from inside the first's NMS
    inner = []

    def nested_nms(heatmap):
        if not inner:
            inner.append(None)
            inner[0] = dec.decode_frames(other, 0.4)
        return _torch_nms(heatmap)
    monkeypatch.setattr(eval_ops, "bev_nms_batch", nested_nms)
    for got, want in zip(dec.decode_frames(pred, 0.4), alone):
        _same(got, want)
    for b, got in enumerate(inner[0]):
        _same(got, dec.batch_decode({k: v[b:b + 1] for k, v in other.items()}, 0.4))
    assert not hasattr(dec, "_conf") and not hasattr(eval_ops.BEVDecoder, "_conf")
