"""The AP/AOS metric without a GPU (the ABI of its entry points: tests/test_abi.py): the float64 tail of the metric against the reference's
recorded match tables (tests/golden/ap_aos_mc.npz, generated from the reference by tests/golden/make_ap_aos.py), the margins the
fixtures promise, the ``vfa.evaluation.pyeval.evaluateAPAOS`` alias and the refusals of the host wrappers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_path
from native_common import write_checkout

THRESHOLDS = (0.75, 0.5, 0.25)


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


def test_ap_aos_tail_reproduces_the_reference_from_its_match_rows():
    """``ap_aos_from_matches`` fed with the rows the reference's ``cal_frame_TPFP_iou`` produced (confidence, TP flag, angle
    difference) gives the AP and AOS of the reference's ``CLEAR_MOD_HUN2``: float64 sums of a few hundred terms of order one, so
    1e-12 relative leaves room for the order of summation only."""
    from vfa_amd import eval_ops
    d = np.load(golden_path("ap_aos_mc.npz"))
    nine = d["nine"]
    for k, key in enumerate(("rows_75", "rows_50", "rows_25")):
        rows = d[key]
        ap, aos = eval_ops.ap_aos_from_matches(torch.from_numpy(rows[:, 0].copy()), torch.from_numpy(rows[:, 4] == 1),
                                               torch.from_numpy(rows[:, 3].copy()), int(d["n_gt"]))
        print(f"threshold {THRESHOLDS[k]}: AP {ap * 100:.12f} (reference {nine[3 * k]:.12f}), AOS {aos * 100:.12f} "
              f"(reference {nine[3 * k + 1]:.12f})")
        assert abs(ap * 100 - nine[3 * k]) <= 1e-12 * abs(nine[3 * k])
        assert abs(aos * 100 - nine[3 * k + 1]) <= 1e-12 * abs(nine[3 * k + 1])
        assert abs(aos / ap - nine[3 * k + 2]) <= 1e-12 * abs(nine[3 * k + 2])
    assert 5 < nine[0] < nine[3] < nine[6] < 95  # the set separates the thresholds


def test_ap_aos_tail_on_hand_made_tables():
    """A table small enough to do by hand: 4 detections in confidence order TP FP TP TP, 5 ground truths."""
    from vfa_amd import eval_ops
    ap, aos = eval_ops.ap_aos_from_matches(torch.tensor([.6, .9, .7, .8]), torch.tensor([True, True, True, False]),
                                           torch.tensor([np.pi, 0.0, 0.0, 123.0]), 5)
    # precision 1, 1/2, 2/3, 3/4; recall .2 .2 .4 .6.  Points 0 .1 .2 -> 1; .3 .4 -> 3/4 (tail from index 2); .5 -> 3/4; the point
    # "0.6" of arange(0, 1.1, 0.1) is 0.6000000000000001 > 3/5: not reached, like every later one -> 0
    assert ap == pytest.approx((3 * 1 + 3 * 0.75) / 11, rel=1e-14)
    # running similarity 1, 1/2, 2/3, 2/4 (the last match is turned by pi: (1 + cos pi) / 2 = 0)
    assert aos == pytest.approx((3 * 1 + 2 * (2 / 3) + 0.5) / 11, rel=1e-14)
    assert eval_ops.ap_aos_from_matches(torch.zeros(0), torch.zeros(0, dtype=torch.bool), torch.zeros(0), 3) == (0.0, 0.0)
    with pytest.raises(ValueError):  # recall is TP / n_gt
        eval_ops.ap_aos_from_matches(torch.tensor([.5]), torch.tensor([True]), torch.tensor([0.0]), 0)


def test_fixtures_keep_their_margins():
    """The conditions tests/golden/make_ap_aos.py asserts, re-checked from the stored arrays: no IoU near a threshold, no near-tie
    for the best match, distinct confidences, no exact -1.0 in a matched row, and the reference itself within the project's
    bound of the float64 truth on every stored pair."""
    d = np.load(golden_path("ap_aos_mc.npz"))
    iou, det_begin, gt_begin, pair_begin = d["iou"], d["det_begin"], d["gt_begin"], d["pair_begin"]
    assert len(iou) == pair_begin[-1] and len(iou) > 300
    assert min(np.abs(iou - t).min() for t in THRESHOLDS) >= 1e-3
    contested = 0
    for f in range(len(det_begin) - 1):
        P, G = det_begin[f + 1] - det_begin[f], gt_begin[f + 1] - gt_begin[f]
        assert pair_begin[f + 1] - pair_begin[f] == P * G
        if P and G >= 2:
            m = np.sort(iou[pair_begin[f]:pair_begin[f + 1]].reshape(P, G), axis=1)
            close = m[:, -2] >= 0.2
            contested += int(close.sum())
            assert ((m[:, -1] - m[:, -2])[close] >= 1e-3).all()
    assert contested >= 1
    det, gt = d["det"], d["gt"]
    assert len(np.unique(det[:, 8])) == len(det)
    for key in ("rows_75", "rows_50", "rows_25"):
        rows = d[key]
        matched = rows[:, 1] >= 0
        assert len(rows) == det_begin[-1] and 0 < matched.sum() < len(rows)
        assert not (rows[matched][:, [0, 3]] == -1.0).any() and np.array_equal(rows[:, 4] == 1, matched)
    # the shape of the set: frame numbers with gaps, a frame with detections and no ground truth among the walked ones, ground
    # truth in a frame without detections, detections after the last frame that has ground truth
    det_frames, gt_frames = np.unique(det[:, 0]), np.unique(gt[:, 0])
    assert (np.diff(det_frames) > 1).any() and set(gt_frames) - set(det_frames)
    assert any(det_begin[f + 1] > det_begin[f] and gt_begin[f + 1] == gt_begin[f] for f in range(len(det_begin) - 1))
    assert det_frames.max() > gt_frames.max() and det_begin[-1] < len(det)
    assert int(d["n_gt"]) == gt_begin[-1] == int(np.isin(gt[:, 0], det_frames).sum()) < len(gt)

    p = np.load(golden_path("iou3d_pairs.npz"))
    kinds = set(p["kind"].tolist())
    assert {"random", "identical", "contained", "disjoint", "cows_cm", "z_equal", "z_partial", "z_apart", "axis_aligned"} <= kinds
    area = np.maximum(p["box1"][:, 3] * p["box1"][:, 4], p["box2"][:, 3] * p["box2"][:, 4]).astype(np.float64)
    a1 = p["box1"][:, 3].astype(np.float64) * p["box1"][:, 4]
    a2 = p["box2"][:, 3].astype(np.float64) * p["box2"][:, 4]
    ref_bev = p["ref_iou_bev"].astype(np.float64)
    ref_overlap = ref_bev * (a1 + a2) / (1 + ref_bev)  # overlap / (a1 + a2 - overlap) = iou
    assert (np.abs(ref_overlap - p["overlap"]) <= 1e-4 * area).all()
    assert (np.abs(ref_bev - p["iou_bev"]) <= 1e-4).all()
    up = p["z_overlap"] > 0
    assert (np.abs(p["ref_iou3d"][up] - p["iou3d"][up]) <= 1e-4).all()
    apart = p["kind"] == "z_apart"
    assert (p["z_overlap"][apart] < 0).all() and (p["ref_iou3d"][apart] < 0).all() and (p["iou3d"][apart] < 0).all()
    assert (p["ref_iou3d"][p["kind"] == "disjoint"] == 0).all() and np.isfinite(p["ref_iou3d"]).all()


CHECKOUT_FILES = {  # a stand-in for the reference checkout behind compat/ (native_common.write_checkout)
    "vfa/__init__.py": "",
    "vfa/evaluation/__init__.py": "",
    "vfa/evaluation/evaluate.py": "from .pyeval.evaluateAPAOS import evaluateDetectionAPAOS\n",
    "vfa/evaluation/pyeval/__init__.py": "",
    "vfa/evaluation/pyeval/evaluateAPAOS.py": "ORIGIN = 'checkout'\n\n\ndef evaluateDetectionAPAOS(a, b):\n    return ORIGIN\n",
    "vfa/evaluation/pyeval/CLEAR_MOD_HUN.py": "ORIGIN = 'checkout'\n",
    "vfa/evaluation/pyeval/cuda_op/__init__.py": "",
    "vfa/evaluation/pyeval/cuda_op/cuda_ext.py": "import sort_vertices\n\nbound = sort_vertices.sort_vertices_forward\n",
    "vfa/evaluation/pyeval/IoU.py": "from .cuda_op.cuda_ext import bound\n",
}


@pytest.mark.parametrize("found_through", ["path", "VFA_REFERENCE_ROOT"])
def test_evaluation_alias_binds_the_metric_and_leaves_the_rest_to_the_checkout(tmp_path, found_through):
    checkout = write_checkout(tmp_path / "checkout", CHECKOUT_FILES)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "compat"), REPO]))
    env.pop("VFA_REFERENCE_ROOT", None)
    if found_through == "path":
        env["PYTHONPATH"] += os.pathsep + checkout
    else:
        env["VFA_REFERENCE_ROOT"] = checkout
    code = (f"import vfa.evaluation.pyeval.evaluateAPAOS as m, vfa_amd.eval_ops as e; checkout = {checkout!r};"
            "assert m.evaluateDetectionAPAOS is e.evaluate_ap_aos;"
            "import vfa.evaluation.pyeval.IoU as i, vfa.evaluation.pyeval.CLEAR_MOD_HUN as c, vfa.evaluation.evaluate as ev;"
            "assert i.__file__.startswith(checkout) and i.bound is e.sort_vertices and c.ORIGIN == 'checkout';"
            "assert ev.__file__.startswith(checkout) and ev.evaluateDetectionAPAOS is e.evaluate_ap_aos; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_evaluation_alias_resolves_without_a_checkout():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "compat"), REPO]))
    env.pop("VFA_REFERENCE_ROOT", None)
    code = ("from vfa.evaluation.pyeval.evaluateAPAOS import evaluateDetectionAPAOS as f; import vfa_amd.eval_ops as e;"
            "assert f is e.evaluate_ap_aos; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_kernel_wrappers_refuse_cpu_tensors(built_lib):
    from vfa_amd import eval_ops
    from vfa_amd._lib import VFAHipError
    b7, b5 = torch.ones(2, 3, 7), torch.ones(4, 5)
    frames = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(VFAHipError):
        eval_ops.iou3d(b7, b7)
    with pytest.raises(VFAHipError):
        eval_ops.iou_bev(b5, b5)
    with pytest.raises(VFAHipError):
        eval_ops.iou3d_matrix(b7[0], b7[1])
    with pytest.raises(VFAHipError):
        eval_ops.match_frames(b7.reshape(6, 7), frames, b7.reshape(6, 7), frames, n_frames=1)
    d = np.load(golden_path("ap_aos_mc.npz"))
    with pytest.raises(VFAHipError):
        eval_ops.ap_aos(d["gt"], d["det"], device="cpu")


def test_ap_aos_refuses_thresholds_that_are_not_positive():
    from vfa_amd import eval_ops
    d = np.load(golden_path("ap_aos_mc.npz"))
    for bad in ((0.5, 0.0), (-0.25,), (), (float("nan"),)):
        with pytest.raises(ValueError):
            eval_ops.ap_aos(d["gt"], d["det"], thresholds=bad)
    with pytest.raises(ValueError):
        eval_ops.ap_aos(d["gt"], np.zeros((0, 9)))
