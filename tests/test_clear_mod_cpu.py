"""The CLEAR-MOD metric (MODA / MODP) without a GPU: the ABI of the new entry point; the assignment solver of
vfa_amd/csrc/vfa_assign.h (shared host / device code) compiled with g++ into tests/native/assign_harness.cpp and checked against
brute force and against scipy's per-frame records of tests/golden/clear_mod.npz (generated from the reference by
tests/golden/make_clear_mod.py), once more under the host sanitizers; the host-only branches of ``clear_mod``; the
``vfa.evaluation.pyeval.evaluateDetection`` alias; the refusals of the wrappers; the margins the fixture promises."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, golden_path
from native_common import build_harness, run_harness, write_checkout

TD = 30.0
SETS = ("demo1", "demo2", "syn")
GXX_FLAGS = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"]


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "assign", "assign_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "assign", "assign_harness.cpp", GXX_FLAGS, sanitized=True)


def _frames_file(path):
    """The per-frame records of the fixture as the flat file of doubles the harness reads."""
    d = np.load(golden_path("clear_mod.npz"))
    parts, n_frames = [], 0
    for name in SETS:
        gt, det, at = d[f"{name}_gt"], d[f"{name}_det"], 0
        for k, f in enumerate(d[f"{name}_frame_ids"]):
            g_xy, d_xy = gt[gt[:, 0] == f, 1:3], det[det[:, 0] == f, 1:3]
            g, n_det, c, _ = d[f"{name}_records"][k]
            assert (g, n_det) == (len(g_xy), len(d_xy))
            compare = bool(d[f"{name}_unique"][k]) and not bool(d[f"{name}_tied"][k])
            parts += [np.array([g, n_det, c, compare, d[f"{name}_cost_sum"][k], TD]), g_xy.ravel(), d_xy.ravel(),
                      d[f"{name}_gt_match"][at:at + len(g_xy)].astype(np.float64)]
            at += len(g_xy)
            n_frames += 1
        assert at == len(d[f"{name}_gt_match"])
    np.concatenate([np.array([float(n_frames)])] + parts).astype(np.float64).tofile(path)
    return n_frames


def test_entry_point_is_declared_exported_and_bound():
    """Declared, exported, bound, the same number of arguments: tests/test_abi.py, for every symbol.  Here: the cap is one number."""
    from vfa_amd import eval_ops
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    cap = int(re.search(r"#define\s+VFA_CLEAR_MOD_MAX_SIDE\s+(\d+)", text).group(1))
    solver = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_assign.h")).read()
    assert cap == eval_ops.CLEAR_MOD_MAX_SIDE == int(re.search(r"kMaxSide\s*=\s*(\d+)", solver).group(1)) == 512


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_solver_against_brute_force(harness, seed):
    """Every shape up to 7 x 7: optimal cost, a one-to-one table, no loop bound met; matrices with NaN / +inf return."""
    out = run_harness(harness, "brute", str(seed), "3920")
    finite, odd = (int(v) for v in re.findall(r"(\d+) (?:finite|with)", out))
    assert finite + odd == 3920 and finite >= 2900 and odd >= 500


def test_solver_against_scipy_records_of_the_fixture(harness, tmp_path):
    path = str(tmp_path / "frames.bin")
    n_frames = _frames_file(path)
    out = run_harness(harness, "frames", path)
    frames, stored, recomputed, compared = (int(v) for v in re.findall(r"\d+", out))
    assert frames == n_frames == 98 and stored >= 80 and recomputed >= 5 and compared >= 90
    run_harness(harness, "wide", "1")  # frames of the cap's size


def test_solver_under_the_host_sanitizers(sanitized_harness, tmp_path):
    run_harness(sanitized_harness, "brute", "4", "3920")
    path = str(tmp_path / "frames.bin")
    _frames_file(path)
    run_harness(sanitized_harness, "frames", path)
    run_harness(sanitized_harness, "wide", "2")


def test_clear_mod_host_only_branches():
    """What ``clear_mod`` decides before it touches the device."""
    from vfa_amd import eval_ops
    gt = np.array([[0, 1.0, 2.0], [2, 3.0, 4.0]])
    det = np.array([[0, 1.0, 2.5], [1, 7.0, 7.0]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert eval_ops.clear_mod(gt, np.zeros((0, 3))) == (0, 0, 0, 0)          # evaluateDetection.py:37-39
    with pytest.raises(ValueError, match="no ground truth"):
        eval_ops.clear_mod(np.array([[5, 1.0, 2.0]]), det)                       # ground truth only in a frame without detections
    with pytest.raises(ValueError, match="no ground truth"):
        eval_ops.clear_mod(np.zeros((0, 3)), det)
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            g, d = gt.copy(), det.copy()
            (g, d)[which][0, 2] = bad
            with pytest.raises(ValueError, match="finite"):
                eval_ops.clear_mod(g, d)
    with pytest.raises(ValueError, match="columns"):
        eval_ops.clear_mod(gt[:, :2], det)
    cap = eval_ops.CLEAR_MOD_MAX_SIDE
    many = np.column_stack([np.full(cap + 1, 7.0), np.arange(cap + 1.0), np.zeros(cap + 1)])
    with pytest.raises(ValueError, match="frame 7 "):
        eval_ops.clear_mod(np.array([[7, 0.0, 0.0]]), many)                      # too many detections
    with pytest.raises(ValueError, match="frame 7 "):
        eval_ops.clear_mod(many, np.array([[3, 0.0, 0.0], [7, 0.0, 0.0]]))       # too many ground truths


def test_evaluate_detection_of_an_empty_result_file(tmp_path):
    from vfa_amd import eval_ops
    res, gtf = tmp_path / "res.txt", tmp_path / "gt.txt"
    res.write_text("")
    gtf.write_text("0 1 2\n")
    assert eval_ops.evaluate_detection(str(res), str(gtf), "Wildtrack") == (0, 0, 0, 0)


CHECKOUT_FILES = {  # a stand-in for the reference checkout behind compat/ (native_common.write_checkout)
    "vfa/__init__.py": "",
    "vfa/evaluation/__init__.py": "",
    "vfa/evaluation/evaluate.py": "from .pyeval.evaluateDetection import evaluateDetection_py\n",
    "vfa/evaluation/pyeval/__init__.py": "",
    "vfa/evaluation/pyeval/evaluateDetection.py": "ORIGIN = 'checkout'\n\n\ndef evaluateDetection_py(a, b, c):\n    return ORIGIN\n",
    "vfa/evaluation/pyeval/CLEAR_MOD_HUN.py": "ORIGIN = 'checkout'\n",
}


@pytest.mark.parametrize("found_through", ["path", "VFA_REFERENCE_ROOT"])
def test_alias_binds_the_metric_and_leaves_clear_mod_hun_to_the_checkout(tmp_path, found_through):
    checkout = write_checkout(tmp_path / "checkout", CHECKOUT_FILES)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "compat"), REPO]))
    env.pop("VFA_REFERENCE_ROOT", None)
    if found_through == "path":
        env["PYTHONPATH"] += os.pathsep + checkout
    else:
        env["VFA_REFERENCE_ROOT"] = checkout
    code = (f"import vfa.evaluation.pyeval.evaluateDetection as m, vfa_amd.eval_ops as e; checkout = {checkout!r};"
            "assert m.evaluateDetection_py is e.evaluate_detection;"
            "import vfa.evaluation.pyeval.CLEAR_MOD_HUN as c, vfa.evaluation.evaluate as ev;"
            "assert c.__file__.startswith(checkout) and c.ORIGIN == 'checkout';"
            "assert ev.__file__.startswith(checkout) and ev.evaluateDetection_py is e.evaluate_detection; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_alias_resolves_without_a_checkout():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "compat"), REPO]))
    env.pop("VFA_REFERENCE_ROOT", None)
    code = ("from vfa.evaluation.pyeval.evaluateDetection import evaluateDetection_py as f; import vfa_amd.eval_ops as e;"
            "assert f is e.evaluate_detection; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_wrappers_refuse_cpu_tensors(built_lib):
    from vfa_amd import eval_ops
    from vfa_amd._lib import VFAHipError
    xy, frames = torch.ones(4, 2), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(VFAHipError):
        eval_ops.match_frames_hungarian(xy, frames, xy, frames, n_frames=1)
    with pytest.raises(VFAHipError):
        eval_ops.match_frames_hungarian(xy, frames, xy, frames)
    d = np.load(golden_path("clear_mod.npz"))
    with pytest.raises(VFAHipError):
        eval_ops.clear_mod(d["syn_gt"], d["syn_det"], device="cpu")


def test_fixture_keeps_its_margins():
    """The conditions tests/golden/make_clear_mod.py asserts, re-checked from the stored arrays."""
    d = np.load(golden_path("clear_mod.npz"))
    sizes = []
    for name in SETS:
        gt, det, records = d[f"{name}_gt"], d[f"{name}_det"], d[f"{name}_records"]
        at_td = 0
        for k, f in enumerate(d[f"{name}_frame_ids"]):
            g_xy, d_xy = gt[gt[:, 0] == f, 1:3], det[det[:, 0] == f, 1:3]
            assert (len(g_xy), len(d_xy)) == tuple(records[k, :2]) and 0 <= records[k, 2] <= min(records[k, :2])
            dx, dy = g_xy[:, None, 0] - d_xy[None, :, 0], g_xy[:, None, 1] - d_xy[None, :, 1]
            dist = np.sqrt(dx * dx + dy * dy)
            at_td += int((dist == TD).sum())
            integer = (g_xy == np.round(g_xy)).all() and (d_xy == np.round(d_xy)).all()
            if not integer and dist.size:
                assert np.abs(dist - TD).min() >= 1e-6      # margin: no float distance near td
            if name == "syn":
                sizes.append((len(g_xy), len(d_xy)))
                if integer and dist.size:
                    assert (dist == TD).sum() >= 4 and d["syn_cost_sum"][k] - records[k, 3] >= TD  # a pair at td is assigned
            # the cost sum holds the matched distances and the pairs at exactly td, nothing else
            at_td_assigned = (d[f"{name}_cost_sum"][k] - records[k, 3]) / TD
            assert at_td_assigned > -1e-9 and abs(at_td_assigned - round(at_td_assigned)) < 1e-9
        assert at_td >= 2                                    # the quirk at exactly td is live in each set
        c, fp, m, g = d[f"{name}_totals"]
        four = d[f"{name}_four"]
        assert np.allclose([c / g * 100, c / (fp + c) * 100, (1 - (m + fp) / g) * 100], four[:3], rtol=1e-12, atol=0)
        assert d[f"{name}_unique"].sum() >= 0.75 * len(records)
    assert d["demo1_unique"].all() and d["demo2_unique"].all()
    assert np.allclose(d["demo1_four"], [95.48319327731093, 94.09937888198758, 89.49579831932773, 83.27931600146269], rtol=1e-14, atol=0)
    assert np.allclose(d["demo2_four"], [91.17647058823529, 92.34042553191489, 83.61344537815127, 83.650244164872], rtol=1e-14, atol=0)
    for want in [(0, 0), (0, 5), (5, 0), (1, 1), (1, 70), (70, 1), (64, 65), (65, 64), (130, 70), (70, 130)]:
        assert want in sizes
    tied = d["syn_tied"]
    assert tied.sum() == 1 and not d["syn_unique"][tied].any() and d["syn_unique"][~tied].all()
    assert sizes[-1][0] == 0 and sizes[-2][0] == 0 and sizes[-1][1] > 0  # trailing frames: detections and no ground truth
    assert any(g > 0 and p > 0 and c == 0 for g, p, c, _ in d["syn_records"])  # the frame with every pair beyond td
    sq = ((d["near_td_det"] - d["near_td_gt"]) ** 2).sum(axis=1)
    assert (np.abs(sq - 900.0) <= 16 * np.spacing(900.0)).all() and (sq < 900).any() and (sq > 900).any() and (sq == 900).any()
