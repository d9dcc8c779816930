"""The fused BEV decode without a GPU: the ABI of the new entry points; the selection logic of vfa_amd/csrc/vfa_decode.h (shared host /
device code) compiled with g++ into tests/native/decode_select_harness.cpp and checked against std::sort, once more under the host
sanitizers; the numpy restatement of tests/decode_common.py against the reference's recorded outputs (tests/golden/decode_*.npz); the
margins of those fixtures that make the comparison on the GPU unambiguous; the refusals and the host-side helpers of the wrapper."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import decode_common as dc
from native_common import build_harness, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"]


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "decode_select", "decode_select_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "decode_select", "decode_select_harness.cpp", GXX_FLAGS, sanitized=True)


def test_entry_points_are_declared_exported_and_bound():
    """Declared, exported, bound, the same number of arguments: tests/test_abi.py, for every symbol.  Here: the cap is one number."""
    from vfa_amd import eval_ops
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    cap = int(re.search(r"#define\s+VFA_BEV_DECODE_MAX_TOPK\s+(\d+)", text).group(1))
    shared = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_decode.h")).read()
    assert cap == eval_ops.DECODE_MAX_TOPK == int(re.search(r"kMaxTopk\s*=\s*(\d+)", shared).group(1)) == 1024


def test_workspace_size_and_the_refusals_of_the_entry_point(built_lib):
    """What the call decides before it launches anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_bev_decode_workspace_bytes(8, 120, 360, 100) == 8 * 120 * 360 * 4
    assert lib.vfa_bev_decode_workspace_bytes(0, 120, 360, 100) == 0 and lib.vfa_bev_decode_workspace_bytes(1, 0, 5, 100) == 0
    stride = (ctypes.c_longlong * 4)(0, 0, 0, 0)
    mean = (ctypes.c_float * 3)(1, 1, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)

    def call(B=1, L=4, W=4, n_rot=0, topk=100, thresh=0.4, heat=p, loc=p, loc_stride=stride, dim=None, rot=None, ws=p, ws_bytes=64,
             count=p):
        return lib.vfa_bev_decode_f32(heat, loc, loc_stride, dim, stride, rot, stride, B, L, W, n_rot, topk, thresh, 1.0, 1.0, 1.0, 1.0,
                                      mean, 0, ws, ws_bytes, count, p, p, p, p, p, None)
    BAD, UNSUPPORTED = 10001, 10002
    assert call(B=-1) == BAD and call(L=-1) == BAD and call(W=-2) == BAD and call(topk=0) == BAD and call(topk=-3) == BAD
    assert call(thresh=-0.1) == BAD and call(thresh=float("nan")) == BAD
    assert call(heat=None) == BAD and call(loc=None) == BAD and call(loc_stride=None) == BAD and call(count=None) == BAD
    assert call(ws=None) == BAD and call(ws_bytes=63) == BAD
    assert call(dim=p, n_rot=360) == BAD and call(rot=p, n_rot=360) == BAD      # one 3D head without the other
    assert call(dim=p, rot=p, n_rot=0) == BAD
    assert call(topk=1025) == UNSUPPORTED and call(B=65536, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(B=0) == 0 and call(L=0) == 0 and call(W=0, topk=1025) == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_selection_against_std_sort(harness, seed):
    """0 candidates, fewer than k, exactly k, all equal, ties across the k-th place, k = 1, k = 1024 of 1025, 70 000 cells, and 300
    random frames: the selected keys and their order are std::sort's."""
    out = run_harness(harness, "cases", str(seed))
    passes, early, deep = (int(v) for v in re.findall(r"(\d+) (?:passes|selects|went)", out))
    assert passes > early > 100 and deep >= 20


def test_key_packing(harness):
    run_harness(harness, "keys")


def test_selection_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "keys")
    run_harness(sanitized_harness, "cases", "4")


@pytest.mark.parametrize("name", dc.FIXTURES)
def test_restatement_reproduces_the_reference_outputs(name):
    """Confidences from the recorded NMS, a stable arg-sort, the box arithmetic in float32 -> the reference's recorded detections at
    the tolerance tests/test_eval_ops.py compares the decode at."""
    d, three_d = dc.load(name)
    got = dc.restate_fixture(d)
    order_got, order_ref = dc.by_conf_x_y(got["conf"], got["location"]), dc.by_conf_x_y(d["out_conf"], d["out_location"])
    for k in ("conf", "location") + (("dimension", "rotation") if three_d else ()):
        assert got[k].shape == d["out_" + k].shape and got[k].dtype == d["out_" + k].dtype, k
        np.testing.assert_allclose(got[k][order_got], d["out_" + k][order_ref], rtol=1e-5, atol=1e-5, err_msg=k)
    assert (np.diff(got["conf"]) <= 0).all() and len(set(got["cell"].tolist())) == len(got["cell"])


def test_fixtures_have_no_tie_at_the_100th_place():
    """More than 100 candidates in the two 2D fixtures, 36 in the 3D one, and a gap between the 100th and the 101st confidence: the
    selected SET does not depend on how ties are broken."""
    want = {"decode_wt.npz": (0.8548, 0.8343), "decode_mx.npz": (0.8528, 0.8520)}
    for name in dc.FIXTURES:
        d, _ = dc.load(name)
        conf = np.sort(d["nms"].ravel())[::-1]
        n_cand = int((conf > np.float32(dc.THRESH)).sum())
        if name == "decode_mc.npz":
            assert n_cand == 36 == len(d["out_conf"])
            continue
        assert n_cand > 100 and len(d["out_conf"]) == 100
        assert conf[99] > conf[100] > dc.THRESH
        np.testing.assert_allclose([conf[99], conf[100]], want[name], rtol=0, atol=5e-5)


def test_rotation_argmax_of_the_fixture_has_a_margin():
    """At every MultiviewC peak the two largest rotation sigmoids are thousands of ulps apart: the arg-max does not hang on the last
    bit of expf."""
    d, _ = dc.load("decode_mc.npz")
    got = dc.restate_fixture(d)
    l, w = got["cell"] // d["nms"].shape[3], got["cell"] % d["nms"].shape[3]
    s = np.sort(dc.sigmoid32(d["rotation_logits"][0][l, w]), axis=-1)
    margin = s[:, -1] - s[:, -2]
    print("smallest rotation margin", margin.min())
    assert len(margin) == 36 and margin.min() >= 3.3e-4


def test_wrapper_refuses_bad_arguments_and_cpu_tensors(built_lib):
    from vfa_amd._lib import VFAHipError
    d, _ = dc.load("decode_mc.npz")
    pred = {"heatmap": torch.from_numpy(d["heatmap"]), "loc_offset": torch.from_numpy(d["loc_offset"]),
            "dim_offset": torch.from_numpy(d["dim_offset"]), "rotation": torch.from_numpy(d["rotation_logits"])}
    with pytest.raises(ValueError, match="cls_thresh"):
        dc.decoder_of(d).decode_fused(pred, -0.1)
    with pytest.raises(ValueError, match="cls_thresh"):
        dc.decoder_of(d).decode_fused(pred, float("nan"))
    with pytest.raises(ValueError, match="topk"):
        dc.decoder_of(d, topk=1025).decode_fused(pred, 0.4)
    with pytest.raises(ValueError, match="topk"):
        dc.decoder_of(d, topk=0).decode_fused(pred, 0.4)
    with pytest.raises(ValueError, match="dimension_mean"):
        dc.decoder_of(d, with_mean=False).decode_fused(pred, 0.4)
    with pytest.raises(VFAHipError):
        dc.decoder_of(d).decode_fused(pred, 0.4)


def _hand_made_fused():
    B, k = 3, 4
    count = torch.tensor([2, 0, 3], dtype=torch.int32)
    conf = torch.zeros(B, k)
    loc, dim, rot = torch.zeros(B, k, 3), torch.zeros(B, k, 3), torch.zeros(B, k)
    cell = torch.full((B, k), -1, dtype=torch.int32)
    for b, n in enumerate(count.tolist()):
        for r in range(n):
            conf[b, r] = 0.9 - 0.1 * r - 0.01 * b
            loc[b, r] = torch.tensor([10.0 * b + r, 100.0 * b + r, 0.0])
            dim[b, r] = torch.tensor([1.0 + r, 2.0 + b, 3.0])
            rot[b, r] = 0.1 * (b + r)
            cell[b, r] = 7 * b + r
    return {"count": count, "conf": conf, "location": loc, "cell": cell, "dimension": dim, "rotation": rot}


def test_split_gives_batch_decode_format():
    from vfa_amd.eval_ops import BEVDecoder
    fused = _hand_made_fused()
    frames = BEVDecoder.split(fused)
    assert [len(f["conf"]) for f in frames] == [2, 0, 3]
    for b, f in enumerate(frames):
        n = len(f["conf"])
        assert sorted(f) == ["conf", "dimension", "location", "rotation"]
        assert f["location"].shape == (n, 3) and f["dimension"].shape == (n, 3) and f["rotation"].shape == (n,)
        assert all(v.dtype == torch.float32 for v in f.values())
        assert torch.equal(f["location"], fused["location"][b, :n])
    two_d = {k: v for k, v in fused.items() if k not in ("dimension", "rotation")}
    assert sorted(BEVDecoder.split(two_d)[2]) == ["conf", "location"]


def test_flat_detections_compacts_by_frame():
    """Detections first, in (frame, rank) order; unused rows behind them under the counter ``n_frames``, so the offset tables
    ``match_frames`` / ``match_frames_hungarian`` build from the counters end before them."""
    from vfa_amd import eval_ops
    fused = _hand_made_fused()
    rows, frame_index, n_frames = eval_ops.flat_detections(fused)
    assert n_frames == 3 and frame_index.tolist() == [0, 0, 2, 2, 2] + [3] * 7
    assert rows["cell"].tolist()[:5] == [0, 1, 14, 15, 16] and (rows["cell"][5:] == -1).all()
    assert rows["box"].shape == (12, 7) and rows["xy"].shape == (12, 2) and rows["conf"].shape == (12,)
    assert torch.equal(rows["box"][2], torch.tensor([20.0, 200.0, 0.0, 3.0, 4.0, 1.0, 0.2]))   # x y z, the dimension reversed, alpha
    begin = torch.searchsorted(frame_index, torch.arange(n_frames + 1))                        # the tables' construction
    assert begin.tolist() == [0, 2, 2, 5]
    rows2, _, _ = eval_ops.flat_detections({k: v for k, v in fused.items() if k not in ("dimension", "rotation")})
    assert "box" not in rows2 and torch.equal(rows2["xy"], rows["xy"])
