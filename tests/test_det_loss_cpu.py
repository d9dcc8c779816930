"""The sparse target encoder and the fused detection loss without a GPU: the restatement of tests/loss_common.py against the reference's
records (tests/golden/det_loss_*.npz, made by tests/golden/make_det_loss.py); the rules of vfa_amd/csrc/vfa_loss.h (shared host /
device code) compiled with g++ into tests/native/loss_harness.cpp and checked against brute force and against the records, once more
under the host sanitizers; the ABI of the new entry points and every refusal they make before a device is touched; the Python surface
(``pack_objects``, ``DetTargets.from_dense``, the refusal of CPU tensors)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO
import loss_common as lc
from native_common import build_harness, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"]
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "loss_rules", "loss_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "loss_rules", "loss_harness.cpp", GXX_FLAGS, sanitized=True)


# ---- 1. the restatement against the reference's records ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.FIXTURES)
def test_restated_targets_are_the_references(name):
    """Cells, offsets, labels and CSL rows bit for bit; the duplicate cell keeps the later object; the last cell is taken."""
    d, three_d = lc.load(name)
    L, W = (int(v) for v in d["grid_lw"])
    t = lc.encode(d["obj_location"], d["world_size"], (L, W), str(d["base"]), d["obj_dimension"], d["obj_rotation"], d["dimension_mean"])
    cells = np.flatnonzero(d["gt_mask"].ravel() == 1)
    assert np.array_equal(t["cells"], cells) and len(cells) == len(d["obj_location"]) - 1 and cells[-1] == L * W - 1
    assert np.array_equal(t["loc_offset"].view(np.uint32), d["gt_loc_offset"].reshape(-1, 2)[cells].view(np.uint32))
    assert not np.delete(d["gt_loc_offset"].reshape(-1, 2), cells, axis=0).any()
    if three_d:
        assert np.array_equal(t["dim_offset"].view(np.uint32), d["gt_dim_offset"].reshape(-1, 3)[cells].view(np.uint32))
        rows = lc.label_rows(t["label"], int(d["angle_range"]), float(d["angle_radius"]))
        assert np.array_equal(rows.view(np.uint32), d["gt_rotation_rows"].view(np.uint32))
        assert ((rows == 1).sum(axis=1) == 1).all() and np.array_equal(np.argmax(rows, axis=1), t["label"] % 360)
        assert (t["label"] < 0).any() and (t["label"] >= 180).any()
        degrees = d["obj_rotation"].astype(np.float32) * np.float32(57.29577951308232)      # within one ulp of an integer: 30, 90, 90, 135, 180
        assert (np.abs(degrees - np.round(degrees)) <= np.spacing(np.abs(degrees))).sum() >= 4


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_restated_loss_is_the_references(name):
    """float32: the five numbers and every gradient within 1 ulp of the reference's float32 run; float64: to 1e-12."""
    d, three_d = lc.load(name)
    pred, targets, gt = lc.fixture_case(d, three_d)
    for tag, dtype, tol in (("f32", torch.float32, 2.0 ** -23), ("f64", torch.float64, 1e-12)):
        vals, grads = lc.evaluate(pred, targets, gt, d["loss_weight"].tolist(), dtype)
        for k, v in vals.items():
            assert lc.rel(v[0], d[f"{tag}_{k}"]) <= tol, (tag, k, v[0], float(d[f"{tag}_{k}"]))
        for k, g in grads.items():
            ref = d[f"{tag}_grad_" + ("rotation_rows" if k == "rotation_at" else k)]
            assert lc.maxabs(g.reshape(ref.shape), ref) <= tol, (tag, k)


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_fixture_margins(name):
    """What makes the GPU comparison unambiguous: saturated logits are there, none sits where the clamp switches the gradient off."""
    d, _ = lc.load(name)
    x = d["heatmap"]
    assert (np.abs(x) == 15).sum() >= 4 and (np.abs(np.abs(x) - 11.5129) > 1e-3).all()
    assert int((d["gt_heatmap"] == 1).sum()) == int((d["gt_mask"] == 1).sum())
    assert d["gt_mask"].shape[0] != d["gt_mask"].shape[1]


# ---- 2. the shared rules on the CPU -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rules_against_brute_force(harness, seed):
    out = run_harness(harness, "cases", str(seed))
    live, dropped, overwritten = (int(v) for v in re.search(r"(\d+) live, (\d+) dropped, (\d+) overwritten", out).groups())
    assert live > 2000 and dropped > 2000 and overwritten > 1000 and "labels ok" in out


def test_rules_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "cases", "4")


def _harness_encode(exe, d):
    L, W = (int(v) for v in d["grid_lw"])
    from vfa_amd import _lib
    bits = np.stack([d["obj_location"][:, 0], d["obj_location"][:, 1], d["obj_rotation"]], axis=1).astype(np.float32).view(np.uint32)
    out = run_harness(exe, "encode", str(L), str(W), str(_lib.CONV_KIND[str(d["base"])]), str(float(d["world_size"][0])),
               str(float(d["world_size"][1])), str(len(bits)), *[str(int(v)) for v in bits.ravel()])
    lines = out.strip().split("\n")
    rows = np.array([[int(v) for v in line.split()] for line in lines[1:]], dtype=np.int64).reshape(-1, 4)
    assert int(lines[0].split()[1]) == len(rows)
    return rows


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_rules_against_the_fixtures(harness, sanitized_harness, name):
    """The header's cell assignment, duplicate resolution, ranks and labels on the fixture's objects give the reference's records."""
    d, three_d = lc.load(name)
    cells = np.flatnonzero(d["gt_mask"].ravel() == 1)
    for exe in (harness, sanitized_harness):
        rows = _harness_encode(exe, d)
        assert np.array_equal(rows[:, 0], cells)
        assert np.array_equal(rows[:, 1:3].astype(np.uint32), d["gt_loc_offset"].reshape(-1, 2)[cells].view(np.uint32))
        if three_d:
            got = lc.label_rows(rows[:, 3], int(d["angle_range"]), float(d["angle_radius"]))
            assert np.array_equal(got.view(np.uint32), d["gt_rotation_rows"].view(np.uint32))


# ---- 3. the library's plumbing ----------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    """Declared, exported, bound, the same number of arguments: tests/test_abi.py, for every symbol.  Here: each cap is one number,
    and the Makefile builds the file."""
    from vfa_amd import loss
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    shared = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_loss.h")).read()
    for macro, constant in (("VFA_DET_MAX_OBJECTS", "kMaxObjects"), ("VFA_DET_MAX_ROT", "kMaxRot")):
        cap = int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1))
        assert cap == int(re.search(constant + r"\s*=\s*(\d+)", shared).group(1)) == loss.MAX_OBJECTS == 1024
    makefile = open(os.path.join(REPO, "vfa_amd", "csrc", "Makefile")).read()
    assert "vfa_loss.hip" in makefile and "vfa_loss.h" in makefile.split("HDRS")[1]


def test_refusals_of_the_encoder(built_lib):
    """Everything the call decides before it launches (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    p, mean = ctypes.c_void_p(4096), (ctypes.c_float * 3)(1, 1, 1)   # (p is never dereferenced)

    def call(B=1, K=8, L=4, W=4, width=3, loc=p, count=p, dim=p, rot=p, mean=mean, world0=100.0, kind=0, cells=p, n_pos=p, loc_o=p, dim_o=p,
             label=p):
        return lib.vfa_det_targets_f32(loc, width, count, dim, rot, mean, B, K, L, W, world0, 100.0, kind, cells, n_pos, loc_o, dim_o, label,
                                       None)
    assert call(B=-1) == BAD and call(K=-1) == BAD and call(L=-1) == BAD and call(W=-3) == BAD
    assert call(width=1) == BAD and call(width=4) == BAD and call(kind=3) == BAD and call(kind=-1) == BAD
    assert call(world0=0.0) == BAD and call(world0=float("nan")) == BAD
    assert call(loc=None) == BAD and call(count=None) == BAD and call(cells=None) == BAD and call(n_pos=None) == BAD and call(loc_o=None) == BAD
    assert call(dim=None) == BAD and call(rot=None) == BAD and call(mean=None) == BAD and call(dim_o=None) == BAD and call(label=None) == BAD
    assert call(K=1025) == UNSUPPORTED and call(B=65536) == UNSUPPORTED and call(L=1 << 16, W=1 << 16) == UNSUPPORTED
    assert call(B=0) == 0 and call(B=0, loc=None, count=None) == 0


def test_workspace_size_and_the_refusals_of_the_loss(built_lib):
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_det_loss_workspace_bytes(4, 156, 156) == 4 * 24 * 24 and lib.vfa_det_loss_workspace_bytes(1, 1, 1) == 24
    assert lib.vfa_det_loss_workspace_bytes(0, 5, 5) == 0 and lib.vfa_det_loss_workspace_bytes(2, 0, 5) == 0
    p = ctypes.c_void_p(4096)
    s3, s4, weights = (ctypes.c_longlong * 3)(16, 4, 1), (ctypes.c_longlong * 4)(48, 12, 3, 1), (ctypes.c_float * 4)(1, 1, 1, 1)
    neg3, neg4 = (ctypes.c_longlong * 3)(16, -4, 1), (ctypes.c_longlong * 4)(48, 12, 3, -1)

    def operands(heat=p, heat_s=s3, gt=p, gt_s=s3, loc=p, loc_s=s4, dim=p, dim_s=s4, rot=p, rot_s=s3, cells=p, n_pos=p, loc_t=p, dim_t=p,
                 label=p, table=p):
        return [heat, heat_s, gt, gt_s, loc, loc_s, dim, dim_s, rot, rot_s, cells, n_pos, loc_t, dim_t, label, table]

    def forward(B=1, L=4, W=4, k=8, R=360, weights=weights, ws=p, ws_bytes=64, terms=p, loss=p, counts=p, **kw):
        return lib.vfa_det_loss_f32(*operands(**kw), weights, B, L, W, k, R, ws, ws_bytes, terms, loss, counts, None)

    def backward(B=1, L=4, W=4, k=8, R=360, ws_bytes=0, coef=p, counts=p, d_heat=p, d_loc=p, d_dim=p, d_rot=p, **kw):
        return lib.vfa_det_loss_backward_f32(coef, *operands(**kw), counts, B, L, W, k, R, d_heat, d_loc, d_dim, d_rot, None)

    for call in (forward, backward):
        assert call(B=-1) == BAD and call(L=-1) == BAD and call(W=-1) == BAD and call(k=-1) == BAD and call(R=-2) == BAD
        assert call(k=1025) == UNSUPPORTED and call(R=1026) == UNSUPPORTED and call(R=359) == UNSUPPORTED and call(R=1025) == UNSUPPORTED
        assert call(B=65536, ws_bytes=1 << 40) == UNSUPPORTED and call(L=1 << 16, W=1 << 16, ws_bytes=1 << 40) == UNSUPPORTED
        for name in ("heat", "heat_s", "gt", "gt_s", "loc", "loc_s", "n_pos", "cells", "loc_t", "dim_s", "rot_s", "dim_t", "label", "table"):
            assert call(**{name: None}) == BAD, name
        assert call(dim=None) == BAD and call(rot=None) == BAD           # one 3D head without the other
        assert call(heat_s=neg3) == BAD and call(gt_s=neg3) == BAD and call(loc_s=neg4) == BAD and call(dim_s=neg4) == BAD
        assert call(rot_s=neg3) == BAD
        assert call(B=0) == 0 and call(L=0) == 0 and call(W=0, heat=None) == 0
    assert forward(ws=None) == BAD and forward(ws_bytes=23) == BAD and forward(weights=None) == BAD
    assert forward(terms=None) == BAD and forward(loss=None) == BAD and forward(counts=None) == BAD
    assert backward(coef=None) == BAD and backward(counts=None) == BAD and backward(d_heat=None) == BAD and backward(d_loc=None) == BAD
    assert backward(d_dim=None) == BAD and backward(d_rot=None) == BAD


def test_wrappers_refuse_other_dtypes_and_cpu_tensors(built_lib):
    """Non-float32 operands and CPU tensors are refused by the wrappers before the library is called."""
    from vfa_amd import ops, loss
    from vfa_amd._lib import VFAHipError
    d, _ = lc.load("det_loss_mc.npz")
    pred, targets, gt = lc.fixture_case(d, True)
    t = targets[0]
    n = len(t["cells"])
    tg = loss.DetTargets(torch.from_numpy(t["cells"])[None], torch.tensor([n], dtype=torch.int32), torch.from_numpy(t["loc_offset"])[None],
                         torch.from_numpy(t["dim_offset"])[None], torch.from_numpy(t["label"])[None], loss.label_table(360, 6))
    with pytest.raises(VFAHipError):
        loss.detection_loss(pred, tg, gt)
    with pytest.raises(VFAHipError):
        loss.TargetEncoder("MultiviewC", (300, 500), (25, 25, 32), d["dimension_mean"]).encode(
            torch.from_numpy(d["obj_location"])[None], torch.tensor([9], dtype=torch.int32), torch.from_numpy(d["obj_dimension"])[None],
            torch.from_numpy(d["obj_rotation"])[None], grid_lw=(12, 20))
    with pytest.raises(VFAHipError):
        ops.det_targets(torch.zeros(1, 4, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="loss weights"):
        loss.detection_loss(pred, tg, gt, loss_weight=(1.0, 1.0))
    with pytest.raises(ValueError, match="unknown dataset"):
        loss.TargetEncoder("KITTI", (1, 1), (1, 1, 1))
    with pytest.raises(ValueError, match="angle_range"):
        loss.TargetEncoder("MultiviewC", (1, 1), (1, 1, 1), angle_range=361)


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------

def _objects(d, three_d, take):
    return [SimpleNamespace(location=d["obj_location"][i].tolist(), **(dict(dimension=d["obj_dimension"][i].tolist(),
                                                                            rotation=float(d["obj_rotation"][i])) if three_d else {}))
            for i in take]


def test_pack_objects_shapes_and_padding():
    from vfa_amd import pack_objects
    d, _ = lc.load("det_loss_mc.npz")
    frames = [_objects(d, True, range(9)), [], _objects(d, True, [3, 1])]
    p = pack_objects(frames, max_objects=16)
    assert p.location.shape == (3, 16, 3) and p.dimension.shape == (3, 16, 3) and p.rotation.shape == (3, 16) and p.count.tolist() == [9, 0, 2]
    assert p.count.dtype == torch.int32 and p.location.dtype == p.dimension.dtype == p.rotation.dtype == torch.float32
    assert np.array_equal(p.location[0, :9].numpy(), d["obj_location"]) and np.array_equal(p.rotation[2, :2].numpy(), d["obj_rotation"][[3, 1]])
    assert np.array_equal(p.dimension[2, 0].numpy(), d["obj_dimension"][3])
    assert not p.location[0, 9:].any() and not p.location[1].any() and (p.dimension[1] == 1).all() and not p.rotation[2, 2:].any()
    two = pack_objects([[SimpleNamespace(location=[1.0, 2.0])], []], max_objects=4)
    assert two.dimension is None and two.rotation is None and two.location[0, 0].tolist() == [1.0, 2.0, 0.0] and two.count.tolist() == [1, 0]
    with pytest.raises(ValueError, match="max_objects"):
        pack_objects(frames, max_objects=8)
    with pytest.raises(ValueError, match="max_objects"):
        pack_objects(frames, max_objects=1025)


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_from_dense_against_the_fixture(name):
    """The reference encoder's dense dict -> the sparse targets: the fixture's cells in order, its offsets bit for bit, labels modulo R."""
    from vfa_amd import DetTargets
    d, three_d = lc.load(name)
    L, W = (int(v) for v in d["grid_lw"])
    cells = np.flatnonzero(d["gt_mask"].ravel() == 1)
    n = len(cells)
    gt = {"mask": torch.from_numpy(d["gt_mask"])[None, None], "loc_offset": torch.from_numpy(d["gt_loc_offset"])[None]}
    if three_d:
        dense = np.zeros((L * W, 360), np.float32)
        dense[cells] = d["gt_rotation_rows"]
        gt.update(dim_offset=torch.from_numpy(d["gt_dim_offset"])[None], rotation=torch.from_numpy(dense).reshape(1, L, W, 360))
    for k in (n, n + 5, 3):
        t = DetTargets.from_dense(gt, k)
        m = min(n, k)
        assert t.cells.shape == (1, k) and t.cells.dtype == torch.int32 and t.n_pos.tolist() == [m]
        assert np.array_equal(t.cells[0, :m].numpy(), cells[:m]) and (t.cells[0, m:] == -1).all()
        assert np.array_equal(t.loc_offset[0, :m].numpy().view(np.uint32), d["gt_loc_offset"].reshape(-1, 2)[cells[:m]].view(np.uint32))
        assert not t.loc_offset[0, m:].any()
        if three_d:
            want = lc.encode(d["obj_location"], d["world_size"], (L, W), "MultiviewC", d["obj_dimension"], d["obj_rotation"],
                             d["dimension_mean"])
            assert np.array_equal(t.angle_label[0, :m].numpy(), want["label"][:m] % 360)
            assert np.array_equal(t.dim_offset[0, :m].numpy(), want["dim_offset"][:m]) and not t.dim_offset[0, m:].any()
            assert np.array_equal(t.table.numpy().view(np.uint32), lc.table64(360, 6).astype(np.float32).view(np.uint32))
        else:
            assert t.dim_offset is None and t.angle_label is None and t.table is None


def test_public_names_and_the_reference_module_is_not_shadowed():
    import vfa_amd
    for name in ("DetTargets", "PackedObjects", "TargetEncoder", "compute_loss2d", "compute_loss3d", "detection_loss", "pack_objects"):
        assert name in vfa_amd.__all__ and hasattr(vfa_amd, name)
    assert not os.path.exists(os.path.join(REPO, "compat", "vfa", "model", "loss.py"))
