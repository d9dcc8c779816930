"""The heat-map targets without a GPU: the restatement of tests/heatmap_common.py against the reference's records
(tests/golden/heatmap_*.npz, made by tests/golden/make_heatmaps.py) -- RGK bit for bit, GK under the tolerance rule; the rules of
vfa_amd/csrc/vfa_heat.h (shared host / device code) compiled with g++ into tests/native/heat_harness.cpp, a stand-alone program, and
checked against the records and the restatement, once more under the host sanitizers; the ABI of the new entry points and every
refusal they make before a device is touched; the Python surface.  The tolerance rule: heatmap_common."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import REPO
import heatmap_common as hc
from native_common import build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"]
BAD, UNSUPPORTED = 10001, 10002
ALPHA, RATIO = 0.01, 8


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "heat_rules", "heat_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "heat_rules", "heat_harness.cpp", GXX_FLAGS, sanitized=True)


def _geometry(d):
    return d["world_size"], tuple(int(v) for v in d["grid_lw"])


def _f32(v):
    return str(struct.unpack("<I", struct.pack("<f", float(v)))[0])


def _f64(v):
    return str(struct.unpack("<Q", struct.pack("<d", float(v)))[0])


# ---- 1. the restatement against the reference's records ----------------------------------------------------------------------------

def test_restated_rgk_is_the_references_bit_for_bit():
    """Every frame's map, every object's rotated kernel and its arg-max; the float64 restatement against the float64 record at a few
    ulps of float64 (numpy evaluates the same expressions on arrays instead of scalars)."""
    d = hc.load("heatmap_mc.npz")
    world, lw = _geometry(d)
    angles = set()
    for b, (loc, dim, deg) in enumerate(hc.frames_of(d, "rgk")):
        got, clipped = hc.rgk_map(loc, dim, deg, world, lw, alpha=float(d["alpha"]), ratio=int(d["ratio"]))
        assert clipped == 0 and np.array_equal(got.view(np.uint32), d["rgk_ref32"][b].view(np.uint32)), b
        got64, _ = hc.rgk_map(loc, dim, deg, world, lw, dtype=np.float64)
        assert np.abs(got64 - d["rgk_ref64"][b]).max() <= 2.0 ** -49, b
        for i in range(len(loc)):
            rot, _, centre = hc.rotated_kernel(dim[i][2], dim[i][1], deg[i])
            n = int(d["rgk_kernel_n"][b, i])
            assert rot.shape == (n, n) and np.array_equal(rot.view(np.uint32), d["rgk_kernels"][b, i, :n, :n].view(np.uint32)), (b, i)
            assert centre == tuple(d["rgk_centre"][b, i]), (b, i)
            angles.add(float(deg[i]))
    assert {0.0, 90.0, 180.0, -90.0, 45.0, 135.0} < angles
    off_centre = [(b, i) for b in range(3) for i in range(d["rgk_count"][b]) if tuple(d["rgk_centre"][b, i]) != (d["rgk_kernel_n"][b, i] // 2,) * 2]
    assert off_centre, "the records hold no kernel whose arg-max is off the middle tap"
    assert (d["rgk_ref32"][:, 0].max(axis=1) > 0).any() or (d["rgk_ref32"][:, :, 0].max(axis=1) > 0).any()   # a kernel the map cuts off


@pytest.mark.parametrize("name", hc.FIXTURES)
def test_restated_gk_meets_the_tolerance_rule(name):
    d = hc.load(name)
    world, lw = _geometry(d)
    kind = hc.WILDTRACK if str(d["base"]) == "Wildtrack" else 0
    got = np.stack([hc.gk_map(d["gk_location"][b, :n], world, lw, kind, int(d["gk_grid_reduce"]), int(d["gk_radius"]))
                    for b, n in enumerate(d["gk_count"])])
    hc.check_map(got, d["gk_ref32"], d["gk_ref64"], f"{name} GK restated")
    assert d["gk_ref32"].max() > 2.0          # a crowd: no clip above 1
    for b, n in enumerate(d["gk_count"]):
        cells = {hc.cell_of(x, y, world, lw, kind) for x, y, _ in d["gk_location"][b, :n]}
        assert int((got[b] == 1).sum()) == len(cells) and (b != 1 or len(cells) < n)     # duplicates count once


def test_gk_table_is_the_closed_form():
    from vfa_amd.loss import gk_table
    assert np.array_equal(gk_table(4, 8).numpy().view(np.uint32), hc.gk_table(4, 8).view(np.uint32)) and gk_table(4, 8).shape == (17, 17)
    assert gk_table(4, 8)[8, 8] == 1 and gk_table(2, 16).shape == (33, 33)
    with pytest.raises(ValueError):
        gk_table(4, 17)


# ---- 2. the shared header on the CPU -----------------------------------------------------------------------------------------------

def test_rules_against_brute_force(harness):
    run_harness(harness, "cases", "1")


def test_rules_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "cases", "2")


def _harness_kernels(exe, objects):
    """objects: (l, w, deg) -> list of (n, (g_t, g_l), branch (n, n), values (n, n) float32)."""
    args = [a for l, w, deg in objects for a in (_f32(l), _f32(w), _f64(deg))]
    lines = run_harness(exe, "kernels", _f64(ALPHA), str(RATIO), str(len(objects)), *args).splitlines()[1:]
    out = []
    for line in lines[:len(objects)]:
        tok = [int(t) for t in line.split()]
        n = tok[0]
        pairs = np.array(tok[3:], dtype=np.int64).reshape(n * n, 2)
        out.append((n, (tok[1], tok[2]), pairs[:, 0].reshape(n, n), pairs[:, 1].astype(np.uint32).view(np.float32).reshape(n, n)))
    return out


def test_header_reproduces_every_recorded_kernel(harness, sanitized_harness):
    """Kernel size, skip pattern and arg-max exactly; the values under the tolerance rule, with the float64 restatement (pinned to the
    float64 records above) as the float64 reference of a kernel."""
    d = hc.load("heatmap_mc.npz")
    objects, want = [], []
    for b, (_, dim, deg) in enumerate(hc.frames_of(d, "rgk")):
        for i in range(len(deg)):
            n = int(d["rgk_kernel_n"][b, i])
            objects.append((dim[i][2], dim[i][1], deg[i]))
            want.append((d["rgk_kernels"][b, i, :n, :n], tuple(d["rgk_centre"][b, i])))
    for exe in (harness, sanitized_harness):
        got = _harness_kernels(exe, objects)
        worst = worst_ref = 0.0
        for (l, w, deg), (n, centre, branch, values), (ref32, ref_centre) in zip(objects, got, want):
            rot64, branch64, _ = hc.rotated_kernel(l, w, deg, dtype=np.float64)
            assert n == ref32.shape[0] and centre == ref_centre, (l, w, deg, n, centre, ref_centre)
            assert np.array_equal(branch, branch64) and np.array_equal(values == 0, ref32 == 0), (l, w, deg)
            worst = max(worst, float(np.abs(values.astype(np.float64) - rot64).max()))
            worst_ref = max(worst_ref, float(np.abs(ref32.astype(np.float64) - rot64).max()))
        print(f"rotated kernels: header {worst:.3e}  float32 reference {worst_ref:.3e}  bound {4 * worst_ref:.3e}")
        assert worst <= 4 * worst_ref


def test_header_reproduces_size_and_paste_offsets(harness, sanitized_harness):
    d = hc.load("heatmap_mc.npz")
    world, (L, W) = _geometry(d)
    objects = hc.border_objects() + [(loc[0], loc[1], dim[2], dim[1], deg) for locs, dims, degs in hc.frames_of(d, "rgk")
                                   for loc, dim, deg in zip(locs, dims, degs)]
    args = [a for x, y, l, w, deg in objects for a in (_f32(x), _f32(y), _f32(l), _f32(w), _f64(deg))]
    for exe in (harness, sanitized_harness):
        lines = run_harness(exe, "paste", str(L), str(W), "0", _f32(world[0]), _f32(world[1]), _f64(ALPHA), str(RATIO), str(len(objects)),
                            *args).splitlines()[1:]
        cut = 0
        for (x, y, l, w, deg), line in zip(objects, lines):
            got = [int(t) for t in line.split()]
            at, made = hc.cell_of(x, y, world, (L, W), 0), hc.rotated_kernel(l, w, deg)
            n, (g_t, g_l) = (made[0].shape[0], made[2]) if made else (0, (0, 0))
            want = [-1 if at is None else at[0] * W + at[1], n, g_t, g_l, 0, -1, -1, -1, -1]
            if at is not None and made:
                y0, y1 = max(0, at[0] - g_t), min(L, at[0] - g_t + n) - 1
                x0, x1 = max(0, at[1] - g_l), min(W, at[1] - g_l + n) - 1
                want[4:] = [(y1 - y0 + 1) * (x1 - x0 + 1), y0, y1, x0, x1]
                cut += want[4] < n * n
            assert got == want, ((x, y, l, w, deg), got, want)
        assert cut >= 10
    assert hc.kernel_k(900.0, 100.0) is None and hc.kernel_k(640.0, 100.0) == 56 and hc.kernel_k(800.0, 100.0) == 64


@pytest.mark.parametrize("name", hc.FIXTURES)
def test_header_gk_is_the_restatement_and_meets_the_rule(harness, sanitized_harness, name):
    d = hc.load(name)
    world, (L, W) = _geometry(d)
    kind = hc.WILDTRACK if str(d["base"]) == "Wildtrack" else 0
    r, reduce_ = int(d["gk_radius"]), int(d["gk_grid_reduce"])
    for exe in (harness, sanitized_harness):
        maps = []
        for b, n in enumerate(d["gk_count"]):
            args = [a for x, y, _ in d["gk_location"][b, :n] for a in (_f32(x), _f32(y))]
            out = run_harness(exe, "gk", str(L), str(W), str(kind), _f32(world[0]), _f32(world[1]), str(r), _f64(8.0 / reduce_), str(n), *args)
            maps.append(np.array(out.split()[1:], dtype=np.int64).astype(np.uint32).view(np.float32).reshape(L, W))
            assert np.array_equal(maps[-1].view(np.uint32), hc.gk_map(d["gk_location"][b, :n], world, (L, W), kind, reduce_, r).view(np.uint32)), b
        hc.check_map(np.stack(maps), d["gk_ref32"], d["gk_ref64"], f"{name} GK header")


# ---- 3. the library's plumbing ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from vfa_amd import _lib
    declared = declared_parameters()
    for name, count in (("vfa_heat_workspace_bytes", 3), ("vfa_heat_rgk_f32", 17), ("vfa_heat_gk_f32", 16)):
        assert declared.get(name) == count == len(_lib.SIGNATURES[name]), name
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    shared = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_heat.h")).read()
    for macro, constant, value in (("VFA_HEAT_MAX_KERNEL", "kMaxKernel", 65), ("VFA_HEAT_MAX_RADIUS", "kMaxRadius", 16)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == value
        assert int(re.search(constant + r"\s*=\s*(\d+)", shared).group(1)) == value
    assert int(re.search(r"#define\s+VFA_ABI_VERSION\s+(\d+)", text).group(1)) == 9 == _lib.ABI_VERSION    # additive: no new version
    makefile = open(os.path.join(REPO, "vfa_amd", "csrc", "Makefile")).read()
    assert "vfa_heat.hip" in makefile.split("SRCS")[1] and "vfa_heat.h" in makefile.split("HDRS")[1]
    assert "contract=off" in makefile


def test_workspace_size_and_refusals(built_lib):
    """Everything the two calls decide before they launch (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_heat_workspace_bytes(4, 156, 156) == 4 * 156 * 156 and lib.vfa_heat_workspace_bytes(1, 3, 3) == 16
    assert lib.vfa_heat_workspace_bytes(0, 5, 5) == 0 and lib.vfa_heat_workspace_bytes(2, 0, 5) == 0 and lib.vfa_heat_workspace_bytes(2, 5, -1) == 0
    p = ctypes.c_void_p(4096)   # (never dereferenced)

    def rgk(B=1, K=8, L=4, W=4, width=3, loc=p, count=p, dim=p, deg=p, world0=100.0, kind=0, alpha=0.01, ratio=8, heat=p, clipped=p):
        return lib.vfa_heat_rgk_f32(loc, width, count, dim, deg, B, K, L, W, world0, 100.0, kind, alpha, ratio, heat, clipped, None)

    def gk(B=1, K=8, L=4, W=4, width=3, loc=p, count=p, table=p, r=8, world0=100.0, kind=0, ws=p, ws_bytes=16, heat=p):
        return lib.vfa_heat_gk_f32(loc, width, count, table, r, B, K, L, W, world0, 100.0, kind, ws, ws_bytes, heat, None)

    for call in (rgk, gk):
        assert call(B=-1) == BAD and call(K=-1) == BAD and call(L=-1) == BAD and call(W=-3) == BAD
        assert call(width=1) == BAD and call(width=4) == BAD and call(kind=3) == BAD and call(kind=-1) == BAD
        assert call(world0=0.0) == BAD and call(world0=float("nan")) == BAD
        assert call(loc=None) == BAD and call(count=None) == BAD and call(heat=None) == BAD
        assert call(K=1025) == UNSUPPORTED and call(B=65536) == UNSUPPORTED and call(L=1 << 16, W=1 << 16) == UNSUPPORTED
        assert call(B=0) == 0 and call(B=0, loc=None, count=None, heat=None) == 0 and call(L=0) == 0 and call(W=0, heat=None) == 0
    assert rgk(dim=None) == BAD and rgk(deg=None) == BAD and rgk(clipped=None) == BAD
    assert rgk(alpha=0.0) == BAD and rgk(alpha=float("nan")) == BAD and rgk(ratio=0) == BAD and rgk(ratio=1025) == BAD
    assert gk(table=None) == BAD and gk(r=-1) == BAD and gk(r=17) == UNSUPPORTED and gk(ws=None) == BAD and gk(ws_bytes=15) == BAD


def test_wrappers_refuse_cpu_tensors_other_dtypes_and_missing_operands(built_lib):
    from vfa_amd import TargetEncoder, ops
    from vfa_amd._lib import VFAHipError
    enc = TargetEncoder("MultiviewC", (512, 1024), (4, 4, 4))
    loc, count = torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32)
    dim, deg = torch.ones(1, 4, 3), torch.zeros(1, 4, dtype=torch.float64)
    for kw in (dict(heatmap_type="GK"), dict(dimension=dim, rotation_deg=deg), dict(dimension=dim, rotation=deg.float())):
        with pytest.raises(VFAHipError):           # CPU tensors: no fallback
            enc.heatmap(loc, count, grid_lw=(24, 40), **kw)
    with pytest.raises(VFAHipError):
        ops.heat_gk(loc.double(), count, torch.ones(17, 17))
    with pytest.raises(VFAHipError):
        ops.heat_rgk(loc, count, dim.double(), deg)
    assert hasattr(enc, "heatmap") and hasattr(ops, "heat_rgk") and hasattr(ops, "heat_gk")
