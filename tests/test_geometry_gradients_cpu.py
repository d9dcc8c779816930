"""Host side of the geometry gradient (no GPU): the fixtures are the reference's, the float64 restatement reproduces them, the per-box
chain rule the HIP kernel implements is autograd's, and the entry point is declared, bound and guarded."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden_path
import geomgrad_common as gc

CASES = ["geomgrad_mc_c256_nl1.npz", "geomgrad_mc_c256_nl5.npz", "geomgrad_wt_s8.npz", "geomgrad_mx_s16.npz",
         "geomgrad_mc_inside_clamped.npz", "geomgrad_frame_mc_nl1.npz"]
NEW = ["vfa_gather_backward_geometry_workspace_bytes", "vfa_project_gather_backward_geometry_f32"]


def load_case(name):
    z = np.load(golden_path(name), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["data"] = str(d["data"])
    d["image_size"] = tuple(int(v) for v in d["image_size"])
    d["cube_size"] = tuple(float(v) for v in d["cube_size"])
    d["grid_height"] = float(d["grid_height"])
    d["feat_hws"] = [tuple(int(v) for v in hw) for hw in d["feat_hws"]]
    L, W = d["grid"].shape[:2]
    nl = len(gc.z_layers(d["grid_height"], d["cube_size"]))
    d["nl"] = nl
    d["inputs"] = gc.inputs(int(d["seed"]), d["calibs"].shape[0], int(d["C"]), d["feat_hws"], nl, L, W, wscale=float(d["wscale"]),
                            signed=bool(d["signed"]))
    return d


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_are_drawn_again_and_free_of_slivers_where_stated(name):
    d = load_case(name)
    sums = [float(np.sum(f, dtype=np.float64)) for f in d["inputs"]["feats"]]
    assert np.allclose(sums, d["feat_sum"], rtol=0, atol=1e-6), "the seeded inputs no longer reproduce the fixture's"
    assert np.isfinite(d["d_calibs"]).all() and np.isfinite(d["d_grid"]).all()
    assert np.abs(d["d_calibs64"]).max() > 0 and np.abs(d["d_grid64"]).max() > 0


def test_at_least_two_cases_are_sliver_free_with_small_noise():
    quiet = [n for n in CASES if (lambda d: d["min_area"] > 0.1 and max(float(d["noise_calib"]), float(d["noise_grid"])) <= 1e-3)(load_case(n))]
    assert len(quiet) >= 2, quiet


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference_geometry_gradients(name):
    """oracle/torch_reference.py in float64 with autograd on calib and grid against the reference's float64 backward."""
    from oracle import torch_reference as ref
    d = load_case(name)
    inp = d["inputs"]
    zl = torch.tensor(gc.z_layers(d["grid_height"], d["cube_size"]), dtype=torch.float64)
    co = torch.tensor(gc.corner_offsets(d["cube_size"]), dtype=torch.float64)
    cal = torch.from_numpy(d["calibs"]).double().requires_grad_(True)
    grid = torch.from_numpy(d["grid"]).double().requires_grad_(True)
    ortho = 0
    for cam in range(cal.shape[0]):
        o = 0
        for s in range(len(d["feat_hws"])):
            o = o + ref.vfa_forward(torch.from_numpy(inp["feats"][s][cam:cam + 1]).double(), cal[cam], grid,
                                    torch.from_numpy(inp["weights"][s]).double(), torch.from_numpy(inp["biases"][s]).double(), zl, co,
                                    d["data"], d["image_size"])
        ortho = ortho + o
    (ortho * torch.from_numpy(inp["probe"]).double()[None]).sum().backward()
    assert _rel(cal.grad.numpy(), d["d_calibs64"]) <= 1e-9
    assert _rel(grid.grad.numpy(), d["d_grid64"]) <= 1e-9


def _scene(data, seed):
    from vfa_amd.synthetic import look_at_camera, ring_cameras
    g = torch.Generator().manual_seed(seed)
    if data == "MultiviewC":
        cam = ring_cameras(3, (1950.0, 1950.0, 0.0), 2800.0, 600.0, 900.0, (1280, 720))[seed % 3]
        xs, ys = torch.meshgrid(torch.arange(0, 3900, 300.0), torch.arange(0, 3900, 260.0), indexing="ij")
        cube, gh, img = (25, 25, 32), 160, (720, 1280)
    elif data == "Wildtrack":
        cam = ring_cameras(3, (480 * 2.5 / 2 - 300.0, 1440 * 2.5 / 2 - 900.0, 0.0), 0.45 * 1440 * 2.5, 400.0, 1100.0, (1920, 1080))[seed % 3]
        xs, ys = torch.meshgrid(torch.arange(0, 480, 32.0), torch.arange(0, 1440, 60.0), indexing="ij")
        cube, gh, img = (4, 4, 4), 32, (1080, 1920)
    else:
        cam = torch.tensor(look_at_camera((-5.0, 8.0 + seed, 3.0), (12.0, 8.0, 0.0), 1700.0, (1920, 1080)))
        xs, ys = torch.meshgrid(torch.arange(0, 640, 50.0), torch.arange(0, 1000, 40.0), indexing="ij")
        cube, gh, img = (4, 4, 8), 64, (1080, 1920)
    grid = torch.stack([xs, ys, torch.zeros_like(xs)], -1).double()
    feat = torch.relu(torch.randn(1, 5, 45, 80, generator=g, dtype=torch.float64))
    return torch.as_tensor(cam, dtype=torch.float64), grid, feat, cube, gh, img, g


@pytest.mark.parametrize("data", ["MultiviewC", "MultiviewX", "Wildtrack"])
@pytest.mark.parametrize("seed", [0, 1])
def test_per_box_chain_rule_is_autograd_of_the_restatement(data, seed):
    """The formulas of vfa_geom_grad.hip (grid_sample's point derivative, the area term, min / max corner selection, clamp, perspective
    division, conversion scale), restated in float64 torch, against autograd of oracle/torch_reference on a random d vox."""
    from oracle import torch_reference as ref
    calib, grid, feat, cube, gh, img, g = _scene(data, seed)
    zl = torch.tensor(gc.z_layers(gh, cube), dtype=torch.float64)
    co = torch.tensor(gc.corner_offsets(cube), dtype=torch.float64)
    cal = calib.clone().requires_grad_(True)
    gr = grid.clone().requires_grad_(True)
    st = ref.vfa_stages(feat, cal, gr, zl, co, data, img)
    assert 0.2 < float(st["visible"].double().mean()) < 1.0
    G = torch.randn(st["vox"].shape, generator=g, dtype=torch.float64)
    (st["vox"] * G).sum().backward()
    d_cal, d_grid = gc.box_chain_rule(feat[0], calib, grid, zl, co, data, img, G)
    assert _rel(d_cal.numpy(), cal.grad.numpy()) <= 1e-6
    assert _rel(d_grid.numpy(), gr.grad.numpy()) <= 1e-6


def test_entry_point_is_declared_documented_bound_and_exported():
    from vfa_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(?:int|size_t)\s+(vfa_\w+)\s*\(", code))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    text = " ".join(header.split())
    assert "calib and grid carry no gradient" not in text
    for phrase in ("bit-reproducible, no float atomics", "exactly one fp32 add per element", "masked boxes pass nothing",
                   "no device-to-host read", "torch.min / max selects"):
        assert phrase in text, phrase
    assert "#define VFA_ABI_VERSION 9" in header
    fn = lib.vfa_gather_backward_geometry_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert fn(7, 40000) == -(-(5000 * 7 * 48) // 256) * 256 and fn(0, 10) == 0 and fn(3, 0) == 0


def test_ops_wrapper_rejects_cpu_tensors_and_bad_shapes():
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    n, C, nl, cells = 2, 8, 3, 10
    integral = torch.zeros(n, 7, 9, C)
    args = (torch.zeros(3), torch.zeros(8, 3), 0, (1280.0, 720.0))
    gv = torch.zeros(n, cells, nl * C)
    with pytest.raises(VFAHipError):
        ops.project_gather_backward_geometry(gv, integral, torch.zeros(n, 12), torch.zeros(cells, 3), *args)
    bad = [
        (gv, integral, torch.zeros(n, 3, 4), torch.zeros(cells, 3)),          # calibs not (n, 12)
        (gv, integral, torch.zeros(n, 12), torch.zeros(cells, 2)),            # grid not (n_cells, 3)
        (gv[:, :5], integral, torch.zeros(n, 12), torch.zeros(cells, 3)),      # grad_vox not (n, cell_count, nl*C)
        (gv, integral[0], torch.zeros(n, 12), torch.zeros(cells, 3)),          # integral not 4-d
    ]
    for a in bad:
        with pytest.raises(ValueError):
            ops.project_gather_backward_geometry(*a, *args)
    with pytest.raises(ValueError):
        ops.project_gather_backward_geometry(gv, integral, torch.zeros(n, 12), torch.zeros(cells, 3), *args, cell_begin=4, cell_count=8)
    with pytest.raises(ValueError):
        ops.project_gather_backward_geometry(gv, integral, torch.zeros(n, 12), torch.zeros(cells, 3), *args, grad_grid=torch.zeros(cells, 4))
