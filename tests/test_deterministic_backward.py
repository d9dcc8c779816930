"""Bit-reproducible training backward under ``torch.use_deterministic_algorithms(True)``: the sort-and-sum scatter
(``vfa_project_gather_backward_det_f32``), the fixed-order column sum (``vfa_column_sum_f32``) and the whole frame through
``aggregate_views`` on both training paths.   -m gpu."""
import contextlib
import hashlib
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def deterministic(on=True):
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


def _scatter_case(workload, n_cam, cells, crop, C):
    from vfa_amd import _lib, ops
    from vfa_amd.synthetic import make_workload
    import vfa_amd
    dev = torch.device("cuda:0")
    wl = make_workload(workload, channels=C, seed=5, n_cam=n_cam)
    mod = vfa_amd.VFA(C, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev)
    zl, co = mod._kernel_geometry(dev)
    calibs = wl["calibs"].reshape(n_cam, 12).to(dev)
    grid4 = wl["grid"] if crop is None else wl["grid"][:, 60:60 + crop[0], 70:70 + crop[1]].contiguous()
    grid = grid4.reshape(-1, 3).to(dev)
    kind, size = _lib.CONV_KIND[wl["args"].data], wl["args"].image_size[::-1]
    begin, count = cells
    count = grid.shape[0] - begin if count is None else count
    feat = torch.cat([wl["features"][c][1] for c in range(n_cam)]).to(dev)
    integral = ops.integral_image(feat)
    vox = ops.project_gather(integral, calibs, grid, zl, co, kind, size, cell_begin=begin, cell_count=count)
    gen = torch.Generator(device="cpu").manual_seed(11)
    gvox = torch.randn(vox.shape, generator=gen).to(dev)
    _, _, visible = ops.box_params(calibs, grid, zl, co, kind, size, feat.shape[-2:])
    live = visible[:, :, begin:begin + count].permute(0, 2, 1).bool()
    live = live[..., None].expand(-1, -1, -1, C).reshape(vox.shape)
    assert live.any()
    gvox = torch.where(live, gvox, torch.full_like(gvox, 1e30))  # masked voxels pass no gradient, whatever arrives

    def bwd(**kw):
        return ops.project_gather_backward(gvox, tuple(integral.shape), calibs, grid, zl, co, kind, size, cell_begin=begin,
                                           cell_count=count, grid_w=grid4.shape[-2], **kw)
    return dict(integral=integral, vox=vox, gvox=gvox, live=live, bwd=bwd)


SCATTER_CASES = [("multiviewc_156x156x5", 2, (0, None), None, 256),
                 ("multiviewc_200x200x1", 3, (0, None), None, 256),
                 ("wildtrack_120x360x8", 2, (1003, 20011), None, 256),
                 ("multiviewx_160x250x8", 2, (77, 13), None, 256),
                 ("multiviewc_200x200x1", 2, (5, 80), (7, 13), 256),
                 ("multiviewc_156x156x5", 3, (0, None), (9, 5), 256),
                 ("multiviewc_200x200x1", 2, (3, 200), (20, 30), 8)]


@pytest.mark.parametrize("workload,n_cam,cells,crop,C", SCATTER_CASES)
def test_det_scatter_repeats_and_matches_atomic_scatter(workload, n_cam, cells, crop, C):
    k = _scatter_case(workload, n_cam, cells, crop, C)
    det = k["bwd"](deterministic=True)
    again = k["bwd"](deterministic=True)
    assert torch.equal(det, again), "two deterministic calls differ"
    assert torch.isfinite(det).all(), "masked voxels (1e30) leaked into the result"
    ref = k["bwd"](deterministic=False, kernel="direct")
    scale = ref.abs().max().item()
    assert scale > 0
    torch.testing.assert_close(det, ref, rtol=1e-4, atol=2e-5 * scale)
    # accumulate = exactly one add of the plain result
    base = torch.randn(det.shape, generator=torch.Generator().manual_seed(3)).to(det.device)
    acc = k["bwd"](deterministic=True, out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + det)
    # adjoint: <pool(I), G> == <I, pool^T(G)>
    g = torch.where(k["live"], k["gvox"], torch.zeros_like(k["gvox"])).double()
    lhs = (k["vox"].double() * g).sum().item()
    rhs = (k["integral"].double() * det.double()).sum().item()
    norm = (k["vox"].double().abs() * g.abs()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * norm, (lhs, rhs, norm)


def test_det_scatter_ignores_reserved_cus_and_rejects_a_wrong_workspace():
    from vfa_amd import _lib, ops
    k = _scatter_case("multiviewc_200x200x1", 3, (0, None), None, 256)
    a = k["bwd"](deterministic=True, reserved_cus=0)
    b = k["bwd"](deterministic=True, reserved_cus=128)
    assert torch.equal(a, b)
    # a workspace of another size: VFA_ERR_BAD_ARGUMENT, nothing written
    n, Hp, Wp, C = k["integral"].shape
    need = ops.det_workspace_bytes(n, 1, 40000, C, Hp - 2, Wp - 2)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=a.device)
    out = torch.full_like(a, 7.0)
    zl = torch.zeros(1, device=a.device)
    co = torch.zeros(8, 3, device=a.device)
    grid = torch.zeros(40000, 3, device=a.device)
    cal = torch.zeros(n, 12, device=a.device)
    rc = _lib.lib().vfa_project_gather_backward_det_f32(
        _lib.ptr(k["gvox"]), _lib.ptr(cal), _lib.ptr(grid), _lib.ptr(zl), _lib.ptr(co), _lib.ptr(out), n, C, Hp - 2, Wp - 2, 1,
        40000, 0, 40000, 0, 0, 1.0, 1.0, -1.0, 0.95, 0, _lib.ptr(ws), need + 256, None)
    torch.cuda.synchronize()
    assert rc == 10001
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("rows", [1, 7, 20000, 100003])
def test_column_sum_is_fixed_order(rows):
    from vfa_amd import ops
    dev = torch.device("cuda:0")
    x = torch.randn(rows, 256, generator=torch.Generator().manual_seed(rows)).to(dev)
    a = ops.column_sum(x)
    assert torch.equal(a, ops.column_sum(x))
    base = torch.randn(256, generator=torch.Generator().manual_seed(1)).to(dev)
    assert torch.equal(ops.column_sum(x, out=base.clone(), accumulate=True), base + a)
    want = x.double().sum(0)
    tol = 1e-6 * x.double().abs().sum(0).max().item() + 1e-6
    assert (a.double() - want).abs().max().item() <= tol
    y = torch.randn(rows, 37, generator=torch.Generator().manual_seed(2)).to(dev)  # any N
    torch.testing.assert_close(ops.column_sum(y).double(), y.double().sum(0), rtol=1e-5, atol=1e-5 * max(rows, 1) ** 0.5)


FRAMES = [("multiviewc_200x200x1", None), ("wildtrack_120x360x8", (40, 64))]


def _frame(workload, crop):
    """Modules, lateral maps, calibs and grid of a frame: the bench frame (7 cameras) or a Wildtrack crop."""
    import vfa_amd
    from vfa_amd.synthetic import make_workload
    dev = torch.device("cuda:0")
    wl = make_workload(workload, channels=256, seed=0)
    n = wl["n_cam"]
    torch.manual_seed(0)
    mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
    lats = [torch.cat([wl["features"][c][s] for c in range(n)]).to(dev) for s in range(3)]
    grid = wl["grid"] if crop is None else wl["grid"][:, 30:30 + crop[0], 100:100 + crop[1]].contiguous()
    return mods, lats, wl["calibs"].to(dev), grid.to(dev)


def _step_grads(frame, fused):
    import vfa_amd
    from vfa_amd import vfa_op
    mods, lats, calibs, grid = frame
    keep = vfa_op.FUSED_TRAIN
    vfa_op.FUSED_TRAIN = fused
    try:
        for m in mods:
            m.zero_grad(set_to_none=True)
        ls = [l.detach().clone().requires_grad_(True) for l in lats]
        out = vfa_amd.aggregate_views(*mods, *ls, calibs, grid)
        probe = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(out.device)
        (out * probe).sum().backward()
        torch.cuda.synchronize()
        return ([l.grad.clone() for l in ls] + [m.collapse.weight.grad.clone() for m in mods]
                + [m.collapse.bias.grad.clone() for m in mods])
    finally:
        vfa_op.FUSED_TRAIN = keep


def _digest(grads):
    h = hashlib.sha256()
    for g in grads:
        h.update(g.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("workload,crop", FRAMES)
def test_whole_frame_backward_is_bit_reproducible(workload, crop, fused):
    frame = _frame(workload, crop)
    with deterministic():
        a = _step_grads(frame, fused)
        b = _step_grads(frame, fused)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two deterministic training steps gave different gradients"
    ref = _step_grads(frame, fused)  # default mode: the atomic kernels
    for x, y in zip(a, ref):
        torch.testing.assert_close(x, y, rtol=1e-3, atol=1e-4 * y.abs().max().item())


_CHILD = r"""
import sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import test_deterministic_backward as t
frame = t._frame({workload!r}, {crop!r})
with t.deterministic():
    print("DIGEST", t._digest(t._step_grads(frame, {fused!r})))
"""


@pytest.mark.parametrize("fused", [True, False])
def test_gradients_repeat_across_processes(fused):
    workload, crop = FRAMES[1]
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), workload=workload, crop=crop, fused=fused)
    res = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    child = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("DIGEST")]
    assert len(child) == 1, res.stdout[-2000:]
    with deterministic():
        mine = _digest(_step_grads(_frame(workload, crop), fused))
    assert child[0] == mine


_BIAS_ARG = {"vfa_relu_mask_backward_f32": 4, "vfa_collapse_gemm_relu_backward_f32": 5, "vfa_collapse_gemm_relu_backward_f16_f32": 5}
_NEW = {"vfa_project_gather_backward_det_f32", "vfa_column_sum_f32"}
_ATOMIC = {"vfa_project_gather_backward_grid_f32", "vfa_project_gather_backward_f32"}


@pytest.mark.parametrize("fused", [True, False])
def test_kernel_selection_follows_the_switch(monkeypatch, fused):
    from vfa_amd import ops
    calls = []
    real = ops._launch

    def spy(name, *args, **kw):
        calls.append((name, args))
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "_launch", spy)
    frame = _frame(*FRAMES[1])
    with deterministic():
        _step_grads(frame, fused)
    names = [c[0] for c in calls]
    assert not _ATOMIC & set(names), sorted(set(names))
    assert "vfa_project_gather_backward_det_f32" in names and "vfa_column_sum_f32" in names
    for name, args in calls:
        if name in _BIAS_ARG:
            assert args[_BIAS_ARG[name]] is None, f"{name} got a bias-gradient pointer in deterministic mode"
    calls.clear()
    with deterministic(False):
        _step_grads(frame, fused)
    names = [c[0] for c in calls]
    assert not _NEW & set(names), sorted(set(names))
    assert "vfa_project_gather_backward_grid_f32" in names
    assert any(args[_BIAS_ARG[name]] is not None for name, args in calls if name in _BIAS_ARG)
