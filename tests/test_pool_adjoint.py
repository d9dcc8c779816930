"""The backward of the box pooling, every kernel and path ELEMENTWISE against a float64 reference of the adjoint under a derived
bound (tests/adjoint_common.py: the reference, the derivation of the bound, the cases; tests/test_pool_adjoint_cpu.py: the reference
against autograd, fp32 torch inside the bound, the condition of every case).   -m gpu.

Paths of ``ops.project_gather_backward``:
    direct   ``gather_backward_kernel``: the nine ``scatter_run<DYC, DXC>`` variants, runs of up to 32 boxes summed in registers
    lines    ``gather_backward_cached_kernel`` on 32 cells in a line (C = 256, grid_w = 0): 128-entry table, rows of 8, per-box atomics
    patches  the same kernel on 4 x 8 patches of the ground grid (grid_w > 0)
    det      ``vfa_project_gather_backward_det_f32``: emit, radix sort, piece merge, fix-up of lists that cross 256-record pieces
The interior [1:-1, 1:-1] is compared; the border ring is outside the contract and only has to be finite.  Every test prints its
worst err / bound."""
from types import SimpleNamespace

import pytest
import torch

import adjoint_common as ac

pytestmark = pytest.mark.gpu

ATOMIC = ("direct", "lines", "patches")
ALL = ATOMIC + ("det",)


def _device(case):
    """The case's operands on the device -- after the device's boxes have been found equal to the CPU boxes bit for bit."""
    dev = getattr(case, "_dev", None)
    if dev is None:
        from vfa_amd import ops
        d = torch.device("cuda:0")
        dev = case._dev = tuple(t.to(d) for t in (case.calibs, case.grid_flat, case.zl, case.co))
        box, area, visible = ops.box_params(*dev, ac.CONV_KIND, ac.IMAGE_SIZE[::-1], (case.Hf, case.Wf))
        assert torch.equal(box.cpu().view(torch.int32), case.box_all.contiguous().view(torch.int32)), f"{case.name}: device boxes differ"
        assert torch.equal(area.cpu().view(torch.int32), case.area_all.contiguous().view(torch.int32)), f"{case.name}: device areas differ"
        assert torch.equal(visible.cpu().bool(), case.visible_all), f"{case.name}: device visibility differs"
    return dev


def _scatter(case, path, gvox=None, cell_begin=None, cell_count=None, **kw):
    from vfa_amd import ops
    dev = _device(case)
    if path in ("lines", "patches"):
        assert case.C == 256, "the LDS-privatised kernel runs at C = 256 only"
    if path == "patches":
        assert case.grid_w > 0 and case.n_cells % case.grid_w == 0
    sel = dict(direct=dict(kernel="direct", grid_w=0, deterministic=False), lines=dict(grid_w=0, deterministic=False),
               patches=dict(grid_w=case.grid_w, deterministic=False), det=dict(grid_w=case.grid_w, deterministic=True))[path]
    gvox = case.gvox if gvox is None else gvox
    return ops.project_gather_backward(gvox.to(dev[0].device), case.integral_shape, *dev, ac.CONV_KIND, ac.IMAGE_SIZE[::-1],
                                       cell_begin=case.cell_begin if cell_begin is None else cell_begin,
                                       cell_count=case.cell_count if cell_count is None else cell_count, **sel, **kw)


def _check(got, r, label):
    assert bool(torch.isfinite(got).all()), f"{label}: the output (ring included) is not finite"
    ratio = ac.worst_ratio(got, r)
    print(f"[adjoint] {label}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{label}: worst err / bound {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------ scene
@pytest.mark.parametrize("C,path", [(256, p) for p in ALL] + [(C, p) for C in (7, 8, 260) for p in ("direct", "det")])
def test_scene(C, path):
    """Two cameras, three layers, the maps 23 x 40, 12 x 20 and 6 x 10: every (dx, dy) class, clamped boxes, masked boxes.  C = 7: the
    scalar paths; C = 8: the vector path of ``det``; C = 260: a second block of channels."""
    for m in range(3):
        case = ac.scene(m, C)
        _check(_scatter(case, path), case.ref, f"{case.name} {path}")


# ------------------------------------------------------------------------------------------------ duplicates
@pytest.mark.parametrize("nl", [1, 5])
@pytest.mark.parametrize("path", ALL)
def test_duplicates(nl, path):
    """One ground point 2049 times: runs of the full 32 (``direct``, nl = 1), 32 identical boxes per tile (cached), lists of >= 2049
    records per tap over >= 8 merge pieces (``det``).  And linearity: with one gradient for every cell the result is 2049 times the
    result of one cell."""
    case = ac.duplicates(nl)
    _check(_scatter(case, path), case.ref, f"{case.name} {path}")
    k = case.cell_count
    g1 = case.gvox[:, :1].contiguous()
    one = ac.adjoint_reference(case.box[:, :, :1], case.area[:, :, :1], case.visible[:, :, :1], g1, case.Hf, case.Wf)
    many = SimpleNamespace(want=k * one.want, count=k * one.count)
    many.bound = ac.K_X * max(case.Hf, case.Wf) * ac.U * k * one.B + ac.gamma(many.count + ac.K_R)[..., None] * k * one.A
    got_many = _scatter(case, path, gvox=g1.repeat(1, k, 1))
    got_one = _scatter(case, path, gvox=g1, cell_count=1)
    _check(got_many, many, f"{case.name} {path}, one gradient for all")
    _check(got_one, one, f"{case.name} {path}, one cell")
    diff = (got_many.double() - k * got_one.double()).abs().cpu()[:, 1:-1, 1:-1]
    assert bool((diff <= (many.bound + k * one.bound)[:, 1:-1, 1:-1]).all()), f"{case.name} {path}: {k} cells are not {k} x one cell"


# ------------------------------------------------------------------------------------------------ levels of the cached kernel
@pytest.mark.parametrize("kind,path", [("lines", "lines"), ("lines", "direct"), ("lines", "det"),
                                       ("patches", "patches"), ("patches", "lines"), ("patches", "direct"), ("patches", "det")])
def test_levels(kind, path):
    """Tiles clear of the thresholds of ``gather_backward_cached_kernel``, eight or more on each of its three levels, as 32 cells in
    a line and as 4 x 8 patches (counted on the CPU: tests/test_pool_adjoint_cpu.py::test_levels_condition)."""
    case = ac.levels(kind)
    _check(_scatter(case, path), case.ref, f"{case.name} {path}")


# ------------------------------------------------------------------------------------------------ ranges, accumulate
@pytest.mark.parametrize("grid_w", [13, 18])
@pytest.mark.parametrize("path", ALL)
def test_ranges(grid_w, path):
    """A ground grid whose width is no multiple of 8 and whose rows are no multiple of 4, a range that begins inside a patch and
    whose length is no multiple of 32; ``accumulate=True`` onto a random base.
    Accumulation: ``det`` adds its result once -- bit for bit fp32(base + plain).  The atomic paths add their (at most ``count``)
    partial sums to the base one by one, in any order: a sum of count + 1 terms, whose error beyond the bound of the plain result
    (which holds the terms' own errors and their sum) is at most gamma(count + 1) |base|; where nothing contributes, the base stays."""
    case = ac.ranges(grid_w)
    r = case.ref
    plain = _scatter(case, path)
    _check(plain, r, f"{case.name} {path}")
    base = torch.randn(case.integral_shape, generator=torch.Generator().manual_seed(7))
    acc = _scatter(case, path, out=base.to(plain.device), accumulate=True)
    assert bool(torch.isfinite(acc).all())
    if path == "det":
        assert torch.equal(acc, base.to(plain.device) + plain)
    touched = (r.bound > 0).to(torch.float64)  # (count > 0, or a tap only a flipped floor reaches)
    with_base = SimpleNamespace(want=r.want + base.double(), bound=r.bound + touched * ac.gamma(r.count + 1)[..., None] * base.double().abs())
    _check(acc, with_base, f"{case.name} {path}, accumulate")


# ------------------------------------------------------------------------------------------------ masked boxes
@pytest.mark.parametrize("path", ALL)
def test_masked_boxes_pass_nothing(path):
    """The gradient of a masked box may hold anything: NaN and 1e30 leave ``det`` unchanged bit for bit and the atomic paths inside
    the bound (the whole output finite)."""
    case = ac.scene(0, 256)
    clean = _scatter(case, path)
    for fill in (float("nan"), 1e30):
        g = torch.where(case.live, case.gvox, torch.full_like(case.gvox, fill))
        got = _scatter(case, path, gvox=g)
        _check(got, case.ref, f"{case.name} {path}, masked = {fill}")
        if path == "det":
            assert torch.equal(got, clean)


# ------------------------------------------------------------------------------------------------ d integral -> d feature
def _rev(x, dim):
    return x.flip(dim).cumsum(dim).flip(dim)


INTEGRAL_ROUND = ac.U * (1 + 2.0 ** -20)  # (second order: the row pass sums column scans that are themselves rounded)


@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (9, 1), (9, 33), (9, 70)])
@pytest.mark.parametrize("C", [7, 64, 70, 256, 260])
def test_integral_backward_against_float64_reverse_cumsums(C, hw):
    """``integral_image_backward``: the column pass accumulates in double and rounds each column scan once, the row pass sums those
    in double and rounds once:  |got - want| <= u (|want| + sum over the columns x' >= x of |column scan|).  Widths past one and two
    32-column chunks, channel counts that leave a partial wave; the ring holds large values that must not leak."""
    from vfa_amd import ops
    H, W = hw
    g = torch.randn(2, H + 2, W + 2, C, generator=torch.Generator().manual_seed(C * 100 + H * W))
    ring = torch.ones(H + 2, W + 2, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    g[:, ring] *= 1e3
    cols = _rev(g[:, 1:-1, 1:-1].double(), 1)
    want = _rev(cols, 2)
    bound = INTEGRAL_ROUND * (want.abs() + _rev(cols.abs(), 2))
    got = ops.integral_image_backward(g.to("cuda:0")).double().cpu().permute(0, 2, 3, 1)
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"[adjoint] integral backward C {C} map {hw}: worst err / bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, ratio


def test_chain_gradient_of_the_features():
    """grad_vox -> ``det`` scatter -> ``integral_image_backward`` against float64 autograd through cumsum . cumsum and the pooling.
    With b the scatter's bound, R the reverse cumsums (Ry, Rx) and s the reference scatter, the composed bound is
        Ry Rx b  +  u (|want| + Ry Rx b + Rx (|Ry s| + Ry b)):
    the scatter's error through the (linear) scans, plus the scans' own roundings on what they were given."""
    from vfa_amd import ops
    case = ac.scene(1, 70)
    feature = torch.zeros(case.n, case.C, case.Hf, case.Wf, dtype=torch.float64, requires_grad=True)
    vox = ac.pool(torch.cumsum(torch.cumsum(feature, -1), -2), case.box, case.area, case.visible)
    want, = torch.autograd.grad(vox, feature, case.gvox.double())
    want = want.permute(0, 2, 3, 1)
    s, b = case.ref.want[:, 1:-1, 1:-1], case.ref.bound[:, 1:-1, 1:-1]
    through = _rev(_rev(b, 1), 2)
    bound = through + INTEGRAL_ROUND * (want.abs() + through + _rev(_rev(s, 1).abs() + _rev(b, 1), 2))
    got = ops.integral_image_backward(_scatter(case, "det")).double().cpu().permute(0, 2, 3, 1)
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"[adjoint] chain {case.name}: worst err / bound {ratio:.3f}")
    assert want.abs().max() > 0 and bool(torch.isfinite(got).all()) and ratio <= 1.0, ratio
