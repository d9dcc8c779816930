"""``vfa_project_gather_backward_geometry_f32`` ELEMENTWISE against a float64 reference of its own operation under a derived bound
(tests/geombound_common.py: the reference, the derivation, the cases; tests/test_geometry_bound_cpu.py: the reference against float64
autograd, fp32 torch inside the bound, mutants outside it, the condition of every case).   -m gpu.

The tests call ``ops.project_gather_backward_geometry`` directly.  The integral image is ``ops.integral_image``'s, copied to the CPU,
so the reference reads the very fp32 values the kernel did.  No element is excluded: where nothing contributes the bound is 0 and the
kernel's value must be exactly 0.  Every test prints its worst err / bound for d calibs and d grid before it asserts <= 1."""
from types import SimpleNamespace

import pytest
import torch

import geombound_common as gb

pytestmark = pytest.mark.gpu


def _setup(case):
    """The case's operands on the device (once per case), the device's integral image on the CPU and the reference computed from it --
    after the device's boxes have been found equal to the CPU boxes bit for bit."""
    s = getattr(case, "_gpu", None)
    if s is None:
        from vfa_amd import ops
        d = torch.device("cuda:0")
        s = case._gpu = SimpleNamespace(geometry=tuple(t.to(d) for t in (case.calibs, case.grid_flat, case.zl, case.co)))
        s.integral = ops.integral_image(case.features.to(d))
        s.ref = case.reference(s.integral.cpu())
        box, area, visible = ops.box_params(*s.geometry, case.kind, case.image_wh, (case.Hf, case.Wf))
        sl = slice(case.cell_begin, case.cell_begin + case.cell_count)
        assert gb._same_bits(box.cpu()[:, :, sl], s.ref.box) and gb._same_bits(area.cpu()[:, :, sl], s.ref.area), f"{case.name}: device boxes differ"
        assert torch.equal(visible.cpu()[:, :, sl].bool(), s.ref.visible), f"{case.name}: device visibility differs"
    return s


def _call(case, gvox=None, integral=None, grid_flat=None, cell_begin=None, cell_count=None, **kw):
    from vfa_amd import ops
    s = _setup(case)
    calibs, grid, zl, co = s.geometry
    gvox = (case.gvox if gvox is None else gvox).to(calibs.device)
    return ops.project_gather_backward_geometry(gvox, s.integral if integral is None else integral, calibs,
                                                grid if grid_flat is None else grid_flat.to(calibs.device), zl, co, case.kind, case.image_wh,
                                                cell_begin=case.cell_begin if cell_begin is None else cell_begin,
                                                cell_count=case.cell_count if cell_count is None else cell_count, **kw)


def _check(label, got, r, base=None):
    (wc, bc), (wg, bg) = (r.want_calibs, r.bound_calibs), (r.want_grid, r.bound_grid)
    if base is not None:
        (wc, bc), (wg, bg) = gb.with_base(wc, bc, base[0]), gb.with_base(wg, bg, base[1])
    q_cal, q_grid = gb.ratio(got[0], wc, bc), gb.ratio(got[1], wg, bg)
    print(f"[geometry] {label}: worst err / bound, d calibs {q_cal:.2g}, d grid {q_grid:.2g}")
    assert q_cal <= 1.0 and q_grid <= 1.0, f"{label}: worst err / bound, d calibs {q_cal:.2g}, d grid {q_grid:.2g}"


def _run(case):
    _check(case.name, _call(case), _setup(case).ref)
    return _setup(case).ref


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("C", [6, 8, 70, 256, 260])
def test_scene_by_channels(C):
    """2 views, 252 cells = 31 tiles of 8 and a tail of 4, three layers, the 23 x 40 map.  C = 6 and 70: the scalar kernel (fewer
    channels than lanes; some lanes take a second step); 8: two active lanes of float4; 260: one lane in a second float4 step."""
    r = _run(gb.scene(0, C))
    sharp = (r.bound_grid / r.want_grid.abs())[r.want_grid != 0].median().item()
    print(f"[geometry] scene C {C}: median bound / |want| over d grid {sharp:.2e}; {r.cells_empty} cells without a visible box")


@pytest.mark.parametrize("map_index", [1, 2])
def test_scene_other_maps(map_index):
    """The 12 x 20 and 6 x 10 maps: clamped edges on integer pixel coordinates, taps on the zero border."""
    _run(gb.scene(map_index, 8))


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("data", ["MultiviewX", "Wildtrack"])
def test_other_conversions(data, C):
    """The 1/40 scale; the 2.5 scale and its offset.  One view; C = 5: the scalar kernel."""
    _run(gb.conversion(data, C))


@pytest.mark.parametrize("views", [1, 2])
def test_more_than_256_tiles(views):
    """257 tiles: the strided loop of ``geom_calib_reduce_kernel``, a tail tile of one cell."""
    _run(gb.many_tiles(views))


def test_exact_ties():
    """An affine camera: corners k and k + 4 tie exactly and unclamped; the gradient goes to the lower index."""
    assert _run(gb.affine_ties()).items_tied > 0


def test_camera_inside_the_scene():
    """Corners behind the camera: h2 < 0 in the perspective division."""
    assert _run(gb.camera_inside()).items_behind > 0


# ------------------------------------------------------------------------------------------------ ranges, accumulate, wanted outputs
def test_cell_range():
    """cell_begin = 23, cell_count = 201 against the reference of that range; its d grid rows are the whole-range call's bit for bit."""
    case = gb.scene_range()
    got = _call(case)
    _check(case.name, got, _setup(case).ref)
    whole = torch.randn(case.n, case.n_cells, case.nl * case.C, generator=torch.Generator().manual_seed(1))
    whole[:, case.cell_begin:case.cell_begin + case.cell_count] = case.gvox
    _, g_whole = _call(case, gvox=whole, cell_begin=0, cell_count=case.n_cells)
    assert torch.equal(g_whole[case.cell_begin:case.cell_begin + case.cell_count], got[1])


def test_accumulate():
    """``accumulate=True`` onto non-zero outputs: the bound plus one rounding of the add."""
    case = gb.scene(0, 8)
    gen = torch.Generator().manual_seed(2)
    base = torch.randn(case.n, 12, generator=gen), torch.randn(case.cell_count, 3, generator=gen)
    dev = _setup(case).geometry[0].device
    out = tuple(b.to(dev) for b in base)
    got = _call(case, grad_calibs=out[0], grad_grid=out[1], accumulate=True)
    assert got[0] is out[0] and got[1] is out[1]
    _check(case.name + ", accumulate", got, _setup(case).ref, base=base)
    plain = _call(case)
    assert torch.equal(got[0], base[0].to(dev) + plain[0]) and torch.equal(got[1], base[1].to(dev) + plain[1])  # exactly one add


def test_wanted_outputs():
    """``want_calibs`` or ``want_grid`` alone: the bits of the call that wants both."""
    case = gb.scene(0, 8)
    both = _call(case)
    c_only, none_g = _call(case, want_grid=False)
    none_c, g_only = _call(case, want_calibs=False)
    assert none_g is None and none_c is None
    assert torch.equal(c_only, both[0]) and torch.equal(g_only, both[1])
    _check(case.name + ", one output each", (c_only, g_only), _setup(case).ref)


# ------------------------------------------------------------------------------------------------ masked boxes, NaN, alignment
def test_masked_boxes_pass_nothing():
    """``grad_vox`` filled with NaN under every masked box: the bits of the call with zeros there."""
    case = gb.scene(0, 8)
    r = _setup(case).ref
    live = r.visible.permute(0, 2, 1)[..., None].expand(-1, -1, -1, case.C).reshape(case.gvox.shape)
    assert not bool(live.all())
    zeros = _call(case, gvox=torch.where(live, case.gvox, torch.zeros_like(case.gvox)))
    nans = _call(case, gvox=torch.where(live, case.gvox, torch.full_like(case.gvox, float("nan"))))
    _check(case.name + ", NaN under masked boxes", nans, r)
    assert torch.equal(nans[0], zeros[0]) and torch.equal(nans[1], zeros[1])


def test_nan_cell():
    """One grid cell set to NaN: its d grid row is exactly zero; the other cells of its tile, d calibs and every other row are the bits
    of the call where that cell lies far outside every view."""
    case = gb.scene(0, 8)
    r = _setup(case).ref
    seen = r.visible.any(0).any(0)
    cell = next(c for c in range(8 * 12 + 3, case.cell_count, 8) if bool(seen[c - 3:c + 5].all()))   # slot 3 of a tile whose cells are all seen
    away, nan = case.grid_flat.clone(), case.grid_flat.clone()
    away[cell] = torch.tensor([3.0e6, -2.0e6, 0.0])
    nan[cell] = float("nan")
    r_away = case.reference(_setup(case).integral.cpu(), grid_flat=away)
    assert not bool(r_away.visible[:, :, cell].any()) and bool(r.visible[:, :, cell].any())
    got_away, got_nan = _call(case, grid_flat=away), _call(case, grid_flat=nan)
    _check(case.name + ", one cell away", got_away, r_away)
    _check(case.name + ", one cell NaN", got_nan, r_away)
    assert bool((got_nan[1][cell] == 0).all()) and bool((r_away.bound_grid[cell] == 0).all())
    assert torch.equal(got_nan[0], got_away[0]) and torch.equal(got_nan[1], got_away[1])
    assert not torch.equal(got_away[1], _call(case)[1])


def test_misaligned_pointers():
    """A contiguous ``grad_vox`` and integral image at a storage offset of one float, C = 8: the scalar fallback, within the bound."""
    case = gb.scene(0, 8)
    s = _setup(case)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=s.integral.device)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out

    got = _call(case, gvox=shifted(case.gvox.to(s.integral.device)), integral=shifted(s.integral))
    _check(case.name + ", pointers off by one float", got, s.ref)
