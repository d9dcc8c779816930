"""The float64 reference of the pooling adjoint (tests/adjoint_common.py) and the cases of tests/test_pool_adjoint.py, checked on the
CPU (no GPU): the restatement is the adjoint float64 autograd computes, torch's own fp32 autograd of the same composition stays
inside the derived bound, and every case meets the condition it was built for -- counted from the CPU boxes, never from a kernel."""
import pytest
import torch

import adjoint_common as ac

C_SMALL = 6  # the reference and the bound do not depend on the channel count


def _autograd_adjoint(case, dtype):
    """d integral of <pool(integral), grad_vox> by torch autograd through the ``grid_sample`` composition, on the image (n, Hf, Wf, C)."""
    integral = torch.zeros(case.n, case.C, case.Hf, case.Wf, dtype=dtype, requires_grad=True)
    vox = ac.pool(integral, case.box, case.area, case.visible)
    g, = torch.autograd.grad(vox, integral, case.gvox.to(dtype))
    return g.permute(0, 2, 3, 1)


def _cpu_cases():
    return ([ac.scene(m, C_SMALL) for m in range(3)] + [ac.levels("lines", C_SMALL), ac.duplicates(5, C_SMALL, cells=257),
                                                        ac.ranges(13, C_SMALL)])


@pytest.mark.parametrize("index", range(6))
def test_restatement_is_the_adjoint_float64_autograd_computes(index):
    case = _cpu_cases()[index]
    r = case.ref
    got = _autograd_adjoint(case, torch.float64)
    want = r.want[:, 1:-1, 1:-1]
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"[adjoint] {case.name}: restatement vs float64 autograd {err:.2e} on max|want| {scale:.3g}")
    assert scale > 0 and err <= 1e-12 * scale, (err, scale)
    # A and count are the same scatter of |.|: A bounds |want| elementwise, and count is 16 per visible box in all
    assert bool((r.A >= r.want.abs() * (1 - 1e-12)).all()) and bool((r.B >= r.A * (1 - 1e-12)).all())
    assert r.count.sum().item() == 16 * case.stats.n_visible


@pytest.mark.parametrize("index", range(6))
def test_fp32_torch_autograd_stays_inside_the_derived_bound(index):
    """What validates K_X and K_R: another fp32 implementation of the same composition (torch's grid_sample backward, its division
    and sequential index adds), none of whose code the kernels share."""
    case = _cpu_cases()[index]
    r = case.ref
    got = _autograd_adjoint(case, torch.float32)
    padded = torch.zeros(case.integral_shape)
    padded[:, 1:-1, 1:-1] = got
    ratio = ac.worst_ratio(padded, r)
    bound = r.bound[:, 1:-1, 1:-1]
    nz = r.want[:, 1:-1, 1:-1].abs()
    nz = nz[nz > 0]
    print(f"[adjoint] {case.name}: fp32 torch autograd worst err / bound {ratio:.3f}; median bound {bound[bound > 0].median().item():.2e} "
          f"on a median non-zero |want| of {nz.median().item():.2e}")
    assert ratio <= 1.0, ratio
    if index < 3:  # (the scenes; a pile of thousands of boxes on one tap has a bound that grows with the pile)
        assert bound[bound > 0].median().item() <= 1e-3 * nz.median().item()  # a sharp bound: below 0.1 % of a median element


def test_a_wrong_corner_weight_leaves_the_bound():
    """The bound notices what the kernel-to-kernel tolerance lets pass: the adjoint with ONE tap weight of ONE sample negated (the
    ``ne`` tap of ``rt``) on a single box is outside it."""
    case = ac.scene(0, C_SMALL)
    r = case.ref
    box = case.box
    v, l, c = case.visible.nonzero()[case.stats.n_visible // 2].tolist()
    # the tap (y0, x0 + 1) of the sample (right, top) of that box
    X = ((box[v, l, c, 2].double() + 1) * case.Wf - 1) / 2
    Y = ((box[v, l, c, 1].double() + 1) * case.Hf - 1) / 2
    x0, y0 = int(torch.floor(X)), int(torch.floor(Y))
    w = (1 - (Y - y0)) * (X - x0)
    wrong = r.want.clone()
    row, col = min(max(y0, -1), case.Hf) + 1, min(max(x0 + 1, -1), case.Wf) + 1
    delta = 2 * w * case.gvox.view(case.n, case.cell_count, case.nl, case.C)[v, c, l].double() / case.area[v, l, c].double()
    wrong[v, row, col] += delta  # (- (-w g / area) instead of + (-w g / area))
    assert 1 <= row <= case.Hf and 1 <= col <= case.Wf and delta.abs().max() > 0
    assert ac.worst_ratio(wrong, r) > 100.0


# ------------------------------------------------------------------------------------------------ the conditions of the GPU cases
def test_scene_condition():
    classes = 0
    for m in range(3):
        s = ac.scene(m, C_SMALL).stats
        assert 0.05 < s.visible_share < 0.95, s.visible_share
        assert s.clamped_share >= 0.10, s.clamped_share
        classes = classes + s.classes
    assert classes.min() >= 16, classes.tolist()            # each of the nine (dx, dy) classes, over the three maps
    case = ac.scene(0, C_SMALL)
    assert case.n == 2 and case.nl == 3 and case.n_cells == 14 * 18 and case.n_cells % case.grid_w == 0
    assert not bool(case.visible.all()) and s.multi_piece_lists > 0


def test_duplicates_condition():
    one = ac.duplicates(1, C_SMALL).stats
    assert one.visible_share == 1.0 and one.longest_run == ac.RUN_CHUNK                       # runs of the full 32
    assert int((one.lines[:, 0] > 0).sum()) == 65 and one.lines[:64, 0].max() <= 16          # 32 identical boxes per tile: one tap set
    assert one.max_records >= ac.DUP_CELLS and one.max_pieces >= 8
    five = ac.duplicates(5, C_SMALL).stats
    assert five.visible_share == 1.0 and five.max_records >= ac.DUP_CELLS and five.max_pieces >= 8
    case = ac.duplicates(1, C_SMALL)
    assert case.grid_w > 0 and case.n_cells % case.grid_w == 0 and int((one.patches[:, 0] > 0).sum()) > 64


@pytest.mark.parametrize("kind", ["lines", "patches"])
def test_levels_condition(kind):
    case = ac.levels(kind, C_SMALL)
    tiles = case.stats.lines if kind == "lines" else case.stats.patches
    l1, l2, l3 = ac.level_counts(tiles)
    assert l1 >= 8 and l2 >= 8 and l3 >= 8, (l1, l2, l3)
    assert l1 + l2 + l3 == tiles.shape[0]                  # no tile near a threshold
    assert (case.grid_w > 0) == (kind == "patches") and case.n_cells % max(case.grid_w, 1) == 0


@pytest.mark.parametrize("grid_w", [13, 18])
def test_ranges_condition(grid_w):
    case = ac.ranges(grid_w, C_SMALL)
    assert case.grid_w == grid_w and case.n_cells % grid_w == 0
    assert (case.n_cells // grid_w) % 4 != 0                                                  # rows no multiple of 4
    assert case.cell_begin % grid_w % 8 != 0 and (case.cell_begin // grid_w) % 4 != 0         # the range begins inside a patch
    assert case.cell_count % 32 != 0 and case.cell_begin + case.cell_count < case.n_cells
    assert grid_w % 8 != 0 and 0.05 < case.stats.visible_share < 0.95
    assert case.stats.patches.shape[0] > 0 and case.stats.lines.shape[0] > 0


def test_masked_condition():
    case = ac.scene(0, C_SMALL)
    masked = int((~case.visible).sum())
    assert masked >= 16 and masked < case.visible.numel()
