"""The float64 reference of the geometry gradient and its per-element bound (tests/geombound_common.py), checked on the CPU without the
kernel: the reference is what float64 autograd computes, torch's own fp32 autograd of the same composition stays inside the derived
bound (this is what checks the constants), seven wrong variants of the reference leave it, and every case of
tests/test_geometry_bound.py meets the conditions it was built for -- decided by the reference alone, never by a kernel."""
import pytest
import torch

import geombound_common as gb

INDICES = range(len(gb.TABLE))
# mutant -> the case of gb.TABLE that must expose it
EXPOSED_BY = {"a": (gb.scene, (0, 8)), "b": (gb.scene, (0, 8)), "c": (gb.affine_ties, ()), "d": (gb.scene, (0, 8)),
              "e": (gb.many_tiles, (1,)), "f": (gb.conversion, ("MultiviewX", 5)), "g": (gb.scene, (0, 6))}


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("index", INDICES)
def test_reference_is_float64_autograd_on_the_given_boxes(index):
    case = gb.table_case(index)
    r = case.ref
    d_cal, d_grid = gb.autograd_reference(case, case.integral, torch.float64)
    e_cal, e_grid = _rel(d_cal, r.want_calibs), _rel(d_grid, r.want_grid)
    print(f"[geometry] {case.name}: reference vs float64 autograd, d calibs {e_cal:.2e}, d grid {e_grid:.2e} (max norm, relative)")
    assert r.want_calibs.abs().max() > 0 and r.want_grid.abs().max() > 0
    assert e_cal <= 1e-9 and e_grid <= 1e-9, (e_cal, e_grid)


@pytest.mark.parametrize("index", INDICES)
def test_fp32_torch_autograd_stays_inside_the_derived_bound(index):
    """Another fp32 implementation of the same composition, none of whose code the kernel shares: what validates the constants."""
    case = gb.table_case(index)
    r = case.ref
    d_cal, d_grid = gb.autograd_reference(case, case.integral, torch.float32)
    q_cal, q_grid = gb.ratio(d_cal, r.want_calibs, r.bound_calibs), gb.ratio(d_grid, r.want_grid, r.bound_grid)
    nz = r.want_grid != 0
    sharp = float((r.bound_grid[nz] / r.want_grid[nz].abs()).median())
    print(f"[geometry] {case.name}: fp32 torch autograd worst err / bound, d calibs {q_cal:.2g}, d grid {q_grid:.2g}; "
          f"median bound / |want| over d grid {sharp:.2e}")
    assert q_cal <= 1.0 and q_grid <= 1.0, (q_cal, q_grid)


@pytest.mark.parametrize("mutant", sorted(gb.MUTANTS))
def test_the_bound_is_not_vacuous(mutant):
    """Each wrong variant of the float64 restatement, rounded to fp32, leaves the bound on the case named in EXPOSED_BY."""
    fn, args = EXPOSED_BY[mutant]
    assert (fn, args) in gb.TABLE
    case = fn(*args)
    r, wrong = case.ref, case.reference(case.integral, mutant=mutant)
    q_cal = gb.ratio(wrong.want_calibs.float(), r.want_calibs, r.bound_calibs)
    q_grid = gb.ratio(wrong.want_grid.float(), r.want_grid, r.bound_grid)
    print(f"[geometry] mutant {mutant} ({gb.MUTANTS[mutant]}) on {case.name}: err / bound, d calibs {q_cal:.3g}, d grid {q_grid:.3g}")
    assert max(q_cal, q_grid) > 1.0, (q_cal, q_grid)
    # and the unchanged restatement rounded to fp32 is inside it
    assert gb.ratio(r.want_calibs.float(), r.want_calibs, r.bound_calibs) <= 1.0
    assert gb.ratio(r.want_grid.float(), r.want_grid, r.bound_grid) <= 1.0


@pytest.mark.parametrize("index", INDICES)
def test_flipped_floors_are_rare(index):
    """A condition on the inputs: at most 2 % of the cells with a visible box carry a flipped-floor term of an unblocked edge."""
    case = gb.table_case(index)
    r = case.ref
    print(f"[geometry] {case.name}: {r.cells_flipped} of {r.cells_visible} cells with a visible box carry a flipped-floor term; "
          f"{r.cells_empty} cells without a visible box")
    assert r.cells_visible > 0 and r.cells_flipped <= 0.02 * r.cells_visible


def test_cases_meet_their_conditions():
    s = gb.scene(0, 8)
    r = s.ref
    assert s.n == 2 and s.nl == 3 and s.cell_count == 252 and s.cell_count % gb.TILE_CELLS == 4
    assert r.cells_empty > 0 and not bool(r.visible.all()) and not bool(r.passes[r.visible].all())     # empty cells, masked boxes, blocked edges
    assert bool((r.bound_grid == 0).any()) and bool((r.count_grid > 0).any())
    for m in (1, 2):                                                                                   # clamped right edges on integer columns
        assert bool((gb.scene(m, 8).ref.box[..., 2] == 0.95).any())
    for views in (1, 2):
        c = gb.many_tiles(views)
        assert -(-c.cell_count // gb.TILE_CELLS) == 257 and c.cell_count % gb.TILE_CELLS == 1 and c.n == views
        assert c.ref.cells_visible == c.cell_count
    rg = gb.scene_range()
    assert rg.cell_begin % gb.TILE_CELLS != 0 and rg.cell_count % gb.TILE_CELLS != 0 and rg.cell_begin + rg.cell_count < rg.n_cells
    ties = gb.affine_ties().ref
    assert ties.items_tied > 0 and ties.items_tied == int(ties.passes[ties.visible].sum())            # every unblocked edge is a tie
    inside = gb.camera_inside().ref
    assert inside.items_behind > 0 and inside.items_behind < int(inside.passes[inside.visible].sum())
    for data in ("MultiviewX", "Wildtrack"):
        assert gb.conversion(data, 5).ref.n_visible > 0 and gb.conversion(data, 5).C % 4 != 0


def test_a_flipped_floor_moves_only_the_edge_whose_derivative_jumps():
    """The second evaluation of ``geometry_reference`` on the boxes of the 12 x 20 map whose clamped right edge sits on a pixel column
    (X = 19 in fp32, 18.99999988 in float64): with the neighbouring tap pair dl, dt and db move by no more than their coordinate
    term -- the value and the derivative along the other axis are continuous -- while dr, whose derivative jumps, moves by more."""
    case = gb.scene(1, 8)
    r = case.ref
    v, l, c = r.visible.nonzero(as_tuple=True)
    b, area = r.box[v, l, c].double(), r.area[v, l, c].double()
    X = ((b[:, 2] + 1) * case.Wf - 1) / 2
    f = X - torch.floor(X)
    near = gb.K_X * gb.U * max(case.Hf, case.Wf)
    m = f > 1 - near
    assert int(m.sum()) >= 16 and not bool((f < near).any()) and not bool(r.passes[v, l, c][m, 1].any())   # all clamped: blocked
    g = case.gvox.double().view(case.n, case.cell_count, case.nl, case.C)[v, c, l]
    args = (case.integral.double(), v[m], b[m], area[m], g[m], case.Hf, case.Wf, 4)
    val, coord, _ = gb._edges(*args, {})
    val2, coord2, _ = gb._edges(*args, {2: torch.ones(int(m.sum()), dtype=torch.float64)})
    moved = (val2 - val).abs()
    assert bool((moved[:, [0, 2, 3]] <= torch.maximum(coord, coord2)[:, [0, 2, 3]]).all())
    assert bool((moved[:, 1] > 1e3 * torch.maximum(coord, coord2)[:, 1]).any())
