"""Shared by tests/test_geometry_bound_cpu.py and tests/test_geometry_bound.py (not a test module): a float64 reference of the
GEOMETRY gradient of the box pooling (``vfa_project_gather_backward_geometry_f32``, vfa_amd/csrc/vfa_geom_grad.hip), the per-element
error bound the kernel is held to, and the cases.  It follows tests/adjoint_common.py (read that docstring first: u, gamma, K_X).

What is data and what is checked.  The reference computes in float64 FROM the fp32 ``box``, ``area`` and ``visible`` of
``oracle.torch_reference.vfa_stages`` on the CPU (pinned bitwise to the kernels' boxes by tests/test_oracle_golden.py and
tests/test_hip_parity.py) and from the fp32 integral image the entry point is given.  ``corner_coords`` restates the fp32 lines of
``vfa_stages`` that give the per-corner unclamped coordinates; ``geometry_reference`` asserts that the min / max of their clamped
values ARE ``box`` bit for bit and takes from them the discrete facts: which corner carries l, r, t, b (lowest index on ties) and
whether that corner's unclamped value lies inside ``crange`` (the clamp passes the gradient).  What is left -- and what the bound
covers -- is the kernel's own arithmetic: channel sums, edge quotients, the corner chain rule, the reductions.  1 / area and b - t are
then single roundings of given fp32 numbers, so slivers are no special case.

The operation (per visible box; g = d vox row, taps of the zero-bordered integral image; x0 = floor(X), hi = X - x0, lo = 1 - hi):
    S_p  = ylo (xlo nw + xhi ne) + yhi (xlo sw + xhi se)                 p in lt, rb, rt, lb (signs + + - -)
    DX_p = ylo (ne - nw) + yhi (se - sw),   DY_p = xlo (sw - nw) + xhi (se - ne)
    A_p = sum_c g DX_p,  B_p = sum_c g DY_p,  Q = sum_c g (S_lt + S_rb - S_rt - S_lb) / area
    dl = ((A_lt - A_lb) Wf/2 + Q (b - t) Hf Wf) / area        dr = ((A_rb - A_rt) Wf/2 - Q (b - t) Hf Wf) / area
    dt = ((B_lt - B_rt) Hf/2 + Q (r - l) Hf Wf) / area        db = ((B_rb - B_lb) Hf/2 - Q (r - l) Hf Wf) / area
    an edge e with value d_e, carried by corner k (world point X, h = P [X 1]) on image axis a (0: l, r; 1: t, b), q = 2 / img_a:
    dh_a = q d_e / h2,  dh_2 = -q d_e (h_a / h2) / h2;   d P[r][j] += dh_r [X 1]_j;   d grid[cell][j] += s sum_r dh_r P[r][j]
(s = 1, 1/40, 2.5 the conversion's scale).  Each output element is  sum over unblocked (box, edge) items of  d_e T,  T the item's
coefficient for the element.

The bound.  For every element, with the items that reach it and count = their number,

    |got - want| <= sum (E_e |T| + (|d_e| + E_e) dT)  +  gamma(count + K) sum (|d_e| + E_e) |T|,
    E_e = coordinate term + relative term + flipped-floor term of the edge,

|T| formed from absolute values of its products.  Where nothing contributes the bound is 0 and the kernel's value must be exactly 0.

* Coordinate term of an edge.  ``make_axis`` forms X = fma(RN(g + 1), size / 2, -0.5): |dX| <= 1.95 u size, and each of the axis' two
  weights hi = X - floor(X), lo = 1 - hi is off by at most D(size) = (1.95 size + 1) u absolute (adjoint_common: "First term").  The
  error moves weight from lo to hi.  A_p depends on the y weights, B_p on the x weights, S_p on both:
      |d A_p| <= D(Hf) C_p,   |d B_p| <= D(Wf) C_p,   |d sum_c g S_p| <= D(Wf) sum|g||DX_p| + D(Hf) sum|g||DY_p| + D(Wf) D(Hf) C_p,
      C_p = sum_c |g| |se - sw - ne + nw|,
  carried through the (linear) edge formulas above with absolute values.
* Relative term of an edge: gamma(K_A + n_lane) |A part| + gamma(K_Q + n_lane) |Q part|, each part the edge formula with every product
  replaced by its absolute value (sum|g| (|ylo||ne - nw| + |yhi||se - sw|) for A_p, sum|g| sum_taps |w||tap| for S_p).  Roundings
  along ``geom_grad_kernel``, n_lane = 4 ceil(C / 256) >= the terms one lane adds into A[p], B[p], qn (scalar kernel: ceil(C / 64)):
    - K_A = 16: the tap difference (1), lo = 1 - hi (1), its product (1), the sum of the two (1), gc * dx (1) | lane sum |
      A0 - A3 (1), * half_w (1), + wy (1), inv = 1 / area and * inv (2), the wave butterfly (6);
    - K_Q = 25: the tap weight ylo xlo (2 + 1, ``bilinear_weights``), * tap (1), the sum of four (3), n_acc (3), gc * n_acc (1)
      | lane sum | inv and qn * inv (2), (b - t) (1), * hw (1), qa * (..) (1), + wy (1), inv and * inv (2), the butterfly (6).
* Flipped floor.  dS/dx jumps where X crosses an integer; the value and the derivative along the other axis do not.  A coordinate
  within near = K_X u max(Hf, Wf) of an integer may floor differently in fp32.  For such an axis the reference evaluates the box a
  second time with the neighbouring tap pair; the edge whose derivative jumps (xl -> l, xr -> r, yt -> t, yb -> b) gets the absolute
  difference added to E_e, and the coordinate and relative terms of all four edges take the larger of the two evaluations (the
  continuous quantities change slope there).  Two axes of one box flipping together is second order in ``near`` and ignored.  An edge
  the clamp blocks reaches no element, so its widening counts nothing.
* h, u, v are recomputed in float64 from the fp32 inputs; their fp32 error enters through dT.  The world point costs <= 3 roundings
  (grid + offset, the scale, Wildtrack's shift), a row of P [X 1] 4 more (product, three adds, ``project_corner_ex``):
  |dh_r| <= gamma(K_H) Habs_r, K_H = 7, Habs_r = sum_j |P[r][j]| (|s (g + off)_j| + |shift_j|) + |P[r][3]|.  With e2 = |dh_2| / |h2|
  (to all orders e2 / (1 - e2); a corner with e2 >= 1/2 gets an infinite bound: its sign of h2 is not decided in fp32) and
  uv = h_a / h2:  d(1 / h2) <= e2 / |h2|,  d uv <= (|dh_a| + |uv| |dh_2|) / |h2| (1 + e2), and dT is T with those in place of its factors.
* The last term, relative to the item.  Roundings from the edge to the element:
    - d grid, K_G = 13: the sum of the corner's two edges (1), / img (1), u = h0 / h2 (1), du * u (1), + dv * w (1), / h2 (1),
      dh * pm (1), the sum of three (2), the scale (1) | dg += per box, at most ``count`` | the butterfly over eight corners (3);
    - d calibs, K_C = 24 + ceil(tiles / 256): the same six up to dh (6), * X (1) with X's own three (3) | dP += , at most ``count`` |
      the wave butterfly (6), ``geom_calib_reduce_kernel``: thread t adds slots t, t + 256, ... (ceil(tiles / 256)), the LDS tree (8).
  ``accumulate`` adds once more: the tests add u (|base + want| + bound).
The constants come from these sequences, not from the kernel's output; what validates them is torch's own fp32 autograd of the same
composition on the CPU (tests/test_geometry_bound_cpu.py prints its err / bound), and the mutants there show the bound is not vacuous.
"""
import functools
import math
from types import SimpleNamespace

import torch

import adjoint_common as ac
from adjoint_common import K_X, U, gamma
from geomgrad_common import SCALE, corner_offsets
from oracle import torch_reference as ref

K_A, K_Q, K_H, K_G, K_C = 16, 25, 7, 13, 24
TILE_CELLS, REDUCE_THREADS = 8, 256              # kTileCells, kReduceThreads (vfa_geom_grad.hip)
DATA_OF_KIND = {0: "MultiviewC", 1: "MultiviewX", 2: "Wildtrack"}
SHIFT = {"Wildtrack": (300.0, 900.0, 0.0)}
EDGE_AXIS, EDGE_COLUMN = (0, 0, 1, 1), (0, 2, 1, 3)   # edges l, r, t, b: image axis, column of ``box``
MUTANTS = {"a": "the area term is dropped", "b": "dt and db are swapped", "c": "ties go to the highest corner index",
           "d": "the clamp passes the gradient", "e": "the last cell of a ragged tile is left out",
           "f": "the MultiviewX conversion uses scale 1", "g": "the channel sum stops at C - C % 4"}


# ------------------------------------------------------------------------------------------------ the fp32 geometry
def corner_coords(calib, grid_flat, zl, co, data, image_size, dtype):
    """The lines of ``oracle.torch_reference.vfa_stages`` in front of the clamp, op for op: calib (3, 4), grid_flat (cells, 3) ->
    unclamped normalised image coordinates (nl, cells, 8, 2) in ``dtype`` (differentiable in calib and grid_flat)."""
    nl = zl.numel()
    z_corners = torch.zeros(nl, 1, 1, 3, dtype=zl.dtype)
    z_corners[:, 0, 0, 2] = zl
    corners = grid_flat.view(-1, 1, 3).to(dtype)[None].unsqueeze(0) + z_corners.view(-1, 1, 1, 3)
    corners = corners.unsqueeze(-2)
    corners3d = corners.repeat((1, 1, 1, 1, 8, 1)) + co.to(dtype).view(1, 1, 1, 1, 8, 3)
    corners3d = ref.world_coords(corners3d, data)
    img = ref.project(corners3d, calib.to(dtype).view(-1, 1, 1, 1, 1, 3, 4))
    img_size = corners.new_tensor(list(image_size[::-1]))
    return (2 * img / img_size - 1)[0, :, :, 0]


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())).all())


def _pick(x, m, highest=False):
    """The corner index attaining m over the last dimension of x: the lowest (what torch.min / max select), or the highest."""
    if highest:
        return 7 - (x.flip(-1) == m[..., None]).to(torch.int64).argmax(-1)
    return (x == m[..., None]).to(torch.int64).argmax(-1)


def _corners64(calib, grid_flat, zl, co, data):
    """float64 from the fp32 inputs, own formulas: world point X, its magnitude Xabs, h = P [X 1], Habs -- each (nl, cells, 8, 3)."""
    s = SCALE[data]
    shift = torch.tensor(SHIFT.get(data, (0.0, 0.0, 0.0)), dtype=torch.float64)
    pts = (grid_flat.double()[None, :, None, :] + co.double()[None, None]).repeat(zl.numel(), 1, 1, 1)
    pts[..., 2] += zl.double()[:, None, None]
    X, Xabs = pts * s - shift, pts.abs() * s + shift
    P = calib.double().view(3, 4)
    return X, Xabs, X @ P[:, :3].t() + P[:, 3], Xabs @ P[:, :3].abs().t() + P[:, 3].abs()


# ------------------------------------------------------------------------------------------------ the edges of a box
def _edges(I, view, b, area, g, Hf, Wf, n_lane, shifts, drop_area=False):
    """The four edge gradients (l, r, t, b) of boxes b (Nb, 4) with d vox rows g (Nb, C), taps from I (n, Hf+2, Wf+2, C): values, the
    coordinate term and the relative term, each (Nb, 4).  ``shifts``: box column -> what to add to that axis' floor (Nb)."""
    def axis(col, size):
        X = ((b[:, col] + 1) * size - 1) / 2
        x0 = torch.floor(X) + shifts.get(col, 0)
        return x0.long(), (X - x0)[:, None]

    def tap(y, x):
        return I[view, y.clamp(-1, Hf) + 1, x.clamp(-1, Wf) + 1]

    ax = {col: axis(col, Wf if col in (0, 2) else Hf) for col in range(4)}
    ga = g.abs()
    dxe, dye = (1.95 * Wf + 1) * U, (1.95 * Hf + 1) * U
    P = {}
    for name, cx, cy in (("lt", 0, 1), ("rb", 2, 3), ("rt", 2, 1), ("lb", 0, 3)):
        (x0, xhi), (y0, yhi) = ax[cx], ax[cy]
        xlo, ylo = 1 - xhi, 1 - yhi
        nw, ne, sw, se = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        DX = ylo * (ne - nw) + yhi * (se - sw)
        DY = xlo * (sw - nw) + xhi * (se - ne)
        S = ylo * (xlo * nw + xhi * ne) + yhi * (xlo * sw + xhi * se)
        Sabs = ylo.abs() * (xlo.abs() * nw.abs() + xhi.abs() * ne.abs()) + yhi.abs() * (xlo.abs() * sw.abs() + xhi.abs() * se.abs())
        P[name] = SimpleNamespace(
            A=(g * DX).sum(1), Aabs=(ga * (ylo.abs() * (ne - nw).abs() + yhi.abs() * (se - sw).abs())).sum(1),
            B=(g * DY).sum(1), Babs=(ga * (xlo.abs() * (sw - nw).abs() + xhi.abs() * (se - ne).abs())).sum(1),
            N=(g * S).sum(1), Nabs=(ga * Sabs).sum(1), sdx=(ga * DX.abs()).sum(1), sdy=(ga * DY.abs()).sum(1),
            C=(ga * (se - sw - ne + nw).abs()).sum(1))
    lt, rb, rt, lb = P["lt"], P["rb"], P["rt"], P["lb"]
    hw = Hf * Wf
    bh, bw = (b[:, 3] - b[:, 1]) * hw, (b[:, 2] - b[:, 0]) * hw
    Q = (lt.N + rb.N - rt.N - lb.N) / area * (0.0 if drop_area else 1.0)
    Qabs = (lt.Nabs + rb.Nabs + rt.Nabs + lb.Nabs) / area
    NS = sum(dxe * p.sdx + dye * p.sdy + dxe * dye * p.C for p in P.values()) / area      # the coordinate term of Q
    gA, gQ = gamma(K_A + n_lane), gamma(K_Q + n_lane)
    val = torch.stack([((lt.A - lb.A) * (Wf / 2) + Q * bh) / area, ((rb.A - rt.A) * (Wf / 2) - Q * bh) / area,
                       ((lt.B - rt.B) * (Hf / 2) + Q * bw) / area, ((rb.B - lb.B) * (Hf / 2) - Q * bw) / area], 1)
    coord = torch.stack([(dye * (lt.C + lb.C) * (Wf / 2) + NS * bh.abs()) / area, (dye * (rb.C + rt.C) * (Wf / 2) + NS * bh.abs()) / area,
                         (dxe * (lt.C + rt.C) * (Hf / 2) + NS * bw.abs()) / area, (dxe * (rb.C + lb.C) * (Hf / 2) + NS * bw.abs()) / area], 1)
    rel = torch.stack([(gA * (lt.Aabs + lb.Aabs) * (Wf / 2) + gQ * Qabs * bh.abs()) / area,
                       (gA * (rb.Aabs + rt.Aabs) * (Wf / 2) + gQ * Qabs * bh.abs()) / area,
                       (gA * (lt.Babs + rt.Babs) * (Hf / 2) + gQ * Qabs * bw.abs()) / area,
                       (gA * (rb.Babs + lb.Babs) * (Hf / 2) + gQ * Qabs * bw.abs()) / area], 1)
    return val, coord, rel


# ------------------------------------------------------------------------------------------------ the reference
def geometry_reference(grad_vox, integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, crange=(-1, 0.95),
                       cell_begin=0, cell_count=None, mutant=None):
    """The operands of ``ops.project_gather_backward_geometry`` (CPU tensors) -> namespace of float64 ``want_calibs`` / ``bound_calibs``
    (n, 12), ``want_grid`` / ``bound_grid`` (cell_count, 3), the contributions per element ``count_calibs`` / ``count_grid``, the
    statistics ``cells_visible``, ``cells_empty`` (no visible box), ``cells_flipped`` (cells whose bound carries a flipped-floor term of
    an unblocked edge), ``items_behind`` (unblocked edges on a corner with h2 < 0), ``items_tied`` (unblocked edges whose value two
    corners attain), and the dense fp32 facts ``box``, ``area`` (n, nl, cells, ..), ``visible``, ``corner`` and ``passes``
    (n, nl, cells, 4; edges l, r, t, b).  ``mutant``: a key of MUTANTS -- a deliberately wrong ``want`` (the bound is the right one's)."""
    n, Hp, Wp, C = integral.shape
    Hf, Wf = Hp - 2, Wp - 2
    data, image_size = DATA_OF_KIND[int(conv_kind)], (image_wh[1], image_wh[0])
    calibs, grid_flat = calibs.reshape(n, 12).float().cpu(), grid_flat.reshape(-1, 3).float().cpu()
    zl, co = z_layers.float().cpu(), corner_off.float().cpu()
    nl, n_cells = zl.numel(), grid_flat.shape[0]
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    sl = slice(cell_begin, cell_begin + cell_count)
    cmin, cmax = (torch.tensor(float(c), dtype=torch.float32) for c in crange)
    I = integral.detach().cpu().double()
    gv = grad_vox.detach().cpu().double().view(n, cell_count, nl, C)
    if mutant == "g":
        gv = gv.clone()
        gv[..., C - C % 4:] = 0
    n_lane, tiles = 4 * math.ceil(C / 256), math.ceil(cell_count / TILE_CELLS)
    near = K_X * U * max(Hf, Wf)

    dense, rec = [], []
    for v in range(n):
        st = ref.vfa_stages(torch.zeros(1, 1, Hf, Wf), calibs[v].view(3, 4), grid_flat.view(-1, 1, 3), zl, co, data, image_size, crange)
        box, area, vis = st["box"][0][:, sl], st["area"][0, 0][:, sl], st["visible"][0, 0][:, sl]
        pre = corner_coords(calibs[v].view(3, 4), grid_flat, zl, co, data, image_size, torch.float32)[:, sl]   # (nl, cells, 8, 2)
        cl = pre.clamp(crange[0], crange[1])
        mine = torch.stack([cl[..., 0].min(-1)[0], cl[..., 1].min(-1)[0], cl[..., 0].max(-1)[0], cl[..., 1].max(-1)[0]], -1)
        assert _same_bits(mine, box), "the restated corner coordinates do not reproduce vfa_stages' boxes bit for bit"
        corner = torch.stack([_pick(cl[..., EDGE_AXIS[e]], box[..., EDGE_COLUMN[e]], mutant == "c") for e in range(4)], -1)
        at = torch.stack([pre[..., EDGE_AXIS[e]].gather(-1, corner[..., e:e + 1])[..., 0] for e in range(4)], -1)
        passes = (at >= cmin) & (at <= cmax)
        tied = torch.stack([(cl[..., EDGE_AXIS[e]] == box[..., EDGE_COLUMN[e], None]).sum(-1) > 1 for e in range(4)], -1)
        dense.append((box, area, vis, corner, passes))
        layer, cell = vis.nonzero(as_tuple=True)
        X, Xabs, h, Habs = (t[layer, cell] for t in _corners64(calibs[v], grid_flat[sl], zl, co, data))            # (Nb, 8, 3)
        k = corner[layer, cell]                                                                                     # (Nb, 4)
        at_k = lambda t: t.gather(1, k[..., None].expand(-1, -1, 3))                                                # noqa: E731
        rec.append(dict(view=torch.full_like(layer, v), cell=cell, b=box[layer, cell].double(), area=area[layer, cell].double(),
                        g=gv[v, cell, layer], passes=passes[layer, cell], tied=tied[layer, cell], X=at_k(X), Xabs=at_k(Xabs),
                        h=at_k(h), Habs=at_k(Habs)))
    r = {key: torch.cat([d[key] for d in rec]) for key in rec[0]}
    view, cell, b, area, g = r["view"], r["cell"], r["b"], r["area"], r["g"]
    nb = view.numel()

    val, coord, rel = _edges(I, view, b, area, g, Hf, Wf, n_lane, {}, drop_area=mutant == "a")
    flip = torch.zeros(nb, 4, dtype=torch.float64)
    flagged = torch.zeros(nb, 4, dtype=torch.bool)
    for e in range(4):                                    # the axis whose floor decides the jump of edge e
        col, size = EDGE_COLUMN[e], (Wf, Wf, Hf, Hf)[e]
        X = ((b[:, col] + 1) * size - 1) / 2
        f = X - torch.floor(X)
        shift = (f > 1 - near).double() - (f < near).double()
        if not bool((shift != 0).any()):
            continue
        m = shift != 0
        val2, coord2, rel2 = _edges(I, view, b, area, g, Hf, Wf, n_lane, {col: shift}, drop_area=mutant == "a")
        flip[:, e] = torch.where(m, (val2[:, e] - val[:, e]).abs(), flip[:, e])
        flagged[:, e] = m
        coord = torch.where(m[:, None], torch.maximum(coord, coord2), coord)
        rel = torch.where(m[:, None], torch.maximum(rel, rel2), rel)
    if mutant == "b":
        val = val[:, [0, 1, 3, 2]]
    E = coord + rel + flip

    passes = torch.ones_like(r["passes"]) if mutant == "d" else r["passes"].clone()
    if mutant == "e" and cell_count % TILE_CELLS:
        passes &= (cell != cell_count - 1)[:, None]
    s = 1.0 if (mutant == "f" and data == "MultiviewX") else SCALE[data]
    Pm = calibs.double().view(n, 3, 4)
    img = (float(image_wh[0]), float(image_wh[1]))
    acc = {name: [torch.zeros(size, dtype=torch.float64) for _ in range(4)] for name, size in (("calibs", n * 12), ("grid", cell_count * 3))}

    def add(name, index, m, d, Ee, T, Tabs, dT):
        mag = (d.abs() + Ee)[m, None]
        for slot, term in enumerate((d[m, None] * T[m], Ee[m, None] * Tabs[m] + mag * dT[m], mag * Tabs[m], torch.ones_like(T[m]))):
            acc[name][slot].index_add_(0, index[m].reshape(-1), term.reshape(-1))

    behind = tied = 0
    one = torch.ones(nb, 1, dtype=torch.float64)
    for e in range(4):
        a_, q = EDGE_AXIS[e], 2.0 / img[EDGE_AXIS[e]]
        m = passes[:, e]
        X1, X1a = torch.cat([r["X"][:, e], one], 1), torch.cat([r["Xabs"][:, e], one], 1)
        h, dh = r["h"][:, e], gamma(K_H) * r["Habs"][:, e]
        h2, uv = h[:, 2], h[:, a_] / h[:, 2]
        e2 = dh[:, 2] / h2.abs()
        e2 = torch.where(e2 < 0.5, e2 / (1 - e2), torch.full_like(e2, float("inf")))
        duv = (dh[:, a_] + uv.abs() * dh[:, 2]) / h2.abs() * (1 + e2)
        a, a2 = q / h2, -q * uv / h2
        da, da2 = a.abs() * e2, q * duv / h2.abs() * (1 + e2) + a2.abs() * e2
        j4, j3 = torch.arange(4)[None], torch.arange(3)[None]
        for row, c, dc in ((a_, a, da), (2, a2, da2)):
            add("calibs", view[:, None] * 12 + row * 4 + j4, m, val[:, e], E[:, e], c[:, None] * X1, c.abs()[:, None] * X1a, dc[:, None] * X1a)
        Pa, P2 = Pm[view, a_, :3], Pm[view, 2, :3]
        add("grid", cell[:, None] * 3 + j3, m, val[:, e], E[:, e], s * (a[:, None] * Pa + a2[:, None] * P2),
            s * (a.abs()[:, None] * Pa.abs() + a2.abs()[:, None] * P2.abs()), s * (da[:, None] * Pa.abs() + da2[:, None] * P2.abs()))
        behind += int((m & (h2 < 0)).sum())
        tied += int((m & r["tied"][:, e]).sum())

    out = SimpleNamespace()
    for name, K, shape in (("calibs", K_C + math.ceil(tiles / REDUCE_THREADS), (n, 12)), ("grid", K_G, (cell_count, 3))):
        want, e1, rsum, count = (t.view(shape) for t in acc[name])
        bound = torch.where(count > 0, e1 + gamma(count + K) * rsum, torch.zeros_like(e1))
        setattr(out, "want_" + name, want), setattr(out, "bound_" + name, bound), setattr(out, "count_" + name, count)
    seen = torch.zeros(cell_count, dtype=torch.bool)
    seen[cell] = True
    flipped = torch.zeros(cell_count, dtype=torch.bool)
    flipped[cell[(flagged & passes).any(1)]] = True
    out.cells_visible, out.cells_empty, out.cells_flipped = int(seen.sum()), int((~seen).sum()), int(flipped.sum())
    out.items_behind, out.items_tied, out.n_visible = behind, tied, nb
    out.box, out.area, out.visible, out.corner, out.passes = (torch.stack([d[i] for d in dense]) for i in range(5))
    return out


def ratio(got, want, bound):
    """max err / bound; where the bound is zero the element must be exactly zero (inf otherwise); NaN if ``got`` is not finite."""
    err = (got.detach().double().cpu() - want).abs()
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(q.max()) if q.numel() else 0.0


def with_base(want, bound, base):
    """``accumulate=True`` onto ``base``: the bound plus one rounding of the add."""
    want = want + base.double()
    return want, bound + U * (want.abs() + bound)


# ------------------------------------------------------------------------------------------------ autograd of the composition
def autograd_reference(case, integral, dtype):
    """torch autograd of the ``grid_sample`` composition (``adjoint_common.pool``) -> (d calibs (n, 12), d grid (cell_count, 3)).
    float64: on the GIVEN fp32 boxes and areas (the area's value is the fp32 one, its derivative the product rule's), chained through
    the float64 projection with the fp32 selection of ``case.ref``.  float32: torch's own composition end to end -- its projection,
    clamp, min / max, area and pooling, with torch's own selection."""
    Hf, Wf, sl = case.Hf, case.Wf, slice(case.cell_begin, case.cell_begin + case.cell_count)
    I = integral[:, 1:-1, 1:-1].permute(0, 3, 1, 2).to(dtype)
    cal = case.calibs.to(dtype).requires_grad_(True)
    grd = case.grid_flat.to(dtype).requires_grad_(True)
    pre = torch.stack([corner_coords(cal[v].view(3, 4), grd, case.zl, case.co, case.data, case.image_size, dtype)[:, sl] for v in range(case.n)])
    if dtype == torch.float64:
        r = case.ref
        box = r.box.double().requires_grad_(True)
        exact = (box[..., 2:] - box[..., :2]).prod(-1) * Hf * Wf + ref.EPSILON
        area = r.area.double() + (exact - exact.detach())
        d_box, = torch.autograd.grad(ac.pool(I, box, area, r.visible), box, case.gvox.double())
        d_edge = d_box[..., list(EDGE_COLUMN)] * r.passes
        at = torch.stack([pre[..., EDGE_AXIS[e]].gather(-1, r.corner[..., e:e + 1])[..., 0] for e in range(4)], -1)
        (d_edge * at).sum().backward()
    else:
        norm = pre.clamp(-1, 0.95)
        box = torch.stack([norm[..., 0].min(-1)[0], norm[..., 1].min(-1)[0], norm[..., 0].max(-1)[0], norm[..., 1].max(-1)[0]], -1)
        area = (box[..., 2:] - box[..., :2]).prod(-1) * Hf * Wf + ref.EPSILON
        visible = torch.logical_and(area > ref.EPSILON, area < (Hf * Wf * ref.MAXIMUM_AREA_RATIO))
        ac.pool(I, box, area, visible).backward(case.gvox)
    return cal.grad.detach(), grd.grad.detach()[sl]


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """Geometry, features, d vox and (lazily, for the CPU's integral image) the float64 reference of one call."""

    def __init__(self, name, calibs, grid_flat, cube, grid_height, hw, C, data="MultiviewC", image_size=ac.IMAGE_SIZE, cell_begin=0,
                 cell_count=None, seed=0):
        self.name, self.C, (self.Hf, self.Wf), self.data, self.image_size = name, C, hw, data, tuple(image_size)
        self.calibs = torch.as_tensor(calibs).reshape(-1, 12).float().contiguous()
        self.grid_flat = torch.as_tensor(grid_flat).reshape(-1, 3).float().contiguous()
        self.zl = torch.arange(0, grid_height, cube[2]).float()
        self.co = torch.tensor(corner_offsets(cube), dtype=torch.float32)
        self.n, self.nl, self.n_cells = self.calibs.shape[0], self.zl.numel(), self.grid_flat.shape[0]
        self.cell_begin = cell_begin
        self.cell_count = self.n_cells - cell_begin if cell_count is None else cell_count
        self.kind, self.image_wh = {v: k for k, v in DATA_OF_KIND.items()}[data], (float(image_size[1]), float(image_size[0]))
        gen = torch.Generator().manual_seed(seed)
        self.features = torch.randn(self.n, C, self.Hf, self.Wf, generator=gen)
        self.gvox = torch.randn(self.n, self.cell_count, self.nl * C, generator=gen)

    @functools.cached_property
    def integral(self):
        """The zero-bordered channels-last fp32 integral image by torch on the CPU (the GPU tests take ``ops.integral_image``'s)."""
        out = torch.zeros(self.n, self.Hf + 2, self.Wf + 2, self.C)
        out[:, 1:-1, 1:-1] = torch.cumsum(torch.cumsum(self.features, -1), -2).permute(0, 2, 3, 1)
        return out

    def reference(self, integral, gvox=None, grid_flat=None, **kw):
        return geometry_reference(self.gvox if gvox is None else gvox, integral, self.calibs, self.grid_flat if grid_flat is None else grid_flat,
                                  self.zl, self.co, self.kind, self.image_wh, cell_begin=self.cell_begin, cell_count=self.cell_count, **kw)

    @functools.cached_property
    def ref(self):
        return self.reference(self.integral)


@functools.lru_cache(maxsize=None)
def scene(map_index, C):
    """``adjoint_common.scene_geometry``: 2 views, 14 x 18 = 252 cells = 31 tiles of 8 and a tail of 4, three layers."""
    calibs, grid = ac.scene_geometry()
    return Case(f"scene {ac.MAPS[map_index]} C {C}", calibs, grid, ac.SCENE_CUBE, ac.SCENE_GRID_HEIGHT, ac.MAPS[map_index], C, seed=500 + map_index)


@functools.lru_cache(maxsize=None)
def scene_range(C=8):
    calibs, grid = ac.scene_geometry()
    r = ac.RANGES[18]
    return Case(f"scene range C {C}", calibs, grid, ac.SCENE_CUBE, ac.SCENE_GRID_HEIGHT, ac.MAPS[0], C, cell_begin=r["cell_begin"],
                cell_count=r["cell_count"], seed=500)


@functools.lru_cache(maxsize=None)
def conversion(data, C):
    """The one-view scenes of tests/test_geometry_gradients_cpu.py::_scene on their 45 x 80 map."""
    from test_geometry_gradients_cpu import _scene
    cam, grid, feat, cube, gh, img, _ = _scene(data, 0)
    return Case(f"{data} C {C}", cam.float(), grid.float(), cube, gh, tuple(feat.shape[2:]), C, data=data, image_size=img, seed=600 + C)


@functools.lru_cache(maxsize=None)
def many_tiles(views):
    """``adjoint_common.duplicates(nl=1, C=8, cells=2049)``: 257 tiles, the last of one cell; alone or with the scene's second view."""
    dup = ac.duplicates(1, 8, 2049)
    calibs = dup.calibs if views == 1 else ac.scene_geometry()[0][:2]
    return Case(f"2049 cells, {views} view(s)", calibs, dup.grid_flat, (50, 50, 40), 40, ac.MAPS[0], 8, seed=700 + views)


@functools.lru_cache(maxsize=None)
def affine_ties():
    """An affine camera -- third row (0, 0, 0, 1), no z term in the first two rows: corners k and k + 4 of a cube project to the same
    fp32 point, so every unclamped edge is an exact tie between two corners that differ in z (hence in d P[.][2])."""
    _, grid = ac.scene_geometry()
    cam = torch.tensor([[0.30, 0.05, 0.0, 10.0], [-0.04, 0.18, 0.0, 8.0], [0.0, 0.0, 0.0, 1.0]])
    return Case("affine ties", cam[None], grid, ac.SCENE_CUBE, ac.SCENE_GRID_HEIGHT, ac.MAPS[0], 8, seed=800)


@functools.lru_cache(maxsize=None)
def camera_inside():
    """A camera inside the ground grid, low above it and looking along it: cubes behind it have h2 < 0 at every corner."""
    from vfa_amd.synthetic import look_at_camera
    _, grid = ac.scene_geometry()
    cam = look_at_camera((330.0, 440.0, 150.0), (700.0, 900.0, 20.0), 150.0 * ac.IMAGE_SIZE[1] / 176.0, (ac.IMAGE_SIZE[1], ac.IMAGE_SIZE[0]))
    return Case("camera inside", torch.tensor(cam, dtype=torch.float32)[None], grid, ac.SCENE_CUBE, ac.SCENE_GRID_HEIGHT, ac.MAPS[0], 8, seed=900)


TABLE = ([(scene, (0, C)) for C in (6, 8, 70, 256, 260)] + [(scene, (1, 8)), (scene, (2, 8))] +
         [(conversion, (d, C)) for d in ("MultiviewX", "Wildtrack") for C in (5, 8)] + [(many_tiles, (1,)), (many_tiles, (2,))] +
         [(scene_range, ()), (affine_ties, ()), (camera_inside, ())])


def table_case(index):
    fn, args = TABLE[index]
    return fn(*args)
