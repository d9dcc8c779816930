"""Shared by tests/test_pool_adjoint_cpu.py and tests/test_pool_adjoint.py (not a test module): a float64 reference of the ADJOINT
of the box pooling on the CPU, the error bound the HIP scatters are held to, and the cases with the statistics they are built for.

The operation.  The forward pools  vox = (lt + rb - rt - lb) / area * visible  (reference vfa_op.py:112-119), each of the four a
bilinear ``grid_sample`` (align_corners=False, zero padding) of the integral image at a corner (gx, gy) of the box.  Its adjoint
scatters, for every visible box, sample s in {lt, rb, rt, lb} (sign +, +, -, -) and tap (j, i) in {0, 1}^2,

    d integral[y0 + j, x0 + i] += sign_s * wy_j * wx_i * grad_vox / area,      X = ((gx + 1) * Wf - 1) / 2,  x0 = floor(X),
                                                                              wx_0 = 1 - (X - x0),  wx_1 = X - x0   (Y alike)

into the zero-bordered image (n, Hf+2, Wf+2, C): pixel (y, x) sits at [y + 1, x + 1], a tap outside the image lands on the border
ring (which carries no gradient and is outside the contract).  ``adjoint_reference`` restates exactly this in float64 from the fp32
``box``, ``area``, ``visible`` of ``oracle.torch_reference.vfa_stages`` (fp32, CPU: pinned bitwise to the reference's boxes by
tests/test_oracle_golden.py) -- no code shared with the kernels, no autograd (tests/test_pool_adjoint_cpu.py compares it with
float64 autograd of the ``grid_sample`` composition).

The bound.  With u = 2^-24, for every element

    |got - want|  <=  K_X u max(Hf, Wf) B  +  gamma(count + K_R) A,           gamma(m) = m u / (1 - m u)

    A     = sum |w| |g| / area      over the contributions (sample, tap) to the element,
    B     = sum |g| / area          over every tap of every sample that touches the element, unit weights,
    count = the number of contributions.

* First term: the fp32 pixel coordinate.  ``make_axis`` (vfa_geom.h) forms X = fma(RN(g + 1), size / 2, -0.5).  g + 1 <= 1.95 is
  rounded once (relative u, worth <= 0.975 u size in X), size / 2 is exact, the fma rounds once (<= u |X| <= 0.975 u size):
  |dX| <= 1.95 u size.  hi = X - floor(X) is exact except for X in (-0.5, 0), where X + 1 rounds by <= u / 2; lo = 1 - hi rounds by
  <= u / 2 when hi < 1/2.  So each of an axis' two weights is off by <= 1.95 u size + u (absolute), and a tap weight wy wx, both
  factors <= 1, by <= 1.95 u (Hf + Wf) + 2 u <= 5 u max(Hf, Wf) for every map with max(Hf, Wf) >= 2: K_X = 5 (4 would
  ignore the two u / 2 roundings and hold only for Hf != Wf).  The error MOVES weight between neighbouring
  taps, it is not relative to the tap's own weight -- hence B with unit weights.  torch's own fp32 sequence
  ((g + 1) * size - 1) / 2 rounds twice at <= 0.975 u size each: the same bound.
  A coordinate within that error of an integer may floor differently in fp32: the tap pair moves by one, and a tap the float64
  floor does not touch receives a weight <= |dX|.  B therefore also covers the tap before the pair when X - x0 < K_X u max(Hf, Wf)
  and the tap behind it when X - x0 > 1 - K_X u max(Hf, Wf): no element is excluded from the comparison.
* Second term: what is relative to the contribution.  Per contribution, before anything is summed: the product wy wx (1 rounding,
  ``bilinear_weights``) and
    - ``gather_backward_kernel``: up to 3 roundings merging the <= 4 coincident taps of a box into W[r][c] (``scatter_run``), the
      quotient g / area (1), then fma(gv, W, T) per box of a run and one atomic per run: sums;
    - ``gather_backward_cached_kernel``: the quotient +-w / area (1), up to 3 roundings merging coincident taps by ds_add into
      coef[tap][box], then one fma per box and one atomic per tile: sums; its per-box level: g / area (1), the product with w (1);
    - ``vfa_project_gather_backward_det_f32``: the quotient w / area (1), then fma(coef, g, acc) in list order, piece sums added in
      piece order: sums.
  At most 5 roundings each of relative size u (merging coincident taps is bounded by the sum of their |w|, which A holds), then a
  sum of at most ``count`` terms in some order ((count - 1) u to first order, whatever the order): count + 4.  K_R = 8: the 4 to
  spare cover the contributions a flipped floor adds to ``count`` and the one add of ``accumulate``.  gamma() instead of (count + K_R) u keeps the
  bound true to second order, which matters only for the 10^4 contributions per element of the "duplicates" cases (+ 0.3 %).
The constants come from these operation sequences, not from any kernel's output; what validates them is torch's own fp32 autograd
of the same composition on the CPU (tests/test_pool_adjoint_cpu.py prints its err / bound).

The statistics (``case_stats``) are counted on the CPU from the same fp32 boxes with ``make_axis`` emulated exactly (the fp32 sum,
then product and sum in float64, rounded once): distinct taps per tile of the cached kernel, both ways
``vfa_project_gather_backward_grid_f32`` forms tiles, and per row of 8; the (dx, dy) class of every visible box; the longest run of
boxes with one tap set inside a 32-box chunk of ``gather_backward_kernel``; records per tap and the 256-record merge pieces a tap's
list crosses in ``vfa_project_gather_backward_det_f32``.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from geomgrad_common import corner_offsets
from oracle import torch_reference as ref

U = 2.0 ** -24
K_X, K_R = 5, 8
DATA, CONV_KIND = "MultiviewC", 0
IMAGE_SIZE = (184, 320)                       # (H, W) the boxes are normalised by
MAPS = ((23, 40), (12, 20), (6, 10))          # feature maps of strides 8 / 16 / 32 of that image
SAMPLES = ((0, 1, 1.0), (2, 3, 1.0), (2, 1, -1.0), (0, 3, -1.0))  # lt, rb, rt, lb: box column of x, of y, sign
BWD_BOXES, BWD_HASH, ROW_BOXES, ROW_HASH = 32, 128, 8, 64         # kBwdBoxes, kBwdHash, kCacheBoxes, kCacheHash (vfa_kernels.hip)
RUN_CHUNK, PIECE = 32, 256                                        # kPerWave (vfa_kernels.hip), kPiece (vfa_det.hip)


def gamma(m):
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------------------------------------------ boxes
def cpu_boxes(calibs, grid_flat, zl, co, Hf, Wf):
    """fp32 boxes of ``oracle.torch_reference.vfa_stages`` on the CPU: box (n, nl, cells, 4), area (n, nl, cells), visible (bool)."""
    dummy = torch.zeros(1, 1, Hf, Wf)
    st = [ref.vfa_stages(dummy, calibs[v].view(3, 4), grid_flat.view(-1, 1, 3), zl, co, DATA, IMAGE_SIZE) for v in range(calibs.shape[0])]
    return (torch.cat([s["box"] for s in st]), torch.cat([s["area"][:, 0] for s in st]), torch.cat([s["visible"][:, 0] for s in st]))


def pool(integral, box, area, visible):
    """The ``grid_sample`` composition of oracle/torch_reference.py:65-71 on given boxes, in ``integral``'s dtype:
    integral (n, C, Hf, Wf), box (n, nl, cells, 4) -> vox (n, cells, nl * C) layer-major."""
    dt = integral.dtype
    box, area = box.to(dt), area.to(dt)[:, None]
    lt = F.grid_sample(integral, box[..., [0, 1]], align_corners=False)
    rb = F.grid_sample(integral, box[..., [2, 3]], align_corners=False)
    rt = F.grid_sample(integral, box[..., [2, 1]], align_corners=False)
    lb = F.grid_sample(integral, box[..., [0, 3]], align_corners=False)
    vox = (lt + rb - rt - lb) / area
    vox = vox * visible[:, None]
    return vox.permute(0, 3, 2, 1).flatten(2)  # (n, C, nl, cells) -> (n, cells, nl, C)


# ------------------------------------------------------------------------------------------------ the float64 adjoint
def adjoint_reference(box, area, visible, grad_vox, Hf, Wf):
    """box (n, nl, cells, 4), area, visible (n, nl, cells) fp32 / bool; grad_vox (n, cells, nl * C) layer-major (masked boxes may
    hold anything) -> namespace of float64 (n, Hf+2, Wf+2, C): want, A, B, bound; count (n, Hf+2, Wf+2)."""
    n, nl, cells, _ = box.shape
    C = grad_vox.shape[-1] // nl
    Hp, Wp = Hf + 2, Wf + 2
    sel = visible.reshape(-1).nonzero()[:, 0]
    g = grad_vox.double().view(n, cells, nl, C).permute(0, 2, 1, 3).reshape(-1, C)[sel]
    b = box.double().reshape(-1, 4)[sel]
    g = g / area.double().reshape(-1)[sel, None]
    gabs = g.abs()
    view = torch.arange(n).view(n, 1, 1).expand(n, nl, cells).reshape(-1)[sel]
    want, A, B = (torch.zeros(n * Hp * Wp, C, dtype=torch.float64) for _ in range(3))
    count = torch.zeros(n * Hp * Wp, dtype=torch.float64)
    near = K_X * max(Hf, Wf) * U
    one = torch.ones(sel.numel(), dtype=torch.float64)
    for ix, iy, sign in SAMPLES:
        X, Y = ((b[:, ix] + 1) * Wf - 1) / 2, ((b[:, iy] + 1) * Hf - 1) / 2
        x0, y0 = torch.floor(X), torch.floor(Y)
        fx, fy = X - x0, Y - y0
        x0, y0 = x0.long(), y0.long()
        wx, wy = {0: 1 - fx, 1: fx}, {0: 1 - fy, 1: fy}
        mx = {-1: fx < near, 0: None, 1: None, 2: fx > 1 - near}
        my = {-1: fy < near, 0: None, 1: None, 2: fy > 1 - near}
        for dy in (-1, 0, 1, 2):
            row = (y0 + dy).clamp(-1, Hf) + 1
            for dx in (-1, 0, 1, 2):
                col = (x0 + dx).clamp(-1, Wf) + 1
                idx = (view * Hp + row) * Wp + col
                if dy in wy and dx in wx:
                    w = wy[dy] * wx[dx]
                    want.index_add_(0, idx, g * (sign * w)[:, None])
                    A.index_add_(0, idx, gabs * w[:, None])
                    B.index_add_(0, idx, gabs)
                    count.index_add_(0, idx, one)
                    continue
                m = mx[dx] if my[dy] is None else (my[dy] if mx[dx] is None else mx[dx] & my[dy])
                if bool(m.any()):
                    B.index_add_(0, idx[m], gabs[m])
    shape = (n, Hp, Wp, C)
    count = count.view(n, Hp, Wp)
    bound = near * B.view(shape) + gamma(count + K_R)[..., None] * A.view(shape)
    return SimpleNamespace(want=want.view(shape), A=A.view(shape), B=B.view(shape), count=count, bound=bound)


def worst_ratio(got, r, interior=True):
    """max err / bound of ``got`` against the reference ``r`` on the interior [1:-1, 1:-1]; where the bound is zero (nothing
    contributes) the element must be exactly zero (inf otherwise)."""
    err = (got.detach().double().cpu() - r.want).abs()
    bound = r.bound
    if interior:
        err, bound = err[:, 1:-1, 1:-1], bound[:, 1:-1, 1:-1]
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ statistics of a case
def _axis32(g, size):
    """``make_axis``'s floor in fp32, emulated: RN(g + 1) in fp32, the product with size / 2 and the sum with -0.5 exact in float64,
    one rounding to fp32 (= the fma)."""
    X = ((g + 1.0).double() * (size / 2.0) - 0.5).float()
    return torch.floor(X).long()


def tap_keys(box, Hf, Wf):
    """box (..., 4) fp32 -> (keys (..., 16): the 16 taps as row * (Wf + 2) + col inside the padded view, cols (..., 4), rows (..., 4),
    dx class, dy class), from the emulated fp32 floors; out-of-image taps clamped to the ring as ``fill_record`` does."""
    xl, xr = _axis32(box[..., 0], Wf), _axis32(box[..., 2], Wf)
    yt, yb = _axis32(box[..., 1], Hf), _axis32(box[..., 3], Hf)
    cols = torch.stack([xl, xl + 1, xr, xr + 1], -1).clamp(-1, Wf) + 1
    rows = torch.stack([yt, yt + 1, yb, yb + 1], -1).clamp(-1, Hf) + 1
    keys = (rows[..., :, None] * (Wf + 2) + cols[..., None, :]).flatten(-2)
    return keys.numpy(), cols.numpy(), rows.numpy(), (xr - xl).clamp(0, 2).numpy(), (yb - yt).clamp(0, 2).numpy()


def case_stats(box, area, visible, Hf, Wf, cell_begin, cell_count, grid_w):
    """box / area / visible of ALL cells of the grid (n, nl, n_cells, ...); the statistics of the processed range."""
    n, nl, n_cells, _ = box.shape
    Hp, Wp = Hf + 2, Wf + 2
    sl = slice(cell_begin, cell_begin + cell_count)
    bx, vis = box[:, :, sl], visible[:, :, sl].numpy().astype(bool)
    keys, cols, rows, dxc, dyc = tap_keys(bx, Hf, Wf)                               # keys (n, nl, cells, 16)
    classes = np.zeros((3, 3), dtype=np.int64)                                       # [dx class, dy class] of visible boxes
    np.add.at(classes, (dxc[vis], dyc[vis]), 1)

    def distinct(v, l, cells):
        cells = [c for c in cells if 0 <= c < cell_count and vis[v, l, c]]
        return len(np.unique(keys[v, l, cells])) if cells else 0

    def tiles(tile_cells):  # tile_cells: list over tiles of four lists (rows of 8) of local cells
        out = [[distinct(v, l, sum(t, []))] + [distinct(v, l, r) for r in t] for v in range(n) for l in range(nl) for t in tile_cells]
        return np.array(out, dtype=np.int64).reshape(-1, 5)

    lines = [[list(range(BWD_BOXES * t + ROW_BOXES * s, BWD_BOXES * t + ROW_BOXES * (s + 1))) for s in range(4)]
             for t in range(-(-cell_count // BWD_BOXES))]
    patches = []
    if grid_w > 0 and cell_count > 0:
        row_a, row_b = cell_begin // grid_w, (cell_begin + cell_count - 1) // grid_w
        for tr in range(row_a // 4, row_b // 4 + 1):
            for tc in range((grid_w + 7) // 8):
                patches.append([[(4 * tr + ry) * grid_w + 8 * tc + cx - cell_begin for cx in range(8) if 8 * tc + cx < grid_w]
                                for ry in range(4)])
    # runs of gather_backward_kernel: boxes in (view, cell, layer) order, chunks of 32, one tap set = same view, class and origins
    order = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 2)).reshape(n * cell_count * nl, *a.shape[3:])  # noqa: E731
    tag = np.concatenate([order(np.broadcast_to(np.arange(n)[:, None, None, None], (n, nl, cell_count, 1))),
                          order(cols[..., [0, 2]]), order(rows[..., [0, 2]]),
                          order(dxc[..., None]), order(dyc[..., None])], axis=1)
    v_flat = order(vis[..., None])[:, 0]
    longest = run = 0
    for i in range(tag.shape[0]):
        cont = i % RUN_CHUNK != 0 and v_flat[i] and v_flat[i - 1] and bool((tag[i] == tag[i - 1]).all())
        run = run + 1 if cont else (1 if v_flat[i] else 0)
        longest = max(longest, run)
    # lists of the deterministic scatter: records per tap, in key order; the pieces of 256 sorted positions a list lies in
    gkeys = (np.arange(n)[:, None, None, None] * Hp * Wp + keys)[vis].reshape(-1)
    records = np.bincount(gkeys, minlength=n * Hp * Wp)
    ends = np.cumsum(records)
    starts = ends - records
    pieces = np.where(records > 0, (ends - 1) // PIECE - starts // PIECE + 1, 0)
    clamped = ((bx == -1.0) | (bx == 0.95)).any(-1).numpy()
    return SimpleNamespace(classes=classes, lines=tiles(lines), patches=tiles(patches), longest_run=longest,
                           max_records=int(records.max()) if records.size else 0, max_pieces=int(pieces.max()) if pieces.size else 0,
                           multi_piece_lists=int((pieces > 1).sum()), visible_share=float(vis.mean()),
                           clamped_share=float(clamped[vis].mean()) if vis.any() else 0.0, n_visible=int(vis.sum()))


def level_counts(tiles):
    """How many tiles (rows of ``case_stats(...).lines`` / ``.patches``) lie clear of the cached kernel's thresholds on each level:
    (<= 120 distinct taps, >= 136 with every row of 8 <= 56, a row of 8 >= 72)."""
    if tiles.size == 0:
        return 0, 0, 0
    total, rows = tiles[:, 0], tiles[:, 1:]
    return (int(((total > 0) & (total <= BWD_HASH - 8)).sum()), int(((total >= BWD_HASH + 8) & (rows <= ROW_HASH - 8).all(1)).sum()),
            int(((total >= BWD_HASH + 8) & (rows >= ROW_HASH + 8).any(1)).sum()))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """Geometry, gradient, boxes, statistics and (lazily) the float64 reference of one call of the scatter."""

    def __init__(self, name, calibs, grid_flat, cube, grid_height, hw, C, cell_begin=0, cell_count=None, grid_w=0, seed=0):
        self.name, self.C, (self.Hf, self.Wf) = name, C, hw
        self.calibs = calibs.reshape(-1, 12).float().contiguous()
        self.grid_flat = grid_flat.reshape(-1, 3).float().contiguous()
        self.zl = torch.arange(0, grid_height, cube[2]).float()
        self.co = torch.tensor(corner_offsets(cube), dtype=torch.float32)
        self.n, self.nl, self.n_cells = self.calibs.shape[0], self.zl.numel(), self.grid_flat.shape[0]
        self.cell_begin = cell_begin
        self.cell_count = self.n_cells - cell_begin if cell_count is None else cell_count
        self.grid_w = grid_w
        self.box_all, self.area_all, self.visible_all = cpu_boxes(self.calibs, self.grid_flat, self.zl, self.co, self.Hf, self.Wf)
        sl = slice(self.cell_begin, self.cell_begin + self.cell_count)
        self.box, self.area, self.visible = self.box_all[:, :, sl], self.area_all[:, :, sl], self.visible_all[:, :, sl]
        self.gvox = torch.randn(self.n, self.cell_count, self.nl * C, generator=torch.Generator().manual_seed(seed))
        self.live = self.visible.permute(0, 2, 1)[..., None].expand(-1, -1, -1, C).reshape(self.gvox.shape)  # (n, cells, nl * C)
        self.integral_shape = (self.n, self.Hf + 2, self.Wf + 2, C)

    @functools.cached_property
    def stats(self):
        return case_stats(self.box_all, self.area_all, self.visible_all, self.Hf, self.Wf, self.cell_begin, self.cell_count, self.grid_w)

    @functools.cached_property
    def ref(self):
        return adjoint_reference(self.box, self.area, self.visible, self.gvox, self.Hf, self.Wf)

    def reference(self, gvox):
        return adjoint_reference(self.box, self.area, self.visible, gvox, self.Hf, self.Wf)


SCENE_CUBE, SCENE_GRID_HEIGHT = (50, 50, 40), 120   # three layers of 40


def scene_geometry():
    """Two near ring cameras over a 14 x 18 ground grid (the rig of tests/test_hip_backward.py::_case, radius pulled in so that
    boxes reach the image border and the clamp): calibs (2, 3, 4), grid (14, 18, 3)."""
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.utils import make_grid
    grid = make_grid((700, 900), cube_LW=(50, 50), dataset=DATA)
    calibs = ring_cameras(3, (450., 350., 0.), 520., 350., 150. * IMAGE_SIZE[1] / 176., (IMAGE_SIZE[1], IMAGE_SIZE[0]), phase=0.4)[:2]
    return calibs, grid


@functools.lru_cache(maxsize=None)
def scene(map_index, C):
    calibs, grid = scene_geometry()
    return Case(f"scene {MAPS[map_index]} C {C}", calibs, grid, SCENE_CUBE, SCENE_GRID_HEIGHT, MAPS[map_index], C,
                grid_w=grid.shape[1], seed=100 + map_index)


DUP_CELLS = 2049  # 64 full tiles of 32 and one box more; 16 x 2049 records per (layer), lists of >= 2049 records


@functools.lru_cache(maxsize=None)
def duplicates(nl, C=256, cells=DUP_CELLS):
    """One ground point that camera 0 sees on every layer, ``cells`` times."""
    calibs, grid = scene_geometry()
    cube, gh = (50, 50, 40), 40 * nl
    probe = Case("probe", calibs[:1], grid, cube, gh, MAPS[0], 1)
    seen = probe.visible[0].all(0).nonzero()[:, 0]
    point = probe.grid_flat[seen[seen.numel() // 2]]
    return Case(f"duplicates nl {nl} x {cells}", calibs[:1], point[None].repeat(cells, 1), cube, gh, MAPS[0], C,
                grid_w=683 if cells % 683 == 0 else 0, seed=200 + nl)


LEVEL_TILES, LEVELS_GRID_W = 8, 16  # tiles per level; the patch variant lays the tiles two abreast


@functools.lru_cache(maxsize=None)
def level_tiles():
    """3 x LEVEL_TILES tiles of 4 rows x 8 ground points (camera 0, one layer, the 23 x 40 map), chosen on the CPU from a 10 cm
    lattice over the scene by their distinct taps: level 1 = a compact 4 x 8 block of the lattice (<= 120 distinct taps), level 2 =
    four rows of 8 neighbours (36..52 taps each) from places with no tap in common (>= 144), level 3 = rows of 8 boxes of 16 taps
    each with no tap in common (128 per row).  -> (24, 4, 8, 3), levels interleaved 1, 2, 3, 1, ..."""
    from vfa_amd.utils import make_grid
    calibs, _ = scene_geometry()
    fine = make_grid((700, 900), cube_LW=(10, 10), dataset=DATA)
    L, W = fine.shape[:2]
    pool_case = Case("pool", calibs[:1], fine, (50, 50, 40), 40, MAPS[0], 1)
    keys = tap_keys(pool_case.box[0, 0], *MAPS[0])[0].reshape(L, W, 16)
    vis = pool_case.visible[0, 0].numpy().reshape(L, W)
    sets = [[set(keys[r, c].tolist()) for c in range(W)] for r in range(L)]

    def union(cells):
        return set().union(*(sets[r][c] for r, c in cells))

    level1, level2, level3 = [], [], []
    for r in range(2, L - 4, 7):                      # level 1: compact blocks
        for c in range(2, W - 8, 11):
            cells = [[(r + ry, c + cx) for cx in range(8)] for ry in range(4)]
            flat = sum(cells, [])
            if all(vis[p] for p in flat) and len(union(flat)) <= BWD_HASH - 16 and len(level1) < LEVEL_TILES:
                level1.append(cells)
    rows2 = []                                        # level 2: rows of 8 neighbours with 36..52 distinct taps
    for r in range(1, L, 3):
        for c in range(1, W - 8, 9):
            row = [(r, c + cx) for cx in range(8)]
            if all(vis[p] for p in row) and 36 <= len(union(row)) <= 52:
                rows2.append(row)
    used = [False] * len(rows2)
    for i in range(len(rows2)):
        if used[i] or len(level2) == LEVEL_TILES:
            continue
        tile, taps = [rows2[i]], union(rows2[i])
        for j in range(i + 1, len(rows2)):
            if not used[j] and len(tile) < 4 and not (taps & union(rows2[j])):
                tile.append(rows2[j])
                taps |= union(rows2[j])
        if len(tile) == 4:
            for row in tile:
                used[rows2.index(row)] = True
            level2.append(tile)
    big = [(r, c) for r in range(0, L, 2) for c in range(0, W, 2) if vis[r, c] and len(sets[r][c]) == 16]
    start = 0                                         # level 3: rows of 8 boxes with no tap in common
    while len(level3) < LEVEL_TILES and start < len(big):
        tile = []
        for s in range(4):
            row, taps = [], set()
            for p in big[start + s::7]:
                if len(row) < 8 and not (taps & sets[p[0]][p[1]]):
                    row.append(p)
                    taps |= sets[p[0]][p[1]]
            tile.append(row)
        if all(len(row) == 8 for row in tile):
            level3.append(tile)
        start += 29
    assert len(level1) == len(level2) == len(level3) == LEVEL_TILES, (len(level1), len(level2), len(level3))
    tiles = [t for trio in zip(level1, level2, level3) for t in trio]
    return torch.stack([torch.stack([torch.stack([fine[p] for p in row]) for row in t]) for t in tiles])


@functools.lru_cache(maxsize=None)
def levels(kind, C=256):
    """The tiles of ``level_tiles`` as 32 cells in a line each ("lines", grid_w = 0) or as 4 x 8 patches of a ground grid 16 wide
    ("patches")."""
    calibs, _ = scene_geometry()
    tiles = level_tiles()
    if kind == "lines":
        grid, gw = tiles.reshape(-1, 3), 0
    else:
        t = tiles.view(-1, LEVELS_GRID_W // 8, 4, 8, 3)           # (tile row, tile column, ry, cx)
        grid, gw = t.permute(0, 2, 1, 3, 4).reshape(-1, 3), LEVELS_GRID_W
    return Case(f"levels {kind}", calibs[:1], grid, (50, 50, 40), 40, MAPS[0], C, grid_w=gw, seed=300)


RANGES = {18: dict(map_index=0, cols=18, cell_begin=23, cell_count=201), 13: dict(map_index=1, cols=13, cell_begin=17, cell_count=150)}


@functools.lru_cache(maxsize=None)
def ranges(grid_w, C=256):
    """The scene's 14 rows (no multiple of 4) x ``grid_w`` columns, a range that begins inside a patch and whose length is no
    multiple of 32."""
    calibs, grid = scene_geometry()
    r = RANGES[grid_w]
    return Case(f"ranges grid_w {grid_w}", calibs, grid[:, :r["cols"]].contiguous(), SCENE_CUBE, SCENE_GRID_HEIGHT, MAPS[r["map_index"]], C,
                cell_begin=r["cell_begin"], cell_count=r["cell_count"], grid_w=grid_w, seed=400 + grid_w)
