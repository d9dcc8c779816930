"""What tests/test_det_loss_cpu.py and tests/test_det_loss.py share: a restatement of the reference's target encoder
(vfa/data/encoder.py:152-217) and detection loss (vfa/model/loss.py) in the sparse form -- the positive cells of a frame in ascending
order and their targets -- with torch operations, generic in the dtype: float32 is pinned to the reference's records
(tests/golden/det_loss_*.npz) on the CPU, float64 is what the GPU tests measure the kernels against, and the float32 evaluation's own
error against float64 is the scale of their bounds."""
import numpy as np
import torch

from conftest import golden_path

FIXTURES = ("det_loss_mc.npz", "det_loss_mx.npz", "det_loss_wt.npz")
F = np.float32
EPS = 1e-5
MARGIN = 4.0            # for the other summation order and the device's expf / logf
FLOOR = 2.0 ** -23      # no bound below one float32 ulp, relative
TERMS = ("loss_heatmap", "loss_pos", "loss_hwl", "loss_ang")


def load(name):
    d = np.load(golden_path(name))
    return d, str(d["base"]) == "MultiviewC"


def table64(R, sigma):
    x = np.arange(-(R // 2), R // 2, dtype=np.float64)
    return np.exp(-x ** 2 / (2.0 * float(sigma) ** 2))


def label_rows(labels, R, sigma):
    """The CSL rows of integer labels, float32: row[j] = table[(j + R/2 - label) mod R]."""
    table = table64(R, sigma).astype(F)
    index = (np.arange(R)[None, :] + R // 2 - np.asarray(labels, np.int64)[:, None]) % R
    return table[index]


def encode(location, world_size, grid_lw, base, dimension=None, rotation=None, mean=None):
    """One frame of objects (numpy float32) -> the sparse targets, the rules in float32 numpy one operation at a time: dict of
    ``cells (n)`` ascending, ``loc_offset (n, 2)`` and in 3D ``dim_offset (n, 3)``, ``label (n)``.  Later objects overwrite earlier
    ones of the same cell; objects outside the map are dropped."""
    L, W = grid_lw
    loc = np.asarray(location, F).reshape(-1, np.asarray(location).shape[-1])
    with np.errstate(all="ignore"):
        u = (loc[:, 0] / F(world_size[0]) * F(L)).astype(F)
        v = (loc[:, 1] / F(world_size[1]) * F(W)).astype(F)
    by_cell = {}
    for i in range(len(loc)):
        if not (np.isfinite(u[i]) and np.isfinite(v[i]) and abs(u[i]) < 2.0 ** 31 and abs(v[i]) < 2.0 ** 31):
            continue
        cx, cy = int(u[i]), int(v[i])
        row, col = (cx, cy) if base == "Wildtrack" else (cy, cx)
        if 0 <= row < L and 0 <= col < W:
            by_cell[row * W + col] = (i, F(u[i] - F(cx)), F(v[i] - F(cy)))
    cells = np.array(sorted(by_cell), dtype=np.int32)
    who = np.array([by_cell[c][0] for c in cells], dtype=np.int64)
    out = {"cells": cells, "loc_offset": np.array([by_cell[c][1:] for c in cells], dtype=F).reshape(-1, 2)}
    if dimension is not None:
        quotient = (np.asarray(dimension, F)[who] / np.asarray(mean, F)[None, :]).astype(F)
        out["dim_quotient"] = quotient
        out["dim_offset"] = torch.log(torch.from_numpy(quotient)).numpy()   # (torch's float32 log, the reference's)
        out["label"] = np.array([int(F(a) * F(57.29577951308232)) for a in np.asarray(rotation, F)[who]], dtype=np.int32)
    return out


def focal(x, gt):
    """The focal loss with 'mean' reduction and its two special cases; no entries: 0."""
    p = torch.sigmoid(x).clamp(EPS, 1.0 - EPS)
    positive = gt == 1
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    pos = torch.where(positive, -(((1 - p) ** 2) * torch.log(p)), zero).sum()
    neg = torch.where(positive, zero, -(((1 - gt) ** 4) * (p ** 2) * torch.log(1 - p))).sum()
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 and n_neg == 0:
        return zero
    if n_pos == 0:
        return neg / n_neg
    if n_neg == 0:
        return pos / n_pos
    return neg / n_neg + pos / n_pos


def smooth_l1(d):
    z = d.abs()
    return torch.where(z < 1, 0.5 * z * z, z - 0.5)


def frame_terms(heatmap, gt_heatmap, loc, cells, loc_t, dim=None, dim_t=None, rot_rows=None, gt_rows=None):
    """One frame, any dtype: heatmap / gt_heatmap (L, W), loc (L, W, 2), cells (n) long, loc_t (n, 2); 3D: dim (L, W, 3), dim_t
    (n, 3), rot_rows / gt_rows (n, R) -- the logits and the CSL rows AT the cells.  -> the four unweighted terms."""
    zero = torch.zeros((), dtype=heatmap.dtype, device=heatmap.device)
    n = max(len(cells), 1)
    out = {"loss_heatmap": focal(heatmap, gt_heatmap),
           "loss_pos": (smooth_l1(torch.sigmoid(loc.reshape(-1, 2)[cells]) - loc_t) / n).sum() if len(cells) else zero}
    if dim is not None:
        out["loss_hwl"] = (smooth_l1(dim.reshape(-1, 3)[cells] - dim_t) / n).sum() if len(cells) else zero
        out["loss_ang"] = focal(rot_rows, gt_rows) if len(cells) else zero
    return out


def weighted(terms, weights):
    """loss.py:66-67's order: location, dimension, heat map, angle."""
    w = dict(zip(TERMS, weights))
    total = terms["loss_pos"] * w["loss_pos"]
    if "loss_hwl" in terms:
        total = total + terms["loss_hwl"] * w["loss_hwl"]
    total = total + terms["loss_heatmap"] * w["loss_heatmap"]
    if "loss_ang" in terms:
        total = total + terms["loss_ang"] * w["loss_ang"]
    return total


def evaluate(pred, targets, gt_heatmap, weights, dtype):
    """A batch through ``frame_terms`` with autograd.  pred: heatmap (B, 1, L, W), loc_offset (B, L, W, 2) and in 3D dim_offset
    (B, L, W, 3), rotation_at (B, k, R), float32 CPU tensors; targets: per frame the dict of ``encode`` plus ``rows`` (n, R) in 3D;
    gt_heatmap (B, L, W).  -> ({name: (B,) numpy of WEIGHTED values, 'loss'}, {head: gradient of sum_b loss[b]})."""
    three_d = "dim_offset" in pred
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in pred.items()}
    names = ("loss",) + TERMS[:4 if three_d else 2]
    per_frame = {k: [] for k in names}
    total = 0
    for b, t in enumerate(targets):
        cells = torch.from_numpy(np.asarray(t["cells"], np.int64))
        n = len(cells)
        extra = {}
        if three_d:
            extra = dict(dim=leaves["dim_offset"][b], dim_t=torch.from_numpy(t["dim_offset"]).to(dtype),
                         rot_rows=leaves["rotation_at"][b, :n], gt_rows=torch.from_numpy(t["rows"]).to(dtype))
        terms = frame_terms(leaves["heatmap"][b, 0], gt_heatmap[b].to(dtype), leaves["loc_offset"][b], cells,
                            torch.from_numpy(t["loc_offset"]).to(dtype), **extra)
        loss = weighted(terms, weights)
        total = total + loss
        per_frame["loss"].append(loss.item())
        for k, w in zip(TERMS, weights):
            if k in terms:
                per_frame[k].append(terms[k].item() * w)
    total.backward()
    return ({k: np.array(v, dtype=np.float64) for k, v in per_frame.items()},
            {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in leaves.items()})


def bound(err_ref32):
    """The bound of the issue: the float32 reference's own error against float64 times a margin, never below one ulp."""
    return max(MARGIN * float(err_ref32), FLOOR)


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if got.size else 0.0


def normwise(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    scale = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / scale) if scale > 0 else float(np.abs(got).max(initial=0.0))


def maxabs(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    scale = np.abs(want).max(initial=0.0)
    return float(np.abs(got - want).max(initial=0.0) / scale) if scale > 0 else float(np.abs(got).max(initial=0.0))


def fixture_case(d, three_d):
    """The fixture as the operands of ``evaluate`` / ``detection_loss``: pred (rotation_at = the stored logits at the mask rows),
    the targets restated from the object arrays, the dense heat-map target."""
    L, W = (int(v) for v in d["grid_lw"])
    t = encode(d["obj_location"], d["world_size"], (L, W), str(d["base"]), d["obj_dimension"] if three_d else None,
               d["obj_rotation"] if three_d else None, d["dimension_mean"])
    pred = {"heatmap": torch.from_numpy(d["heatmap"]), "loc_offset": torch.from_numpy(d["loc_offset"])}
    if three_d:
        t["rows"] = label_rows(t["label"], int(d["angle_range"]), float(d["angle_radius"]))
        pred["dim_offset"] = torch.from_numpy(d["dim_offset"])
        pred["rotation_at"] = torch.from_numpy(d["rotation_rows"])[None]
    return pred, [t], torch.from_numpy(d["gt_heatmap"])[None]


def synthetic_case(seed, B, L, W, counts, R=0, base="MultiviewC", saturate=True):
    """Seeded frames: ``counts[b]`` objects (two of them share a cell when there are at least three), heads with a few saturated
    heat-map logits, a dense heat-map target that is 1 exactly at the positive cells.  world = 4 L x 4 W, placed so that the
    kind's convention keeps every object inside.  -> dict with the object arrays (padded to K = max(counts, 1)), pred, targets.

    The focal logits (heat map, rotation) are N(-2, 1.5): mostly background, as in training.  The reason is the conditioning of the
    reference's float32 formula, not the kernels: it rounds p = sigmoid(x) and then takes log(1 - p), so an element's error is
    ulp(p) / (1 - p) -- 1e-5 of the element at p = 0.999, and those elements are the largest of the sum.  With many logits above
    +3 the float32 error of a term is one draw of a wide distribution (1e-9 .. 1e-6 for the same shape), for the reference's
    evaluation and for any other float32 evaluation alike, and four times one draw does not bound another.  Below p = 0.9 the
    elements' errors stay near one ulp.  The fixtures keep the reference's wide logits (N(-1, 3), N(0, 2.5))."""
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    three_d = R > 0
    K = max(max(counts), 1)
    world = (4.0 * L, 4.0 * W)
    wild = base == "Wildtrack"
    mean = np.array([140.0, 60.0, 230.0], F)
    location, dimension = np.zeros((B, K, 3), F), np.ones((B, K, 3), F)
    rotation = np.zeros((B, K), F)
    targets, gt_heat = [], torch.zeros(B, L, W)
    for b, n in enumerate(counts):
        rows, cols = rng.uniform(0, L, n), rng.uniform(0, W, n)
        if n >= 3:
            rows[n - 1], cols[n - 1] = np.floor(rows[0]) + 0.25, np.floor(cols[0]) + 0.75   # the last object lands on the first's cell
        # u = loc0 / (4 L) * L = loc0 / 4 indexes the row for Wildtrack and the column otherwise; v = loc1 / 4 the other one
        first, second = (rows, cols) if wild else (cols, rows)
        location[b, :n, 0], location[b, :n, 1] = first * 4.0, second * 4.0
        dimension[b, :n] = mean[None] * np.exp(rng.randn(n, 3) * 0.2)
        rotation[b, :n] = rng.uniform(-np.pi, 2.9 * np.pi, n)
        t = encode(location[b, :n], world, (L, W), base, dimension[b, :n] if three_d else None, rotation[b, :n] if three_d else None,
                   mean)
        if three_d:
            t["rows"] = label_rows(t["label"], R, 6)
        targets.append(t)
        heat = torch.rand(L, W, generator=g) * 0.9
        heat.view(-1)[torch.from_numpy(t["cells"].astype(np.int64))] = 1.0
        gt_heat[b] = heat
    pred = {"heatmap": (torch.randn(B, 1, L, W, generator=g) * 1.5 - 2.0).clamp(max=2.0), "loc_offset": torch.randn(B, L, W, 2, generator=g)}
    if saturate:
        pred["heatmap"][:, 0, 0, :2] = torch.tensor([15.0, -15.0])
    edge = (pred["heatmap"].abs() - 11.5129).abs() < 1e-3
    pred["heatmap"][edge] = 0.5      # (no logit where one ulp of expf decides whether the clamp passes a gradient)
    if three_d:
        pred["dim_offset"] = torch.randn(B, L, W, 3, generator=g) * 0.4
        pred["rotation_at"] = (torch.randn(B, K, R, generator=g) * 1.5 - 2.0).clamp(max=2.0)
    return dict(location=location, dimension=dimension, rotation=rotation, count=np.array(counts, np.int32), world=world, mean=mean,
                base=base, K=K, pred=pred, targets=targets, gt_heatmap=gt_heat, three_d=three_d)
