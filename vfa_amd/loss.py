"""Training targets and the detection loss without a host wait: the encode half of the reference's ``ObjectEncoder``
(``vfa/data/encoder.py:152-217``) and ``compute_loss3d`` / ``compute_loss2d`` (``vfa/model/loss.py``) in the sparse form that
``VFANet.heads(rotation_at=cells)`` defines -- a list of positive cells per frame instead of dense ``(B, 360, L, W)`` targets.

    objs = pack_objects(frames, device)                                       # the only place that touches Python objects
    targets = encoder.encode(objs.location, objs.count, objs.dimension, objs.rotation, grid_lw=(L, W))
    gt_heatmap = encoder.heatmap(objs.location, objs.count, objs.dimension, rotation_deg=degrees, heatmap_type="RGK", grid_lw=(L, W))
    pred = model(images, calibs, grid, rotation_at=targets.cells)
    detection_loss(pred, targets, gt_heatmap)["loss"].sum().backward()

``gt_heatmap`` is rendered on the device from the same object tensors (``TargetEncoder.heatmap``: the reference's ``vfa/data/GK.py``
maps, which its datasets precompute on the host and cache): its cells equal to 1 are ``targets.cells``, and the object lists are
the only input of the step.  Everything between the object tensors and ``backward()`` is stream-ordered HIP
(``vfa_amd/csrc/vfa_loss.hip``, ``vfa_heat.hip``): no ``.item()``, no
``int(tensor)``, outputs of fixed shape, so the step can be captured in a graph.  Deviations from the reference, all in cases where it
has no defined value: an object outside the map (or with a non-finite coordinate) is dropped instead of raising / wrapping a negative
index; an angle label outside ``-R/2 .. 3R/2 - 1`` wraps modulo ``R``; a frame without positives has 0 for the three sparse terms
(the reference's empty encode is a tuple, its empty focal loss 0 / 0); the ``loss_dict`` of ``compute_loss3d`` / ``compute_loss2d``
holds 0-dim device tensors instead of floats.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, ops

MAX_OBJECTS = 1024  # VFA_DET_MAX_OBJECTS
TERMS = ("loss_heatmap", "loss_pos", "loss_hwl", "loss_ang")  # the order of ``loss_weight`` and of the kernels' ``terms``


def label_table(angle_range=360, angle_radius=6):
    """``table[i] = exp(-(i - R/2)^2 / (2 sigma^2))`` in float64, rounded to float32 like the reference's ``torch.tensor(smooth_label)``
    assignment: the CSL row of a label is ``table[(j + R/2 - label) mod R]`` (``gaussian_label`` for an even ``R``)."""
    R = int(angle_range)
    if R < 2 or R % 2 or R > 1024:
        raise ValueError(f"angle_range must be even and in 2 .. 1024, got {angle_range}")
    x = np.arange(-(R // 2), R // 2, dtype=np.float64)
    return torch.from_numpy(np.exp(-x ** 2 / (2.0 * float(angle_radius) ** 2)).astype(np.float32))


def gk_table(grid_reduce=4, radius=8):
    """``table[y][x] = exp(-(x^2 + y^2) / (2 sigma^2))``, ``sigma^2 = 8 / grid_reduce``, in float64, rounded to float32: the
    ``(2 radius + 1)^2`` kernel of the reference's ``GaussianKernel`` (``multivariate_normal.pdf / max``)."""
    r = int(radius)
    if not 0 <= r <= 16 or not float(grid_reduce) > 0:
        raise ValueError(f"gk_table: radius in 0 .. 16 and grid_reduce > 0, got {radius}, {grid_reduce}")
    x = np.arange(-r, r + 1, dtype=np.float64)
    return torch.from_numpy(np.exp(-(x[None, :] ** 2 + x[:, None] ** 2) / (2.0 * (8.0 / float(grid_reduce)))).astype(np.float32))


class PackedObjects(NamedTuple):
    location: torch.Tensor             # (B, K, 3) float32, zero padded
    count: torch.Tensor                # (B,) int32
    dimension: Optional[torch.Tensor]  # (B, K, 3), padded with ones
    rotation: Optional[torch.Tensor]   # (B, K)


def pack_objects(frames, device=None, max_objects=128):
    """A list, per frame, of objects with ``.location`` (2 or 3 numbers) and -- all of them or none -- ``.dimension`` (3) and
    ``.rotation`` (radians) -> padded ``(B, K, ...)`` tensors and the counts.  The host side is ONE buffer (pinned when a device is
    given) and goes over in one non-blocking copy; the fields are views of it.  More than ``max_objects`` objects in a frame raise."""
    B, K = len(frames), int(max_objects)
    if not 0 < K <= MAX_OBJECTS:
        raise ValueError(f"max_objects must be in 1 .. {MAX_OBJECTS}, got {max_objects}")
    three_d = any(hasattr(o, "dimension") and o.dimension is not None for objs in frames for o in objs)
    words = B + B * K * (7 if three_d else 3)
    pin = device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available()
    host = torch.zeros(words, dtype=torch.int32, pin_memory=pin)
    arr = host.numpy()
    count = arr[:B]
    real = arr[B:].view(np.float32)
    loc = real[:B * K * 3].reshape(B, K, 3)
    dim = real[B * K * 3:B * K * 6].reshape(B, K, 3) if three_d else None
    rot = real[B * K * 6:].reshape(B, K) if three_d else None
    if three_d:
        dim[...] = 1.0
    for b, objs in enumerate(frames):
        if len(objs) > K:
            raise ValueError(f"pack_objects: frame {b} has {len(objs)} objects, max_objects is {K}")
        count[b] = len(objs)
        for i, o in enumerate(objs):
            xyz = np.asarray(o.location, dtype=np.float32).reshape(-1)
            loc[b, i, :len(xyz)] = xyz
            if three_d:
                dim[b, i] = np.asarray(o.dimension, dtype=np.float32).reshape(3)
                rot[b, i] = float(o.rotation)
    if device is not None:
        host = host.to(device, non_blocking=True)
    real_t = host[B:].view(torch.float32)
    return PackedObjects(real_t[:B * K * 3].view(B, K, 3), host[:B],
                         real_t[B * K * 3:B * K * 6].view(B, K, 3) if three_d else None,
                         real_t[B * K * 6:].view(B, K) if three_d else None)


class DetTargets(NamedTuple):
    """The training targets of a batch in the sparse form: per frame the positive cells in ascending order (the order of
    ``pred[...][mask]``) and the targets of those cells, padded to a fixed ``k``."""
    cells: torch.Tensor                   # (B, k) int32 row * W + column, -1 behind n_pos: what VFANet.forward(rotation_at=...) takes
    n_pos: torch.Tensor                   # (B,) int32
    loc_offset: torch.Tensor              # (B, k, 2)
    dim_offset: Optional[torch.Tensor]    # (B, k, 3) log(dimension / mean); None in 2D
    angle_label: Optional[torch.Tensor]   # (B, k) int32 degrees; the CSL row is table[(j + R/2 - label) mod R]
    table: Optional[torch.Tensor]         # (R,) float32

    @staticmethod
    def from_dense(batch_gt, max_positives, angle_radius=6):
        """From the reference encoder's dense dict (``mask (B, 1, L, W)``, ``loc_offset (B, L, W, 2)`` and in 3D ``dim_offset
        (B, L, W, 3)``, ``rotation (B, L, W, R)``): torch operations only, no host wait.  The first ``max_positives`` positives of
        a frame in cell order are kept; the label is the arg-max of the cell's rotation row (its single entry equal to 1)."""
        mask = batch_gt["mask"]
        B, (L, W) = mask.shape[0], mask.shape[-2:]
        n_cells = L * W
        k = min(int(max_positives), n_cells)
        index = torch.arange(n_cells, device=mask.device)
        score = torch.where(mask.reshape(B, n_cells) == 1, n_cells - index, torch.zeros_like(index))  # positives first, low cells first
        top, at = torch.topk(score, k, dim=1)
        valid = top > 0
        cells = torch.where(valid, at, torch.full_like(at, -1)).to(torch.int32)
        n_pos = valid.sum(dim=1).to(torch.int32)

        def rows(dense):
            c = dense.shape[-1]
            got = torch.gather(dense.reshape(B, n_cells, c), 1, at.unsqueeze(-1).expand(B, k, c))
            return got * valid.unsqueeze(-1).to(got.dtype)
        three_d = "rotation" in batch_gt
        dim = rows(batch_gt["dim_offset"]) if three_d else None
        label = table = None
        if three_d:
            rot = rows(batch_gt["rotation"])
            label = torch.argmax(rot, dim=-1).to(torch.int32)
            table = label_table(rot.shape[-1], angle_radius).to(mask.device)
        return DetTargets(cells, n_pos, rows(batch_gt["loc_offset"]), dim, label, table)


class TargetEncoder:
    """The encode half next to ``eval_ops.BEVDecoder``: ``base`` is the dataset class name, ``world_size`` / ``cube_LWH`` as in the
    dataset configs, ``dimension_mean`` = ``classAverage.get_mean(...)`` (3D only), ``angle_range`` / ``angle_radius`` the CSL
    parameters of the reference's ``ObjectEncoder``, ``max_objects`` the padded length ``pack_objects`` should be given."""

    def __init__(self, base, world_size, cube_LWH, dimension_mean=None, angle_range=360, angle_radius=6, max_objects=128):
        if base not in _lib.CONV_KIND and base != "MVM3D":
            raise ValueError(f"TargetEncoder: unknown dataset {base!r}")
        self.base, self.kind = base, _lib.CONV_KIND.get(base, 0)
        self.world_size = np.array(world_size)
        self.grid_size = self.world_size / np.array(cube_LWH)[:2]
        self.dimension_mean = dimension_mean
        self.angle_range, self.angle_radius, self.max_objects = int(angle_range), angle_radius, int(max_objects)
        self._table_host = label_table(angle_range, angle_radius)
        self._tables = {}
        self._gk_tables = {}

    def table(self, device):
        """The label table on ``device`` (uploaded once per device, outside any captured region)."""
        key = str(device)
        if key not in self._tables:
            self._tables[key] = self._table_host.to(device)
        return self._tables[key]

    def encode(self, location, count, dimension=None, rotation=None, grid_lw=None):
        """Device tensors ``location (B, K, 2|3)``, ``count (B)`` int32 and in 3D ``dimension (B, K, 3)``, ``rotation (B, K)`` ->
        ``DetTargets`` with ``k = K``, from one library call (``vfa_det_targets_f32``)."""
        L, W = (int(round(v)) for v in self.grid_size) if grid_lw is None else grid_lw
        three_d = dimension is not None or rotation is not None
        if three_d and self.dimension_mean is None:
            raise ValueError("TargetEncoder.encode: 3D targets need dimension_mean")
        _lib.require_device(location, count, dimension, rotation)
        cells, n_pos, loc_offset, dim_offset, label = ops.det_targets(location, count, dimension, rotation, self.dimension_mean,
                                                                      self.world_size, (L, W), self.kind)
        return DetTargets(cells, n_pos, loc_offset, dim_offset, label, self.table(location.device) if three_d else None)


    def gk_table(self, device, grid_reduce=4, radius=8):
        """The GK table ``float32(exp(-(x^2 + y^2) / (2 sigma^2)))``, ``sigma^2 = 8 / grid_reduce``, ``(2 radius + 1)^2``, on
        ``device``: made once in float64 numpy and uploaded once per device, outside any captured region (what the reference's
        ``multivariate_normal.pdf / max`` gives, in every float32 bit)."""
        key = (str(device), float(grid_reduce), int(radius))
        if key not in self._gk_tables:
            self._gk_tables[key] = gk_table(grid_reduce, radius).to(device)
        return self._gk_tables[key]

    def heatmap(self, location, count, dimension=None, rotation=None, rotation_deg=None, heatmap_type="RGK", grid_lw=None, alpha=0.01,
                ratio=8, grid_reduce=4, radius=8, return_clipped=False):
        """The dense heat-map target ``(B, L, W)`` float32 of ``detection_loss`` from the tensors ``encode`` takes, rendered on the
        device (``vfa_heat_rgk_f32`` / ``vfa_heat_gk_f32``, rules in ``vfa_amd/csrc/vfa_heat.h``); its cells equal to 1 are
        ``encode(...).cells``.

        ``"RGK"`` (the reference's ``RotationGaussianKernel``) needs ``dimension (B, K, 3)`` = (h, w, l) and the angle:
        ``rotation_deg (B, K)``, float32 or float64, the ANNOTATION's degrees -- the reference renders from that number, so this
        is the path that reproduces its maps -- or else ``rotation (B, K)`` in radians, converted on the device with
        ``torch.rad2deg(rotation.double())``: not the annotation's bits (the radians were rounded to float32), the same map up to
        the rounding of the angle.  ``alpha`` / ``ratio`` as in the reference; an object whose kernel would have more than 65 taps
        per side gives its centre only (``return_clipped=True`` also returns their number per frame, ``(B,)`` int32).
        ``"GK"`` (``GaussianKernel``) needs neither: ``radius`` and ``sigma^2 = 8 / grid_reduce`` of its table.
        Deviations, where the reference has no value: an arg-max tie of a rotated kernel takes the first cell, kernel cells outside
        the map are dropped, an object outside the map is dropped, two objects in a cell count once."""
        L, W = (int(round(v)) for v in self.grid_size) if grid_lw is None else grid_lw
        _lib.require_device(location, count, dimension, rotation, rotation_deg)
        if heatmap_type == "GK":
            heat = ops.heat_gk(location, count, self.gk_table(location.device, grid_reduce, radius), self.world_size, (L, W), self.kind)
            return (heat, torch.zeros_like(count)) if return_clipped else heat
        if heatmap_type != "RGK":
            raise ValueError(f"TargetEncoder.heatmap: heatmap_type must be 'RGK' or 'GK', got {heatmap_type!r}")
        if dimension is None or (rotation is None and rotation_deg is None):
            raise ValueError("TargetEncoder.heatmap: 'RGK' needs dimension and rotation_deg (degrees) or rotation (radians)")
        if rotation_deg is not None and rotation_deg.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"TargetEncoder.heatmap: rotation_deg must be float32 or float64, got {rotation_deg.dtype}")
        degrees = rotation_deg.double() if rotation_deg is not None else torch.rad2deg(rotation.double())
        heat, clipped = ops.heat_rgk(location, count, dimension, degrees, self.world_size, (L, W), self.kind, alpha, ratio)
        return (heat, clipped) if return_clipped else heat


class _DetLoss(torch.autograd.Function):
    """One node on ``vfa_det_loss_f32`` / ``vfa_det_loss_backward_f32``: (heads) -> (loss (B), terms (B, 4))."""

    @staticmethod
    def forward(ctx, heatmap, loc, dim, rot, gt_heatmap, targets, weights):
        operands = (heatmap, gt_heatmap, loc, dim, rot, targets.cells, targets.n_pos, targets.loc_offset,
                    targets.dim_offset if dim is not None else None, targets.angle_label if dim is not None else None,
                    targets.table if dim is not None else None)
        terms, loss, counts = ops.det_loss_forward(*operands, loss_weight=weights)
        ctx.operands, ctx.counts, ctx.weights = operands, counts, weights
        ctx.mark_non_differentiable(counts)
        return loss, terms, counts

    @staticmethod
    def backward(ctx, g_loss, g_terms, _):
        coef = g_terms + torch.stack([g_loss * w for w in ctx.weights], dim=1)
        d_heat, d_loc, d_dim, d_rot = ops.det_loss_backward(coef, ctx.counts, *ctx.operands)
        return d_heat, d_loc, d_dim, d_rot, None, None, None


def detection_loss(pred, targets, gt_heatmap, loss_weight=(1.0, 1.0, 1.0, 1.0)):
    """The reference's loss (``loss.py:45-102``) per frame of a batch: ``pred`` is what ``VFANet`` returns (3D if it has
    ``dim_offset``), ``targets`` a ``DetTargets``, ``gt_heatmap (B, L, W)`` or ``(B, 1, L, W)`` the dense heat-map target: what
    ``TargetEncoder.heatmap`` renders from the same object tensors (or a map the dataset precomputed).  Returns
    ``{"loss", "loss_heatmap", "loss_pos"[, "loss_hwl", "loss_ang"]}``, device tensors of shape ``(B,)``, weighted like the
    reference's ``loss_dict``; differentiable with respect to the heads.  ``pred["rotation_at"]`` must have been evaluated at
    ``targets.cells`` (``pred["rotation_cells"]``, the same tensor); a dense ``pred["rotation"]`` is gathered at those cells."""
    heatmap, loc = pred["heatmap"], pred["loc_offset"]
    three_d = "dim_offset" in pred
    w = [float(v) for v in loss_weight]
    if len(w) not in ((4,) if three_d else (2, 4)):     # (2D: heat map and location, the first two of four)
        raise ValueError(f"detection_loss: {'3D' if three_d else '2D'} takes {4 if three_d else 2} loss weights, got {len(w)}")
    _lib.require_device(heatmap, loc, gt_heatmap, targets.cells)
    w = tuple(w[:4 if three_d else 2] + [0.0, 0.0][:0 if three_d else 2])
    B, _, L, W = heatmap.shape
    if gt_heatmap.dim() == 4:
        gt_heatmap = gt_heatmap.reshape(B, L, W) if gt_heatmap.is_contiguous() else gt_heatmap[:, 0]
    dim = rot = None
    if three_d:
        dim = pred["dim_offset"]
        if "rotation_at" in pred:
            rot, at = pred["rotation_at"], pred.get("rotation_cells")
            if at is not None and (at.data_ptr() != targets.cells.data_ptr() or at.shape != targets.cells.shape):
                raise ValueError("detection_loss: pred['rotation_at'] was not evaluated at targets.cells")
        elif "rotation" in pred:
            dense = pred["rotation"]
            at = targets.cells.long().clamp(0, L * W - 1)
            rot = torch.gather(dense.reshape(B, L * W, dense.shape[-1]), 1, at.unsqueeze(-1).expand(-1, -1, dense.shape[-1]))
        else:
            raise ValueError("detection_loss: a 3D pred needs 'rotation_at' or 'rotation'")
        if targets.dim_offset is None or targets.angle_label is None or targets.table is None:
            raise ValueError("detection_loss: a 3D pred needs 3D targets")
    loss, terms, _ = _DetLoss.apply(heatmap, loc, dim, rot, gt_heatmap, targets, w)
    out = {"loss": loss}
    for i, name in enumerate(TERMS[:4 if three_d else 2]):
        out[name] = terms[:, i] * w[i]
    return out


def _single(batch_pred, batch_gt, loss_weight, three_d):
    mask = batch_gt["mask"]
    L, W = mask.shape[-2:]
    gt = {k: (v.reshape(1, 1, L, W) if k in ("mask", "heatmap") else v) for k, v in batch_gt.items()}
    targets = DetTargets.from_dense(gt, min(MAX_OBJECTS, L * W))
    pred = {k: v for k, v in batch_pred.items() if three_d or k in ("heatmap", "loc_offset")}
    out = detection_loss(pred, targets, gt["heatmap"], loss_weight)
    return out["loss"][0], {k: v.detach()[0] for k, v in out.items()}


def compute_loss3d(batch_pred, batch_gt, loss_weight=(1.0, 1.0, 1.0, 1.0)):
    """The reference's ``compute_loss3d`` for its batch of one (``loss.py:45-75``) on the dense dicts of the reference's encoder:
    ``DetTargets.from_dense`` + ``detection_loss``.  Returns ``(loss, loss_dict)``; ``loss_dict`` holds 0-dim device tensors where
    the reference calls ``.item()`` five times (the one difference)."""
    return _single(batch_pred, batch_gt, loss_weight, True)


def compute_loss2d(batch_pred, batch_gt, loss_weight=(1.0, 1.0)):
    """The reference's ``compute_loss2d`` (``loss.py:77-102``), as ``compute_loss3d``."""
    return _single(batch_pred, batch_gt, loss_weight, False)
