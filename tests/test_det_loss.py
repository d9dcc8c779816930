"""The sparse target encoder and the fused detection loss on the GPU (``TargetEncoder.encode`` on ``vfa_det_targets_f32``,
``detection_loss`` on ``vfa_det_loss_f32`` / ``vfa_det_loss_backward_f32``) against the reference's records
(tests/golden/det_loss_*.npz) and, for the synthetic cases, against the float64 restatement of tests/loss_common.py, which
tests/test_det_loss_cpu.py pins to those records.

THE BOUND of every loss term (relative) and every gradient (normwise, and max-abs over max-abs) is the error of the reference's own
float32 evaluation against the same float64 -- the fixture's record, or the float32 restatement on the CPU -- times 4 for the other
summation order and the device's expf / logf, never below 2^-23.  Every figure is printed before it is asserted.

Shapes are the smallest that reach each way the kernels can go: 12 x 20 (one dense workgroup), 37 x 53 (odd, two dense workgroups with
a ragged tail), k in {0, 1, 7, 65}, R in {360, 24}, B in {1, 3} with unequal counts and an empty frame, the three index conventions;
one full-size 156 x 156 3D and one 120 x 360 2D frame."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_common as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = ("heatmap", "loc_offset", "dim_offset", "rotation_at")


def _encoder(base, world, mean, R=360, K=128):
    from vfa_amd import TargetEncoder
    return TargetEncoder(base, world, (4, 4, 4), dimension_mean=mean, angle_range=R or 360, angle_radius=6, max_objects=K)


def _encode_case(case, L, W, R):
    enc = _encoder(case["base"], case["world"], case["mean"], R, case["K"])
    three_d = case["three_d"]
    return enc.encode(torch.from_numpy(case["location"]).to(DEV), torch.from_numpy(case["count"]).to(DEV),
                      torch.from_numpy(case["dimension"]).to(DEV) if three_d else None,
                      torch.from_numpy(case["rotation"]).to(DEV) if three_d else None, grid_lw=(L, W))


def _check_targets(targets, want, R=360):
    """Cells, counts, offsets and labels bit for bit the restatement's; dim_offset against the float64 log of the same float32
    quotient at 2 ulps (the device's logf); padding rows behind n_pos."""
    cells, n_pos = targets.cells.cpu().numpy(), targets.n_pos.cpu().numpy()
    loc = targets.loc_offset.cpu().numpy()
    for b, t in enumerate(want):
        n = len(t["cells"])
        assert n_pos[b] == n, (b, n_pos[b], n)
        assert np.array_equal(cells[b, :n], t["cells"]) and (cells[b, n:] == -1).all(), b
        assert np.array_equal(loc[b, :n].view(np.uint32), t["loc_offset"].view(np.uint32)) and not loc[b, n:].any(), b
        if "label" in t:
            assert np.array_equal(targets.angle_label[b, :n].cpu().numpy(), t["label"]) and not targets.angle_label[b, n:].any(), b
            dim = targets.dim_offset[b].cpu().numpy()
            exact = np.log(t["dim_quotient"].astype(np.float64))
            np.testing.assert_allclose(dim[:n], exact, rtol=2.0 ** -22, atol=1e-9, err_msg=f"dim_offset of frame {b}")
            assert not dim[n:].any()


def _restated_targets(want, K, R=0):
    """The restatement's targets as a ``DetTargets`` on the device: the loss comparisons give the kernels and the float64 restatement
    the SAME targets (the encoder's own output differs from them by the device's logf in dim_offset, checked in ``_check_targets``)."""
    from vfa_amd import DetTargets
    from vfa_amd.loss import label_table
    B, three_d = len(want), "label" in want[0]
    cells, n_pos = np.full((B, K), -1, np.int32), np.array([len(t["cells"]) for t in want], np.int32)
    loc, dim, label = np.zeros((B, K, 2), np.float32), np.zeros((B, K, 3), np.float32), np.zeros((B, K), np.int32)
    for b, t in enumerate(want):
        n = n_pos[b]
        cells[b, :n], loc[b, :n] = t["cells"], t["loc_offset"]
        if three_d:
            dim[b, :n], label[b, :n] = t["dim_offset"], t["label"]
    dev = [torch.from_numpy(v).to(DEV) for v in (cells, n_pos, loc, dim, label)]
    return DetTargets(dev[0], dev[1], dev[2], dev[3] if three_d else None, dev[4] if three_d else None,
                      label_table(R, 6).to(DEV) if three_d else None)


def _device_pred(pred):
    return {k: v.to(DEV).requires_grad_(True) for k, v in pred.items()}


def _run(pred, targets, gt_heatmap, weights):
    """detection_loss and the gradients of sum_b loss[b] -> ({name: (B,) float64}, {head: numpy})."""
    from vfa_amd import detection_loss
    leaves = _device_pred(pred)
    if "rotation_at" in leaves:
        leaves["rotation_cells"] = targets.cells
    out = detection_loss(leaves, targets, gt_heatmap.to(DEV), weights)
    out["loss"].sum().backward()
    vals = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}
    return vals, {k: leaves[k].grad.cpu().numpy() for k in HEADS if k in leaves}


def _check_against(vals, grads, want64, grads64, err32_vals, err32_grads, what):
    for k, v in vals.items():
        for b in range(len(v)):
            got, bound = lc.rel(v[b], want64[k][b]) if want64[k][b] != 0 else abs(v[b]), lc.bound(err32_vals[k][b])
            print(f"{what} frame {b} {k}: kernel {got:.3e}  float32 reference {err32_vals[k][b]:.3e}  bound {bound:.3e}")
            assert got <= bound, (what, k, b, got, bound)
    for k, g in grads.items():
        for measure in (lc.normwise, lc.maxabs):
            got, bound = measure(g, grads64[k]), lc.bound(err32_grads[k][measure.__name__])
            print(f"{what} grad {k} {measure.__name__}: kernel {got:.3e}  float32 reference {err32_grads[k][measure.__name__]:.3e}  "
                  f"bound {bound:.3e}")
            assert got <= bound, (what, k, measure.__name__, got, bound)


def _check_exact_zeros(pred, grads, want):
    """No gradient off the positive cells, behind n_pos, or at a saturated heat-map logit."""
    B, _, L, W = pred["heatmap"].shape
    for b, t in enumerate(want):
        off = np.ones(L * W, bool)
        off[t["cells"]] = False
        for k in ("loc_offset", "dim_offset"):
            if k in grads:
                assert not grads[k][b].reshape(L * W, -1)[off].any(), (k, b)
        if "rotation_at" in grads:
            assert not grads["rotation_at"][b, len(t["cells"]):].any(), b
    saturated = pred["heatmap"].abs().numpy() >= 15
    assert not grads["heatmap"][saturated].any()


# ---- 1. the fixtures ---------------------------------------------------------------------------------------------------------------

def _fixture_targets(d, three_d, K=16):
    from vfa_amd import TargetEncoder, pack_objects
    objs = [SimpleNamespace(location=d["obj_location"][i], **(dict(dimension=d["obj_dimension"][i], rotation=d["obj_rotation"][i])
                                                               if three_d else {})) for i in range(len(d["obj_location"]))]
    packed = pack_objects([objs], DEV, max_objects=K)
    enc = TargetEncoder(str(d["base"]), tuple(d["world_size"]), tuple(d["cube_LWH"]), dimension_mean=d["dimension_mean"],
                        angle_range=int(d["angle_range"]), angle_radius=float(d["angle_radius"]), max_objects=K)
    return enc.encode(packed.location, packed.count, packed.dimension, packed.rotation, grid_lw=tuple(int(v) for v in d["grid_lw"]))


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_fixture_through_encode(name):
    """pack_objects + TargetEncoder.encode give the reference encoder's records: the later object of the duplicate cell, the last row
    and column, negative angles and angles >= 180 degrees, the angles one float32 step around 90 degrees."""
    d, three_d = lc.load(name)
    _, want, _ = lc.fixture_case(d, three_d)
    targets = _fixture_targets(d, three_d)
    assert targets.cells.shape == (1, 16) and targets.cells.dtype == torch.int32 and (targets.dim_offset is not None) == three_d
    _check_targets(targets, want)
    cells = np.flatnonzero(d["gt_mask"].ravel() == 1)
    assert np.array_equal(targets.cells[0, :len(cells)].cpu().numpy(), cells)


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_fixture_through_detection_loss(name):
    """The kernels against the reference's float64 run, bounded by the reference's float32 run."""
    d, three_d = lc.load(name)
    pred, want, gt = lc.fixture_case(d, three_d)
    if three_d:
        pred["rotation_at"] = torch.cat([pred["rotation_at"], torch.zeros(1, 16 - pred["rotation_at"].shape[1], 360)], dim=1)
    vals, grads = _run(pred, _restated_targets(want, 16, 360), gt, d["loss_weight"].tolist())
    n = len(want[0]["cells"])
    want64 = {k: np.array([float(d["f64_" + k])]) for k in vals}
    err32 = {k: [lc.rel(float(d["f32_" + k]), float(d["f64_" + k]))] for k in vals}
    stored = {"rotation_at": "rotation_rows"}
    grads64, err32_grads = {}, {}
    for k, g in grads.items():
        g64, g32 = d["f64_grad_" + stored.get(k, k)], d["f32_grad_" + stored.get(k, k)]
        if k == "rotation_at":
            assert not g[0, n:].any()
            grads[k] = g = g[:, :n]
        grads64[k] = g64.reshape(g.shape)
        err32_grads[k] = {m.__name__: m(g32, g64) for m in (lc.normwise, lc.maxabs)}
    _check_against(vals, grads, want64, grads64, err32, err32_grads, name)
    _check_exact_zeros(pred, grads, want)


# ---- 2. synthetic cases against the float64 restatement ----------------------------------------------------------------------------

CASES = {
    "12x20_k7_R360": (11, 12, 20, (7,), 360, "MultiviewC"),
    "12x20_k1_R24": (12, 12, 20, (1,), 24, "MultiviewC"),
    "37x53_k65_B3_R24": (13, 37, 53, (65, 1, 0), 24, "MultiviewC"),
    "37x53_k7_B3_R360": (14, 37, 53, (3, 7, 5), 360, "MultiviewC"),
    "37x53_B3_wildtrack": (15, 37, 53, (5, 0, 9), 0, "Wildtrack"),
    "12x20_k1_multiviewx": (16, 12, 20, (1,), 0, "MultiviewX"),
    "156x156_k40_R360": (17, 156, 156, (40,), 360, "MultiviewC"),
    "120x360_k40_wildtrack": (18, 120, 360, (40,), 0, "Wildtrack"),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case and its float64 / float32 restatements on the CPU, computed once and shared."""
    seed, L, W, counts, R, base = CASES[name]
    case = lc.synthetic_case(seed, len(counts), L, W, counts, R, base)
    weights = [1.0, 0.7, 1.3, 0.9] if R else [1.0, 0.7]
    v64, g64 = lc.evaluate(case["pred"], case["targets"], case["gt_heatmap"], weights, torch.float64)
    v32, g32 = lc.evaluate(case["pred"], case["targets"], case["gt_heatmap"], weights, torch.float32)
    err_v = {k: [lc.rel(v32[k][b], v64[k][b]) if v64[k][b] != 0 else abs(v32[k][b]) for b in range(len(counts))] for k in v64}
    err_g = {k: {m.__name__: m(g32[k], g64[k]) for m in (lc.normwise, lc.maxabs)} for k in g64}
    return case, weights, v64, g64, err_v, err_g


@pytest.mark.parametrize("name", list(CASES))
def test_synthetic_case(name):
    _, L, W, counts, R, _ = CASES[name]
    case, weights, v64, g64, err_v, err_g = _reference(name)
    targets = _encode_case(case, L, W, R)
    _check_targets(targets, case["targets"], R)
    vals, grads = _run(case["pred"], _restated_targets(case["targets"], case["K"], R), case["gt_heatmap"], weights)
    assert sorted(vals) == sorted(v64) and all(v.shape == (len(counts),) for v in vals.values())
    _check_against(vals, grads, v64, g64, err_v, err_g, name)
    _check_exact_zeros(case["pred"], grads, case["targets"])
    for b, n in enumerate(counts):
        if n == 0:   # a frame without objects inside a batch: the sparse terms are 0, the heat map still counts
            assert vals["loss_pos"][b] == 0 and vals.get("loss_ang", np.zeros(len(counts)))[b] == 0 and vals["loss_heatmap"][b] > 0


def test_duplicate_cells_and_wildtrack_indexing():
    """Two objects of a cell: one positive, the later object's targets.  Wildtrack on a non-square map: the row is the x cell."""
    case = _reference("37x53_B3_wildtrack")[0]
    targets = _encode_case(case, 37, 53, 0)
    n = targets.n_pos.cpu().tolist()
    assert n == [len(t["cells"]) for t in case["targets"]] and n[0] < 5 and n[1] == 0 and n[2] < 9     # one duplicate in each frame
    loc = case["location"]
    for b in (0, 2):
        last = case["count"][b] - 1
        cell = int(loc[b, last, 0] / 4) * 53 + int(loc[b, last, 1] / 4)
        row = targets.cells[b].cpu().tolist().index(cell)
        assert np.abs(targets.loc_offset[b, row].cpu().numpy() - [0.25, 0.75]).max() < 1e-5               # the later object's
    # the same objects under the other convention: row and column change places (and what then leaves the 37 rows is dropped)
    swapped = _encode_case(dict(case, base="MultiviewX"), 37, 53, 0)
    for b in (0, 2):
        rc = [divmod(c, 53) for c in targets.cells[b, :n[b]].cpu().tolist()]
        want = sorted(c * 53 + r for r, c in rc if c < 37)
        assert swapped.cells[b, :int(swapped.n_pos[b])].cpu().tolist() == want and len(want) > 0


def test_no_positives_and_an_empty_list():
    """The heat-map target without a 1 (only the negative part counts) and k = 0 (cells of shape (B, 0))."""
    from vfa_amd import DetTargets, detection_loss
    case = lc.synthetic_case(21, 2, 12, 20, (0, 0), 24)
    gt = case["gt_heatmap"]
    assert not (gt == 1).any()
    v64, g64 = lc.evaluate(case["pred"], case["targets"], gt, [1.0] * 4, torch.float64)
    v32, g32 = lc.evaluate(case["pred"], case["targets"], gt, [1.0] * 4, torch.float32)
    targets = _encode_case(case, 12, 20, 24)
    assert targets.n_pos.cpu().tolist() == [0, 0] and (targets.cells == -1).all()
    vals, grads = _run(case["pred"], targets, gt, [1.0] * 4)
    for b in range(2):
        got, ref = lc.rel(vals["loss_heatmap"][b], v64["loss_heatmap"][b]), lc.rel(v32["loss_heatmap"][b], v64["loss_heatmap"][b])
        print(f"no positives, frame {b}: kernel {got:.3e}  float32 reference {ref:.3e}")
        assert got <= lc.bound(ref) and vals["loss"][b] == vals["loss_heatmap"][b]
        assert vals["loss_pos"][b] == vals["loss_hwl"][b] == vals["loss_ang"][b] == 0
    assert lc.normwise(grads["heatmap"], g64["heatmap"]) <= lc.bound(lc.normwise(g32["heatmap"], g64["heatmap"]))
    assert not grads["loc_offset"].any() and not grads["dim_offset"].any() and not grads["rotation_at"].any()
    empty = DetTargets(targets.cells[:, :0], targets.n_pos, targets.loc_offset[:, :0], targets.dim_offset[:, :0],
                       targets.angle_label[:, :0], targets.table)
    pred = _device_pred(case["pred"])
    pred["rotation_at"] = torch.zeros(2, 0, 24, device=DEV, requires_grad=True)
    out = detection_loss(pred, empty, gt.to(DEV))
    out["loss"].sum().backward()
    assert np.array_equal(out["loss"].detach().cpu().numpy().astype(np.float64), vals["loss"])
    assert np.array_equal(pred["heatmap"].grad.cpu().numpy(), grads["heatmap"]) and not pred["loc_offset"].grad.any()


# ---- 3. strides, reproducibility, isolation of the frames --------------------------------------------------------------------------

def _forward_backward(pred, targets, gt, weights):
    vals, grads = _run(pred, targets, gt, weights)
    return {**{"v_" + k: v for k, v in vals.items()}, **{"g_" + k: g for k, g in grads.items()}}


def test_permuted_views_give_the_bits_of_contiguous_heads():
    """VFANet returns permute(0, 2, 3, 1) views of NCHW storage: read through their strides, the same bits as contiguous NHWC."""
    from vfa_amd import detection_loss
    case, weights = _reference("37x53_k7_B3_R360")[:2]
    targets = _encode_case(case, 37, 53, 360)
    want = _forward_backward(case["pred"], targets, case["gt_heatmap"], weights)
    nchw = {k: case["pred"][k].permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True) for k in ("loc_offset", "dim_offset")}
    pred = {"heatmap": case["pred"]["heatmap"].to(DEV).requires_grad_(True), "rotation_at": case["pred"]["rotation_at"].to(DEV),
            **{k: v.permute(0, 2, 3, 1) for k, v in nchw.items()}}
    assert not pred["loc_offset"].is_contiguous() and pred["loc_offset"].data_ptr() == nchw["loc_offset"].data_ptr()
    out = detection_loss(pred, targets, case["gt_heatmap"].to(DEV)[:, None], weights)      # (the target as (B, 1, L, W))
    out["loss"].sum().backward()
    for k, v in out.items():
        assert np.array_equal(v.detach().cpu().numpy().astype(np.float64), want["v_" + k]), k
    for k, v in nchw.items():
        assert np.array_equal(v.grad.permute(0, 2, 3, 1).cpu().numpy(), want["g_" + k]), k


def test_two_runs_and_single_frames_give_identical_bits():
    case, weights = _reference("37x53_k65_B3_R24")[:2]
    targets = _encode_case(case, 37, 53, 24)
    first = _forward_backward(case["pred"], targets, case["gt_heatmap"], weights)
    second = _forward_backward(case["pred"], _encode_case(case, 37, 53, 24), case["gt_heatmap"], weights)
    for k in first:
        assert np.array_equal(first[k], second[k], equal_nan=True), k
    for b in range(3):   # frame b alone: the partition of a frame's work does not depend on B
        one = dict(case, location=case["location"][b:b + 1], dimension=case["dimension"][b:b + 1], rotation=case["rotation"][b:b + 1],
                   count=case["count"][b:b + 1])
        alone = _forward_backward({k: v[b:b + 1] for k, v in case["pred"].items()}, _encode_case(one, 37, 53, 24),
                                  case["gt_heatmap"][b:b + 1], weights)
        for k in first:
            assert np.array_equal(first[k][b:b + 1], alone[k]), (k, b)


def test_non_finite_logits_stay_inside_their_frame():
    case, weights = _reference("37x53_k7_B3_R360")[:2]
    targets = _encode_case(case, 37, 53, 360)
    clean = _forward_backward(case["pred"], targets, case["gt_heatmap"], weights)
    pred = {k: v.clone() for k, v in case["pred"].items()}
    pred["heatmap"][1, 0, 5, 5] = float("nan")
    pred["heatmap"][1, 0, 6, 6] = float("inf")
    pred["rotation_at"][1, 0, 3] = float("-inf")
    pred["loc_offset"].view(3, -1, 2)[1, int(case["targets"][1]["cells"][0]), 0] = float("nan")
    dirty = _forward_backward(pred, targets, case["gt_heatmap"], weights)
    torch.cuda.synchronize()
    assert np.isnan(dirty["v_loss"][1]) and np.isnan(dirty["v_loss_heatmap"][1]) and np.isnan(dirty["v_loss_pos"][1])
    assert np.isfinite(dirty["v_loss_ang"][1])                      # (an infinite logit saturates: the clamp holds it)
    for k in clean:
        for b in (0, 2):
            assert np.array_equal(clean[k][b], dirty[k][b]), (k, b)


# ---- 4. graph capture, the drop-in wrappers, end to end ----------------------------------------------------------------------------

def test_forward_captured_in_a_graph_and_replayed_on_new_inputs():
    """Encode + loss forward under no_grad in ``torch.cuda.graph``: replayed on other objects (other counts) and other heads it gives
    what the eager calls give."""
    from vfa_amd import detection_loss
    first = lc.synthetic_case(31, 2, 12, 20, (7, 2), 24)
    second = lc.synthetic_case(32, 2, 12, 20, (3, 6), 24)
    second = dict(second, **{k: np.concatenate([second[k], np.zeros_like(first[k])[:, second[k].shape[1]:]], axis=1)
                             for k in ("location", "dimension", "rotation")}, K=first["K"])
    second["pred"]["rotation_at"] = torch.cat([second["pred"]["rotation_at"], torch.zeros(2, first["K"] - 6, 24)], dim=1)
    enc = _encoder("MultiviewC", first["world"], first["mean"], 24, first["K"])
    enc.table(torch.device(DEV))

    def operands(case):
        return ([torch.from_numpy(case[k]).to(DEV) for k in ("location", "count", "dimension", "rotation")],
                {k: v.to(DEV) for k, v in case["pred"].items()}, case["gt_heatmap"].to(DEV))

    def step(objs, pred, gt):
        with torch.no_grad():
            targets = enc.encode(*objs, grid_lw=(12, 20))
            return detection_loss(pred, targets, gt), targets.n_pos

    eager = [step(*operands(case)) for case in (first, second)]
    objs, pred, gt = operands(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(objs, pred, gt)                                        # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, n_pos = step(objs, pred, gt)
    for case, (want, want_n) in zip((first, second), eager):
        new_objs, new_pred, new_gt = operands(case)
        for dst, src in zip(objs, new_objs):
            dst.copy_(src)
        for k in pred:
            pred[k].copy_(new_pred[k])
        gt.copy_(new_gt)
        graph.replay()
        assert torch.equal(n_pos, want_n)
        for k in want:
            assert torch.equal(out[k], want[k]), k
    assert eager[0][1].tolist() != eager[1][1].tolist()


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_drop_in_wrappers_equal_detection_loss(name):
    """compute_loss3d / compute_loss2d on the reference encoder's dense dicts (batch of one) = detection_loss on the same targets in the
    sparse form, bit for bit, values and gradients."""
    from vfa_amd import compute_loss2d, compute_loss3d
    d, three_d = lc.load(name)
    L, W = (int(v) for v in d["grid_lw"])
    pred, want, gt = lc.fixture_case(d, three_d)
    cells = want[0]["cells"].astype(np.int64)
    batch_gt = {"mask": torch.from_numpy(d["gt_mask"])[None, None].to(DEV), "heatmap": gt[None].to(DEV),
                "loc_offset": torch.from_numpy(d["gt_loc_offset"])[None].to(DEV)}
    batch_pred = {"heatmap": pred["heatmap"].to(DEV).requires_grad_(True), "loc_offset": pred["loc_offset"].to(DEV).requires_grad_(True)}
    if three_d:
        dense_gt, dense = torch.zeros(L * W, 360), torch.zeros(L * W, 360)
        dense_gt[cells], dense[cells] = torch.from_numpy(d["gt_rotation_rows"]), torch.from_numpy(d["rotation_rows"])
        batch_gt.update(dim_offset=torch.from_numpy(d["gt_dim_offset"])[None].to(DEV), rotation=dense_gt.reshape(1, L, W, 360).to(DEV))
        batch_pred.update(dim_offset=pred["dim_offset"].to(DEV).requires_grad_(True),
                          rotation=dense.reshape(1, L, W, 360).to(DEV).requires_grad_(True))
        pred["rotation_at"] = torch.cat([pred["rotation_at"], torch.zeros(1, 16 - len(cells), 360)], dim=1)
    weights = d["loss_weight"].tolist()
    loss, parts = (compute_loss3d if three_d else compute_loss2d)(batch_pred, batch_gt, weights)
    loss.backward()
    vals, grads = _run(pred, _restated_targets(want, 16, 360), gt, weights)   # (the dense dict's targets: torch's log, not the device's)
    assert loss.dim() == 0 and loss.is_cuda and sorted(parts) == sorted(vals)
    for k, v in parts.items():
        assert v.dim() == 0 and v.is_cuda and not v.requires_grad and float(v) == vals[k][0], k
    for k in ("heatmap", "loc_offset") + (("dim_offset",) if three_d else ()):
        assert np.array_equal(batch_pred[k].grad.cpu().numpy(), grads[k]), k
    if three_d:
        g = batch_pred["rotation"].grad.reshape(L * W, 360).cpu().numpy()
        assert np.array_equal(g[cells], grads["rotation_at"][0, :len(cells)]) and not np.delete(g, cells, axis=0).any()


def test_training_step_end_to_end():
    """Objects -> targets -> VFANet.forward(rotation_at=targets.cells) -> detection_loss -> backward, no value seen by the host in
    between: finite gradients on every trainable parameter."""
    import vfa_amd
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.vfanet import VFANet
    args = SimpleNamespace(data="MultiviewC", image_size=(192, 320))
    torch.manual_seed(0)
    net = VFANet(args, grid_height=96, cube_size=(50, 50, 32), angle_range=36).to(DEV).eval()
    images = torch.rand(3, 3, 192, 320, generator=torch.Generator().manual_seed(4)).to(DEV)
    calibs = ring_cameras(3, (600., 500., 0.), 1500., 500., 250., (320, 192)).to(DEV)
    grid = vfa_amd.make_grid((1000, 1200), cube_LW=(50, 50), dataset="MultiviewC").to(DEV)[None]
    L, W = grid.shape[1:3]
    rng = np.random.RandomState(3)
    objs = [SimpleNamespace(location=[rng.uniform(0, W * 1000.0 / L), rng.uniform(0, L * 1200.0 / W), 0.0],
                            dimension=[140.0 + i, 60.0, 230.0], rotation=rng.uniform(0, 6.0)) for i in range(6)]
    packed = vfa_amd.pack_objects([objs], DEV, max_objects=8)
    enc = vfa_amd.TargetEncoder("MultiviewC", (1000, 1200), (50, 50, 32), dimension_mean=[140.0, 60.0, 230.0], angle_range=36,
                                max_objects=8)
    targets = enc.encode(packed.location, packed.count, packed.dimension, packed.rotation, grid_lw=(L, W))
    spare = torch.where(targets.cells < 0, L * W, targets.cells).long()                      # (padding rows land behind the map)
    gt_heatmap = torch.zeros(1, L * W + 1, device=DEV).scatter_(1, spare, 1.0)[:, :L * W].reshape(1, L, W)
    pred = net(images, calibs, grid, rotation_at=targets.cells)
    out = vfa_amd.detection_loss(pred, targets, gt_heatmap)
    out["loss"].sum().backward()
    assert int(targets.n_pos[0]) >= 4 and torch.isfinite(out["loss"]).all()
    missing = [n for n, p in net.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert torch.isfinite(p.grad).all(), n
    assert any(p.grad.abs().max() > 0 for p in net.orient_pred.parameters())
