"""The convolution at listed cells on the GPU (``ops.conv3x3_at_cells`` on ``vfa_conv3x3_at_cells_f32`` and its backward,
``VFANet.heads(..., rotation_at=...)``, ``BEVDecoder.decode_fused`` with ``rotation_head``).

The truth for logits and gradients is the dense ``F.conv2d`` in float64 on the same float32 inputs, gathered at the cells.  The
tolerance is derived: a sum of n float32 products in any order, fused or not, differs from the exact sum by at most
gamma_n * sum |a_i b_i| with gamma_n = n u / (1 - n u), u = 2^-24; sum |a_i b_i| is the same float64 reference on the absolute values.
n = 9 C for a logit, the number of valid rows for d_weight, O * (the largest number of (row, tap) pairs on one location, counted
from the cell list here) for d_feat.  A wrong tap, border or stride misses that by orders of magnitude.  The rotation is compared
with today's decode on the kernel's own logits bit for bit, with no margin."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def _case(name):
    """-> dict(B, C, L, W, O, d, cells (B, k) int32, channels_last)"""
    if name == "low_grid":        # a grid lower than 2 d + 1: row taps fall outside almost everywhere; corners, centre, one -1
        L, W = 7, 9
        corners = [0, W - 1, (L - 1) * W, L * W - 1]
        cells = [corners + [3 * W + 4, -1], [-1, 3 * W + 4] + corners[::-1]]
        return dict(B=2, C=32, L=L, W=W, O=5, d=4, cells=cells, channels_last=False)
    if name == "shared_taps":     # k no multiple of any tile; cells 4 apart in a row, a column, a diagonal; a duplicate; ids outside
        L, W, d = 12, 13, 4
        c = 5 * W + 6
        named = [c, c + d, c + d * W, c + d * W + d, L * W, c, -7]
        rng = np.random.default_rng(5)
        rest = [int(v) for v in rng.permutation(L * W) if int(v) not in named][:37 - len(named)]
        cells = named[:4] + rest[:10] + named[4:] + rest[10:]
        assert len(cells) == 37
        return dict(B=1, C=64, L=L, W=W, O=360, d=d, cells=[cells], channels_last=False)
    d = {"channels_last_d1": 1, "channels_last_d2": 2}[name]   # feat channels-last, read through its strides; one frame all -1
    rng = np.random.default_rng(7)
    cells = [[0, 9, 90, 99] + [int(v) for v in rng.integers(0, 100, 7)], [-1] * 11, [55, 55 + d, 55 + 10 * d, 44, -1, 100, 5, 95, 50, 59, 55]]
    return dict(B=3, C=256, L=10, W=10, O=65, d=d, cells=cells, channels_last=True)


CASES = ("low_grid", "shared_taps", "channels_last_d1", "channels_last_d2")


def _gather(dense, cells):
    """dense (B, O, L, W) -> (B, k, O), zeros for the cells outside the map"""
    B, O, L, W = dense.shape
    flat = dense.reshape(B, O, L * W)
    out = torch.zeros(B, cells.shape[1], O, dtype=dense.dtype)
    for b in range(B):
        for j, cell in enumerate(cells[b].tolist()):
            if 0 <= cell < L * W:
                out[b, j] = flat[b, :, cell]
    return out


def _max_pairs_per_location(cells, L, W, d):
    most = 0
    for frame in cells.tolist():
        seen = {}
        for cell in frame:
            if not 0 <= cell < L * W:
                continue
            for t in range(9):
                y, x = cell // W + (t // 3 - 1) * d, cell % W + (t % 3 - 1) * d
                if 0 <= y < L and 0 <= x < W:
                    seen[(y, x)] = seen.get((y, x), 0) + 1
        most = max(most, max(seen.values(), default=0))
    return most


@functools.lru_cache(maxsize=None)
def _problem(name):
    """The inputs (CPU, float32), the float64 truth and the bounds of a case, computed once and never changed."""
    c = _case(name)
    B, C, L, W, O, d = (c[k] for k in "BCLWOd")
    g = torch.Generator().manual_seed(CASES.index(name) + 11)
    feat = torch.randn(B, C, L, W, generator=g)
    weight = torch.randn(O, C, 3, 3, generator=g) * 0.1
    cells = torch.tensor(c["cells"], dtype=torch.int32)
    grad = torch.randn(B, cells.shape[1], O, generator=g)
    valid = (cells >= 0) & (cells < L * W)

    def truth(f64, w64, g64):
        f64, w64 = f64.clone().requires_grad_(), w64.clone().requires_grad_()
        logits = _gather(F.conv2d(f64, w64, padding=d, dilation=d), cells)
        (logits * g64 * valid[..., None]).sum().backward()
        return logits.detach(), f64.grad, w64.grad
    logits, d_feat, d_weight = truth(feat.double(), weight.double(), grad.double())
    a_logits, a_feat, a_weight = truth(feat.double().abs(), weight.double().abs(), grad.double().abs())
    pairs = _max_pairs_per_location(cells, L, W, d)
    return dict(c, feat=feat, weight=weight, cells=cells, grad=grad, valid=valid, logits=logits, d_feat=d_feat, d_weight=d_weight,
                bound_logits=gamma(9 * C) * a_logits, bound_feat=gamma(O * pairs) * a_feat, bound_weight=gamma(int(valid.sum())) * a_weight,
                touched=a_feat != 0, pairs=pairs)


def _device_feat(p, requires_grad=False):
    feat = p["feat"].to(DEV)
    if p["channels_last"]:
        feat = feat.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # (B, C, L, W) view of NHWC storage
        assert feat.stride(1) == 1 and not feat.is_contiguous()
    return feat.detach().requires_grad_(requires_grad)


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error {float(err.max()):.3e}, largest error / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: error / bound up to {worst:.3g}"


# ---- 1. forward --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_logits_against_the_dense_convolution(name):
    from vfa_amd import ops
    p = _problem(name)
    feat, weight, cells = _device_feat(p), p["weight"].to(DEV), p["cells"].to(DEV)
    with torch.no_grad():
        logits = ops.conv3x3_at_cells(feat, weight, cells, dilation=p["d"])
        with_rot, rotation = ops.conv3x3_at_cells(feat, weight, cells, dilation=p["d"], want_rotation=True)
        again = ops.conv3x3_at_cells(feat, weight, cells, dilation=p["d"])
    k = cells.shape[1]
    assert logits.shape == (p["B"], k, p["O"]) and logits.dtype == torch.float32 and rotation.shape == (p["B"], k)
    _within(logits, p["logits"], p["bound_logits"], f"{name} logits")
    skipped = ~p["valid"].to(DEV)
    assert int(skipped.sum()) >= 1 and not logits[skipped].any() and not rotation[skipped].any()
    assert torch.equal(logits.view(torch.int32), with_rot.view(torch.int32)), "the logits know whether the rotation is wanted"
    assert torch.equal(logits.view(torch.int32), again.view(torch.int32)), "two runs differ"
    if p["channels_last"]:      # the same bits from NCHW storage: only the addresses differ
        with torch.no_grad():
            nchw = ops.conv3x3_at_cells(p["feat"].to(DEV), weight, cells, dilation=p["d"])
        assert torch.equal(nchw.view(torch.int32), logits.view(torch.int32))


def test_only_the_rotation_gives_the_rotation_of_both():
    from vfa_amd import ops
    p = _problem("shared_taps")
    feat, weight, cells = _device_feat(p), p["weight"].to(DEV), p["cells"].to(DEV)
    _, both = ops.conv3x3_at_cells_forward(feat, weight, cells, p["d"], want_logits=True, want_rotation=True)
    none, alone = ops.conv3x3_at_cells_forward(feat, weight, cells, p["d"], want_logits=False, want_rotation=True)
    assert none is None and torch.equal(both.view(torch.int32), alone.view(torch.int32))
    empty = ops.conv3x3_at_cells(feat, weight, cells[:, :0], dilation=p["d"])
    assert empty.shape == (1, 0, 360)


# ---- 2. the rotation rule, bit for bit against today's decode ----------------------------------------------------------------------

LATTICE_L, LATTICE_W = 12, 13
LATTICE = [l * LATTICE_W + w for l in (1, 4, 7, 10) for w in (1, 4, 7, 10)]   # 3 apart: each its own 5 x 5 maximum; no tap (d = 4) of
                                                                              # one cell lies on another


def _decode_rotation_of(logits, cells):
    """Today's ``decode_fused`` on a dense (1, L, W, O) map that holds `logits` at `cells` and -30 elsewhere, with a heat map whose
    peaks are those cells -> its rotation, in the order of `cells`."""
    from vfa_amd import eval_ops
    L, W, O = LATTICE_L, LATTICE_W, logits.shape[-1]
    g = torch.Generator().manual_seed(3)
    dense = torch.full((1, L * W, O), -30.0, device=DEV)
    dense[0, cells.long()] = logits
    heat = torch.full((1, 1, L * W), -20.0, device=DEV)
    heat[0, 0, cells.long()] = 3.0 - 0.1 * torch.arange(len(cells), device=DEV, dtype=torch.float32)
    pred = {"heatmap": heat.reshape(1, 1, L, W), "loc_offset": torch.randn(1, L, W, 2, generator=g).to(DEV),
            "dim_offset": (torch.randn(1, L, W, 3, generator=g) * 0.3).to(DEV), "rotation": dense.reshape(1, L, W, O)}
    dec = eval_ops.BEVDecoder("MultiviewC", (L * 4, W * 4), (4, 4, 4), dimension_mean=np.array([140, 60, 230], np.float32), topk=100)
    out = dec.decode_fused(pred, 0.4)
    assert int(out["count"][0]) == len(cells) and out["cell"][0, :len(cells)].tolist() == cells.tolist()   # by descending heat
    return out["rotation"][0, :len(cells)]


def test_rotation_rule_unsaturated():
    from vfa_amd import ops
    g = torch.Generator().manual_seed(41)
    feat = torch.randn(1, 64, LATTICE_L, LATTICE_W, generator=g)
    weight = torch.randn(360, 64, 3, 3, generator=g) * 0.05
    truth = F.conv2d(feat.double(), weight.double(), padding=4, dilation=4)
    assert float(truth.abs().max()) < 8.0, "the float64 logits must stay inside (-8, 8)"
    cells = torch.tensor([LATTICE + [-1]], dtype=torch.int32, device=DEV)
    logits, rotation = ops.conv3x3_at_cells(feat.to(DEV), weight.to(DEV), cells, dilation=4, want_rotation=True)
    want = _decode_rotation_of(logits[0, :-1], cells[0, :-1])
    assert torch.equal(rotation[0, :-1].view(torch.int32), want.view(torch.int32))
    assert float(rotation[0, -1]) == 0.0 and len(set(rotation[0, :-1].tolist())) > 8


def test_rotation_rule_saturated_by_construction():
    """feat is 1 at each cell's centre tap (on 64 - i channels for cell i) and the weights are small integers there, so the logits
    are exact integers; four angles hold 64 - i >= 49, where the sigmoid is 1.0f: the first of them wins."""
    from vfa_amd import ops
    g = torch.Generator().manual_seed(42)
    L, W = LATTICE_L, LATTICE_W
    feat = torch.zeros(1, 64, L * W)
    for i, cell in enumerate(LATTICE):
        feat[0, :64 - i, cell] = 1.0
    weight = torch.randint(-1, 2, (360, 64, 3, 3), generator=g).float()
    weight[:, 8:, 1, 1] = 0.0                            # every other angle stays inside [-8, 8]: no sigmoid of theirs rounds to 1.0f
    weight[[250, 100, 17, 359], :, 1, 1] = 1.0
    cells = torch.tensor([LATTICE], dtype=torch.int32, device=DEV)
    logits, rotation = ops.conv3x3_at_cells(feat.reshape(1, 64, L, W).to(DEV), weight.to(DEV), cells, dilation=4, want_rotation=True)
    want_logits = torch.stack([weight[:, :64 - i, 1, 1].sum(1) for i in range(len(LATTICE))])
    assert torch.equal(logits[0].cpu(), want_logits), "the logits are exact integers"
    assert int((logits[0] >= 40).sum(1).min()) >= 4 and float(want_logits[:, [250, 100, 17, 359]].min()) == 49.0
    want = _decode_rotation_of(logits[0], cells[0])
    assert torch.equal(rotation[0].view(torch.int32), want.view(torch.int32))
    assert np.array_equal(rotation[0].cpu().numpy(), np.full(16, np.float32(17) * np.float32(np.pi / 180), np.float32))


# ---- 3. backward -------------------------------------------------------------------------------------------------------------------

def _backward(p, grad=None):
    from vfa_amd import ops
    feat, weight = _device_feat(p, requires_grad=True), p["weight"].to(DEV).requires_grad_()
    logits = ops.conv3x3_at_cells(feat, weight, p["cells"].to(DEV), dilation=p["d"])
    logits.backward((p["grad"] if grad is None else grad).to(DEV))
    return feat.grad, weight.grad


@pytest.mark.parametrize("name", CASES)
def test_gradients_against_the_dense_convolution(name):
    p = _problem(name)
    d_feat, d_weight = _backward(p)
    assert d_feat.shape == p["feat"].shape and d_weight.shape == p["weight"].shape
    print(f"{name}: up to {p['pairs']} pairs on one location, {int(p['valid'].sum())} valid rows")
    _within(d_weight, p["d_weight"], p["bound_weight"], f"{name} d_weight")
    _within(d_feat, p["d_feat"], p["bound_feat"], f"{name} d_feat")
    assert not d_feat.cpu()[~p["touched"]].any(), "d_feat is not exactly zero where no tap lies"
    assert int((~p["touched"]).sum()) > 0 and (name != "shared_taps" or p["pairs"] >= 2)
    # skipped rows contribute nothing, whatever their gradient holds
    poisoned = p["grad"].clone()
    poisoned[~p["valid"]] = float("nan")
    d_feat2, d_weight2 = _backward(p, poisoned)
    assert torch.equal(d_feat2.view(torch.int32), d_feat.view(torch.int32)) and torch.equal(d_weight2.view(torch.int32), d_weight.view(torch.int32))


def test_gradients_are_the_same_bits_on_every_run():
    p = _problem("shared_taps")
    first, second = _backward(p), _backward(p)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 4. VFANet.heads ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_and_topdown():
    from types import SimpleNamespace
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(5)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").to(DEV).eval()
    topdown = torch.randn(2, 256, 24, 24, generator=torch.Generator().manual_seed(6)).to(DEV)
    rng = np.random.default_rng(8)
    cells = torch.tensor([[0, 23, 300, 304, 396, 575, -1] + [int(v) for v in rng.integers(0, 576, 5)],
                          [100, 100, 104, 196, -1, 576] + [int(v) for v in rng.integers(0, 576, 6)]], dtype=torch.int32, device=DEV)
    return net, topdown, cells


@contextlib.contextmanager
def _torch_deterministic():
    """The other heads are torch's own convolutions: two calls of them give the same bits only under torch's deterministic switch
    (the library's non-deterministic solvers add partial sums with atomics), and after a first call that has settled the solver."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


def _abs_fuse_backward(net, topdown, at_fused):
    """|J|^T applied to `at_fused` in float64 on the CPU, J the Jacobian of ``net.fuse`` (eval mode) at `topdown`: the convolutions with
    the absolute weights, the batch-norm scales' magnitudes, the ReLU masks of the real forward."""
    fuse = copy.deepcopy(net.fuse).double().cpu()
    conv1, bn1, conv2, bn2 = fuse[0], fuse[1], fuse[3], fuse[4]
    x = topdown.double().cpu()
    s1, s2 = ((bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach() for bn in (bn1, bn2))
    with torch.no_grad():
        y = bn1(conv1(x))
        mask1 = (y > 0).double()
        mask2 = (bn2(conv2(F.relu(y))) > 0).double()
    probe = torch.zeros_like(x, requires_grad=True)
    h = F.conv2d(probe, conv1.weight.detach().abs(), padding=1) * s1.abs().view(1, -1, 1, 1) * mask1
    h = F.conv2d(h, conv2.weight.detach().abs(), padding=2, dilation=2) * s2.abs().view(1, -1, 1, 1) * mask2
    (h * at_fused).sum().backward()
    return probe.grad.detach()


def test_heads_with_rotation_at_cells():
    net, topdown, cells = _net_and_topdown()
    conv = net.orient_pred[0]
    B, _, L, W = topdown.shape
    R = conv.out_channels
    G = torch.randn(B, cells.shape[1], R, generator=torch.Generator().manual_seed(9)).to(DEV)
    valid = ((cells >= 0) & (cells < L * W))
    safe = torch.where(valid, cells, torch.zeros_like(cells)).long()

    def route(sparse):
        x = topdown.clone().requires_grad_()
        net.zero_grad()
        pred = net.heads(x, rotation_at=cells if sparse else None)
        if sparse:
            at = pred["rotation_at"]
        else:
            at = torch.gather(pred["rotation"].reshape(B, L * W, R), 1, safe[..., None].expand(-1, -1, R)) * valid[..., None]
        (at * G * valid[..., None]).sum().backward()
        return pred, at.detach(), x.grad.clone(), conv.weight.grad.clone()
    with _torch_deterministic():
        route(False)
        dense, at_dense, dx_dense, dw_dense = route(False)
        sparse, at_sparse, dx_sparse, dw_sparse = route(True)
        with torch.no_grad():                # the float32 fused map both routes convolved, the same bits
            fused = net.heads(topdown, rotation_at="detections")["rotation_head"][0]
    assert "rotation" not in sparse and sorted(sparse) == ["dim_offset", "heatmap", "loc_offset", "rotation_at", "rotation_cells"]
    assert sparse["rotation_cells"] is cells and at_sparse.shape == (B, cells.shape[1], R)
    for k in ("heatmap", "loc_offset", "dim_offset"):
        assert torch.equal(sparse[k].view(torch.int32), dense[k].view(torch.int32)), k

    # the truth from that fused map, in float64 on the CPU
    cells_c, valid_c, G64 = cells.cpu(), valid.cpu(), G.double().cpu()

    def truth(f64, w64, g64):
        f64, w64 = f64.clone().requires_grad_(), w64.clone().requires_grad_()
        at = _gather(F.conv2d(f64, w64, padding=4, dilation=4), cells_c)
        (at * g64 * valid_c[..., None]).sum().backward()
        return at.detach(), f64.grad, w64.grad
    f64, w64 = fused.double().cpu(), conv.weight.detach().double().cpu()
    at64, dfused64, dw64 = truth(f64, w64, G64)
    a_at, a_dfused, a_dw = truth(f64.abs(), w64.abs(), G64.abs())
    n_dense = B * L * W                      # the longest chain a dense weight gradient can sum, zeros included
    pairs = _max_pairs_per_location(cells_c, L, W, 4)
    _within(at_sparse, at64, gamma(9 * 256) * a_at, "heads rotation_at")
    print("dense route at the cells, error / bound:", float(((at_dense.double().cpu() - at64).abs() / (gamma(9 * 256) * a_at).clamp_min(1e-300)).max()))
    _within(dw_sparse, dw64, gamma(int(valid_c.sum())) * a_dw, "heads d orient_pred.weight")
    _within(dw_sparse - dw_dense, torch.zeros_like(dw64), (gamma(int(valid_c.sum())) + gamma(n_dense)) * a_dw, "d weight, sparse - dense")
    # d topdown: both routes push their d fused through the same fuse backward (two 3x3 convolutions over 256 channels, two scales) in
    # float32.  Their d fused differ by at most e = (gamma(O pairs) + gamma(9 O)) |.| (the dense input gradient sums 9 taps x O), which
    # |J|^T carries to the input; each route's own rounding of J^T is at most gamma(m) |J|^T |d fused| with m = 2 * (9 * 256 + 2).
    e = (gamma(R * pairs) + gamma(9 * R)) * a_dfused
    m = 2 * (9 * 256 + 2)
    bound = _abs_fuse_backward(net, topdown, e) + 2 * gamma(m) * _abs_fuse_backward(net, topdown, dfused64.abs())
    _within(dx_sparse - dx_dense, torch.zeros_like(bound), bound, "d topdown, sparse - dense")
    assert float(dx_sparse.abs().max()) > 0 and float((dx_sparse - dx_dense).abs().max()) < 1e-3 * float(dx_dense.abs().max())


# ---- 5. decode_fused with the head in place of its map -----------------------------------------------------------------------------

def _decoder():
    from vfa_amd import eval_ops
    return eval_ops.BEVDecoder("MultiviewC", (96, 96), (4, 4, 4), dimension_mean=np.array([140, 60, 230], np.float32), topk=100)


def test_decode_fused_with_rotation_head():
    from vfa_amd import ops
    net, topdown, _ = _net_and_topdown()
    dec = _decoder()
    with torch.no_grad(), _torch_deterministic():
        net.heads(topdown)
        dense = net.heads(topdown)
        lazy = net.heads(topdown, rotation_at="detections")
        thresh = float(torch.sigmoid(dense["heatmap"]).median())           # half of the cells are candidates, whatever the init
        want, got = dec.decode_fused(dense, thresh), dec.decode_fused(lazy, thresh)
    assert sorted(got) == sorted(want) and int(got["count"].min()) > 0
    for k in ("count", "conf", "cell", "location", "dimension"):
        assert torch.equal(got[k], want[k]), k
    # the rotation is the new kernel's at the selected cells (its rule against the decode's: section 2)
    fused, weight, dilation = lazy["rotation_head"]
    _, rotation = ops.conv3x3_at_cells_forward(fused, weight, got["cell"], dilation, want_rotation=True)
    assert got["rotation"].shape == want["rotation"].shape and torch.equal(got["rotation"], rotation)
    behind = torch.arange(got["cell"].shape[1], device=DEV)[None, :] >= got["count"][:, None]
    assert not got["rotation"][behind].any()
    print("rotations equal to the dense route's:", float((got["rotation"] == want["rotation"]).float().mean()))


def test_decode_fused_with_rotation_head_is_captured_and_replayed_on_new_inputs():
    net, topdown, _ = _net_and_topdown()
    dec = _decoder()
    with torch.no_grad():
        first_in = net.heads(topdown, rotation_at="detections")
        second_in = net.heads(topdown.flip(3) * 1.5, rotation_at="detections")
        thresh = float(torch.sigmoid(first_in["heatmap"]).median())

    def tensors(pred):
        return [pred["heatmap"], pred["loc_offset"], pred["dim_offset"], pred["rotation_head"][0]]
    static = dict(first_in)
    static.update(heatmap=first_in["heatmap"].clone(), loc_offset=first_in["loc_offset"].clone(), dim_offset=first_in["dim_offset"].clone(),
                  rotation_head=(first_in["rotation_head"][0].clone(),) + tuple(first_in["rotation_head"][1:]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            dec.decode_fused(static, thresh)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        captured = dec.decode_fused(static, thresh)
    graph.replay()
    with torch.no_grad():
        eager = dec.decode_fused(first_in, thresh)
    for k in eager:
        assert torch.equal(captured[k], eager[k]), k
    first_cells = captured["cell"].clone()
    for dst, src in zip(tensors(static), tensors(second_in)):
        dst.copy_(src)
    graph.replay()
    with torch.no_grad():
        eager = dec.decode_fused(second_in, thresh)
    for k in eager:
        assert torch.equal(captured[k], eager[k]), k
    assert int(captured["count"].min()) > 0 and not torch.equal(captured["cell"], first_cells)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from types import SimpleNamespace
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    from vfa_amd.vfanet import VFANet
    cells = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(VFAHipError, match="10002"):                        # VFA_ERR_UNSUPPORTED
        ops.conv3x3_at_cells(torch.zeros(1, 48, 6, 6, device=DEV), torch.zeros(5, 48, 3, 3, device=DEV), cells, dilation=4)
    with pytest.raises(VFAHipError):
        ops.conv3x3_at_cells(torch.zeros(1, 32, 6, 6), torch.zeros(5, 32, 3, 3), cells.cpu(), dilation=4)
    with pytest.raises(ValueError, match="weight"):
        ops.conv3x3_at_cells(torch.zeros(1, 32, 6, 6, device=DEV), torch.zeros(5, 64, 3, 3, device=DEV), cells)
    with pytest.raises(ValueError, match="cells"):
        ops.conv3x3_at_cells(torch.zeros(1, 32, 6, 6, device=DEV), torch.zeros(5, 32, 3, 3, device=DEV), cells.long())
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="2D").to(DEV).eval()
    with pytest.raises(ValueError, match="3D"):
        net.heads(torch.zeros(1, 256, 8, 8, device=DEV), rotation_at=cells)
