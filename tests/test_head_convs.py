"""The heads' dense 3x3 convolutions on the MI355X (``ops.conv3x3``, ``ops.conv3x3_few``, ``ops.group_norm_affine``,
``VFANet.heads(convs="hip")``) against the float64 ``F.conv2d`` / module chain of the same float32 inputs on the CPU, under the two
yardsticks of tests/conv_common.py: (E) elementwise with n = 27 C + 12 (dense) or 9 C + 4 (few outputs), (N) normwise within 4 x the
float32 library chain on the CPU.  Shapes are the smallest that can still go wrong: maps smaller than the dilation's halo, maps that
cross the 4 x 32 cell tile in both directions, ragged output tiles, NCHW / channels-last / sliced inputs, B = 2 with frames of
different scales.

Measured on the MI355X, the ratios of (N) (each test prints its own before it asserts): dense kernel 0.9-1.6 x at C = 32 and
2.3-2.4 x at C = 256 (5.1e-7 against the CPU's 2.2e-7) -- inside the 1.7-2.6 x of the numpy restatement, so the MFMA's rounding adds
nothing visible; epilogues 0.9 x; few-output kernel 1.6-1.9 x; GroupNorm's a, b 0.3-0.4 x and the normalised map 1.0 x; the model's
outputs on the (2, 256, 20, 28) map 2.1-2.4 x, the library path's own orient_pred on the new fused map included."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_common as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layout(x, layout):
    """The same values as NCHW, channels-last, or a non-contiguous slice of a larger tensor, on the device."""
    x = x.to(DEV)
    if layout == "nchw":
        return x.contiguous()
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    B, C, L, W = x.shape
    big = torch.full((B + 1, C + 8, L + 2, W + 3), 7.0, device=DEV)
    big[1:, 4:4 + C, 1:1 + L, 2:2 + W] = x
    view = big[1:, 4:4 + C, 1:1 + L, 2:2 + W]
    assert not view.is_contiguous() or view.numel() < 2
    return view


DENSE_CASES = {  # name: (C, O, L, W, dilation, layout)
    "halo_o1": (32, 1, 3, 5, 4, "nchw"),
    "small_o40_nhwc": (32, 40, 9, 11, 2, "nhwc"),
    "c256_o256_slice": (256, 256, 9, 11, 1, "slice"),
    "tiles_o360": (32, 360, 37, 70, 1, "nchw"),
    "c256_o40_d4_nhwc": (256, 40, 37, 70, 4, "nhwc"),
    "tiles_o256_d2_slice": (32, 256, 37, 70, 2, "slice"),
    "halo_c256_d2": (256, 40, 3, 5, 2, "nchw"),
}


@functools.lru_cache(maxsize=None)
def _dense(name):
    """Inputs, the three CPU references (computed once, never written to) and the kernel's output."""
    from vfa_amd import ops
    C, O, L, W, d, layout = DENSE_CASES[name]
    x, w = cc.inputs(2, C, O, L, W, seed=len(name) + C + O)
    with torch.no_grad():
        y = ops.conv3x3(_layout(x, layout), w.to(DEV), dilation=d)
    return x, w, d, cc.conv64(x, w, d), cc.conv32(x, w, d), y


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_kernel_against_float64(name):
    x, w, d, y64, y32, y = _dense(name)
    assert y.shape == y64.shape and y.dtype == torch.float32 and y.is_contiguous()
    cc.check_elementwise(y, x, w, d, cc.n_dense(x.shape[1]), name)
    cc.check_normwise(y, y64, y32, name)


def _bn(O, seed):
    gen = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(O).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(O, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(O, generator=gen) * 0.3)
        bn.running_mean.copy_(torch.randn(O, generator=gen) * 0.5)
        bn.running_var.copy_(torch.rand(O, generator=gen) * 2 + 0.1)
    return bn


def test_epilogue_scale_shift_relu_and_folded_batchnorm():
    from vfa_amd import ops
    C, O, L, W, d = 32, 40, 9, 37, 2
    x, w = cc.inputs(2, C, O, L, W, seed=11)
    gen = torch.Generator().manual_seed(12)
    bias, scale, shift = torch.randn(O, generator=gen), torch.randn(O, generator=gen), torch.randn(O, generator=gen)
    bn = _bn(O, 13)
    xd, wd = x.to(DEV), w.to(DEV)

    def chain(dtype, kind):
        y = F.conv2d(x.to(dtype), w.to(dtype), padding=d, dilation=d)
        if kind == "affine":
            return y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
        if kind == "bias_relu":
            return F.relu(y + bias.to(dtype).view(1, -1, 1, 1))
        return F.relu(copy.deepcopy(bn).to(dtype)(y + bias.to(dtype).view(1, -1, 1, 1)))
    with torch.no_grad():
        bn_d, bias_d = copy.deepcopy(bn).to(DEV), bias.to(DEV)
        folded = ops.bn_fold(bn_d.weight, bn_d.bias, bn_d.running_mean, bn_d.running_var, bn_d.eps, bias_d)
        got = {"affine": ops.conv3x3(xd, wd, d, scale=scale.to(DEV), shift=shift.to(DEV)),
               "bias_relu": ops.conv3x3(xd, wd, d, shift=bias.to(DEV), relu=True),
               "batchnorm": ops.conv3x3(xd, wd, d, scale=folded[0], shift=folded[1], relu=True)}
        for kind, y in got.items():
            cc.check_normwise(y, chain(torch.float64, kind), chain(torch.float32, kind), kind)
        assert float(got["bias_relu"].min()) == 0.0 and float(got["batchnorm"].min()) == 0.0 and float(got["affine"].min()) < 0
        # the folded vectors themselves, against float64
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        h64 = bn.bias.double() + (bias.double() - bn.running_mean.double()) * s64
    assert torch.allclose(folded[0].double().cpu(), s64, rtol=2 ** -23, atol=0) and torch.allclose(folded[1].double().cpu(), h64, rtol=0, atol=2 ** -22)
    assert ops.bn_fold(bn_d.weight, bn_d.bias, bn_d.running_mean, bn_d.running_var, bn_d.eps, bias_d)[0] is folded[0]   # kept ...
    bn_d.running_var.mul_(4.0)                                                                                          # ... by version
    refolded = ops.bn_fold(bn_d.weight, bn_d.bias, bn_d.running_mean, bn_d.running_var, bn_d.eps, bias_d)
    assert refolded[0] is not folded[0] and float((refolded[0] / folded[0]).max()) < 0.51


def _affine(B, C, seed, positive_shift=False):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(B, C, generator=gen) + 0.5
    b = torch.rand(B, C, generator=gen) + 0.25 if positive_shift else torch.randn(B, C, generator=gen)
    return a, b


@pytest.mark.parametrize("O,d,prologue", [(1, 4, None), (2, 1, None), (3, 1, "mixed"), (1, 4, "mixed"), (3, 4, "positive"), (2, 1, "positive")])
def test_few_output_kernel_against_float64(O, d, prologue):
    """``positive``: every b > 0 on a map with a border -- a padding applied BEFORE the activation would read relu(b) > 0 outside."""
    from vfa_amd import ops
    B, C, L, W = 2, 256, 9, 70
    x, w = cc.inputs(B, C, O, L, W, seed=20 + 3 * O + d)
    affine, xp64, xp32 = None, x, x
    if prologue:
        a, b = affine = _affine(B, C, 30 + O, positive_shift=prologue == "positive")
        xp64 = torch.relu(a.double()[:, :, None, None] * x.double() + b.double()[:, :, None, None])
        xp32 = torch.relu(a[:, :, None, None] * x + b[:, :, None, None])
    with torch.no_grad():
        y = ops.conv3x3_few(x.to(DEV), w.to(DEV), dilation=d, affine=None if affine is None else tuple(t.to(DEV) for t in affine))
        y_nhwc = ops.conv3x3_few(_layout(x, "nhwc"), w.to(DEV), dilation=d, affine=None if affine is None else tuple(t.to(DEV) for t in affine))
    assert y.shape == (B, O, L, W) and y.is_contiguous() and torch.equal(_bits(y), _bits(y_nhwc))
    cc.check_elementwise(y, xp64, w, d, cc.n_few(C), f"few O={O} d={d} {prologue}")
    cc.check_normwise(y, cc.conv64(xp64, w, d), cc.conv32(xp32, w, d), f"few O={O} d={d} {prologue}")
    if prologue == "positive":      # padding first reads relu(b) > 0 outside the map: far outside the yardstick, which sees it
        padded = F.pad(x.double(), (d, d, d, d))
        padded_first = F.conv2d(torch.relu(a.double()[:, :, None, None] * padded + b.double()[:, :, None, None]), w.double(), dilation=d)
        assert padded_first.shape == y.shape and cc.normwise(padded_first, cc.conv64(xp64, w, d)) > 1e-2


def test_group_norm_affine_against_float64():
    from vfa_amd import ops
    B, C, L, W, G = 2, 256, 9, 37, 16
    gen = torch.Generator().manual_seed(40)
    x = torch.randn(B, C, L, W, generator=gen)
    x[1] = x[1] * 3.0 + 1.5                                  # two frames with different statistics
    x = x * (1 + torch.arange(C).view(1, C, 1, 1) % 5) + torch.arange(C).view(1, C, 1, 1) % 3
    gamma_, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    eps = 1e-5
    with torch.no_grad():
        a, b = ops.group_norm_affine(_layout(x, "slice"), G, gamma_.to(DEV), beta.to(DEV), eps)
        a2, b2 = ops.group_norm_affine(x.to(DEV), G, gamma_.to(DEV), beta.to(DEV), eps)
        alone = ops.group_norm_affine(x[1:].to(DEV), G, gamma_.to(DEV), beta.to(DEV), eps)
    assert a.shape == (B, C) and b.shape == (B, C) and torch.equal(_bits(a), _bits(a2)) and torch.equal(_bits(b), _bits(b2))
    assert torch.equal(_bits(alone[0][0]), _bits(a[1])) and torch.equal(_bits(alone[1][0]), _bits(b[1]))   # per frame

    def affine_of(dtype):
        xg = x.to(dtype).view(B, G, -1)
        mean, var = xg.mean(2), xg.var(2, unbiased=False)
        rstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(C // G, 1)
        aa = gamma_.to(dtype)[None] * rstd
        return aa, beta.to(dtype)[None] - mean.repeat_interleave(C // G, 1) * aa
    a64, b64 = affine_of(torch.float64)
    a32, b32 = affine_of(torch.float32)
    assert float((a64[0] - a64[1]).abs().min()) > 0.01 * float(a64.abs().max())     # the frames' statistics do differ
    cc.check_normwise(a, a64, a32, "group norm a")
    cc.check_normwise(b, b64, b32, "group norm b")
    y = torch.relu(a.cpu()[:, :, None, None] * x + b.cpu()[:, :, None, None])
    want64 = F.relu(F.group_norm(x.double(), G, gamma_.double(), beta.double(), eps))
    want32 = F.relu(F.group_norm(x, G, gamma_, beta, eps))
    cc.check_normwise(y, want64, want32, "normalised, activated map")


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def _head_chain(x, w, w_few, gn, d=1):
    """One head as the model runs it: the dense kernel, the statistics, the few-output kernel with the prologue."""
    from vfa_amd import ops
    y = ops.conv3x3(x, w, dilation=d, shift=gn[1])
    affine = ops.group_norm_affine(y, 16, gn[0], gn[1], 1e-5)
    return y, affine[0], affine[1], ops.conv3x3_few(y, w_few, dilation=d, affine=affine)


@functools.lru_cache(maxsize=None)
def _chain_inputs():
    x, w = cc.inputs(2, 32, 160, 9, 37, seed=50)
    gen = torch.Generator().manual_seed(51)
    w_few = torch.randn(3, 160, 3, 3, generator=gen) / 38.0
    gn = (torch.rand(160, generator=gen) + 0.5, torch.randn(160, generator=gen) * 0.3)
    return x.to(DEV), w.to(DEV), w_few.to(DEV), tuple(t.to(DEV) for t in gn)


def test_same_bits_on_every_run_alone_and_in_a_batch_and_in_every_layout():
    x, w, w_few, gn = _chain_inputs()
    with torch.no_grad():
        first = _head_chain(x, w, w_few, gn)
        again = _head_chain(x, w, w_few, gn)
        nhwc = _head_chain(_layout(x, "nhwc"), w, w_few, gn)
        sliced = _head_chain(_layout(x, "slice"), w, w_few, gn)
        alone = [_head_chain(x[b:b + 1], w, w_few, gn) for b in range(2)]
    for i, (a, b, c, e) in enumerate(zip(first, again, nhwc, sliced)):
        assert torch.equal(_bits(a), _bits(b)), f"two runs, output {i}"
        assert torch.equal(_bits(a), _bits(c)), f"channels-last, output {i}"
        assert torch.equal(_bits(a), _bits(e)), f"slice, output {i}"
        for f in range(2):
            assert torch.equal(_bits(a[f:f + 1]), _bits(alone[f][i])), f"frame {f} alone, output {i}"
    assert float(first[0].abs().max()) > 0 and float(first[3].abs().max()) > 0


def test_all_zero_input_gives_zeros():
    from vfa_amd import ops
    _, w, w_few, _ = _chain_inputs()
    zero = torch.zeros(2, 32, 9, 37, device=DEV)
    with torch.no_grad():
        y = ops.conv3x3(zero, w, dilation=2)
        z = ops.conv3x3_few(torch.zeros(2, 160, 9, 37, device=DEV), w_few, dilation=4)
    assert y.shape == (2, 160, 9, 37) and not y.any() and not z.any()
    mixed = torch.zeros(2, 32, 9, 37, device=DEV)
    mixed[1] = _chain_inputs()[0][1]
    with torch.no_grad():
        ym = ops.conv3x3(mixed, w, dilation=2)
    assert not ym[0].any() and ym[1].any()


def test_graph_replay_equals_the_eager_call():
    x, w, w_few, gn = _chain_inputs()
    static = x.clone()
    with torch.no_grad():
        eager_first = _head_chain(x, w, w_few, gn)
        second = x.flip(3) * 1.5
        eager_second = _head_chain(second, w, w_few, gn)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            _head_chain(static, w, w_few, gn)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        captured = _head_chain(static, w, w_few, gn)
    graph.replay()
    for a, b in zip(captured, eager_first):
        assert torch.equal(_bits(a), _bits(b))
    static.copy_(second)
    graph.replay()
    for a, b in zip(captured, eager_second):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(_bits(eager_first[3]), _bits(eager_second[3]))


def test_one_nan_reaches_exactly_its_receptive_field():
    from vfa_amd import ops
    C, O, L, W, d = 32, 40, 9, 70, 2
    x, w = cc.inputs(2, C, O, L, W, seed=60)
    fy, fx = 4, 31                                            # next to a tile edge in x: the NaN is in two tiles' windows
    poisoned = x.clone()
    poisoned[1, 5, fy, fx] = float("nan")
    with torch.no_grad():
        y = ops.conv3x3(poisoned.to(DEV), w.to(DEV), dilation=d).cpu()
        z = ops.conv3x3_few(poisoned.to(DEV), w[:3].to(DEV), dilation=d).cpu()
    want = torch.zeros(2, 1, L, W, dtype=torch.bool)
    for dy in (-d, 0, d):
        for dx in (-d, 0, d):
            if 0 <= fy + dy < L and 0 <= fx + dx < W:
                want[1, 0, fy + dy, fx + dx] = True
    assert int(want.sum()) == 9
    assert torch.equal(torch.isnan(y), want.expand_as(y)) and torch.equal(torch.isnan(z), want.expand_as(z))
    keep = (~want).double()
    y64, y32 = cc.conv64(x, w, d) * keep, cc.conv32(x, w, d) * keep.float()
    cc.check_normwise(torch.where(want.expand_as(y), torch.zeros_like(y), y), y64, y32, "the other cells")


def test_wrappers_are_inference_only_on_the_device():
    from vfa_amd import ops
    x, w, w_few, gn = _chain_inputs()
    wg = w.clone().requires_grad_()
    with pytest.raises(ValueError, match="inference only"):
        ops.conv3x3(x, wg)
    with pytest.raises(ValueError, match="inference only"):
        ops.conv3x3_few(x.clone().requires_grad_(), w[:2])
    with torch.no_grad():
        assert torch.equal(ops.conv3x3(x, wg), ops.conv3x3(x, w))
    with pytest.raises(ValueError):
        ops.conv3x3(x, w, dilation=5)
    with pytest.raises(ValueError):
        ops.conv3x3_few(x, w)          # 160 outputs


# ---- the model -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_and_topdown(mode):
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(5 if mode == "3D" else 6)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode=mode).eval()
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for bn in (net.fuse[1], net.fuse[4]):                 # perturbed running statistics and affine parameters
            bn.running_mean.copy_(torch.randn(256, generator=gen) * 0.2)
            bn.running_var.copy_(torch.rand(256, generator=gen) * 1.5 + 0.25)
            bn.weight.copy_(torch.rand(256, generator=gen) + 0.5)
            bn.bias.copy_(torch.randn(256, generator=gen) * 0.2)
    topdown = torch.randn(2, 256, 20, 28, generator=gen)
    topdown[1] *= 2.5
    with torch.no_grad():
        want64 = copy.deepcopy(net).double().heads(topdown.double())
        want32 = net.heads(topdown)
    return net.to(DEV), topdown.to(DEV), want64, want32


@pytest.mark.parametrize("mode", ["2D", "3D"])
def test_model_heads_against_the_float64_modules(mode):
    net, topdown, want64, want32 = _net_and_topdown(mode)
    with torch.no_grad():
        library = net.heads(topdown)
        got = net.heads(topdown, convs="hip")
        net.head_convs = "hip"
        try:
            by_attribute = net.heads(topdown)
        finally:
            net.head_convs = "library"
    assert sorted(got) == sorted(library) == sorted(want64) == (["dim_offset", "heatmap", "loc_offset", "rotation"] if mode == "3D" else ["heatmap", "loc_offset"])
    for k in got:
        assert got[k].shape == library[k].shape and got[k].dtype == library[k].dtype and got[k].device == library[k].device, k
        if k != "rotation":                                   # (the dense orient_pred stays the library's: two calls of it may differ)
            assert torch.equal(_bits(got[k]), _bits(by_attribute[k])), k
        cc.check_normwise(got[k], want64[k], want32[k], f"{mode} {k}")


def test_model_heads_keys_for_each_rotation_at_form():
    net, topdown, _, _ = _net_and_topdown("3D")
    cells = torch.tensor([[0, 5, 559, -1], [17, 17, 300, 400]], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for rotation_at in (None, "detections", cells):
            library, got = net.heads(topdown, rotation_at), net.heads(topdown, rotation_at, convs="hip")
            assert sorted(got) == sorted(library)
            for k in got:
                if k == "rotation_head":
                    assert got[k][0].shape == library[k][0].shape and got[k][1] is library[k][1] and got[k][2] == library[k][2]
                elif k == "rotation_cells":
                    assert got[k] is cells
                else:
                    assert got[k].shape == library[k].shape and got[k].dtype == library[k].dtype, k
        # the cell kernel reads the hip path's fused map through its strides: the same logits as from the "detections" form
        from vfa_amd import ops
        fused, weight, dilation = net.heads(topdown, "detections", convs="hip")["rotation_head"]
        at = net.heads(topdown, cells, convs="hip")["rotation_at"]
        assert torch.equal(_bits(at), _bits(ops.conv3x3_at_cells_forward(fused, weight, cells, dilation)[0]))
    with pytest.raises(ValueError, match="convs"):
        net.heads(topdown, convs="rocm")


def test_model_in_training_mode_or_with_gradients_runs_the_library_path():
    net, topdown, _, _ = _net_and_topdown("3D")
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)   # (two calls of the library's convolutions: the same bits only so)
    try:
        net.heads(topdown)
        library = net.heads(topdown)
        with_grad = net.heads(topdown, convs="hip")
        assert with_grad["heatmap"].requires_grad
        for k in library:
            assert torch.equal(_bits(with_grad[k].detach()), _bits(library[k].detach())), k
        state = copy.deepcopy(net.state_dict())
        net.train()
        try:
            with torch.no_grad():
                net.load_state_dict(state)
                library = net.heads(topdown)
                net.load_state_dict(state)                    # (training mode moves the running statistics)
                training = net.heads(topdown, convs="hip")
        finally:
            net.load_state_dict(state)
            net.eval()
        for k in library:
            assert torch.equal(_bits(training[k]), _bits(library[k])), k
    finally:
        torch.use_deterministic_algorithms(was)


def _decoder():
    from vfa_amd import eval_ops
    return eval_ops.BEVDecoder("MultiviewC", (80, 112), (4, 4, 4), dimension_mean=np.array([140, 60, 230], np.float32), topk=50)


def test_decode_accepts_the_hip_heads_and_the_graph_replay_is_bit_equal():
    """What ``detect`` runs behind the fused map -- the heads with ``rotation_at="detections"`` on the new kernels, then
    ``decode_fused`` -- eager, captured, and replayed on a second map."""
    net, topdown, _, _ = _net_and_topdown("3D")
    dec = _decoder()
    net.head_convs = "hip"
    try:
        def run(x):
            return dec.decode_fused(net.heads(x, rotation_at="detections"), thresh)
        with torch.no_grad():
            thresh = float(torch.sigmoid(net.heads(topdown)["heatmap"]).median())
            second = topdown.flip(3) * 1.5
            eager_first, eager_second = run(topdown), run(second)
        static = topdown.clone()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                run(static)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            captured = run(static)
        graph.replay()
        for k in eager_first:
            assert torch.equal(captured[k], eager_first[k]), k
        static.copy_(second)
        graph.replay()
        for k in eager_second:
            assert torch.equal(captured[k], eager_second[k]), k
        assert int(captured["count"].min()) > 0 and not torch.equal(eager_first["cell"], eager_second["cell"])
    finally:
        net.head_convs = "library"


def test_detect_runs_with_hip_head_convs():
    """``VFANet.detect`` from camera frames to detections with ``head_convs = "hip"``: the keys and shapes of the library path's, the
    same detections' cells where the two heat maps agree on the order (not asserted: printed), and the same bits on a second call."""
    import vfa_amd
    from vfa_amd import eval_ops, ops
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.vfanet import VFANet
    args = SimpleNamespace(data="MultiviewC", image_size=(192, 320), resize_size=(192, 320))
    torch.manual_seed(0)
    net = VFANet(args, grid_height=96, cube_size=(50, 50, 32), angle_range=36).to(DEV).eval()
    calibs = ring_cameras(2, (600., 500., 0.), 1500., 500., 250., (320, 192)).to(DEV)
    grid = vfa_amd.make_grid((1000, 1200), cube_LW=(50, 50), dataset="MultiviewC").to(DEV)[None]
    images = torch.rand(2, 3, 192, 320, generator=torch.Generator().manual_seed(1)).to(DEV)
    dec = eval_ops.BEVDecoder("MultiviewC", (1000, 1200), (50, 50, 32), dimension_mean=np.array([140, 60, 230], np.float32), topk=20)
    library = net.detect(images, calibs, grid, dec, 0.0)
    net.head_convs = "hip"
    with ops.KernelTimer() as kt:
        found = net.detect(images, calibs, grid, dec, 0.0)
    again = net.detect(images, calibs, grid, dec, 0.0)
    torch.cuda.synchronize()
    assert {"vfa_conv3x3_f32", "vfa_conv3x3_few_f32", "vfa_group_norm_affine_f32"} <= set(kt.summary())
    assert kt.summary()["vfa_conv3x3_f32"]["launches"] == 4 and kt.summary()["vfa_conv3x3_few_f32"]["launches"] == 3
    assert set(found) == set(library) and all(found[k].shape == library[k].shape and found[k].dtype == library[k].dtype for k in found)
    assert int(found["count"].min()) > 0
    print("cells equal to the library path's:", float((found["cell"] == library["cell"]).float().mean()))
    with torch.no_grad():
        stable = torch.equal(_bits(net.ortho_features(images, calibs, grid)), _bits(net.ortho_features(images, calibs, grid)))
    if stable:
        for k in found:                                       # (the fused map in front of the heads is the same: so is everything behind it)
            assert torch.equal(found[k], again[k]), k


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (the dynamic-LDS attribute is per device)")
def test_a_second_device_runs_the_dense_kernels_after_the_first():
    """The kernels need 65-108 KB of dynamic LDS, which is allowed per kernel AND per device: a process that has run them on device 0
    runs them on device 1 -- the forward (d = 4, the largest window) and ``conv3x3_train`` forward and backward (the weight
    gradient's kernel has its own allowance) -- with the bits of device 0."""
    from vfa_amd import ops
    x, w = cc.inputs(2, 32, 40, 9, 11, seed=31)
    xt, wt = cc.inputs(2, 32, 32, 9, 11, seed=32)

    def run(dev):
        with torch.cuda.device(dev):
            with torch.no_grad():
                y = ops.conv3x3(x.to(dev), w.to(dev), dilation=4)
            xd, wd = xt.to(dev).requires_grad_(), wt.to(dev).requires_grad_()
            yt = ops.conv3x3_train(xd, wd, dilation=2)
            yt.backward(torch.ones_like(yt))
            torch.cuda.synchronize(dev)
            return [t.detach().cpu() for t in (y, yt, xd.grad, wd.grad)]
    first, second = run(torch.device("cuda:0")), run(torch.device("cuda:1"))
    assert float(first[0].abs().max()) > 0 and float(first[3].abs().max()) > 0
    for name, a, b in zip(("conv3x3", "conv3x3_train", "input gradient", "weight gradient"), first, second):
        assert torch.equal(_bits(a), _bits(b)), name
