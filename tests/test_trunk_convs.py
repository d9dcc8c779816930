"""The trunk's residual stages on the MI355X (``ops.trunk_conv``, ``ops.residual_join``, ``_Block.forward_hip``,
``VFANet.trunk_convs = "hip"``) against the float64 ``F.conv2d`` / module chain of the same float32 inputs on the CPU, under the two
yardsticks of tests/trunk_common.py: (E) elementwise with n = 27 C + 12 (nine taps) or 3 C + 12 (one tap) on the float32 prologue
result, (N) normwise within 4 x the float32 library chain on the CPU.  Shapes are the smallest that can still go wrong: a 1 x 1 map,
odd sizes at stride 2, outputs that cross the 4 x 32 cell tile in both directions, ragged output tiles, C = 512 (two accumulator
chains), NCHW / channels-last / sliced inputs, B = 2 with images of different scales.  Every test prints its ratios before it asserts.

Measured on the MI355X, the ratios of (N): nine taps 0.95-1.26 x without a prologue at C = 32 / 64, 1.5-2.3 x with one at C = 64 / 128,
2.13-2.17 x at C = 512 (two accumulator chains); one tap 0.67-1.42 x; (E) at most 1.2 % of its bound; blocks 1.27 / 1.43 / 1.80 x; the
model's f8 / f16 / f32 1.29 / 1.59 / 1.68 x (resnet18) and 1.33 / 1.63 / 1.77 x (resnet34)."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_common as cc
import trunk_common as tc

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


@contextlib.contextmanager
def _deterministic_library():
    """The stem stays the library's: two calls of its convolution give the same bits only under the deterministic setting."""
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn_only)


def _dev(affine):
    return None if affine is None else tuple(t.to(DEV) for t in affine)


CONV_CASES = {  # name: (C, O, L, W, kernel, stride, layout, prologue, non-negative input)
    "one_cell_s2": (32, 1, 1, 1, 3, 2, "nchw", None, False),
    "odd_9x11_s2": (32, 40, 9, 11, 3, 2, "nchw", None, False),
    "tiles_10x70_s2_nhwc": (64, 128, 10, 70, 3, 2, "nhwc", None, False),
    "c128_o130_7x66_s2_slice_prologue": (128, 130, 7, 66, 3, 2, "slice", "mixed", False),
    "c64_9x37_s1_prologue": (64, 64, 9, 37, 3, 1, "nchw", "mixed", False),
    "c512_o160_s1": (512, 160, 6, 7, 3, 1, "nchw", None, True),
    "c512_o160_s2": (512, 160, 6, 7, 3, 2, "nchw", None, True),
    "k1_c64_o128_9x11_s2": (64, 128, 9, 11, 1, 2, "nchw", None, False),
    "k1_c256_o512_4x70_s2": (256, 512, 4, 70, 1, 2, "nchw", None, False),
    "k1_c64_o64_5x33_s1": (64, 64, 5, 33, 1, 1, "nchw", None, False),
}


@functools.lru_cache(maxsize=None)
def _conv(name):
    """Inputs (never written to) and the kernel's output."""
    from vfa_amd import ops
    C, O, L, W, k, stride, layout, prologue, nonneg = CONV_CASES[name]
    x, w = tc.inputs(2, C, O, L, W, seed=len(name) + C + O, k=k, nonneg=nonneg)
    affine = tc.affine_of(2, C, seed=C + O) if prologue else None
    with torch.no_grad():
        y = ops.trunk_conv(_layout(x, layout), w.to(DEV), stride, affine=_dev(affine))
    return x, w, stride, affine, y


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_trunk_conv_against_float64(name):
    x, w, stride, affine, y = _conv(name)
    B, C, L, W = x.shape
    assert y.shape == (B, w.shape[0], tc.out_size(L, stride), tc.out_size(W, stride)) and y.dtype == torch.float32 and y.is_contiguous()
    if affine is not None:
        assert float((affine[0][:, :, None, None] * x + affine[1][:, :, None, None]).min()) < 0 < float(affine[1].max())   # mixed signs
    tc.check_both(y, x, w, stride, affine, name)


@pytest.mark.parametrize("stride", [1, 2])
def test_padding_is_applied_after_the_prologue(stride):
    """Every b > 0 on a map with a border: a padding applied BEFORE the activation would read relu(b) > 0 outside the map."""
    from vfa_amd import ops
    B, C, O, L, W = 2, 64, 40, 9, 37
    x, w = tc.inputs(B, C, O, L, W, seed=70 + stride)
    a, b = affine = tc.affine_of(B, C, seed=71, positive_shift=True)
    assert float(b.min()) > 0
    with torch.no_grad():
        y = ops.trunk_conv(x.to(DEV), w.to(DEV), stride, affine=_dev(affine))
    tc.check_both(y, x, w, stride, affine, f"positive shift, stride {stride}")
    padded = F.pad(x.double(), (1, 1, 1, 1))
    padded_first = F.conv2d(torch.relu(a.double()[:, :, None, None] * padded + b.double()[:, :, None, None]), w.double(), stride=stride)
    want = tc.conv(tc.prologue(x, affine, torch.float64), w, stride, torch.float64)
    assert padded_first.shape == y.shape and cc.normwise(padded_first, want) > 1e-2      # far outside the yardstick, which sees it
    border = torch.zeros_like(want, dtype=torch.bool)
    border[:, :, 0, :] = border[:, :, :, 0] = True
    assert float((y.double().cpu() - want)[border].abs().max()) < 1e-3 * float((padded_first - want)[border].abs().max())


# ---- the join ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("projected", [False, True])
def test_residual_join_is_bit_exact_in_place_and_out_of_place(projected):
    from vfa_amd import ops
    B, C, L, W = 2, 48, 7, 37                                        # 259 positions: no multiple of the block's 1024, of 256 or of 4
    gen = torch.Generator().manual_seed(80 + projected)
    y, r = torch.randn(B, C, L, W, generator=gen) * 3, torch.randn(B, C, L, W, generator=gen)
    y[1, 5, 3, 11] = float("nan")
    affine = (torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen))
    r_affine = (torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen)) if projected else None
    want = tc.emulate_join(y, affine, r, r_affine)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 1 and bool(nan[1, 5, 3, 11]) and float(want[~nan].min()) == 0.0 and float(want[~nan].max()) > 0
    yd, rd = y.to(DEV), r.to(DEV)
    with torch.no_grad():
        out = ops.residual_join(yd, _dev(affine), rd, _dev(r_affine))
        assert out.data_ptr() != yd.data_ptr() and torch.equal(yd.cpu().nan_to_num(7.0), y.nan_to_num(7.0))     # y is left alone
        in_place = ops.residual_join(yd, _dev(affine), rd, _dev(r_affine), out=yd)
    assert in_place is yd
    for got in (out, in_place):
        got = got.cpu()
        assert torch.equal(torch.isnan(got), nan)                   # the NaN reaches its own element and no other
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    big = torch.randn(1, 3, 40, 70, generator=gen)                   # 2800 positions: three blocks of a plane, the last one ragged
    ab = (torch.randn(1, 3, generator=gen), torch.randn(1, 3, generator=gen))
    with torch.no_grad():
        got = ops.residual_join(big.to(DEV), _dev(ab), big.flip(3).contiguous().to(DEV))
    assert torch.equal(_bits(got).cpu(), _bits(tc.emulate_join(big, ab, big.flip(3).contiguous())))


# ---- bits ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,stride,prologue", [(3, 2, True), (3, 1, False), (1, 2, False)])
def test_same_bits_on_every_run_alone_and_in_a_batch_and_in_every_layout(k, stride, prologue):
    from vfa_amd import ops
    x, w = tc.inputs(2, 64, 130, 9, 37, seed=90 + k + stride, k=k)
    x[1] *= 100.0
    affine = _dev(tc.affine_of(2, 64, seed=91)) if prologue else None
    wd = w.to(DEV)
    with torch.no_grad():
        first = ops.trunk_conv(x.to(DEV), wd, stride, affine)
        again = ops.trunk_conv(x.to(DEV), wd, stride, affine)
        nhwc = ops.trunk_conv(_layout(x, "nhwc"), wd, stride, affine)
        sliced = ops.trunk_conv(_layout(x, "slice"), wd, stride, affine)
        alone = [ops.trunk_conv(x[b:b + 1].to(DEV), wd, stride, None if affine is None else tuple(t[b:b + 1] for t in affine)) for b in range(2)]
    assert float(first.abs().max()) > 0
    assert torch.equal(_bits(first), _bits(again)) and torch.equal(_bits(first), _bits(nhwc)) and torch.equal(_bits(first), _bits(sliced))
    for b in range(2):
        assert torch.equal(_bits(first[b:b + 1]), _bits(alone[b])), f"image {b} alone"


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_the_trunk_and_the_heads_give_the_same_bits_where_they_are_the_same_convolution(layout):
    """Three by three, stride 1, dilation 1, no prologue and no epilogue operands: one kernel with two epilogues."""
    from vfa_amd import ops
    x, w = cc.inputs(2, 64, 130, 9, 37, seed=93)
    with torch.no_grad():
        trunk = ops.trunk_conv(_layout(x, layout), w.to(DEV), 1)
        heads = ops.conv3x3(_layout(x, layout), w.to(DEV), 1)
    assert float(trunk.abs().max()) > 0 and trunk.shape == heads.shape
    assert torch.equal(_bits(trunk), _bits(heads))


def test_all_zero_input_gives_zeros():
    from vfa_amd import ops
    x, w = tc.inputs(2, 64, 130, 9, 37, seed=95)
    mixed = x.clone()
    mixed[0] = 0.0
    with torch.no_grad():
        for stride in (1, 2):
            y = ops.trunk_conv(torch.zeros(2, 64, 9, 37, device=DEV), w.to(DEV), stride)
            ym = ops.trunk_conv(mixed.to(DEV), w.to(DEV), stride)
            assert y.shape == (2, 130, tc.out_size(9, stride), tc.out_size(37, stride)) and not y.any()
            assert not ym[0].any() and ym[1].any()


@pytest.mark.parametrize("k", [3, 1])
def test_one_nan_reaches_exactly_its_receptive_field_at_stride_two(k):
    from vfa_amd import ops
    C, O, L, W, stride = 32, 40, 9, 70, 2
    x, w = tc.inputs(2, C, O, L, W, seed=60 + k, k=k)
    fy, fx = (4, 63) if k == 3 else (4, 64)                          # 3 x 3: outputs 31 and 32 of a row, on both sides of a tile edge
    poisoned = x.clone()
    poisoned[1, 5, fy, fx] = float("nan")
    affine = tc.affine_of(2, C, seed=61)
    with torch.no_grad():
        y = ops.trunk_conv(poisoned.to(DEV), w.to(DEV), stride, affine=_dev(affine)).cpu()
    Lo, Wo = tc.out_size(L, stride), tc.out_size(W, stride)
    want = torch.zeros(2, 1, Lo, Wo, dtype=torch.bool)
    pad = k // 2
    for oy in range(Lo):
        for ox in range(Wo):
            if abs(stride * oy - fy) <= pad and abs(stride * ox - fx) <= pad:
                want[1, 0, oy, ox] = True
    assert int(want.sum()) == (2 if k == 3 else 1)
    assert torch.equal(torch.isnan(y), want.expand_as(y))
    if k == 1:                                                       # a NaN at a position the strided 1 x 1 never reads changes nothing
        unread = x.clone()
        unread[1, 5, 3, 63] = float("nan")
        with torch.no_grad():
            clean = ops.trunk_conv(x.to(DEV), w.to(DEV), stride, affine=_dev(affine))
            assert torch.equal(_bits(ops.trunk_conv(unread.to(DEV), w.to(DEV), stride, affine=_dev(affine))), _bits(clean))
    keep = (~want).double()
    y64 = tc.conv(tc.prologue(x, affine, torch.float64), w, stride, torch.float64) * keep
    y32 = tc.conv(tc.prologue(x, affine, torch.float32), w, stride, torch.float32) * keep.float()
    cc.check_normwise(torch.where(want.expand_as(y), torch.zeros_like(y), y), y64, y32, "the other cells")


def test_packed_weights_are_kept_by_identity_and_version():
    from vfa_amd import ops
    x, w = tc.inputs(1, 32, 8, 5, 6, seed=99)
    wd = w.to(DEV)
    with torch.no_grad():
        first = ops.trunk_conv(x.to(DEV), wd)
        packed = ops.trunk_packed_weight(wd)[0]
        assert ops.trunk_packed_weight(wd)[0] is packed
        wd.mul_(2.0)
        assert ops.trunk_packed_weight(wd)[0] is not packed
        assert torch.equal(_bits(ops.trunk_conv(x.to(DEV), wd)), _bits(first * 2.0))      # a power of two: the same split
    with pytest.raises(ValueError, match="inference only"):
        ops.trunk_conv(x.to(DEV), wd.clone().requires_grad_())
    with pytest.raises(ValueError):
        ops.trunk_conv(x.to(DEV), wd, stride=3)
    with pytest.raises(ValueError):
        ops.trunk_conv(x.to(DEV), torch.zeros(8, 32, 5, 5, device=DEV))


# ---- blocks and the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout,stride", [(64, 64, 1), (64, 128, 2), (256, 512, 2)])
def test_block_against_the_float64_module(cin, cout, stride):
    from vfa_amd.vfanet import _Block
    torch.manual_seed(cin + cout)
    block = tc.randomise_group_norms(_Block(cin, cout, stride), cin).eval()
    x = torch.randn(2, cin, 12, 40, generator=torch.Generator().manual_seed(cout)).abs()      # an activated map, as a block reads
    x[1] *= 3.5
    with torch.no_grad():
        want32 = block(x.clone())
        want64 = tc.module64(block, x)
        got = block.to(DEV).forward_hip(x.to(DEV))
        again = block.forward_hip(x.to(DEV))
        alone = block.forward_hip(x[1:].to(DEV))
    assert got.shape == want64.shape and got.is_contiguous() and float(got.min()) == 0.0
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got[1:]), _bits(alone))
    cc.check_normwise(got, want64, want32, f"block {cin} -> {cout}, stride {stride}")


@functools.lru_cache(maxsize=None)
def _net_and_images(base):
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(len(base))
    net = tc.randomise_group_norms(VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base=base, mode="2D"), 3).eval()
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    x[1] *= 1.7
    with torch.no_grad():
        want32 = net.base(x)
    want64 = tc.module64(net.base, x)
    return net.to(DEV), x.to(DEV), want64, want32


@pytest.mark.parametrize("base", ["resnet18", "resnet34"])
def test_model_trunk_against_the_float64_trunk(base):
    from vfa_amd import ops
    net, x, want64, want32 = _net_and_images(base)
    net.trunk_convs = "hip"
    try:
        with torch.no_grad(), _deterministic_library(), ops.KernelTimer() as kt:
            got = net.trunk(x)
        with torch.no_grad(), _deterministic_library():
            again = net.trunk(x)
            kept = len(ops._CONV_KEPT)
            net.trunk(x)
            assert len(ops._CONV_KEPT) == kept                       # nothing is packed on a later frame
    finally:
        net.trunk_convs = "library"
    torch.cuda.synchronize()
    blocks = sum(len(getattr(net.base, f"layer{i}")) for i in (1, 2, 3, 4))
    assert kt.summary()["vfa_trunk_conv_f32"]["launches"] == 2 * blocks + 3 and kt.summary()["vfa_residual_join_f32"]["launches"] == blocks
    assert blocks == (8 if base == "resnet18" else 16)
    for name, y, y2, y64, y32 in zip(("f8", "f16", "f32"), got, again, want64, want32):
        assert y.shape == y64.shape and y.dtype == torch.float32 and y.is_contiguous() and y.device == x.device
        assert torch.equal(_bits(y), _bits(y2))
        cc.check_normwise(y, y64, y32, f"{base} {name}")


def test_model_in_training_mode_or_with_gradients_runs_the_library_trunk():
    net, x, _, _ = _net_and_images("resnet18")
    net.trunk_convs = "hip"
    try:
        with _deterministic_library():
            net.base(x)
            library = [t.detach() for t in net.base(x)]
            with_grad = net.trunk(x)
            assert with_grad[0].requires_grad
            for a, b in zip(with_grad, library):
                assert torch.equal(_bits(a.detach()), _bits(b))
            net.train()
            try:
                with torch.no_grad():
                    training = net.trunk(x)
            finally:
                net.eval()
            for a, b in zip(training, library):
                assert torch.equal(_bits(a), _bits(b))
            with torch.no_grad():
                assert not torch.equal(_bits(net.trunk(x)[2]), _bits(library[2]))     # ... and the setting does choose another path in eval mode
    finally:
        net.trunk_convs = "library"


def test_graph_replay_of_the_trunk_equals_the_eager_call():
    from vfa_amd import ops
    net, x, _, _ = _net_and_images("resnet18")
    net.trunk_convs = "hip"
    try:
        stack = contextlib.ExitStack()
        stack.enter_context(_deterministic_library())
        second = x.flip(3) * 1.5
        with torch.no_grad():
            eager_first, eager_second = net.trunk(x), net.trunk(second)
        static = x.clone()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                net.trunk(static)
        torch.cuda.current_stream(DEV).wait_stream(side)
        kept = len(ops._CONV_KEPT)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            captured = net.trunk(static)
        assert len(ops._CONV_KEPT) == kept
        graph.replay()
        for a, b in zip(captured, eager_first):
            assert torch.equal(_bits(a), _bits(b))
        static.copy_(second)
        graph.replay()
        for a, b in zip(captured, eager_second):
            assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(eager_first[2]), _bits(eager_second[2]))
    finally:
        stack.close()
        net.trunk_convs = "library"


def test_lateral_integrals_and_detect_run_with_hip_trunk_and_head_convs():
    """``VFANet.detect`` from camera frames to detections with both settings on "hip": the keys and shapes of the library path's, the
    trunk's and the heads' kernels in the frame, the same bits on a second call."""
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
    stack = contextlib.ExitStack()
    stack.enter_context(_deterministic_library())
    library = net.detect(images, calibs, grid, dec, 0.0)
    with torch.no_grad():
        integrals_library = net.lateral_integrals(images)
    net.trunk_convs = net.head_convs = "hip"
    with torch.no_grad():
        integrals = net.lateral_integrals(images)
        integrals_again = net.lateral_integrals(images)
    with ops.KernelTimer() as kt:
        found = net.detect(images, calibs, grid, dec, 0.0)
    again = net.detect(images, calibs, grid, dec, 0.0)
    torch.cuda.synchronize()
    assert {"vfa_trunk_conv_f32", "vfa_residual_join_f32", "vfa_conv3x3_f32", "vfa_group_norm_affine_f32"} <= set(kt.summary())
    assert kt.summary()["vfa_trunk_conv_f32"]["launches"] == 19 and kt.summary()["vfa_residual_join_f32"]["launches"] == 8
    assert len(integrals) == len(integrals_library) == 3
    for a, b, c in zip(integrals, integrals_again, integrals_library):
        assert a.shape == c.shape and a.dtype == c.dtype and torch.equal(_bits(a), _bits(b))
        print("integral image, hip trunk against the library trunk:", cc.normwise(a, c.double().cpu()))
        assert cc.normwise(a, c.double().cpu()) < 1e-4               # the same function: float32 summation orders apart, not a different map
    assert set(found) == set(library) and all(found[k].shape == library[k].shape and found[k].dtype == library[k].dtype for k in found)
    assert int(found["count"].min()) > 0
    print("cells equal to the library path's:", float((found["cell"] == library["cell"]).float().mean()))
    for k in found:                                                  # (every kernel of the frame has a fixed order now: so has the frame)
        assert torch.equal(found[k], again[k]), k
    stack.close()
