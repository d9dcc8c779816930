"""The trunk's stem on the MI355X (``ops.stem_conv``, ``ops.stem_pool``, ``_Trunk.stem_hip``, ``VFANet.trunk_stem = "hip"``) against the
float64 ``F.conv2d`` / module chain of the same float32 inputs on the CPU, under the yardsticks of tests/stem_common.py: (E)
elementwise with n = 147, (N) normwise within 4 x the float32 library chain on the CPU; the pooling bit for bit against its numpy
restatement.  Shapes are the smallest that can still go wrong: a 1 x 1 image, odd sizes, an image narrower than the 7-wide kernel, raw
maps that cross the 4 x 32 cell tile in both directions with ragged last tiles, more tiles than workgroups (a workgroup walks over
two tiles), O = 64 and an O below it, NCHW / channels-last / sliced inputs, B = 2 with images of different scales, a pooled plane
larger than a workgroup's 1024 cells.  Every test prints its ratios before it asserts.

Measured on the MI355X: (E) at most 0.040 of its bound (1 x 1: 0.007, 5 x 6: 0.019, 10 x 71: 0.032, two tiles per workgroup: 0.040); (N)
0.76 x (1 x 1), 0.97 x (9 x 11), 1.01 x (O = 5), 1.00 x (19 x 141), 1.44 x (2 x 3), 0.99 x (two tiles per workgroup), equal in all three
layouts; the pooling at most 0.995 u |out64|; the stem of the model 0.96 x; the model's f8 / f16 / f32 with library stages 0.94 / 1.02 /
1.01 x (resnet18) and 0.97 / 0.98 / 0.98 x (resnet34), with hip stages 1.38 / 1.64 / 1.72 x and 1.40 / 1.68 / 1.74 x.  Times
(tools/bench_stem.py, resnet18, 720 x 1280, library / hip): 7 images: stem 2.00 / 0.78 ms (convolution 0.395, statistics 0.151, pooling
0.231), 28 images: 5.52 / 3.10 ms; ``detect`` on 7 images 12.68 -> 7.23 ms with every setting on "hip".  Kernel resources: convolution 165
VGPRs, 48 808 B LDS, three workgroups per CU; pooling 49 VGPRs; scratch 0."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conv_common as cc
import frontend_common as fc
import stem_common as sc
import trunk_common as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYOUTS = ("nchw", "nhwc", "slice")


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
    big = torch.full((B + 1, C + 2, L + 2, W + 3), 7.0, device=DEV)
    big[1:, 1:1 + C, 1:1 + L, 2:2 + W] = x
    return big[1:, 1:1 + C, 1:1 + L, 2:2 + W]


@contextlib.contextmanager
def _deterministic_library():
    """Where a test compares two runs of the LIBRARY stem: its convolution gives the same bits twice only under this setting."""
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn_only)


CONV_CASES = {  # name: (B, O, L, W): the raw map
    "smallest_1x1": (2, 64, 1, 1),              # 1 x 1
    "odd_9x11": (2, 64, 9, 11),                 # 5 x 6
    "odd_9x11_o5": (2, 5, 9, 11),               # fewer outputs than the tile's 64
    "tiles_19x141": (2, 64, 19, 141),           # 10 x 71: three tile rows and three tile columns, both last ones ragged
    "narrow_2x3": (2, 64, 2, 3),                # 1 x 2, narrower than the kernel
}
WALK = (13, 4, 38, 1531)                        # 19 x 766: 13 x 120 tiles > 1536 workgroups, so every workgroup walks over two tiles


@functools.lru_cache(maxsize=None)
def _case(name):
    B, O, L, W = CONV_CASES[name]
    return sc.inputs(B, O, L, W, seed=len(name) + O + L)


@functools.lru_cache(maxsize=None)
def _conv(name, layout):
    """The kernel's output on inputs that are never written to."""
    from vfa_amd import ops
    x, w = _case(name)
    with torch.no_grad():
        return ops.stem_conv(_layout(x, layout), w.to(DEV))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_stem_conv_against_float64(name, layout):
    (x, w), y = _case(name), _conv(name, layout)
    B, O, L, W = CONV_CASES[name]
    assert y.shape == (B, O, sc.out_size(L), sc.out_size(W)) and y.dtype == torch.float32 and y.is_contiguous()
    sc.check_both(y, x, w, f"{name} {layout}")


def test_stem_conv_where_a_workgroup_walks_over_several_tiles():
    from vfa_amd import ops
    B, O, L, W = WALK
    assert B * ((sc.out_size(L) + 3) // 4) * ((sc.out_size(W) + 31) // 32) > 1536
    x, w = sc.inputs(B, O, L, W, seed=5)
    with torch.no_grad():
        y = ops.stem_conv(x.to(DEV), w.to(DEV))
    sc.check_both(y, x, w, "two tiles per workgroup")


@pytest.mark.parametrize("name", ["odd_9x11", "tiles_19x141"])
def test_stem_conv_is_its_restatement_bit_for_bit(name):
    """The f32 MFMA is a k-ordered fmaf chain: the kernel's stated order gives the restatement's bits, not only its error."""
    (x, w), y = _case(name), _conv(name, "nchw")
    assert torch.equal(_bits(y).cpu(), _bits(sc.emulate_conv(x, w)))


def test_same_bits_on_every_run_alone_and_in_a_batch_and_in_every_layout():
    from vfa_amd import ops
    x, w = _case("tiles_19x141")
    first = _conv("tiles_19x141", "nchw")
    wd = w.to(DEV)
    with torch.no_grad():
        again = ops.stem_conv(x.to(DEV), wd)
        alone = [ops.stem_conv(x[b:b + 1].to(DEV), wd) for b in range(2)]
    assert float(first.abs().max()) > 0
    assert torch.equal(_bits(first), _bits(again))
    for layout in LAYOUTS:
        assert torch.equal(_bits(first), _bits(_conv("tiles_19x141", layout))), layout
    for b in range(2):
        assert torch.equal(_bits(first[b:b + 1]), _bits(alone[b])), f"image {b} alone"


def test_all_zero_image_gives_a_zero_raw_map():
    from vfa_amd import ops
    x, w = _case("tiles_19x141")
    mixed = x.clone()
    mixed[0] = 0.0
    with torch.no_grad():
        y = ops.stem_conv(torch.zeros_like(x).to(DEV), w.to(DEV))
        ym = ops.stem_conv(mixed.to(DEV), w.to(DEV))
    assert y.shape == (2, 64, 10, 71) and not y.any()
    assert not ym[0].any() and ym[1].any()


def test_one_nan_reaches_exactly_its_receptive_field():
    from vfa_amd import ops
    x, w = _case("tiles_19x141")
    poisoned = x.clone()
    poisoned[1, 2, 9, 65] = float("nan")                            # output rows 3 .. 6 and columns 31 .. 34: across a tile edge both ways
    with torch.no_grad():
        y = ops.stem_conv(poisoned.to(DEV), w.to(DEV)).cpu()
    want = torch.zeros(2, 1, 10, 71, dtype=torch.bool)
    for oy in range(10):
        for ox in range(71):
            want[1, 0, oy, ox] = abs(2 * oy - 9) <= 3 and abs(2 * ox - 65) <= 3
    assert int(want.sum()) == 4 * 4
    assert torch.equal(torch.isnan(y), want.expand_as(y))


def test_wrappers_refuse_other_weights():
    from vfa_amd import ops
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    for bad in (torch.zeros(65, 3, 7, 7), torch.zeros(8, 3, 3, 3), torch.zeros(8, 4, 7, 7)):
        with pytest.raises(ValueError):
            ops.stem_conv(x, bad.to(DEV))
    with pytest.raises(ValueError, match="inference only"):
        ops.stem_conv(x, torch.zeros(8, 3, 7, 7, device=DEV).requires_grad_())
    assert ops.stem_conv(torch.zeros(0, 3, 8, 8, device=DEV), torch.zeros(8, 3, 7, 7, device=DEV)).shape == (0, 8, 4, 4)


# ---- the pooling -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,W", [(1, 1), (9, 11), (10, 70), (70, 70)])
def test_stem_pool_is_its_restatement_bit_for_bit(L, W):
    """(a, b) are the device's own: ``group_norm_affine`` of the clean map with weights and biases of both signs; 70 x 70 pools to
    1225 cells, more than a workgroup's 1024."""
    from vfa_amd import ops
    B, C, groups = 2, 6, 3
    gen = torch.Generator().manual_seed(L + W)
    y = torch.randn(B, C, L, W, generator=gen) * 3
    gamma, beta = torch.tensor([1.5, -0.7, 0.9, -1.2, 0.4, -2.0]), torch.tensor([0.3, -0.2, -0.5, 0.6, 0.1, -0.4])
    with torch.no_grad():
        affine = ops.group_norm_affine(y.to(DEV), groups, gamma.to(DEV), beta.to(DEV), 1e-5)
    a, b = (t.cpu() for t in affine)
    assert float(a.min()) < 0 < float(a.max()) and float(b.min()) < 0 < float(b.max())
    if L > 1:
        y[1, 2, 4, 5] = float("nan")                                # placed after the statistics: (a, b) stay finite
    want = sc.emulate_pool(y, (a, b))
    with torch.no_grad():
        out = ops.stem_pool(y.to(DEV), affine).cpu()
    assert out.shape == (B, C, sc.out_size(L), sc.out_size(W)) and out.dtype == torch.float32
    nan = torch.isnan(want)
    assert int(nan.sum()) == (0 if L == 1 else 2) and torch.equal(torch.isnan(out), nan)
    assert torch.equal(_bits(out)[~nan], _bits(want)[~nan])
    assert float(out[~nan].max()) > 0.0 and (L == 1 or float(out[~nan].min()) == 0.0)      # (a 1 x 1 map: twelve cells, all positive)
    sc.check_pool(out, y, (a, b), f"{L}x{W}")


# ---- the model -----------------------------------------------------------------------------------------------------------------------

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


@contextlib.contextmanager
def _settings(net, stem, convs, heads="library"):
    net.trunk_stem, net.trunk_convs, net.head_convs = stem, convs, heads
    try:
        yield net
    finally:
        net.trunk_stem = net.trunk_convs = net.head_convs = "library"


@pytest.mark.parametrize("convs", ["library", "hip"])
@pytest.mark.parametrize("base", ["resnet18", "resnet34"])
def test_model_trunk_with_the_hip_stem_against_the_float64_trunk(base, convs):
    from vfa_amd import ops
    net, x, want64, want32 = _net_and_images(base)
    with _settings(net, "hip", convs), torch.no_grad():
        net.trunk(x)
        kept = len(ops._CONV_KEPT)
        with ops.KernelTimer() as kt:
            got = net.trunk(x)
        assert len(ops._CONV_KEPT) == kept                           # the stem keeps nothing, the stages nothing new
    torch.cuda.synchronize()
    launches = {k: v["launches"] for k, v in kt.summary().items()}
    blocks = sum(len(getattr(net.base, f"layer{i}")) for i in (1, 2, 3, 4))
    assert launches["vfa_stem_conv_f32"] == 1 and launches["vfa_stem_pool_f32"] == 1
    assert launches.get("vfa_trunk_conv_f32", 0) == (2 * blocks + 3 if convs == "hip" else 0)
    assert launches.get("vfa_residual_join_f32", 0) == (blocks if convs == "hip" else 0)
    for name, y, y64, y32 in zip(("f8", "f16", "f32"), got, want64, want32):
        assert y.shape == y64.shape and y.dtype == torch.float32 and y.is_contiguous() and y.device == x.device
        cc.check_normwise(y, y64, y32, f"{base} hip stem, {convs} stages, {name}")


def test_stem_hip_against_the_float64_stem():
    import copy
    net, x, _, _ = _net_and_images("resnet18")
    with torch.no_grad():
        got = net.base.stem_hip(x)
        cpu = copy.deepcopy(net.base).cpu()
        want32, want64 = cpu.stem(x.cpu()), cpu.double().stem(x.double().cpu())
    assert got.shape == want64.shape == (2, 64, 16, 24)
    cc.check_normwise(got, want64, want32, "stem")


@pytest.mark.parametrize("base", ["resnet18", "resnet34"])
def test_whole_hip_trunk_has_the_same_bits_twice_and_alone_without_the_deterministic_setting(base):
    net, x, _, _ = _net_and_images(base)
    assert not torch.are_deterministic_algorithms_enabled()
    with _settings(net, "hip", "hip"), torch.no_grad():
        first, again, alone = net.trunk(x), net.trunk(x), net.trunk(x[1:])
    for a, b, c in zip(first, again, alone):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a[1:]), _bits(c))


def test_model_in_training_mode_or_with_gradients_runs_the_library_trunk():
    net, x, _, _ = _net_and_images("resnet18")
    with _settings(net, "hip", "hip"), _deterministic_library():
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
        net.trunk_convs = "library"                                   # the stem's setting alone chooses another path in eval mode
        with torch.no_grad():
            assert not torch.equal(_bits(net.trunk(x)[0]), _bits(library[0]))


def test_graph_replay_of_the_whole_hip_trunk_equals_the_eager_call():
    from vfa_amd import ops
    net, x, _, _ = _net_and_images("resnet18")
    with _settings(net, "hip", "hip"):
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


def test_detect_from_camera_bytes_with_every_setting_on_hip():
    """``VFANet.detect`` from uint8 frames (``pack_frames``) to detections with ``trunk_stem = trunk_convs = head_convs = "hip"``: no
    library convolution in the frame, so two calls give the same bits without the deterministic setting."""
    import vfa_amd
    from vfa_amd import eval_ops, ops
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.vfanet import VFANet
    args = SimpleNamespace(data="MultiviewC", image_size=(192, 320), resize_size=(192, 320))
    torch.manual_seed(0)
    net = VFANet(args, grid_height=96, cube_size=(50, 50, 32), angle_range=36).to(DEV).eval()
    calibs = ring_cameras(2, (600., 500., 0.), 1500., 500., 250., (320, 192)).to(DEV)
    grid = vfa_amd.make_grid((1000, 1200), cube_LW=(50, 50), dataset="MultiviewC").to(DEV)[None]
    frames = vfa_amd.pack_frames(list(fc.noise((2, 288, 480, 3), 24)), DEV)
    assert frames.dtype == torch.uint8
    dec = eval_ops.BEVDecoder("MultiviewC", (1000, 1200), (50, 50, 32), dimension_mean=np.array([140, 60, 230], np.float32), topk=20)
    library = net.detect(frames, calibs, grid, dec, 0.0)
    with torch.no_grad():
        integrals_library = net.lateral_integrals(frames)
    assert not torch.are_deterministic_algorithms_enabled()
    with _settings(net, "hip", "hip", "hip"):
        with torch.no_grad():
            integrals = net.lateral_integrals(frames)
            integrals_again = net.lateral_integrals(frames)
        with ops.KernelTimer() as kt:
            found = net.detect(frames, calibs, grid, dec, 0.0)
        again = net.detect(frames, calibs, grid, dec, 0.0)
    torch.cuda.synchronize()
    launches = {k: v["launches"] for k, v in kt.summary().items()}
    assert launches["vfa_stem_conv_f32"] == 1 and launches["vfa_stem_pool_f32"] == 1 and launches["vfa_trunk_conv_f32"] == 19
    assert {"vfa_image_frames_u8_f32", "vfa_residual_join_f32", "vfa_conv3x3_f32", "vfa_group_norm_affine_f32"} <= set(launches)
    assert len(integrals) == len(integrals_library) == 3
    for a, b, c in zip(integrals, integrals_again, integrals_library):
        assert a.shape == c.shape and a.dtype == c.dtype and torch.equal(_bits(a), _bits(b))
        print("integral image, hip trunk against the library trunk:", cc.normwise(a, c.double().cpu()))
        assert cc.normwise(a, c.double().cpu()) < 1e-4               # the same function: float32 summation orders apart, not a different map
    assert set(found) == set(library) and all(found[k].shape == library[k].shape and found[k].dtype == library[k].dtype for k in found)
    assert int(found["count"].min()) > 0
    print("cells equal to the library path's:", float((found["cell"] == library["cell"]).float().mean()))
    for k in found:
        assert torch.equal(found[k], again[k]), k
