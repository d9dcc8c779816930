"""The image front end on the GPU (``ops.image_frontend`` on ``vfa_image_plan`` / ``vfa_image_frames_u8_f32`` and the uint8 route of
``VFANet``) against Pillow's records (tests/golden/frontend_pil.npz) and against the restatement of tests/frontend_common.py, which
tests/test_frontend_cpu.py pins to those records and to Pillow itself bit for bit.  EVERY comparison is ``torch.equal`` on the bits:
this feature has no tolerance."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frontend_common as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """got: a device tensor, want: a numpy array or a tensor -> the same shape, dtype and bits."""
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    return got.dtype == want.dtype == torch.float32 and got.shape == want.shape and torch.equal(_bits(got.cpu()), _bits(want.cpu()))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _tiled_case():
    """200 x 300 -> 133 x 200, three images: 1.5x, two tiles across and five down, none of them whole."""
    src = fc.noise((3, 200, 300, 3), 21)
    return src, fc.frontend(src, (133, 200), fc.MEAN, fc.STD)


@pytest.mark.parametrize("index", range(len(fc.SHAPES)), ids=["%dx%d_%dx%d" % (*a, *b) for a, b in fc.SHAPES])
def test_record(index):
    """Partial tiles, upscaling, one-axis passes, 3 / 5 / 9 / 13 / 17 taps: Pillow's own pixels."""
    from vfa_amd import ops
    d, shape = fc.load(), fc.SHAPES[index]
    for name in ("noise", "binary"):
        src, want_u8 = d[fc.key(shape, name + "_in")], d[fc.key(shape, name + "_out")]
        got = ops.image_frontend(_dev(src[None]), size=shape[1], mean=fc.MEAN, std=fc.STD)
        assert _same(got[0], fc.to_tensor(want_u8, fc.MEAN, fc.STD)), (shape, name)
        plain = ops.image_frontend(_dev(src[None]), size=shape[1])
        assert _same(plain[0], fc.to_tensor(want_u8)), (shape, name)
        assert torch.equal((plain[0] * 255).round().to(torch.uint8).cpu(), torch.from_numpy(want_u8).permute(2, 0, 1)), (shape, name)
    if index in fc.TENSOR_SHAPES:
        src = _dev(d[fc.key(shape, "noise_in")][None])
        assert _same(ops.image_frontend(src, size=shape[1], mean=fc.MEAN, std=fc.STD)[0], d[fc.key(shape, "tensor_model")]), shape
        assert _same(ops.image_frontend(src, size=shape[1])[0], d[fc.key(shape, "tensor_plain")]), shape


def test_several_tiles_in_both_axes():
    from vfa_amd import ops
    src, want = _tiled_case()
    assert _same(ops.image_frontend(_dev(src), size=(133, 200), mean=fc.MEAN, std=fc.STD), want)


def test_full_frame():
    from vfa_amd import ops
    (ih, iw), size = fc.FULL
    src = fc.noise((1, ih, iw, 3), 22)
    assert _same(ops.image_frontend(_dev(src), size=size, mean=fc.MEAN, std=fc.STD), fc.frontend(src, size, fc.MEAN, fc.STD))


@pytest.mark.parametrize("constants", [(fc.MEAN, fc.STD), PLAIN], ids=["model", "plain"])
def test_table_exhaustively(constants):
    """Every byte value in every channel, no resize, against CPU torch's ``(u8.float() / 255 - mean) / std`` (IEEE divisions)."""
    from vfa_amd import ops
    mean, std = constants
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous()
    want = (u8.permute(0, 3, 1, 2).float() / 255 - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    assert _same(ops.image_frontend(u8.to(DEV), mean=mean, std=std), want)
    tensors = ops.image_frontend(u8.to(DEV), mean=torch.tensor(mean, device=DEV), std=torch.tensor(std, device=DEV))
    assert _same(tensors, want)
    on_device = (u8.to(DEV).permute(0, 3, 1, 2).float() / 255 - torch.tensor(mean, device=DEV).view(3, 1, 1)) / torch.tensor(std, device=DEV).view(3, 1, 1)
    print(f"device torch expression: {int((_bits(on_device.cpu()) != _bits(want)).sum())} of 768 entries differ from CPU torch in some bit")


def test_row_pitch_and_image_stride():
    from vfa_amd import ops
    src, want = _tiled_case()
    n, h, w, _ = src.shape
    pitched = torch.zeros(n, h, 3 * w + 7, dtype=torch.uint8, device=DEV)           # rows of 907 bytes: every skew of a row's first byte
    pitched[:, :, :3 * w] = _dev(src).view(n, h, 3 * w)
    view = pitched[:, :, :3 * w].view(n, h, 3 * w).unflatten(2, (w, 3))
    assert view.stride() == (h * (3 * w + 7), 3 * w + 7, 3, 1) and view.data_ptr() == pitched.data_ptr()
    assert _same(ops.image_frontend(view, size=(133, 200), mean=fc.MEAN, std=fc.STD), want)
    spaced = torch.zeros(2 * n, h, w, 3, dtype=torch.uint8, device=DEV)
    spaced[::2] = _dev(src)
    every_second = spaced[::2]
    assert every_second.stride(0) == 2 * h * w * 3 and every_second.data_ptr() == spaced.data_ptr()
    assert _same(ops.image_frontend(every_second, size=(133, 200), mean=fc.MEAN, std=fc.STD), want)
    odd = torch.zeros(n * h * w * 3 + 1, dtype=torch.uint8, device=DEV)             # a first byte that is not dword aligned
    odd[1:] = _dev(src).flatten()
    assert _same(ops.image_frontend(odd[1:].view(n, h, w, 3), size=(133, 200), mean=fc.MEAN, std=fc.STD), want)


def test_batch_of_frames_is_the_frames_one_by_one():
    from vfa_amd import ops
    src, want = _tiled_case()
    batch = _dev(np.stack([src[:2], src[1:]]))                                       # (2, 2, 200, 300, 3)
    got = ops.image_frontend(batch, size=(133, 200), mean=fc.MEAN, std=fc.STD)
    assert got.shape == (2, 2, 3, 133, 200)
    for b in range(2):
        for n in range(2):
            one = ops.image_frontend(batch[b, n][None], size=(133, 200), mean=fc.MEAN, std=fc.STD)
            assert torch.equal(_bits(got[b, n]), _bits(one[0])) and _same(got[b, n], want[b + n])
    out = torch.empty(2, 2, 3, 133, 200, device=DEV)
    assert ops.image_frontend(batch, size=(133, 200), mean=fc.MEAN, std=fc.STD, out=out) is out and torch.equal(_bits(out), _bits(got))
    assert ops.image_frontend(batch[:0], size=(133, 200)).shape == (0, 2, 3, 133, 200)
    with pytest.raises(ValueError):
        ops.image_frontend(batch, size=(133, 200), out=out[0])
    with pytest.raises(ValueError):
        ops.image_frontend(batch, size=(24, 200))                                    # 200 -> 24: more than 17 taps


def test_other_constants_make_another_plan():
    from vfa_amd import ops
    src, want = _tiled_case()
    frames = _dev(src[:1])
    assert _same(ops.image_frontend(frames, size=(133, 200), mean=fc.MEAN, std=fc.STD), want[:1])
    assert _same(ops.image_frontend(frames, size=(133, 200)), fc.frontend(src[:1], (133, 200)))
    other = ((0.5, 0.25, 0.125), (0.25, 0.5, 2.0))
    assert _same(ops.image_frontend(frames, size=(133, 200), mean=other[0], std=other[1]), fc.frontend(src[:1], (133, 200), *other))
    mean, std = torch.tensor(fc.MEAN, device=DEV), torch.tensor(fc.STD, device=DEV)
    assert _same(ops.image_frontend(frames, size=(133, 200), mean=mean, std=std), want[:1])
    mean.copy_(torch.tensor(other[0]))                                               # the same tensors, updated in place
    std.copy_(torch.tensor(other[1]))
    assert _same(ops.image_frontend(frames, size=(133, 200), mean=mean, std=std), fc.frontend(src[:1], (133, 200), *other))
    assert _same(ops.image_frontend(frames, size=(133, 200), mean=fc.MEAN, std=fc.STD), want[:1])


def test_graph_capture_on_one_stream():
    """The plan outside the capture, the frame kernel captured; a replay after the source bytes were overwritten gives the new
    frame's tensor."""
    from vfa_amd import ops
    src, want = _tiled_case()
    second = fc.noise((3, 200, 300, 3), 23)
    static = _dev(src)
    out = torch.empty(3, 3, 133, 200, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.image_frontend(static, size=(133, 200), mean=fc.MEAN, std=fc.STD, out=out)      # (the plan is made here)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_frontend(static, size=(133, 200), mean=fc.MEAN, std=fc.STD, out=out)
    for frames, expected in ((second, fc.frontend(second, (133, 200), fc.MEAN, fc.STD)), (src, want)):
        static.copy_(_dev(frames))
        out.zero_()
        graph.replay()
        assert _same(out, expected)


# ---- VFANet on a small rig -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rig():
    import vfa_amd
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.vfanet import VFANet
    args = SimpleNamespace(data="MultiviewC", image_size=(192, 320), resize_size=(192, 320))
    torch.manual_seed(0)
    net = VFANet(args, grid_height=96, cube_size=(50, 50, 32), angle_range=36).to(DEV).eval()
    calibs = ring_cameras(2, (600., 500., 0.), 1500., 500., 250., (320, 192)).to(DEV)
    grid = vfa_amd.make_grid((1000, 1200), cube_LW=(50, 50), dataset="MultiviewC").to(DEV)[None]
    frames = fc.noise((2, 288, 480, 3), 24)                                          # the cameras' frames, 1.5x the input size
    floats = torch.from_numpy(fc.resize(frames, (192, 320))).permute(0, 3, 1, 2).float() / 255   # what the reference's dataset hands over
    return net, calibs, grid, vfa_amd.pack_frames(list(frames), DEV), floats.to(DEV)


def test_vfanet_normalises_uint8_frames_like_the_float_route():
    net, _, _, frames, floats = _rig()
    assert frames.dtype == torch.uint8 and frames.shape == (2, 288, 480, 3) and frames.is_cuda
    assert tuple(net.input_size) == (192, 320)
    got = net.normalized(frames)
    assert torch.equal(_bits(got), _bits(net.normalized(floats)))                    # the float route, fed the restated resize / 255
    assert _same(got, (floats.cpu() - net.mean.cpu().view(3, 1, 1)) / net.std.cpu().view(3, 1, 1))   # ... and the expression on the CPU


def test_vfanet_forward_and_detect_take_uint8_frames():
    from vfa_amd import eval_ops
    net, calibs, grid, frames, floats = _rig()
    dec = eval_ops.BEVDecoder("MultiviewC", (1000, 1200), (50, 50, 32), dimension_mean=np.array([140, 60, 230], np.float32), topk=20)
    with torch.no_grad():
        first, again, got = net(floats, calibs, grid), net(floats, calibs, grid), net(frames, calibs, grid)
        batch = net(torch.stack([frames, frames]), calibs, grid)
        found, found_float = net.detect(frames, calibs, grid, dec, 0.0), net.detect(floats, calibs, grid, dec, 0.0)
    assert set(got) == set(first) and all(got[k].shape == first[k].shape for k in first)
    assert all(batch[k].shape == (2, *first[k].shape[1:]) for k in first)
    assert set(found) == set(found_float) and all(found[k].shape == found_float[k].shape for k in found)
    if not all(torch.equal(_bits(first[k]), _bits(again[k])) for k in first):
        pytest.skip("two runs of the float route differ in some bit: forward(u8) cannot be held to either")
    for k in first:
        assert torch.equal(_bits(got[k]), _bits(first[k])), k
