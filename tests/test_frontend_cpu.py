"""The image front end without a GPU: the restatement of tests/frontend_common.py against Pillow's own pixels
(tests/golden/frontend_pil.npz, made by tests/golden/make_frontend.py) bit for bit, and against Pillow itself on the workload's shape
where it is installed; the rules of vfa_amd/csrc/vfa_resize.h (shared host / device code) compiled with g++ into
tests/native/resize_harness.cpp, a stand-alone program, against the same records, once more under the host sanitizers; the ABI of
the new entry points and every refusal they make before a device is touched; the Python surface.  Nothing here has a tolerance."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import REPO
import frontend_common as fc
from native_common import build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"]
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "resize_rules", "resize_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "resize_rules", "resize_harness.cpp", GXX_FLAGS, sanitized=True)


@pytest.fixture(scope="module")
def records():
    return fc.load()


def _f32(v):
    return str(struct.unpack("<I", struct.pack("<f", float(v)))[0])


# ---- 1. the restatement against Pillow -------------------------------------------------------------------------------------------

def test_restatement_is_pillows_bit_for_bit(records):
    taps = set()
    for i, shape in enumerate(fc.SHAPES):
        (ih, iw), (oh, ow) = shape
        taps |= {fc.ksize_of(ih, oh), fc.ksize_of(iw, ow)}
        for name in ("noise", "binary"):
            src = records[fc.key(shape, name + "_in")]
            assert src.shape == (ih, iw, 3) and src.dtype == np.uint8
            assert fc.same_bits(fc.resize(src, (oh, ow)), records[fc.key(shape, name + "_out")]), (shape, name)
        assert set(np.unique(records[fc.key(shape, "binary_in")])) == {0, 255}
        if i in fc.TENSOR_SHAPES:
            src = records[fc.key(shape, "noise_in")]
            assert fc.same_bits(fc.frontend(src, (oh, ow), fc.MEAN, fc.STD), records[fc.key(shape, "tensor_model")]), shape
            assert fc.same_bits(fc.frontend(src, (oh, ow)), records[fc.key(shape, "tensor_plain")]), shape
    assert {3, 5, 9, 13, 17} <= taps
    assert os.path.getsize(fc.GOLDEN) < 300 * 1024


def test_restatement_is_pillows_on_the_full_frame():
    Image = pytest.importorskip("PIL.Image")
    (ih, iw), (oh, ow) = fc.FULL
    for src in (fc.noise((ih, iw, 3), 11), (fc.noise((ih, iw, 3), 12) >> 7) * np.uint8(255)):
        want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
        assert fc.same_bits(fc.resize(src, (oh, ow)), want)


def test_restated_tensor_is_cpu_torchs():
    """``to_tensor`` against the expression of the model on CPU torch, every byte value in every channel."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    for mean, std in ((fc.MEAN, fc.STD), ((0.0,) * 3, (1.0,) * 3)):
        t = torch.from_numpy(u8).permute(2, 0, 1).float() / 255
        want = (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
        assert fc.same_bits(fc.to_tensor(u8, mean, std), want.numpy())


# ---- 2. the shared header on the CPU -----------------------------------------------------------------------------------------------

def test_rules_hold_on_random_axes(harness):
    run_harness(harness, "cases", "1")


def test_rules_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "cases", "2")


def _harness_frame(exe, tmp_path, src, size, mean, std):
    (ih, iw, _), (oh, ow) = src.shape, size
    paths = [str(tmp_path / n) for n in ("in.bin", "out_u8.bin", "out_f32.bin")]
    src.tofile(paths[0])
    run_harness(exe, "frame", paths[0], str(ih), str(iw), str(oh), str(ow), *[_f32(v) for v in mean], *[_f32(v) for v in std], paths[1], paths[2])
    return np.fromfile(paths[1], np.uint8).reshape(oh, ow, 3), np.fromfile(paths[2], np.float32).reshape(3, oh, ow)


def test_header_reproduces_every_record(harness, sanitized_harness, records, tmp_path):
    for exe in (harness, sanitized_harness):
        for i, shape in enumerate(fc.SHAPES):
            for name in ("noise", "binary"):
                u8, tensor = _harness_frame(exe, tmp_path, records[fc.key(shape, name + "_in")], shape[1], fc.MEAN, fc.STD)
                assert fc.same_bits(u8, records[fc.key(shape, name + "_out")]), (shape, name)
                assert fc.same_bits(tensor, fc.to_tensor(u8, fc.MEAN, fc.STD)), (shape, name)
                if i in fc.TENSOR_SHAPES and name == "noise":
                    assert fc.same_bits(tensor, records[fc.key(shape, "tensor_model")]), shape
                    plain = _harness_frame(exe, tmp_path, records[fc.key(shape, "noise_in")], shape[1], (0.0,) * 3, (1.0,) * 3)[1]
                    assert fc.same_bits(plain, records[fc.key(shape, "tensor_plain")]), shape


def test_header_table_is_cpu_torchs(harness, tmp_path):
    """Every byte value through the header's table entry, no resize, against ``(u8.float() / 255 - mean) / std`` of CPU torch."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    for mean, std in ((fc.MEAN, fc.STD), ((0.0,) * 3, (1.0,) * 3)):
        same, tensor = _harness_frame(harness, tmp_path, u8, (256, 1), mean, std)
        t = torch.from_numpy(u8).permute(2, 0, 1).float() / 255
        want = (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
        assert fc.same_bits(same, u8) and fc.same_bits(tensor, want.numpy())


def test_header_reproduces_the_full_frame(harness, tmp_path):
    (ih, iw), size = fc.FULL
    src = fc.noise((ih, iw, 3), 13)
    u8, tensor = _harness_frame(harness, tmp_path, src, size, fc.MEAN, fc.STD)
    assert fc.same_bits(u8, fc.resize(src, size)) and fc.same_bits(tensor, fc.to_tensor(u8, fc.MEAN, fc.STD))


# ---- 3. the library's plumbing ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from vfa_amd import _lib, ops
    declared = declared_parameters()
    for name, count in (("vfa_image_workspace_bytes", 4), ("vfa_image_plan", 9), ("vfa_image_frames_u8_f32", 12)):
        assert declared.get(name) == count == len(_lib.SIGNATURES[name]), name
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    shared = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_resize.h")).read()
    for macro, constant, value, mirrored in (("VFA_IMAGE_MAX_TAPS", "kMaxTaps", 17, ops.IMAGE_MAX_TAPS),
                                             ("VFA_IMAGE_MAX_LENGTH", "kMaxLength", 16384, ops.IMAGE_MAX_LENGTH)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == value == mirrored
        assert int(re.search(constant + r"\s*=\s*(\d+)", shared).group(1)) == value
    assert (fc.MAX_TAPS, fc.MAX_LENGTH) == (17, 16384)
    assert int(re.search(r"#define\s+VFA_ABI_VERSION\s+(\d+)", text).group(1)) == 9 == _lib.ABI_VERSION    # additive: no new version
    makefile = open(os.path.join(REPO, "vfa_amd", "csrc", "Makefile")).read()
    assert "vfa_image.hip" in makefile.split("SRCS")[1] and "vfa_resize.h" in makefile.split("HDRS")[1]
    assert "contract=off" in makefile


def _workspace_bytes(ih, iw, oh, ow):
    """table | x bounds | x coefficients | y bounds | y coefficients, in 4-byte words, rounded up to 16 bytes."""
    words = 3 * 256 + ow * (2 + fc.ksize_of(iw, ow)) + oh * (2 + fc.ksize_of(ih, oh))
    return (words + 3) // 4 * 4 * 4


def test_workspace_size_and_refusals(built_lib):
    """Everything the calls decide before they launch (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    for sizes in ((1080, 1920, 720, 1280), (720, 1280, 720, 1280), (37, 53, 19, 31), (7, 5, 40, 41), (40, 40, 5, 7), (1, 1, 1, 1),
                  (16384, 16384, 2048, 16384)):
        assert lib.vfa_image_workspace_bytes(*sizes) == _workspace_bytes(*sizes), sizes
    assert lib.vfa_image_workspace_bytes(1080, 1920, 720, 1280) == 4 * (768 + 1280 * 7 + 720 * 7)
    for sizes in ((0, 5, 5, 5), (5, -1, 5, 5), (5, 5, 0, 5), (5, 5, 5, 0), (16385, 5, 16385, 5), (5, 5, 5, 16385), (9, 5, 1, 5), (5, 1000, 5, 100)):
        assert lib.vfa_image_workspace_bytes(*sizes) == 0, sizes
    p = ctypes.c_void_p(4096)   # (never dereferenced)
    enough = 1 << 20

    def plan(Hin=37, Win=53, Hout=19, Wout=31, mean=p, std=p, ws=p, ws_bytes=enough):
        return lib.vfa_image_plan(Hin, Win, Hout, Wout, mean, std, ws, ws_bytes, None)

    def frames(src=p, image_stride=37 * 53 * 3, row_stride=53 * 3, N=2, Hin=37, Win=53, ws=p, ws_bytes=enough, dst=p, Hout=19, Wout=31):
        return lib.vfa_image_frames_u8_f32(src, image_stride, row_stride, N, Hin, Win, ws, ws_bytes, dst, Hout, Wout, None)

    for call in (plan, frames):
        assert call(Hin=0) == BAD and call(Win=-1) == BAD and call(Hout=0) == BAD and call(Wout=-5) == BAD
        assert call(ws=None) == BAD
        assert call(ws_bytes=_workspace_bytes(37, 53, 19, 31) - 1) == BAD and call(ws_bytes=0) == BAD
        assert call(Hin=19 * 8 + 1) == UNSUPPORTED and call(Win=31 * 8 + 1) == UNSUPPORTED
        assert call(Hin=16385, Hout=16385) == UNSUPPORTED and call(Wout=16385) == UNSUPPORTED
    assert plan(mean=None) == BAD and plan(std=None) == BAD
    assert frames(src=None) == BAD and frames(dst=None) == BAD and frames(N=-1) == BAD
    assert frames(row_stride=53 * 3 - 1) == BAD and frames(row_stride=0) == BAD and frames(image_stride=-1) == BAD
    assert frames(N=65536) == UNSUPPORTED
    assert frames(N=0) == 0 and frames(N=0, src=None, ws=None, dst=None, ws_bytes=0) == 0
    assert frames(N=0, Hin=0) == BAD            # (the sizes are checked first)


def test_wrappers_refuse_cpu_tensors_other_dtypes_and_channel_counts(built_lib):
    import vfa_amd
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    frames = torch.zeros(2, 8, 12, 3, dtype=torch.uint8)
    for kw in ({}, dict(size=(4, 6)), dict(mean=torch.zeros(3), std=torch.ones(3))):
        with pytest.raises(VFAHipError):           # CPU tensors: no fallback
            ops.image_frontend(frames, **kw)
    with pytest.raises(VFAHipError):
        ops.image_frontend(frames[None], size=(4, 6))
    for bad in (frames.float(), frames.to(torch.int8), torch.zeros(2, 8, 12, 4, dtype=torch.uint8), torch.zeros(2, 3, 8, 12, dtype=torch.uint8),
                frames[0], torch.zeros(1, 1, 2, 8, 12, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):            # (decided before the device is looked at)
            ops.image_frontend(bad)
    packed = vfa_amd.pack_frames([np.full((8, 12, 3), i, np.uint8) for i in range(3)])
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, 8, 12, 3) and packed[2].eq(2).all() and not packed.is_cuda
    for bad in ([], [np.zeros((8, 12, 3), np.float32)], [np.zeros((8, 12, 4), np.uint8)], [np.zeros((8, 12), np.uint8)],
                [np.zeros((8, 12, 3), np.uint8), np.zeros((8, 13, 3), np.uint8)]):
        with pytest.raises(ValueError):
            vfa_amd.pack_frames(bad)
    assert ops.image_taps(1080, 720) == 5 and ops.image_taps(720, 1080) == 3 and ops.image_taps(8, 1) == 17 and ops.image_taps(9, 1) == 19


def test_vfanet_input_size_is_not_state():
    import json
    from types import SimpleNamespace
    from conftest import golden_path
    from vfa_amd.vfanet import VFANet
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280), resize_size=(720, 1280)))
    assert tuple(net.input_size) == (720, 1280)
    assert VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280))).input_size is None
    want = [k for k, _, _ in json.load(open(golden_path("vfanet_state_keys.json")))["resnet18_3D"]]
    assert list(net.state_dict().keys()) == want
    x = torch.rand(2, 3, 8, 8)                     # the float route is the expression it was
    assert torch.equal(net.normalized(x), (x - net.mean.view(3, 1, 1)) / net.std.view(3, 1, 1))
