"""What tests/golden/make_dense_conv_bits.py and tests/test_dense_conv_bits.py share: the cases whose output bits were recorded on the
MI355X before the heads' and the trunk's dense convolutions were folded into one kernel template (vfa_amd/csrc/vfa_dense.h), and how
a case is computed -- public ``ops`` calls on seeded CPU generators (``cc.inputs``, ``tc.inputs``, ``tc.affine_of``) alone.

All cases have B = 2 (frames of different scales) and are the smallest that still exercise two channel chunks, partial tiles in
both directions and a partial second output tile; together they reach every instantiation of the kernel, both channel strides,
the two-chain split (C > 256), the transposed pack and the absmax pre-pass that feeds the weight gradient."""
import hashlib

import torch

import conv_common as cc
import trunk_common as tc

B = 2

HEAD_CASES = {  # name: (C, O, L, W, dilation, layout, scale, shift, relu)
    "heads_d1_c64_o130_9x37_nchw_scale_shift_relu": (64, 130, 9, 37, 1, "nchw", True, True, True),
    "heads_d2_c32_o40_9x37_nhwc_shift": (32, 40, 9, 37, 2, "nhwc", False, True, False),
    "heads_d3_c64_o128_5x33_slice": (64, 128, 5, 33, 3, "slice", False, False, False),
    "heads_d4_c64_o40_9x37_nchw_relu": (64, 40, 9, 37, 4, "nchw", False, False, True),
}
GRAD_CASES = {  # name: (which, C, O, L, W, dilation); the weight is (O, C, 3, 3), the gradient (B, O, L, W)
    "heads_input_grad_d2_c96_o64_9x37": ("input", 96, 64, 9, 37, 2),
    "heads_weight_grad_d2_c32_o32_9x37": ("weight", 32, 32, 9, 37, 2),
}
TRUNK_CASES = {  # name: (C, O, L, W, kernel, stride, layout, prologue)
    "trunk_k3_s1_c64_o130_9x37_nchw_prologue": (64, 130, 9, 37, 3, 1, "nchw", True),
    "trunk_k3_s1_c288_o40_6x7": (288, 40, 6, 7, 3, 1, "nchw", False),
    "trunk_k3_s2_c64_o130_9x67_nhwc_prologue": (64, 130, 9, 67, 3, 2, "nhwc", True),
    "trunk_k3_s2_c288_o40_7x9_prologue": (288, 40, 7, 9, 3, 2, "nchw", True),
    "trunk_k1_s1_c64_o130_9x37_nchw": (64, 130, 9, 37, 1, 1, "nchw", False),
    "trunk_k1_s1_c288_o40_6x7_prologue": (288, 40, 6, 7, 1, 1, "nchw", True),
    "trunk_k1_s2_c64_o130_9x67_slice": (64, 130, 9, 67, 1, 2, "slice", False),
    "trunk_k1_s2_c288_o40_7x9": (288, 40, 7, 9, 1, 2, "nchw", False),
}
NAMES = [*HEAD_CASES, *GRAD_CASES, *TRUNK_CASES]


def layout(x, how, dev):
    """The same values as NCHW, channels-last, or a non-contiguous slice of a larger tensor, on the device."""
    x = x.to(dev)
    if how == "nchw":
        return x.contiguous()
    if how == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    n, C, L, W = x.shape
    big = torch.full((n + 1, C + 8, L + 2, W + 3), 7.0, device=dev)
    big[1:, 4:4 + C, 1:1 + L, 2:2 + W] = x
    return big[1:, 4:4 + C, 1:1 + L, 2:2 + W]


def _seed(name):
    return sum(name.encode()) % 1000


def compute(name, dev):
    """The case's output on ``dev`` -> a contiguous float32 tensor."""
    from vfa_amd import ops
    seed = _seed(name)
    with torch.no_grad():
        if name in HEAD_CASES:
            C, O, L, W, d, how, has_scale, has_shift, relu = HEAD_CASES[name]
            x, w = cc.inputs(B, C, O, L, W, seed)
            scale, shift = (t.reshape(O).to(dev) for t in tc.affine_of(1, O, seed + 1))
            return ops.conv3x3(layout(x, how, dev), w.to(dev), d, scale if has_scale else None, shift if has_shift else None, relu)
        if name in GRAD_CASES:
            which, C, O, L, W, d = GRAD_CASES[name]
            x, w = cc.inputs(B, C, O, L, W, seed)
            g, _ = cc.inputs(B, O, 32, L, W, seed + 1)
            if which == "input":
                return ops.conv3x3_input_grad(g.to(dev), w.to(dev), d)
            return ops.conv3x3_weight_grad(g.to(dev), x.to(dev), d)[0]
        C, O, L, W, k, stride, how, prologue = TRUNK_CASES[name]
        x, w = tc.inputs(B, C, O, L, W, seed, k=k)
        affine = tuple(t.to(dev) for t in tc.affine_of(B, C, seed + 1)) if prologue else None
        return ops.trunk_conv(layout(x, how, dev), w.to(dev), stride, affine)


def digest(y):
    """SHA-256 of the contiguous float32 bytes."""
    assert y.dtype == torch.float32
    return hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest()
