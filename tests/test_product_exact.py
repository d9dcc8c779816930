"""The split-product kernels held to EQUALITY: vfa_grad_weight_f32, vfa_grad_input_f32 (vfa_grad.hip), vfa_collapse_gemm_f32,
vfa_collapse_gemm_relu_backward_f32 and its fp16 form (vfa_collapse_gemm.hip), vfa_collapse_relu_sum_f32 (vfa_collapse.hip),
vfa_lateral_conv_f32 / vfa_lateral_convs_f32 (vfa_lateral.hip) on operands whose arithmetic is exact in fp32 -- integers of one bf16
piece, and elements of two or three pieces on a window of the reduction index (tests/product_common.py: the principle, the operand
sets, the preconditions every test asserts on its inputs before a kernel runs; tests/test_product_exact_cpu.py: the proof that every
set is exact in any order and that it tells a kernel with a wrong set of piece products, a wrong plane, a lost step, row or reduce
part, a shifted index or swapped blocks from the right one).  The expected value is the sum of the KEPT piece products in float64, not
the float64 product.  No tolerance anywhere, apart from one float32 ulp on the GroupNorm affine of the lateral branch (a double
expression the compiler may contract)."""
import numpy as np
import pytest
import torch

import product_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _want(case):
    return pc.f32(pc.expected(case))


# ---- ops.grad_weight ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("rows", pc.GRAD_WEIGHT_SINGLE_ROWS)
def test_weight_gradient_of_integers_is_exact(rows, K):
    """Row counts that give 1, 2, 3, 5, 13, 17 and the capped number of row slabs (all three loops of the reduce kernel) and a ragged
    last step of 1, 7 and 15 live rows; then accumulated onto an integer map."""
    from vfa_amd import ops
    case = pc.grad_weight_single(rows, K)
    base = np.random.default_rng(rows).integers(-1000, 1001, (256, K)).astype(np.float64)
    pc.assert_exact_case(case, extra=base)
    g_lin, vox = _dev(case.A.x), _dev(case.B.x)
    pc.report_equal(ops.grad_weight(g_lin, vox), _want(case), case.name)
    acc = _dev(base)
    ops.grad_weight(g_lin, vox, out=acc, accumulate=True)
    pc.report_equal(acc, pc.f32(pc.expected(case) + base), case.name + ", accumulated")


@pytest.mark.parametrize("rows,offset,K", [(r, o, 256) for r, o in pc.GRAD_WEIGHT_MULTI] + [(31, None, 512)])
def test_weight_gradient_keeps_its_six_piece_products(rows, offset, K):
    """Three- and two-piece elements on 16, 24 and 31 rows, and on a 24-row window at the start, across a step boundary in the middle
    and in the ragged end of 4099 otherwise single-piece rows."""
    from vfa_amd import ops
    case = pc.grad_weight_multi(rows, offset, K)
    pc.assert_exact_case(case, claims=("A1", "A2", "B1", "B2"))
    pc.report_equal(ops.grad_weight(_dev(case.A.x), _dev(case.B.x)), _want(case), case.name)


# ---- ops.grad_input -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(r, K) for K in (256, 512) for r in pc.GRAD_INPUT_SINGLE_ROWS] + [pc.GRAD_INPUT_TALL])
def test_input_gradient_of_integers_is_exact(rows, K):
    """Ragged and whole 256-row blocks; the tall case has more blocks than workgroups (the block loop, the prefetch of the next block's
    first fragment) and a ragged last block."""
    from vfa_amd import ops
    case = pc.grad_input_single(rows, K)
    pc.assert_exact_case(case)
    got = ops.grad_input(_dev(case.A.x.T), _dev(case.B.x))
    pc.report_equal(got, _want(case), case.name)


@pytest.mark.parametrize("offset,rows,K", [(o, 300, 256) for o in pc.GRAD_INPUT_WINDOWS] + [(100, 257, 512)])
def test_input_gradient_keeps_its_six_piece_products(offset, rows, K):
    """The reduction runs over the 256 channels: the multi-piece window moves over all sixteen 16-deep steps (the weight planes of a
    step go through LDS)."""
    from vfa_amd import ops
    case = pc.grad_input_multi(offset, rows, K)
    pc.assert_exact_case(case, claims=("A1", "A2", "B1", "B2"))
    pc.report_equal(ops.grad_input(_dev(case.A.x.T), _dev(case.B.x)), _want(case), case.name)


# ---- ops.collapse_gemm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", pc.COLLAPSE_SINGLE)
def test_collapse_product_of_integers_is_exact(M, K):
    """Every form of the flag (3, 4, and 0 = the entry point's default) on integers; fully masked rows are exact zeros, rows with a masked
    first quarter exact sums; then the call that reuses the workspace, with the weight flipped."""
    from vfa_amd import ops
    case = pc.collapse_single(M, K)
    pc.assert_exact_case(case)
    vox, w = _dev(case.A.x.T), _dev(case.B.x.T)
    for terms in (3, 4, 0):
        pc.report_equal(ops.collapse_gemm(vox, w, terms=terms), _want(case), f"{case.name} terms {terms}")
    pc.report_equal(ops.collapse_gemm(vox, w.flip(0).contiguous(), terms=3), _want(case).flip(1).contiguous(), case.name + ", weight flipped")


@pytest.mark.parametrize("terms", [3, 0])
def test_collapse_product_keeps_three_products_of_two_pieces(terms):
    """Two-piece elements over the whole K = 768 (the unit is 2^9 where two such elements meet: a lo.lo wrongly added is 2^-9 of it)."""
    from vfa_amd import ops
    case = pc.collapse_two_piece("bf3")
    pc.assert_exact_case(case, claims=("A1", "B1"))
    pc.report_equal(ops.collapse_gemm(_dev(case.A.x.T), _dev(case.B.x.T), terms=terms), _want(case), case.name)


@pytest.mark.parametrize("offset", [0, 120, 500, 744])
def test_collapse_product_keeps_four_products_at_terms_4(offset):
    """Two-piece elements on a window (the unit is 1); the same operands at terms = 3 must give the three-product sum."""
    from vfa_amd import ops
    case = pc.collapse_two_piece("bf4", offset=offset)
    pc.assert_exact_case(case, claims=("A1", "B1"))
    vox, w = _dev(case.A.x.T), _dev(case.B.x.T)
    pc.report_equal(ops.collapse_gemm(vox, w, terms=4), _want(case), case.name)
    three = pc.Case(case.name + " at terms 3", case.A, case.B, "bf3", multi=True)
    pc.assert_exact_case(three)
    assert not np.array_equal(pc.expected(three), pc.expected(case))
    pc.report_equal(ops.collapse_gemm(vox, w, terms=3), _want(three), three.name)


# ---- ops.collapse_relu_sum, ops.collapse_gemm_relu_backward ---------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [3, 4])
@pytest.mark.parametrize("n,M", pc.RELU_SUM_CASES)
def test_relu_sum_over_views_of_integers_is_exact(n, M, terms):
    """sum_v relu(vox_v w^T + b) on integers with an integer bias, 30-70 % of the pre-activations negative and some exactly 0; the
    sum over views stays inside the budget; accumulated onto an integer map with and without bias."""
    from vfa_amd import ops
    case, bias = pc.relu_sum_single(n, M, pc.form_of_terms(terms))
    base = np.random.default_rng(n + M).integers(-500, 501, (M, 256)).astype(np.float64)
    pc.assert_exact_case(case)
    pc.assert_epilogue_exact(case, n, M, bias, base)
    vox, w, b = _dev(case.A.x.T).view(n, M, 256), _dev(case.B.x.T), _dev(bias)
    lin = pc.expected(case)
    pc.report_equal(ops.collapse_relu_sum(vox, w, b, terms=terms), pc.f32(pc.relu_sum_observe(n, M, bias)(lin)), case.name)
    for bb, bv in ((b, bias), (None, 0.0 * bias)):
        acc = _dev(base)
        ops.collapse_relu_sum(vox, w, bb, out=acc, accumulate=True, terms=terms)
        pc.report_equal(acc, pc.f32(pc.relu_sum_observe(n, M, bv, base)(lin)), case.name + ", accumulated")


def _check_relu_sum(case, n, M, bias, base, terms):
    from vfa_amd import ops
    vox, w, b = _dev(case.A.x.T).view(n, M, 256), _dev(case.B.x.T), _dev(bias)
    lin = pc.expected(case)
    pc.report_equal(ops.collapse_relu_sum(vox, w, b, terms=terms), pc.f32(pc.relu_sum_observe(n, M, bias)(lin)), case.name)
    if base is not None:
        acc = _dev(base)
        ops.collapse_relu_sum(vox, w, b, out=acc, accumulate=True, terms=terms)
        pc.report_equal(acc, pc.f32(pc.relu_sum_observe(n, M, bias, base)(lin)), case.name + ", accumulated")


@pytest.mark.parametrize("offset", pc.RELU_SUM_WINDOWS)
@pytest.mark.parametrize("terms", [3, 4])
def test_relu_sum_keeps_the_piece_products_of_its_terms(terms, offset):
    """vfa_collapse.hip has its own split, LDS planes and product sequence: two-piece vox and weight rows on a window of K beside
    single-piece ones, at terms 3 (hi.lo, hi.hi, lo.hi) and 4 (+ lo.lo) -- the two expected values differ --, three views, accumulated
    onto a map; bias and map are multiples of the coarsest unit."""
    form = pc.form_of_terms(terms)
    case, bias, base = pc.relu_sum_two_piece(form, offset)
    pc.assert_exact_case(case, claims=("A1", "B1"))
    pc.assert_epilogue_exact(case, 3, 33, bias, base)
    other = pc.Case(case.name, case.A, case.B, "bf3" if form == "bf4" else "bf4", multi=True)
    assert not np.array_equal(pc.relu_sum_observe(3, 33, bias)(pc.expected(other)), pc.relu_sum_observe(3, 33, bias)(pc.expected(case)))
    _check_relu_sum(case, 3, 33, bias, base, terms)


@pytest.mark.parametrize("terms", [3, 4])
def test_relu_sum_sign_is_decided_by_the_kept_piece_products(terms):
    """The operands of the mask test (bias at minus a whole number of terms: 3 of 8 pre-activations exactly 0) through the fused sum."""
    case, bias = pc.mask_two_piece(pc.form_of_terms(terms))
    pc.assert_exact_case(case, extra=np.broadcast_to(bias, (80, 256)), claims=("A1", "B1"))
    pc.assert_epilogue_exact(case, 2, 40, bias)
    _check_relu_sum(case, 2, 40, bias, None, terms)


def _check_backward(case, n, M, bias, **kw):
    from vfa_amd import ops
    K = case.R
    gout = pc.backward_gout(M)
    want = pc.mask_observe(n, M, bias, gout)(pc.expected(case))
    glin, gb = ops.collapse_gemm_relu_backward(_dev(case.A.x.T).view(n, M, K), _dev(case.B.x.T), _dev(bias), _dev(gout), deterministic=False, **kw)
    pc.report_equal(glin, pc.f32(want), case.name + ": d lin")
    pc.report_equal(gb, pc.f32(want.sum(axis=(0, 1))), case.name + ": d b")  # (atomics over integers: |d b| <= 15 n M, far inside 2^24)
    pre = pc.expected(case).reshape(n, M, -1) + bias
    return float((pre == 0).mean()), float((pre < 0).mean())


@pytest.mark.parametrize("terms", [3, 4])
@pytest.mark.parametrize("n,M", [(n, M) for n, M in pc.RELU_SUM_CASES if M >= 32])
def test_relu_backward_of_integers_is_exact(n, M, terms):
    """d lin = d out [lin + b > 0] with lin the exact product (pre-activations exactly 0 mask), d b the exact column sums -- on the
    operands of the forward test (cells >= 32: the entry point's own limit)."""
    case, bias = pc.relu_sum_single(n, M, pc.form_of_terms(terms))
    pc.assert_exact_case(case)
    pc.assert_epilogue_exact(case, n, M, bias)
    _check_backward(case, n, M, bias, terms=terms)


@pytest.mark.parametrize("K", pc.BACKWARD_CHUNKS)
def test_relu_backward_of_integers_is_exact_over_many_chunks(K):
    case, bias, n, M = pc.backward_chunks(K)
    pc.assert_exact_case(case, extra=np.broadcast_to(bias, (n * M, 256)))
    _check_backward(case, n, M, bias, terms=3)


@pytest.mark.parametrize("form", ["bf3", "bf4", "f16"])
def test_relu_mask_is_decided_by_the_kept_piece_products(form):
    """Two-piece operands with the bias at minus a whole number of terms: 3 of 8 pre-activations are exactly 0, and a piece product
    lost or added would decide their sign (tests/product_common.py: mask_two_piece).  The fp16 form is the product of the fused frame
    kernels (two fp16 pieces under power-of-two scales, the bias in the accumulator), reached through the feature statistic."""
    case, bias = pc.mask_two_piece(form)
    n, M = 2, 40
    pc.assert_exact_case(case, extra=np.broadcast_to(bias / case.scale, (n * M, 256)), claims=("A1", "B1"))
    if form == "f16":
        absmax = torch.tensor([int(np.float32(2.0 ** pc.EXP_A).view(np.uint32))], dtype=torch.int32, device=DEV)
        zero, neg = _check_backward(case, n, M, bias, absmax=absmax)
    else:
        zero, neg = _check_backward(case, n, M, bias, terms=4 if form == "bf4" else 3)
    assert zero > 0.25 and neg > 0.2, (zero, neg)


# ---- ops.lateral_conv, ops.lateral_convs ----------------------------------------------------------------------------------------------
def _lateral_inputs(case, bias, K, shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    feat = _dev(case.A.x.reshape(K, n, h * w).transpose(1, 0, 2)).view(n, K, h, w)
    gamma, beta = (torch.randn(256, generator=g) * 0.5 + 1.0).to(DEV), (torch.randn(256, generator=g) * 0.2).to(DEV)
    return feat, _dev(case.B.x.T), _dev(bias), gamma, beta, 1e-5


def _lateral_want(case, bias, shape):
    n, h, w = shape
    return pc.f32((pc.expected(case) + bias).reshape(n, h, w, 256))


def _check_affine(y, gamma, beta, scale, shift, what):
    want_scale, want_shift = pc.group_norm_affine(y.double().numpy().reshape(y.shape[0], -1, 256), gamma.cpu().numpy(), beta.cpu().numpy(), 1e-5)
    for name, got, want in (("scale", scale, want_scale), ("shift", shift, want_shift)):
        apart = pc.ulps_apart(got.cpu().numpy(), want)
        print(f"[ulp] {what} {name}: {int((apart != 0).sum())} of {apart.size} elements differ from the float64 restatement, at most {int(apart.max())} ulp")
        assert apart.max() <= 1, (what, name, int(apart.max()))


@pytest.mark.parametrize("K,shape", [(K, s) for K in (128, 256, 512) for s in pc.LATERAL_SHAPES] + [(128, pc.LATERAL_TWO_BLOCKS)])
def test_lateral_convolution_of_integers_is_exact(K, shape):
    """y = the exact product + the integer bias; scale and shift equal the float64 restatement of the kernel's own formula from the
    exact integer group sums, rounded to float32, to one ulp.  The largest map gives a workgroup two 32-pixel blocks."""
    from vfa_amd import ops
    case, bias = pc.lateral_single(K, shape)
    pc.assert_exact_case(case, extra=np.broadcast_to(bias, (case.pa[0].shape[1], 256)))
    args = _lateral_inputs(case, bias, K, shape, K)
    y, scale, shift = ops.lateral_conv(*args)
    want = _lateral_want(case, bias, shape)
    pc.report_equal(y, want, case.name)
    _check_affine(want, args[3], args[4], scale, shift, case.name)


@pytest.mark.parametrize("K,offset", [(K, o) for K in (128, 256, 512) for o in pc.lateral_windows(K)])
def test_lateral_convolution_keeps_its_six_piece_products(K, offset):
    """The multi-piece window moves over all the 16-deep chunks of K."""
    from vfa_amd import ops
    shape = (2, 3, 5)
    case, bias = pc.lateral_multi(K, offset, shape)
    pc.assert_exact_case(case, extra=np.broadcast_to(bias, (case.pa[0].shape[1], 256)), claims=("A1", "A2", "B1", "B2"))
    y, _, _ = ops.lateral_conv(*_lateral_inputs(case, bias, K, shape, K))
    pc.report_equal(y, _lateral_want(case, bias, shape), case.name)


def test_batched_lateral_launch_is_exact_and_equals_the_single_calls():
    from vfa_amd import ops
    branches, wants = [], []
    for K, shape, off in ((128, (2, 12, 20), None), (256, (2, 3, 5), 48), (512, (2, 3, 5), None)):
        case, bias = pc.lateral_single(K, shape) if off is None else pc.lateral_multi(K, off, shape)
        pc.assert_exact_case(case, extra=np.broadcast_to(bias, (case.pa[0].shape[1], 256)))
        branches.append(_lateral_inputs(case, bias, K, shape, K))
        wants.append((_lateral_want(case, bias, shape), case))
    for b, got, (want, case) in zip(branches, ops.lateral_convs(branches), wants):
        single = ops.lateral_conv(*b)
        pc.report_equal(got[0], want, case.name + ", batched")
        for g, s in zip(got, single):
            assert torch.equal(g, s), case.name
        if not case.multi:
            _check_affine(want, b[3], b[4], got[1], got[2], case.name + ", batched")
