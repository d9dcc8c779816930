"""The proof, on the CPU, that the equality assertions of tests/test_product_exact.py are sound and that they discriminate
(tests/product_common.py states the principle).  For every operand set the GPU tests use:

  * the preconditions hold: the restated split gives the intended pieces, every kept piece product is a multiple of the element's unit,
    the budget sum |kept piece products| is below 2^24 units (2^23 with more than one piece), the expected value is an fp32 number;
  * an fp32 accumulation per 16-deep step and per product, in several shuffled orders, EQUALS the kept-product sum;
  * every mutant kernel differs from it in at least one element: each kept product dropped, each dropped product added, a product taken
    twice in place of its mirror, a piece read from the neighbouring plane (sets with more than one piece); the last reduction index or
    ragged step omitted, a reduce part omitted, the reduction index shifted inside a step, two 32-column blocks swapped, the last output
    row not written (every set)."""
import numpy as np
import pytest

import product_common as pc


def _sets():
    """-> (id, thunk -> (case, observe, reduce parts, accumulator start[, equivalent mutants]))."""
    for K in (256, 512):
        for rows in pc.GRAD_WEIGHT_SINGLE_ROWS:
            yield f"grad_weight-{rows}-{K}", lambda rows=rows, K=K: (pc.grad_weight_single(rows, K), None, pc.grad_weight_parts(rows, K), None)
    for rows, off in pc.GRAD_WEIGHT_MULTI:
        yield f"grad_weight-multi-{rows}-{off}", lambda rows=rows, off=off: (pc.grad_weight_multi(rows, off), None, pc.grad_weight_parts(rows, 256), None)
    yield "grad_weight-multi-31-K512", lambda: (pc.grad_weight_multi(31, None, 512), None, pc.grad_weight_parts(31, 512), None)
    for K in (256, 512):
        for rows in pc.GRAD_INPUT_SINGLE_ROWS:
            yield f"grad_input-{rows}-{K}", lambda rows=rows, K=K: (pc.grad_input_single(rows, K), None, None, None)
    yield "grad_input-tall", lambda: (pc.grad_input_single(*pc.GRAD_INPUT_TALL), None, None, None)
    for off in pc.GRAD_INPUT_WINDOWS:
        yield f"grad_input-multi-{off}", lambda off=off: (pc.grad_input_multi(off), None, None, None)
    yield "grad_input-multi-K512", lambda: (pc.grad_input_multi(100, rows=257, K=512), None, None, None)
    for M, K in pc.COLLAPSE_SINGLE:
        yield f"collapse-{M}-{K}", lambda M=M, K=K: (pc.collapse_single(M, K), None, None, None)
    yield "collapse-bf3-full-K", lambda: (pc.collapse_two_piece("bf3"), None, None, None)
    for off in (0, 120, 500, 744):
        yield f"collapse-bf4-{off}", lambda off=off: (pc.collapse_two_piece("bf4", offset=off), None, None, None)

        def at_terms_3(off=off):  # (the same operands through the three-product form)
            case = pc.collapse_two_piece("bf4", offset=off)
            return pc.Case(case.name + " at terms 3", case.A, case.B, "bf3", multi=True), None, None, None
        yield f"collapse-bf4-{off}-at-terms-3", at_terms_3
    for n, M in pc.RELU_SUM_CASES:
        def relu(n=n, M=M):
            case, bias = pc.relu_sum_single(n, M)
            pc.assert_epilogue_exact(case, n, M, bias)
            # (M = 32: the first two 32-column blocks of A are the whole views 0 and 1, whose order the sum over views does not see)
            return case, pc.relu_sum_observe(n, M, bias), None, None, ("two 32-column blocks swapped (A)",) if M == 32 else ()
        yield f"relu_sum-{n}-{M}", relu
        if M >= 32:
            def relu_backward(n=n, M=M):  # (the same operands under the observable of the backward: the masked gradient)
                case, bias = pc.relu_sum_single(n, M)
                return case, pc.mask_observe(n, M, bias, pc.backward_gout(M)), None, None, ("two 32-column blocks swapped (A)",) if M == 32 else ()
            yield f"relu_backward-{n}-{M}", relu_backward
    for form in ("bf3", "bf4"):
        for off in pc.RELU_SUM_WINDOWS:
            def relu2(form=form, off=off):
                case, bias, base = pc.relu_sum_two_piece(form, off)
                pc.assert_epilogue_exact(case, 3, 33, bias, base)
                return case, pc.relu_sum_observe(3, 33, bias, base), None, None
            yield f"relu_sum-{form}-{off}", relu2
    for K in pc.BACKWARD_CHUNKS:
        def chunks(K=K):
            case, bias, n, M = pc.backward_chunks(K)
            pc.assert_exact_case(case, extra=np.broadcast_to(bias, (n * M, 256)))
            return case, pc.mask_observe(n, M, bias, pc.backward_gout(M)), None, None
        yield f"relu_backward-chunks-{K}", chunks
    for form in ("bf3", "bf4", "f16"):
        def mask(form=form):
            case, bias = pc.mask_two_piece(form)
            pc.assert_epilogue_exact(case, 1, 80, bias)
            return case, pc.mask_observe(2, 40, bias, pc.backward_gout(40)), None, np.broadcast_to(bias / case.scale, (80, 256))
        yield f"mask-{form}", mask
        if form != "f16":
            def mask_relu(form=form):  # (the same operands through the fused ReLU sum over the two views)
                case, bias = pc.mask_two_piece(form)
                pc.assert_epilogue_exact(case, 2, 40, bias)
                return case, pc.relu_sum_observe(2, 40, bias), None, np.broadcast_to(bias / case.scale, (80, 256))
            yield f"mask-{form}-relu_sum", mask_relu
    for K in (128, 256, 512):
        for shape in pc.LATERAL_SHAPES + [pc.LATERAL_TWO_BLOCKS][:K == 128]:
            yield f"lateral-{K}-{shape}", lambda K=K, shape=shape: (pc.lateral_single(K, shape)[0], None, None, None)
        for off in pc.lateral_windows(K):
            yield f"lateral-multi-{K}-{off}", lambda K=K, off=off: (pc.lateral_multi(K, off)[0], None, None, None)


SETS = dict(_sets())


@pytest.mark.parametrize("name", list(SETS))
def test_operand_set_is_exact_and_kills_every_mutant(name):
    case, observe, parts, start, *equivalent = SETS[name]()
    budget = pc.assert_exact_case(case, extra=start, claims=("A1", "B1") + (("A2", "B2") if case.form == "six" else ()) if case.multi else ())
    print(f"{case.name}: largest budget {budget:.3g} units")
    small = case
    if observe is None and case.R * case.pa[0].shape[1] * case.pb[0].shape[1] > 2e7:
        small = case.restrict(96, 96)  # (the tall sets: the proofs on a corner of the output, the preconditions above on all of it)
        start = None if start is None else start[:96, :96]
    for seed in range(3):
        assert np.array_equal(pc.emulate(small, seed, start).astype(np.float64), pc.expected(small) + (0 if start is None else start * small.scale)), seed
    left = pc.survivors(small, observe, parts, *equivalent)
    assert not left, left


def test_the_pitfall_of_independent_signs():
    """2^18 - 2^9 - 1 does NOT split into (2^18, -2^9, -1): the first piece rounds to 255 2^10 and the unit collapses.  This is why every
    piece of an element carries the element's sign, and why the pieces are computed and asserted, never assumed."""
    p0, p1, p2 = pc.pieces(np.array([2.0 ** 18 - 2.0 ** 9 - 1.0], np.float32), "six")
    assert p0[0] == 255 * 2.0 ** 10 and p0[0] + p1[0] + p2[0] == 2.0 ** 18 - 2.0 ** 9 - 1.0
    assert [p[0] for p in pc.pieces(np.array([-(2.0 ** 18 + 2.0 ** 9 + 1.0)], np.float32), "six")] == [-2.0 ** 18, -2.0 ** 9, -1.0]
    assert [p[0] for p in pc.pieces(np.array([2.0 ** 11 + 1.0], np.float32), "f16", 3)] == [2.0 ** 14, 8.0]


def test_a_budget_over_the_limit_is_refused_and_would_round():
    """The limit is what makes the assertion sound: 32 three-piece terms pass 2^23 units, and the check says so."""
    case = pc.grad_weight_multi(31, None)
    pc.assert_exact_case(case)
    rng = np.random.default_rng(0)
    A = pc.operand(rng, 40, 64, window=(0, 40), kinds="T")
    B = pc.operand(rng, 40, 64, window=(0, 40), kinds="T")
    with pytest.raises(AssertionError):
        pc.assert_exact_case(pc.Case("over", A, B, "six", multi=True))
