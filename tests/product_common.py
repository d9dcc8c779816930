"""What the exactness tests of the split-product kernels share (tests/test_product_exact_cpu.py, tests/test_product_exact.py): operands
on which the kernels' arithmetic is EXACT, so that a kernel is held to equality and no constant has to be guessed.

The kernels (vfa_grad.hip, vfa_collapse.hip, vfa_collapse_gemm.hip, vfa_lateral.hip) split both fp32 operands into bf16 or fp16 pieces
and add a fixed set of piece products with the matrix instruction, fp32 accumulation.  Every product here is stated in one canonical
shape, the reduction index first:   out[p, q] = sum_r A[r, p] B[r, q],   A (R, P), B (R, Q).

The principle.  Let every kept piece product that reaches an output element be an integer multiple of a unit 2^u, and let the element's
budget be  sum |kept piece products|  over its whole reduction.  If the budget is below 2^24 units, every partial sum -- in any order and
any grouping -- is an integer below 2^24 units: fp32 holds it exactly, round-to-nearest never rounds, and the kernel must equal the sum
of the kept products bit for bit.  Single-piece cases (integers |v| <= 15: one bf16 piece) may use the 2^24; cases with more than one
piece stay below 2^23 (one spare bit: they are the first to run the matrix instruction over a full 24-bit range).

Operand columns come in classes: T three bf16 pieces +-(2^18, 2^9, 1), D two pieces +-(2^9, 1) (fp16 form: +-(2^11, 1)), S a single
piece.  Multi-piece entries sit on a WINDOW of at most 31 reduction indices (all pieces of an element carry the element's sign: with
independent signs the split regroups them) and are zero outside it; S columns are +-1 inside the window and small integers outside.
One exception: at three products of two bf16 pieces the unit of D x D is 2^9, and collapse_two_piece("bf3") puts its two-piece
elements over the WHOLE K = 768 (its S entries are at most 3 there, so that D x S, unit 1, stays inside the budget).
Every class of A meets every class of B in some output element: T x S isolates p0q0, p1q0, p2q0, S x T p0q1, p0q2, D x D p1q1, and
T x T carries the products the six-product kernels must NOT add (p1q2, p2q1, p2q2)."""
import numpy as np

from test_split_arithmetic import EXP_A, EXP_W, split as split2_bf16, split3, split16, split_exponent

F64 = np.float64
STEP = 16                                   # reduction indices per matrix instruction
LIMIT_SINGLE, LIMIT_MULTI = 2.0 ** 24, 2.0 ** 23
SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))
THREE = ((0, 0), (0, 1), (1, 0))
# form -> (pieces per operand, kept piece products (piece of A, piece of B))
FORMS = {"six": (3, SIX), "bf3": (2, THREE), "bf4": (2, THREE + ((1, 1),)), "f16": (2, THREE)}
T3, D2, D16 = (2.0 ** 18, 2.0 ** 9, 1.0), (2.0 ** 9, 1.0), (2.0 ** 11, 1.0)


def form_of_terms(terms):
    """The product form of the collapse kernels' ``terms`` flag through vfa_collapse_gemm_f32 / vfa_collapse_relu_sum_f32 (0 and 3: three
    products of two bf16 pieces; 4: all four)."""
    return "bf4" if terms == 4 else "bf3"


def pieces(x, form, e=0):
    """The kernels' split of a float32 array, restated (test_split_arithmetic.py): float32 pieces, for the fp16 form of x 2^e."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if form == "six":
        return list(split3(x))
    if form == "f16":
        return list(split16(x, e))
    return list(split2_bf16(x))


class Operand:
    """x (R, C) float32 with the pieces its builder INTENDED, planes (n, R, C) float32 in the scaled domain (x 2^e)."""

    def __init__(self, x, planes, e=0):
        self.x, self.planes, self.e = np.ascontiguousarray(x, dtype=np.float32), planes, e

    def zero(self, rows=slice(None), cols=slice(None)):
        self.x[rows, cols] = 0.0
        self.planes[:, rows, cols] = 0.0
        return self


def operand(rng, R, C, form="six", window=None, kinds="S", s_in=1, s_out=15, e=0, density=1.0, d=None):
    """An operand whose column c has class kinds[c % len(kinds)] (shuffled): T / D entries +-(pieces) inside ``window`` = (begin, end)
    of the reduction index and zero outside, S entries +-1 .. +-s_in inside the window, integers up to s_out outside."""
    n = FORMS[form][0]
    planes = np.zeros((n, R, C), np.float32)  # (every value here is an fp32 number, and so is the sum of an element's pieces)
    planes[0] = rng.integers(-s_out, s_out + 1, (R, C), dtype=np.int8)
    if density < 1.0:
        planes[0] *= rng.random((R, C)) < density
    cls = rng.permutation(np.array(list(kinds))[np.arange(C) % len(kinds)])
    if window is not None:
        w0, w1 = window
        sign = rng.choice([-1.0, 1.0], (w1 - w0, C))
        planes[0, w0:w1] = sign * rng.integers(1, s_in + 1, (w1 - w0, C))
        for k, val in (("T", T3), ("D", d or (D16 if form == "f16" else D2))):
            cols = cls == k
            if not cols.any():
                continue
            assert len(val) <= n, (k, form)
            planes[:, :, cols] = 0.0
            for i, v in enumerate(val):
                planes[i][w0:w1, cols] = sign[:, cols] * v
    x = planes.sum(0)
    planes *= np.float32(2.0 ** e)
    op = Operand(x, planes, e)
    op.cls = cls
    return op


class Case:
    """out[p, q] = sum_r A[r, p] B[r, q] in one product form; ``multi``: some operand has more than one piece (the 2^23 limit)."""

    def __init__(self, name, A, B, form, multi=False):
        self.name, self.A, self.B, self.form, self.multi = name, A, B, form, multi
        self.n, self.kept = FORMS[form]
        self.pa, self.pb = pieces(A.x, form, A.e), pieces(B.x, form, B.e)
        self.scale = 2.0 ** -(A.e + B.e)
        self._expected = self._unit = None

    @property
    def R(self):
        return self.A.x.shape[0]

    def restrict(self, P, Q):
        """The same product on the last P / Q output rows / columns (the CPU proofs of the tall cases)."""
        A = Operand(self.A.x[:, -P:], self.A.planes[:, :, -P:], self.A.e)
        B = Operand(self.B.x[:, -Q:], self.B.planes[:, :, -Q:], self.B.e)
        return Case(self.name, A, B, self.form, self.multi)


def kept_sum(pa, pb, kept, rows=None):
    """sum over ``kept`` of pa[i]^T pb[j] in float64 (exact: integers far below 2^53), in the scaled domain."""
    out = None
    for i, j in kept:
        a, b = (pa[i], pb[j]) if rows is None else (pa[i][rows], pb[j][rows])
        if not a.any() or not b.any():
            continue
        t = a.astype(F64).T @ b.astype(F64)
        out = t if out is None else out + t
    return np.zeros((pa[0].shape[1], pb[0].shape[1]), F64) if out is None else out


def expected(case):
    """What the kernel must return: the kept-product sum (NOT the float64 product of the operands), float64."""
    if case._expected is None:
        case._expected = kept_sum(case.pa, case.pb, case.kept) * case.scale
    return case._expected


def _lowbit(p, columns=True):
    """The smallest power of two dividing every non-zero entry of a column (inf for a zero column), or of each entry; entries must
    be integers."""
    if columns and not p.any():
        return np.full(p.shape[1], np.inf)
    top = float(np.abs(p).max())
    v = np.abs(p).astype(np.int32 if top < 2.0 ** 31 else np.int64)
    assert top < 2.0 ** 53 and np.array_equal(v, np.abs(p)), "not integers"
    low = v & -v
    if columns:  # (the smallest low bit of the non-zero entries of a column)
        low = np.where(v == 0, np.iinfo(v.dtype).max, low).min(axis=0).astype(F64)
        low[low == np.iinfo(v.dtype).max] = np.inf
        return low
    low = low.astype(F64)
    low[v == 0] = np.inf
    return low


def unit_of(case, extra=None):
    """Per output element a power of two that divides every kept piece product reaching it (from the pieces' trailing zeros per
    column: a lower bound of the true unit, so the budget in units is an upper bound) and the element of ``extra``."""
    if case._unit is None:
        la, lb = [_lowbit(p) for p in case.pa], [_lowbit(p) for p in case.pb]
        case._unit = np.full((la[0].size, lb[0].size), np.inf)
        for i, j in case.kept:
            case._unit = np.minimum(case._unit, la[i][:, None] * lb[j][None, :])
    unit = case._unit.copy()
    if extra is not None:
        unit = np.minimum(unit, _lowbit(np.broadcast_to(extra, unit.shape), columns=False))
    unit[np.isinf(unit)] = 1.0
    return unit


def budget_units(case, extra=None):
    """sum |kept piece products| per output element (+ ``extra``, in the scaled domain: a bias, an accumulated map), in units."""
    b = kept_sum([np.abs(p) for p in case.pa], [np.abs(p) for p in case.pb], case.kept)
    if extra is not None:
        b = b + np.abs(extra)
    return b / unit_of(case, extra)


def fp32_representable(v):
    with np.errstate(over="ignore"):
        return bool(np.array_equal(v.astype(np.float32).astype(F64), v))


def assert_exact_case(case, extra=None, claims=()):
    """The preconditions of an equality assertion, checked on the inputs before any kernel runs: the split gives the pieces the
    builder intended (computed, never assumed) and they add up to the operand; the planes in ``claims`` ("A1", "B2", ...) are
    non-zero; the kept products are multiples of the unit (which divides ``extra``, an integer map in the scaled domain, too); the budget is under its limit; the expected value is an
    fp32 number.  -> the largest budget in units."""
    for op, got in ((case.A, case.pa), (case.B, case.pb)):
        for i in range(case.n):
            assert np.array_equal(got[i], op.planes[i]), (case.name, "piece", i)
        live = [p.astype(F64) for p in got if p.any()] or [0.0]
        assert np.array_equal(sum(live), op.x.astype(F64) * 2.0 ** op.e), (case.name, "pieces do not add up")
    for c in claims:
        assert (case.pa if c[0] == "A" else case.pb)[int(c[1])].any(), (case.name, c, "is zero")
    assert case.multi == any(p.any() for p in case.pa[1:] + case.pb[1:]), case.name
    unit = unit_of(case, extra)
    want = expected(case) / case.scale
    assert np.array_equal(np.rint(want / unit), want / unit), (case.name, "not a multiple of the unit")
    budget = budget_units(case, extra)
    limit = LIMIT_MULTI if case.multi else LIMIT_SINGLE
    assert budget.max() < limit, (case.name, float(budget.max()), limit)
    assert fp32_representable(expected(case)), case.name
    return float(budget.max())


def emulate(case, seed, start=None):
    """fp32 accumulation of the kept products, one rounding per 16-deep step and per product, in a seeded shuffled order of (step,
    product); ``start``: the accumulator's first value (scaled domain).  float32 (P, Q)."""
    rng = np.random.default_rng(seed)
    kept = [(i, j) for i, j in case.kept if case.pa[i].any() and case.pb[j].any()]
    order = [(s, k) for s in range(0, case.R, STEP) for k in range(len(kept))]
    rng.shuffle(order)
    acc = np.zeros((case.pa[0].shape[1], case.pb[0].shape[1]), np.float32) if start is None else start.astype(np.float32)
    for s, k in order:
        i, j = kept[k]
        acc = (acc.astype(F64) + case.pa[i][s:s + STEP].T.astype(F64) @ case.pb[j][s:s + STEP].astype(F64)).astype(np.float32)
    return acc * np.float32(case.scale)


def grad_weight_parts(rows, K, n_cu=256):
    """vfa_grad.hip: parts_of -- the row slabs of a launch -- and their row ranges."""
    steps = -(-rows // STEP)
    parts = max(1, min(max(1, n_cu // (K // 256)), steps, 1024))
    return [(steps * p // parts * STEP, min(steps * (p + 1) // parts * STEP, rows)) for p in range(parts)]


def _roll_in_steps(p):
    """The reduction index shifted by one inside every 16-deep step."""
    R = p.shape[0]
    pad = np.concatenate([p, np.zeros(((-R) % STEP,) + p.shape[1:], p.dtype)])
    return np.roll(pad.reshape(-1, STEP, *p.shape[1:]), 1, axis=1).reshape(pad.shape)[:R]


def _swap_blocks(p):
    q = p.copy()
    q[:, 0:32], q[:, 32:64] = p[:, 32:64], p[:, 0:32]
    return q


def piece_mutants(case):
    """-> (name, result) of kernels that are wrong in their SET of piece products or in the plane a piece is read from."""
    n, kept = case.n, list(case.kept)
    run = lambda k, pa=case.pa, pb=case.pb: kept_sum(pa, pb, k) * case.scale
    for k in kept:
        yield f"p{k[0]}q{k[1]} dropped", run([x for x in kept if x != k])
    for k in [(i, j) for i in range(n) for j in range(n) if (i, j) not in kept]:
        yield f"p{k[0]}q{k[1]} added", run(kept + [k])
    for i, j in kept:
        if i != j:
            yield f"p{i}q{j} twice, no p{j}q{i}", run([(i, j) if x == (j, i) else x for x in kept])
    for name, pcs in (("A", case.pa), ("B", case.pb)):
        for p in range(n):
            for p2 in (p - 1, p + 1):
                if 0 <= p2 < n:
                    wrong = list(pcs)
                    wrong[p] = pcs[p2]
                    yield f"{name}: plane {p} read from plane {p2}", (run(kept, pa=wrong) if name == "A" else run(kept, pb=wrong))


def structural_mutants(case, parts=None):
    """-> (name, result) of kernels that lose, shift or misplace part of the reduction or of the output."""
    R, kept, sc = case.R, case.kept, case.scale
    rows = lambda keep: kept_sum(case.pa, case.pb, kept, rows=keep) * sc
    if R > 1:
        yield "last reduction index omitted", rows(slice(0, R - 1))
    if R > STEP:
        yield "last (ragged) step omitted", rows(slice(0, (R - 1) // STEP * STEP))
    if parts is not None and len(parts) > 1:
        for p in sorted({0, len(parts) // 2, len(parts) - 1, len(parts) - 4 if len(parts) > 4 else 0}):
            keep = np.ones(R, bool)
            keep[parts[p][0]:parts[p][1]] = False
            yield f"reduce part {p} of {len(parts)} omitted", rows(keep)
    if R > 1:
        yield "reduction index shifted inside a step", kept_sum(case.pa, [_roll_in_steps(p) for p in case.pb], kept) * sc
    if case.pb[0].shape[1] >= 64:
        yield "two 32-column blocks swapped (B)", kept_sum(case.pa, [_swap_blocks(p) for p in case.pb], kept) * sc
    if case.pa[0].shape[1] >= 64:
        yield "two 32-column blocks swapped (A)", kept_sum([_swap_blocks(p) for p in case.pa], case.pb, kept) * sc
    last = expected(case).copy()
    last[-1] = 0.0
    yield "last output row not written", last


def mutants(case, parts=None):
    if case.multi:
        yield from piece_mutants(case)
    yield from structural_mutants(case, parts)


def survivors(case, observe=None, parts=None, equivalent=()):
    """The mutants whose observable result EQUALS the expected one (must be empty): ``observe`` maps the product to what the kernel
    returns (the ReLU sum over views, the masked gradient); identity by default.  ``equivalent``: mutants that are no error for this
    observable (the caller says why)."""
    observe = observe or (lambda v: v)
    want = observe(expected(case))
    return [name for name, got in mutants(case, parts) if name not in equivalent and np.array_equal(observe(got), want)]


def report_equal(got, want, what=""):
    """torch.equal with the count and the first index of differing elements in the message."""
    import torch
    got, want = got.detach().cpu(), torch.as_tensor(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape), got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | (got.isnan() != want.isnan())
    first = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {first}: got {got[first].item()!r}, "
                         f"want {want[first].item()!r}")


def f32(v):
    """An fp32-representable float64 array as a float32 torch tensor."""
    import torch
    assert fp32_representable(np.asarray(v, F64))
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))


# ---- the operand sets: one builder per kernel, used by the CPU proofs and by the GPU tests alike ---------------------------------------
GRAD_WEIGHT_SINGLE_ROWS = (1, 7, 15, 16, 17, 33, 47, 80, 208, 272, 4099, 60000)
GRAD_WEIGHT_MULTI = [(16, None), (24, None), (31, None), (4099, 0), (4099, 2040), (4099, 4075)]  # (rows, window offset)
GRAD_INPUT_SINGLE_ROWS = (1, 31, 32, 255, 256, 257, 513)
GRAD_INPUT_WINDOWS = tuple(range(0, 217, 24)) + (232,)      # 24 channels: every one of the sixteen 16-deep steps is met
GRAD_INPUT_TALL = (8193 + 77, 2048)                          # more 256-row blocks than workgroups (256 CUs / 8 K tiles), ragged end
WINDOW = 24


def grad_weight_single(rows, K, seed=0):
    """A = g_lin (rows, 256), B = vox (rows, K): integers |v| <= 15 (the tallest case |v| <= 7 for the accumulated map's sake)."""
    rng = np.random.default_rng(1000 * K + rows + seed)
    hi = 7 if rows > 10000 else 15
    return Case(f"grad_weight rows {rows} K {K}", operand(rng, rows, 256, s_out=hi), operand(rng, rows, K, s_out=hi), "six")


def grad_weight_multi(rows, offset, K=256):
    rng = np.random.default_rng(7 * rows + (offset or 0) + K)
    window = (0, rows) if offset is None else (offset, offset + WINDOW)
    A = operand(rng, rows, 256, window=window, kinds="TDS", s_out=7)
    B = operand(rng, rows, K, window=window, kinds="TDS", s_out=7)
    return Case(f"grad_weight rows {rows} window {window} K {K}", A, B, "six", multi=True)


def grad_input_single(rows, K):
    """A = g_lin^T (256, rows), B = w (256, K)."""
    rng = np.random.default_rng(2000 * K + rows)
    return Case(f"grad_input rows {rows} K {K}", operand(rng, 256, rows), operand(rng, 256, K), "six")


def grad_input_multi(offset, rows=300, K=256):
    rng = np.random.default_rng(31 * offset + rows + K)
    window = (offset, offset + WINDOW)
    A = operand(rng, 256, rows, window=window, kinds="TDS", s_out=7)
    B = operand(rng, 256, K, window=window, kinds="TDS", s_out=7)
    return Case(f"grad_input window {window} rows {rows} K {K}", A, B, "six", multi=True)


COLLAPSE_SINGLE = [(M, K) for M in (1, 31, 128, 129, 1000) for K in (256, 768, 2048)]


def _mask_rows(rng, A, M, K):
    """Masked voxels: a fifth of the rows all zero, a fifth with a zero first quarter of k (the columns of A are the rows of vox)."""
    kind = rng.random(M)
    kind[[0, -1]] = 1.0  # (the first and the last row stay live: a row the kernel loses must be one that shows)
    A.zero(cols=kind < 0.2)
    A.zero(rows=slice(0, K // 4), cols=(kind >= 0.2) & (kind < 0.4))
    return A


def collapse_single(M, K):
    """A = vox^T (K, M), B = W^T (K, 256)."""
    rng = np.random.default_rng(3000 * K + M)
    A = _mask_rows(rng, operand(rng, K, M, form="bf3"), M, K)
    return Case(f"collapse_gemm M {M} K {K}", A, operand(rng, K, 256, form="bf3"), "bf3")


def collapse_two_piece(form, M=129, K=768, offset=None):
    """Two-piece operands: over the full K where the unit allows it (three products: 2^9), on a window where it is 1 (four products)."""
    rng = np.random.default_rng(K + M + (offset or 0) + len(form))
    window = (0, K) if offset is None else (offset, offset + WINDOW)
    s_in = 3 if offset is None else 1
    A = operand(rng, K, M, form=form, window=window, kinds="DDS", s_in=s_in, s_out=7)
    if offset is None:
        _mask_rows(rng, A, M, K)
    B = operand(rng, K, 256, form=form, window=window, kinds="DDS", s_in=s_in, s_out=7)
    return Case(f"collapse_gemm {form} M {M} K {K} window {window}", A, B, form, multi=True)


RELU_SUM_CASES = [(n, M) for n in (1, 3, 7) for M in (31, 32, 33, 1000)]


def relu_sum_single(n, M, form="bf3"):
    """vox (n, M, 256) as A = vox^T (256, n M): sparse integers, W (256, 256) |w| <= 3, integer bias: 30-70 % of the pre-activations
    negative, some exactly 0.  -> (case, bias (256))."""
    rng = np.random.default_rng(4000 * n + M)
    A = operand(rng, 256, n * M, form=form, density=0.1)
    masked = rng.random(n * M) < 0.2
    masked[[0, -1]] = False
    A.zero(cols=masked)
    B = operand(rng, 256, 256, form=form, s_out=3)
    case, bias = Case(f"collapse_relu_sum views {n} M {M}", A, B, form), rng.integers(-40, 41, 256).astype(F64)
    pre = expected(case) + bias
    assert 0.3 < (pre < 0).mean() < 0.7 and (pre == 0).any(), (case.name, float((pre < 0).mean()), int((pre == 0).sum()))
    return case, bias


RELU_SUM_WINDOWS = (0, 124, 248)   # K = 256: the first step, a step boundary in the middle, the last step
RELU_SUM_WINDOW = 8                # (narrower than WINDOW: the sum over three views must stay inside the budget as well)


def relu_sum_two_piece(form, offset, n=3, M=33):
    """Two-piece vox rows and weight rows on a window of K = 256 beside single-piece ones (D x S isolates hi.lo and lo.hi, D x D the
    lo.lo that terms = 4 keeps and terms = 3 drops).  The bias and a map to accumulate onto are multiples of 2^9, the coarsest unit
    of an element (D x D at three products).  -> (case, bias (256), base (M, 256))."""
    rng = np.random.default_rng(9000 + offset + len(form))
    window = (offset, offset + RELU_SUM_WINDOW)
    A = operand(rng, 256, n * M, form=form, window=window, kinds="DDS", s_out=7)
    B = operand(rng, 256, 256, form=form, window=window, kinds="DDS", s_out=7)
    case = Case(f"collapse_relu_sum {form} window {window}", A, B, form, multi=True)
    bias = rng.integers(-40, 41, 256).astype(F64) * 2.0 ** 9
    base = rng.integers(-500, 501, (M, 256)).astype(F64) * 2.0 ** 9
    pre = expected(case) + bias
    assert 0.3 < (pre < 0).mean() < 0.7, (case.name, float((pre < 0).mean()))
    return case, bias, base


def backward_gout(M):
    """d out of the backward tests (M, 256): non-zero integers up to 15 of either sign -- a zero would hide its element of the mask."""
    rng = np.random.default_rng(M)
    return (rng.choice([-1.0, 1.0], (M, 256)) * rng.integers(1, 16, (M, 256))).astype(F64)


BACKWARD_CHUNKS = (768, 2048)      # K of the backward on many chunks: 2 views x 500 cells of collapse_single(1000, K)


def backward_chunks(K):
    """-> (case, bias, n, M): the integer operands of collapse_single(1000, K) as two views of 500 cells, with an integer bias."""
    return collapse_single(1000, K), np.random.default_rng(K).integers(-300, 301, 256).astype(F64), 2, 500


def relu_sum_observe(n, M, bias, base=None):
    def observe(lin):
        out = np.maximum(lin.reshape(n, M, -1) + bias, 0.0).sum(0)
        return out if base is None else out + base
    return observe


def mask_observe(n, M, bias, gout):
    def observe(lin):
        return np.where(lin.reshape(n, M, -1) + bias > 0, gout[None], 0.0)
    return observe


def assert_epilogue_exact(case, n, M, bias, base=None, limit=None):
    """The sum over views of relu(lin + b) (+ an accumulated map) stays inside the budget too: sum_v (budget_v + |b|) + |base|."""
    unit = unit_of(case, bias / case.scale).reshape(n, M, -1).min(0)
    total = (budget_units(case) * unit_of(case)).reshape(n, M, -1).sum(0) + n * np.abs(bias) / case.scale
    if base is not None:
        total = total + np.abs(base) / case.scale
        unit = np.minimum(unit, _lowbit(base / case.scale, columns=False))
    limit = limit or (LIMIT_MULTI if case.multi else LIMIT_SINGLE)
    assert (total / unit).max() < limit, (case.name, float((total / unit).max()))


def mask_two_piece(form, n=2, M=40, K=256, offset=232):
    """The ReLU mask of the training backward on two-piece operands.  Every vox row has three entries +-D in the window, every weight
    row is +-D on the window: lin = S T with S = the sum of three signs and T the kept sum of one term; bias = -S0 T with S0 = +-1 per
    column, so that the pre-activation is (S - S0) T: exactly 0 on 3 of 8 elements, and a lost or added piece product decides the
    sign there.  fp16 form: max |W| = 2^12 + 1 gives ew = 2, the feature statistic 2^13 gives ea = 0.  -> (case, bias)."""
    rng = np.random.default_rng(K + offset + len(form))
    d = D16 if form == "f16" else D2
    dw = (2.0 * d[0], d[1])  # (the weight's high piece is another power of two: with equal pieces p0q1 and p1q0 are the same number)
    ew = split_exponent(dw[0] + dw[1], EXP_W) if form == "f16" else 0
    ea = split_exponent(2.0 ** EXP_A, EXP_A) if form == "f16" else 0
    window = (offset, offset + WINDOW)
    A = operand(rng, K, n * M, form=form, window=window, kinds="D", s_out=0, e=ea)
    keep = np.zeros((WINDOW, n * M), bool)
    for m in range(n * M):
        keep[rng.choice(WINDOW, 3, replace=False), m] = True
    for m in np.nonzero(~keep.all(0))[0]:
        A.zero(rows=np.arange(offset, offset + WINDOW)[~keep[:, m]], cols=m)
    B = operand(rng, K, 256, form=form, window=window, kinds="D", s_out=0, e=ew, d=dw)
    case = Case(f"relu mask {form} window {window}", A, B, form, multi=True)
    term = d[0] * dw[0] + d[0] * dw[1] + d[1] * dw[0] + (d[1] * dw[1] if form == "bf4" else 0.0)
    return case, -rng.choice([-1.0, 1.0], 256) * term


LATERAL_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 13, 19), (2, 12, 20)]
LATERAL_TWO_BLOCKS = (8, 71, 115)   # vfa_lateral.hip: blocks_per_workgroup -- 8 views x 128 pairs of 32-pixel blocks: two blocks per workgroup


def lateral_single(K, shape):
    """A = feat as (K, n h w) (view-major columns), B = W^T (K, 256); integer bias.  -> (case, bias)."""
    n, h, w = shape
    rng = np.random.default_rng(5000 * K + n * h * w)
    return Case(f"lateral K {K} {shape}", operand(rng, K, n * h * w), operand(rng, K, 256), "six"), rng.integers(-50, 51, 256).astype(F64)


def lateral_multi(K, offset, shape=(2, 3, 5)):
    n, h, w = shape
    rng = np.random.default_rng(K + offset)
    window = (offset, offset + WINDOW)
    A = operand(rng, K, n * h * w, window=window, kinds="TDS", s_out=7)
    B = operand(rng, K, 256, window=window, kinds="TDS", s_out=7)
    # the bias joins the accumulator of every pixel class: a multiple of the coarsest unit its channel meets (T x T 2^18, T x D 2^9)
    step = np.where(B.cls == "T", 2.0 ** 18, np.where(B.cls == "D", 2.0 ** 9, 1.0))
    return Case(f"lateral K {K} window {window}", A, B, "six", multi=True), rng.integers(-5, 6, 256).astype(F64) * step


def lateral_windows(K):
    return tuple(range(0, K - WINDOW, WINDOW)) + (K - WINDOW,)


def group_norm_affine(y, gamma, beta, eps):
    """The kernel's own formula (vfa_lateral.hip: lateral_stats) in float64 from exact integer sums: y (n, HW, 256) integer-valued
    -> scale, shift (n, 256) float32."""
    n, HW, C = y.shape
    yi = y.astype(np.int64).reshape(n, HW, 16, C // 16)
    assert np.array_equal(yi.reshape(y.shape).astype(F64), y)
    s1, s2 = yi.sum(axis=(1, 3)), (yi * yi).sum(axis=(1, 3))
    assert np.abs(s2).max() < 2 ** 53
    count = float(HW * (C // 16))
    mean = s1.astype(F64) / count
    var = np.maximum(s2.astype(F64) / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + F64(np.float32(eps)))
    g, b = gamma.astype(F64).reshape(16, -1), beta.astype(F64).reshape(16, -1)
    scale = (g[None] * rstd[:, :, None]).astype(np.float32)
    shift = (b[None] - mean[:, :, None] * g[None] * rstd[:, :, None]).astype(np.float32)
    return scale.reshape(n, C), shift.reshape(n, C)


def ulps_apart(a, b):
    """|a - b| in float32 units in the last place (same-sign finite values or zero)."""
    ia, ib = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)
