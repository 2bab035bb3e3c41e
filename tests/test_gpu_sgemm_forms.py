"""Every kernel form of csrc/gemm.hip (th_sgemm, th_linear_fwd) against an exact reference, compared on bits.

WHICH form a row of the case table takes is asserted, not assumed: tests/test_sgemm_plan.py checks through th_debug_sgemm_plan (the host
function gemm_dispatch itself launches from) that tests/sgemm_ref.py's table reaches every form the dispatch can produce.  The operands are
small integers (tests/sgemm_ref.py), so numpy's float64 product is exact and every summation order gives its float32 bits: there is no
tolerance.  Beyond the bits of C each case checks
  * unwritten tiles: with beta == 0 C starts as NaN, and a hole in a tile map stays one;
  * writes outside C: C lies inside a larger buffer whose margins (256 words either side) hold a bit pattern that must come back;
  * reads outside the operands: A and B lie inside larger buffers whose margins are NaN -- clamped loads, the ragged-DMA range and the k
    tail of the last slice must select or zero what lies outside, never multiply it by zero.
Misaligned pointers (DevBuf.offset) are what the library's own callers pass: arena offsets."""
import numpy as np
import pytest

from tests import sgemm_ref as R
from tests.gpu_guard import Out, in_use as _in_use, operand as _operand
from tests.sgemm_ref import f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _sgemm(ctx, case, pa, pb, alpha, beta, c0, ref, what):
    ta, tb, m, n, k = case[:5]
    out = Out(ctx, m, n, case[7], None if beta == 0.0 else c0)
    ctx.call("th_sgemm", ta, tb, m, n, k, alpha, pa, pb, beta, out.ptr)
    return out.check(ref, what)


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_sgemm_exact(ctx, case):
    """C on bits under all three (alpha, beta), NaN around the operands, guard words around C, the pool back where it was"""
    ta, tb, m, n, k, ao, bo, co = case
    p = R.plan(*case)
    a, b, c0, _ = R.operands(case)
    prod = R.product64(case, a, b)
    ba, pa = _operand(ctx, a, ao)
    bb, pb = _operand(ctx, b, bo)
    assert (pa % 16, pb % 16) == (ao, bo)
    used = _in_use(ctx)
    for alpha, beta in R.ALPHA_BETA:
        _sgemm(ctx, case, pa, pb, alpha, beta, c0, R.epilogue(prod, alpha, beta, c0), f"{R.form_name(R.form_of(*case))} {p} alpha={alpha} beta={beta}")
    assert _in_use(ctx) == used      # the K slices' workspace went back


# one NT case per (tile class, load form, split, map, reduce kernel), and the split products whose reduce quads straddle two rows of C
def _linear_cases():
    seen, out = set(), []
    for c in R.CASES:
        f = R.form_of(*c)
        if c[:2] == (0, 1) and (f[1:6] not in seen or c[2:5] in ((130, 1030, 4096), (6, 6, 2048), (2, 6, 2052))):
            seen.add(f[1:6])
            out.append(c)
    return out


LINEAR_CASES = _linear_cases()


@pytest.mark.parametrize("case", LINEAR_CASES, ids=[R.case_id(c) for c in LINEAR_CASES])
def test_linear_fwd_exact(ctx, case):
    """th_linear_fwd = the NT product with bias and ReLU in the epilogue -- of the product or of the reduce pass, whose quads index the bias
    by (i + e) % n: 130 x 1030 and 6 x 6 have m * n % 4 == 0 and n % 4 == 2, so every other quad straddles two rows"""
    _, _, m, n, k, ao, bo, co = case
    x, w, _, bias = R.operands(case)
    prod = R.product64(case, x, w)
    bx, px = _operand(ctx, x, ao)
    bw, pw = _operand(ctx, w, bo)
    db = ctx.upload(bias)
    for with_bias, relu in ((True, 1), (True, 0), (False, 1)):
        ref = R.epilogue(prod, 1.0, 0.0, None, bias if with_bias else None, bool(relu))
        if with_bias and relu and m * n >= 64:
            assert (ref == 0).any() and (ref > 0).any()      # the ReLU has something to do
        out = Out(ctx, m, n, co)
        ctx.call("th_linear_fwd", px, pw, db if with_bias else None, out.ptr, m, k, n, relu)
        out.check(ref, f"{R.form_name(R.form_of(*case))} bias={with_bias} relu={relu}")


# poison placement: once per (layout, tile class, load form), on the smallest case of the table that takes it; 16-tiles: unsplit and split,
# on more than one tile (a 1 x 1 output has no other row to keep clean)
def _poison_cases():
    best = {}
    for c in R.CASES:
        f = R.form_of(*c)[:4]
        if f[1] != 16:
            f = f[:3]
        elif c[2] < 17 or c[3] < 15 or c[4] < 17:
            continue
        if f not in best or c[2] * c[3] * c[4] < best[f][2] * best[f][3] * best[f][4]:
            best[f] = c
    return [best[f] for f in sorted(best)]


POISON_CASES = _poison_cases()


@pytest.mark.parametrize("case", POISON_CASES, ids=[R.case_id(c) for c in POISON_CASES])
def test_poison_stays_in_its_row_and_column(ctx, case):
    """One NaN in op(A) poisons exactly its row of C, one in op(B) exactly its column, at the first and at the last element (the corner
    every edge path handles: last row, last k of the last slice); every other element keeps the reference's bits.  +Inf at A[m-1, k-1] over
    a B without zeros gives a row of +/-Inf with the sign of B[k-1, j] and no NaN: a k tail or an edge row that multiplied a clamped value
    by zero instead of selecting would turn Inf into NaN."""
    ta, tb, m, n, k, ao, bo, co = case
    a, b, c0, _ = R.operands(case, b_nonzero=True, seed=1)
    opa, opb = (a.T if ta else a), (b.T if tb else b)      # views: writing op(A)[i, kk] writes A where it lies
    base = R.product64(case, a, b)
    name = R.form_name(R.form_of(*case))

    def run(what, a_=a, b_=b, row=None, col=None):
        prod = base.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            if row is not None:
                prod[row, :] = (a_.T if ta else a_)[row, :].astype(np.float64) @ opb.astype(np.float64)
            if col is not None:
                prod[:, col] = opa.astype(np.float64) @ (b_.T if tb else b_)[:, col].astype(np.float64)
        ba, pa = _operand(ctx, a_, ao)
        bb, pb = _operand(ctx, b_, bo)
        return _sgemm(ctx, case, pa, pb, 1.0, 0.0, c0, R.epilogue(prod, 1.0, 0.0), f"{name}: {what}"), prod

    for i, kk in ((m - 1, k - 1), (0, 0)):
        a2 = a.copy()
        (a2.T if ta else a2)[i, kk] = np.nan
        got, prod = run(f"NaN at A[{i}, {kk}]", a_=a2, row=i)
        assert np.isnan(prod[i]).all() and np.isnan(got[i]).all() and np.isnan(got).sum() == n
    for kk, j in ((k - 1, n - 1), (0, 0)):
        b2 = b.copy()
        (b2.T if tb else b2)[kk, j] = np.nan
        got, prod = run(f"NaN at B[{kk}, {j}]", b_=b2, col=j)
        assert np.isnan(prod[:, j]).all() and np.isnan(got[:, j]).all() and np.isnan(got).sum() == m
    a2 = a.copy()
    (a2.T if ta else a2)[m - 1, k - 1] = np.inf
    got, prod = run(f"+Inf at A[{m - 1}, {k - 1}]", a_=a2, row=m - 1)
    assert (opb != 0).all() and not np.isnan(got).any()
    np.testing.assert_array_equal(got[m - 1], np.where(opb[k - 1] > 0, np.inf, -np.inf).astype(f32), err_msg=name)


# ------------------------------------------------------------------------------------------------------------------------------ k == 0
@pytest.mark.parametrize("lay", R.LAYOUTS, ids=R.LAYOUT_NAMES.values())
def test_sgemm_k0(ctx, lay):
    """an empty product: C = beta C; beta == 0 leaves zeros without reading C (NaN going in); the operand pointers may be null"""
    ta, tb = lay
    m, n = 5, 7
    c0 = np.random.default_rng(7).integers(-8, 9, (m, n)).astype(f32)
    dummy = ctx.zeros(4)
    for pa, pb in ((dummy, dummy), (None, None)):
        out = Out(ctx, m, n, 0)
        ctx.call("th_sgemm", ta, tb, m, n, 0, 1.0, pa, pb, 0.0, out.ptr)
        out.check(np.zeros((m, n), f32), "k = 0, beta = 0")
        out = Out(ctx, m, n, 4, c0)
        ctx.call("th_sgemm", ta, tb, m, n, 0, 0.5, pa, pb, -2.0, out.ptr)
        out.check(-2 * c0, "k = 0, beta = -2")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
def test_linear_fwd_k0(ctx, with_bias, relu):
    """in_features == 0: the bias (then ReLU) in every row, zeros without one"""
    batch, out_f = 3, 5
    bias = np.array([-3, 0, 2, -8, 8], f32)
    dummy = ctx.zeros(4)
    out = Out(ctx, batch, out_f, 0)
    ctx.call("th_linear_fwd", dummy, dummy, ctx.upload(bias) if with_bias else None, out.ptr, batch, 0, out_f, relu)
    ref = np.tile(bias if with_bias else np.zeros(out_f, f32), (batch, 1))
    out.check(np.maximum(ref, 0) if relu else ref, "in_features = 0")
