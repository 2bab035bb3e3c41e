"""Calibrated int8 inference without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h), the Python face
(Module.quantize_static, QuantizedModule.act_scales) and the numpy restatement itself (tests/qstatic_ref.py) against float64 and
against the int32 range the kernel's exact sums rest on."""
import inspect

import numpy as np
import pytest

from tests import qstatic_ref as R


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS
    for name, nargs in (("th_quantize_act_int8", 8), ("th_pad_rows_int8", 6), ("th_linear_q8q8_fwd", 15), ("th_qlinear_i8_kstep", 0),
                        ("th_act_range_update", 6)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS
    for name, nargs in (("tp_module_quantize_static", 4), ("tp_qmodule_act_scales", 4)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name


def test_plan_query_is_a_debug_hook_and_refuses_nonsense():
    import ctypes as C

    from taper_amd._lib import INCLUDE, hip, parse_header
    assert "th_debug_q8q8_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_q8q8_plan" not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    out = (C.c_int * 4)()
    ptr = C.cast(out, C.c_void_p)
    assert hip.th_debug_q8q8_plan(1, 128, 10, ptr) == 0
    for bad in ((0, 128, 10), (1, 0, 10), (1, 128, 0), (1, 65537, 10)):
        assert hip.th_debug_q8q8_plan(*bad, ptr) != 0 and b"th_debug_q8q8_plan" in hip.th_last_error(), bad
    assert hip.th_debug_q8q8_plan(1, 128, 10, None) != 0


def test_plan_invariants_over_a_grid():
    from tests.test_gpu_qstatic import plan
    switch = max(B for B in range(1, 4097) if plan(B, 64, 64)["skinny"])
    for B in (1, 31, 32, 33, switch - 1, switch, switch + 1, 2 * switch, 4096, 100000):
        for N in (1, 31, 32, 33, 127, 128, 129, 4096, 100000):
            for K in (1, 64, 65536):
                p = plan(B, K, N)
                ts = 32 if p["skinny"] else 128
                assert p["skinny"] == (1 if B <= switch else 0), (B, K, N, p)      # by the batch alone
                assert p["tiles_m"] == -(-B // ts) and p["tiles_n"] == -(-N // ts) and p["grid"] == p["tiles_m"] * p["tiles_n"], (B, K, N, p)


def test_case_table_covers_both_forms_and_their_edges():
    from tests.test_gpu_qstatic import CASES, plan
    switch = max(B for B in range(1, 4097) if plan(B, 64, 64)["skinny"])
    assert {switch, switch + 1} <= {c[0] for c in CASES}, "the table must stand on both sides of the switch between the forms"
    for form, ts in ((1, 32), (0, 128)):
        rows = [c for c in CASES if plan(c[0], c[2], c[1])["skinny"] == form]

        def some(what, pred):
            assert any(pred(*c) for c in rows), (form, what)

        some("a whole number of row tiles, more than one", lambda M, N, K: M % ts == 0 and M > ts)
        some("one row past whole row tiles", lambda M, N, K: M % ts == 1 and M > ts)
        some("one row short of whole row tiles", lambda M, N, K: M % ts == ts - 1)
        some("a whole number of column tiles", lambda M, N, K: N % ts == 0)
        some("one column past whole column tiles", lambda M, N, K: N % ts == 1 and N > ts)
        some("one column short of a column tile", lambda M, N, K: N % ts == ts - 1)
        some("a single column", lambda M, N, K: N == 1)
        some("several row and column tiles at once", lambda M, N, K: M > ts and N > ts)
        for K in (1, 15, 16, 63, 64, 65, 784, 4112):      # below a piece, a piece, around the K step, 12 and 64 steps + a 16-byte tail
            some(f"K = {K}", lambda M, N, k: k == K)
    skinny = [c for c in CASES if plan(c[0], c[2], c[1])["skinny"]]
    assert any(-(-K // 64) < 4 for _, _, K in skinny) and any(-(-K // 64) > 16 for _, _, K in skinny)      # idle waves; more than one trip a wave


def test_the_k_step_is_a_multiple_of_the_code_load():
    from taper_amd._lib import hip
    assert hip.th_qlinear_i8_kstep() > 0 and hip.th_qlinear_i8_kstep() % 16 == 0


def test_python_face():
    import taper_amd as T
    assert list(inspect.signature(T.Module.quantize_static).parameters) == ["self", "calib"]
    assert list(inspect.signature(T.QuantizedModule.act_scales).parameters) == ["self"]
    assert list(inspect.signature(T.Module.quantize).parameters) == ["self", "qtype", "enabled"]      # unchanged
    assert set(T.QuantizedModule.QTYPES) == {"int8", "float16", "int4", "bfloat16", "nf4"}


@pytest.mark.parametrize("B,K,N", [(5, 784, 128), (33, 100, 10), (130, 4096, 70)])
def test_reference_is_within_1e6_of_float64_on_the_same_operands(B, K, N):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), b ~ 0.1 N(0, 1), seed 0: four f32 roundings per output against the float64 product of the
    decoded operands (measured 2.0e-7, 1.6e-7 and 3.0e-7 of max |y|)"""
    rng = np.random.default_rng(0)
    for b, k, n in ((5, 784, 128), (33, 100, 10), (130, 4096, 70)):      # one stream, the shapes in the issue's order
        x, w, bias = R.float_layer(rng, b, k, n)
        if (b, k, n) == (B, K, N):
            break
    sx = R.act_scale_of(x)
    qx, rs = R.quantize_act(x, sx)
    qw, wp = R.pack(w)
    qb, bp = R.pack(bias)
    y, y64 = R.linear_q8q8(qx, sx, qw, wp, qb, bp), R.float64_linear(qx, sx, qw, wp, qb, bp)
    err = float(np.abs(y - y64).max() / np.abs(y64).max())
    print(f"reference vs float64 at {(B, K, N)}: {err:.3e} of max |y|")
    assert y.dtype == np.float32 and err <= 1e-6, err
    np.testing.assert_array_equal(rs, qx.astype(np.int64).sum(axis=1))
    assert np.abs(qx.astype(int)).max() == 127      # the scale comes from this tensor: its extreme takes the code +-127


@pytest.mark.parametrize("cx", [-128, 127])
def test_integer_terms_stay_inside_int32_at_the_largest_k(cx):
    qx, qw = np.full((2, R.MAX_K), cx, np.int8), np.full((3, R.MAX_K), 127, np.int8)
    t, rs = R.int_terms(qx, qw)
    assert (t == cx * 255 * R.MAX_K).all() and (rs == cx * R.MAX_K).all()
    assert -2 ** 31 <= t.min() and t.max() < 2 ** 31
    y = R.linear_q8q8(qx, 1.0, qw, (0.0, 1.0))
    np.testing.assert_array_equal(y, np.float32(cx * 255 * R.MAX_K))


def test_codes_follow_the_fake_quant_rounding():
    x = np.array([[0.5, -0.5, 1.5, -1.5, 2.4999, 126.5, 127.5, -128.5, -129.0, np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0]], np.float32)
    q, rs = R.quantize_act(x, 1.0)
    np.testing.assert_array_equal(q[0], [1, -1, 2, -2, 2, 127, 127, -128, -128, 0, 127, -128, 127, -128, 0, 0])
    assert rs[0] == q[0].astype(int).sum()
    assert R.act_scale(0, 0) == np.float32(1) / np.float32(127)
    assert R.act_scale(2, 2) == np.float32(np.float32(2) * np.float32(1.1)) / np.float32(127)
    assert R.act_scale(-3, 1) == np.float32(3) / np.float32(127)
