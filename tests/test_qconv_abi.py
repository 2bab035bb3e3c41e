"""Calibrated int8 convolution without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h), the plan query, the
Python face (Module.quantize_static_conv), the numpy restatement itself (tests/qconv_ref.py) against float64 and against the int32 range
the kernel's exact sums rest on, and the coverage of the GPU test's case table, asserted through the plan the launch consumes."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import qconv_ref as Q
from tests import qstatic_ref as R

f32 = np.float32


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS
    for name, nargs in (("th_quantize_act_nhwc_int8", 10), ("th_pack_conv_weight_int8", 8), ("th_pack_conv_weight_taper_int8", 8), ("th_qconv_i8_cpitch", 1), ("th_conv2d_q8q8_fwd", 22),
                        ("th_debug_qconv_plan", 12)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS
    for name, nargs in (("tp_module_quantize_static_conv", 4), ("tp_module_quantize_static", 4)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name


def test_plan_query_is_a_debug_hook_and_refuses_nonsense():
    from taper_amd._lib import INCLUDE, hip, parse_header
    assert "th_debug_qconv_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_qconv_plan" not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    out = (C.c_int * 8)()
    ptr = C.cast(out, C.c_void_p)
    good = [2, 16, 9, 9, 32, 3, 3, 1, 1, 1, 1]      # n, c_in, h, w, c_out, k_h, k_w, s_h, s_w, pad_h, pad_w
    assert hip.th_debug_qconv_plan(*good, ptr) == 0
    for i, v in ((0, 0), (1, 0), (2, 0), (3, -1), (4, 0), (5, 0), (6, 0), (7, 0), (8, -2), (9, -1), (10, -1), (5, 12), (6, 12), (1, 7282)):
        bad = list(good)
        bad[i] = v
        assert hip.th_debug_qconv_plan(*bad, ptr) != 0 and b"th_debug_qconv_plan" in hip.th_last_error(), bad
    assert hip.th_debug_qconv_plan(1, 4096, 4, 4, 1, 4, 4, 1, 1, 0, 0, ptr) == 0      # c_in k_h k_w = 65536 is the last shape taken
    assert hip.th_debug_qconv_plan(1, 4097, 4, 4, 1, 4, 4, 1, 1, 0, 0, ptr) != 0
    assert hip.th_debug_qconv_plan(*good, None) != 0
    assert [hip.th_qconv_i8_cpitch(c) for c in (1, 15, 16, 17, 64, 65)] == [16, 16, 16, 32, 64, 80]


def test_plan_invariants_over_a_grid():
    from tests.test_gpu_qconv import plan
    forms = set()
    for n in (1, 3, 256):
        for c_in in (1, 16, 64):
            for h, w in ((1, 1), (7, 5), (28, 28)):
                for c_out in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000):
                    for k, s, pad in (((1, 1), (1, 1), (0, 0)), ((3, 3), (1, 1), (1, 1)), ((3, 2), (2, 1), (2, 1)), ((5, 5), (2, 2), (2, 2))):
                        p = plan(n, c_in, h, w, c_out, k, s, pad)
                        ho, wo = Q.out_hw(h, w, k, s, pad)
                        assert (p["h_out"], p["w_out"]) == (ho, wo)
                        assert p["nt"] == (1 if c_out <= 32 else 2 if c_out <= 64 else 4), (c_out, p)      # by c_out alone
                        assert p["tile_m"] % 32 == 0 and p["tile_n"] == 32 * p["nt"]
                        assert p["tiles_m"] == -(-n * ho * wo // p["tile_m"]) and p["tiles_n"] == -(-c_out // p["tile_n"])
                        assert p["grid"] == p["tiles_m"] * p["tiles_n"]
                        assert p["tile_n"] < 2 * c_out + 32      # no form wastes more than half its channels beyond the 32 of an MFMA tile
                        forms.add(p["nt"])
    assert forms == {1, 2, 4}


def test_case_table_covers_every_form_and_its_edges():
    from tests.test_gpu_qconv import CASES, plan
    rows = [(c, plan(*c)) for c in CASES]
    assert len(set(CASES)) == len(CASES)

    def some(what, pred, among=rows):
        assert any(pred(c, p) for c, p in among), what

    M = lambda c, p: c[0] * p["h_out"] * p["w_out"]      # noqa: E731
    some("one short of whole pixel tiles", lambda c, p: M(c, p) % p["tile_m"] == p["tile_m"] - 1)
    some("exactly a pixel tile", lambda c, p: M(c, p) == p["tile_m"])
    some("whole pixel tiles, more than one", lambda c, p: M(c, p) % p["tile_m"] == 0 and M(c, p) > p["tile_m"])
    some("one past whole pixel tiles", lambda c, p: M(c, p) % p["tile_m"] == 1 and M(c, p) > p["tile_m"])
    some("several pixel tiles", lambda c, p: p["tiles_m"] >= 3)
    some("a tile that spans two images", lambda c, p: c[0] > 1 and (p["h_out"] * p["w_out"]) % p["tile_m"] != 0)
    some("a tile that spans three images", lambda c, p: c[0] > 2 and 2 * p["h_out"] * p["w_out"] < p["tile_m"])
    some("a tile that spans map rows", lambda c, p: p["h_out"] > 1 and p["w_out"] % p["tile_m"] != 0)
    some("a single output channel", lambda c, p: c[4] == 1)
    some("several channel tiles", lambda c, p: p["tiles_n"] >= 3)
    some("one past a channel tile", lambda c, p: c[4] % p["tile_n"] == 1 and c[4] > p["tile_n"])
    assert {p["nt"] for _, p in rows} == {1, 2, 4}, "every tile form the plan can choose"
    for nt in (1, 2, 4):      # each form: one short of its channel tile, exactly it, and more than one pixel tile
        form = [(c, p) for c, p in rows if p["nt"] == nt]
        some(f"nt {nt}: one short of a channel tile", lambda c, p: c[4] % p["tile_n"] == p["tile_n"] - 1, form)
        some(f"nt {nt}: exactly a channel tile", lambda c, p: c[4] % p["tile_n"] == 0, form)
        some(f"nt {nt}: the first count that takes this form", lambda c, p: c[4] == (1 if nt == 1 else 16 * nt + 1), form)
        some(f"nt {nt}: more than one pixel tile", lambda c, p: p["tiles_m"] > 1, form)
    assert {c[1] for c in CASES} >= {1, 3, 15, 16, 17, 32, 64}
    assert {c[5] for c in CASES} >= {(1, 1), (3, 3), (5, 5), (3, 2)}
    assert {c[6] for c in CASES} >= {(1, 1), (2, 2), (2, 1)}
    assert {v for c in CASES for v in c[7]} >= {0, 1, 2}
    some("padding k - 1", lambda c, p: c[7] == (c[5][0] - 1, c[5][1] - 1) and c[5] != (1, 1))
    some("h != w", lambda c, p: c[2] != c[3])
    some("pad_h != pad_w", lambda c, p: c[7][0] != c[7][1])
    some("K pieces that are no whole number of stages", lambda c, p: (c[5][0] * c[5][1] * Q.cpitch(c[1]) // 16) % 4 != 0)
    some("a stage that spans taps", lambda c, p: Q.cpitch(c[1]) < 64 and c[5] != (1, 1))
    for c, p in rows:      # small: the edges need no more
        assert c[2] <= 16 and c[3] <= 17 and M(c, p) <= 640, c


def test_python_face():
    import taper_amd as T
    assert list(inspect.signature(T.Module.quantize_static_conv).parameters) == ["self", "calib"]
    assert list(inspect.signature(T.Module.quantize_static).parameters) == ["self", "calib"]      # unchanged


SHAPES = [(2, 32, 9, 9, 33, 3, 1, 1), (3, 1, 12, 12, 4, 3, 1, 0), (1, 64, 7, 7, 128, 3, 1, 1), (2, 17, 10, 7, 31, 5, 2, 2), (4, 16, 8, 8, 32, 1, 1, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_reference_is_within_1e6_of_float64_on_the_same_operands(shape):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), b ~ 0.1 N(0, 1), seed 0: four f32 roundings per output against the float64 product of the
    decoded operands (the Linear restatement's bound; measured 1.5e-7 to 2.6e-7 of max |y| on the five shapes)"""
    rng = np.random.default_rng(0)
    for sh in SHAPES:      # one stream, the shapes in the issue's order
        n, c_in, h, w, c_out, k, s, p = sh
        x, wt, bias = Q.float_layer(rng, n, c_in, h, w, c_out, (k, k))
        if sh == shape:
            break
    sx = R.act_scale_of(x)
    qx, ps = Q.quantize_act_nchw(x, sx)
    qw, wp = R.pack(wt)
    qb, bp = R.pack(bias)
    y = Q.conv_q8q8(qx, sx, qw, wp, qb, bp, (s, s), (p, p))
    y64 = Q.float64_conv(qx, sx, qw, wp, qb, bp, (s, s), (p, p))
    err = float(np.abs(y - y64).max() / np.abs(y64).max())
    print(f"reference vs float64 at {shape}: {err:.3e} of max |y|")
    assert y.dtype == np.float32 and y.shape == (n, c_out) + Q.out_hw(h, w, (k, k), (s, s), (p, p)) and err <= 1e-6, err
    np.testing.assert_array_equal(ps, qx.astype(np.int64).sum(axis=1))
    assert np.abs(qx.astype(int)).max() == 127      # the scale comes from this tensor: its extreme takes the code +-127


def test_restatement_is_a_direct_convolution():
    """the im2col agrees with a direct window sum, border windows included (integer codes, exact either way)"""
    rng = np.random.default_rng(3)
    qx = rng.integers(-128, 128, (2, 3, 6, 5)).astype(np.int8)
    qw = rng.integers(-128, 128, (4, 3, 3, 2)).astype(np.int8)
    stride, pad = (2, 1), (2, 1)
    y = Q.conv_q8q8(qx, 1.0, qw, (0.0, 1.0), stride=stride, pad=pad)
    ho, wo = Q.out_hw(6, 5, (3, 2), stride, pad)
    for b in range(2):
        for co in range(4):
            for oh in range(ho):
                for ow in range(wo):
                    t = 0
                    for kh in range(3):
                        for kw in range(2):
                            ih, iw = oh * stride[0] - pad[0] + kh, ow * stride[1] - pad[1] + kw
                            if 0 <= ih < 6 and 0 <= iw < 5:
                                t += int((qx[b, :, ih, iw].astype(int) * (qw[co, :, kh, kw].astype(int) + 128)).sum())
                    assert y[b, co, oh, ow] == t
    np.testing.assert_array_equal(Q.nhwc(qx, 16)[1, 2, 3, :3], qx[1, :, 2, 3])
    np.testing.assert_array_equal(Q.pack_weight(qw, 16)[2, 1 * 2 + 1, :3], qw[2, :, 1, 1])
    assert Q.taper_weight(qw, 4, 3, (3, 2))[2, 1, 2, 1] == qw.reshape(-1)[((1 * 3 + 2) * 2 + 1) * 4 + 2]      # w_eff[co][k] = flat[k c_out + co]
    assert not Q.nhwc(qx, 16)[..., 3:].any() and not Q.pack_weight(qw, 16)[..., 3:].any()


@pytest.mark.parametrize("cx", [-128, 127])
def test_integer_terms_stay_inside_int32_at_the_largest_window(cx):
    qx, qw = np.full((1, 4096, 4, 4), cx, np.int8), np.full((2, 4096, 4, 4), 127, np.int8)      # c_in k_h k_w = 65536
    t, rs = R.int_terms(Q.im2col(qx, (4, 4), (1, 1), (0, 0)), qw.reshape(2, -1))
    assert (t == cx * 255 * Q.MAX_K).all() and (rs == cx * Q.MAX_K).all()
    assert -2 ** 31 <= t.min() and t.max() < 2 ** 31
    np.testing.assert_array_equal(Q.conv_q8q8(qx, 1.0, qw, (0.0, 1.0)), np.float32(cx * 255 * Q.MAX_K))
