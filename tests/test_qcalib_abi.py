"""Percentile calibration without a GPU: the C ABI declarations and exports, the TP_CALIB_* constants, the Python face, the
refusals that come before the model or the device is touched, and the numpy restatement itself (tests/qcalib_ref.py) on the outlier
Linear: one activation of 1000 among N(0, 1) makes the min / max scale useless, a 99.9 % clip does not."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import qcalib_ref as K
from tests import qstatic_ref as R

f32 = np.float32
TH = (("th_act_hist_update", 6), ("th_act_scale_from_hist", 7), ("th_act_hist_max_bins", 0))
TP = (("tp_module_quantize_static_cal", 8), ("tp_qmodule_calibration", 4))


def test_kernel_entry_points_are_declared_exported_and_prototyped():
    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    declared = parse_header(INCLUDE / "taper_hip.h")
    for name, nargs in TH:
        assert name in declared and name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert HIP_PROTOS[name][0] is C.c_int and getattr(hip, name).argtypes == HIP_PROTOS[name][1]
        assert name not in parse_header(INCLUDE / "taper_hip_debug.h")      # part of the boundary, no test hook
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    assert HIP_PROTOS["th_act_hist_update"][1] == [p, p, l, p, i, p]                # ctx x n range2 num_bins bins
    assert HIP_PROTOS["th_act_scale_from_hist"][1] == [p, p, i, p, i, p, p]         # ctx bins num_bins range2 keep_ppm scale stats4
    assert hip.th_act_hist_max_bins() == K.MAX_BINS == hip.th_obs_hist_lds_max_bins()
    assert len(HIP_PROTOS["th_act_range_update"][1]) == 6                            # unchanged


def test_host_entry_points_are_declared_exported_and_prototyped():
    from taper_amd._lib import HOST_PROTOS, INCLUDE, host, parse_header
    declared = parse_header(INCLUDE / "taper_host.h")
    for name, nargs in TP:
        assert name in declared and name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name).argtypes == HOST_PROTOS[name][1]
    p, i = C.c_void_p, C.c_int
    assert HOST_PROTOS["tp_module_quantize_static_cal"][1] == [p, p, i, i, i, i, i, p]      # m calib n flags method keep_ppm num_bins out
    assert HOST_PROTOS["tp_qmodule_calibration"][1] == [p, i, p, p]
    assert len(HOST_PROTOS["tp_module_quantize_static_ex"][1]) == 5                        # unchanged


def test_constants():
    from taper_amd import api
    from taper_amd._lib import INCLUDE
    text = (INCLUDE / "taper_host.h").read_text()
    assert "#define TP_CALIB_MINMAX 0\n" in text and "#define TP_CALIB_PERCENTILE 1\n" in text and text.count("#define TP_CALIB_") == 2
    assert text.count("#define TP_QSTATIC_") == 4
    assert (api._CALIB_MINMAX, api._CALIB_PERCENTILE) == (0, 1)


def test_python_face():
    import taper_amd as T
    sig = inspect.signature(T.Module.quantize_static_calibrated).parameters
    assert list(sig) == ["self", "calib", "percentile", "bins", "convs", "chain", "per_channel", "links"]
    assert [sig[k].default for k in list(sig)[2:]] == [99.99, 2048, True, True, False, False]
    assert list(inspect.signature(T.QuantizedModule.calibration).parameters) == ["self"]
    for name in ("quantize_static", "quantize_static_conv", "quantize_static_chain"):      # unchanged
        assert list(inspect.signature(getattr(T.Module, name)).parameters) == ["self", "calib"], name
    assert list(inspect.signature(T.Module.quantize_static_per_channel).parameters) == ["self", "calib", "convs", "chain"]
    assert list(inspect.signature(T.Module.quantize_static_linked).parameters) == ["self", "calib", "per_channel"]
    assert K.keep_ppm_of(99.99) == 999900 and K.keep_ppm_of(100) == 1000000 and K.keep_ppm_of(99.0) == 990000 and K.keep_ppm_of(99.9) == 999000


@pytest.mark.parametrize("args,match", [((0, 2, 999900, 2048), "method"), ((0, -1, 999900, 2048), "method"), ((0, 1, 0, 2048), "keep_ppm"),
                                        ((0, 1, 1000001, 2048), "keep_ppm"), ((0, 1, 999900, 15), "num_bins"), ((0, 1, 999900, 8193), "num_bins"),
                                        ((2, 1, 999900, 2048), "TP_QSTATIC_CHAIN"), ((2 | 4, 0, 0, 0), "TP_QSTATIC_CHAIN"), ((8, 1, 999900, 2048), "unknown")])
def test_refused_arguments_fail_in_the_host_before_the_device(args, match):
    # refused on the arguments alone: no model is read (there is none), and on a machine without a GPU nothing else could have succeeded
    from taper_amd._lib import host
    out = C.c_void_p()
    assert host.tp_module_quantize_static_cal(None, None, 0, *args, C.byref(out)) != 0 and out.value is None
    err = host.tp_last_error().decode()
    assert err.startswith("tp_module_quantize_static_cal: ") and match in err, err
    if match in ("keep_ppm", "num_bins"):
        assert str(args[2] if match == "keep_ppm" else args[3]) in err      # the refused value is named too


def test_kernel_refusals_come_before_a_launch():
    from taper_amd._lib import hip
    for call, name in ((lambda: hip.th_act_hist_update(None, None, 0, None, 2048, None), "th_act_hist_update"),
                       (lambda: hip.th_act_scale_from_hist(None, None, 2048, None, 999900, None, None), "th_act_scale_from_hist")):
        assert call() != 0 and hip.th_last_error().decode().startswith(name + ": null argument")


# ---------------------------------------------------------------- the restatement's own rules
def test_bin_rule_at_its_edges():
    nb = 16
    rng2 = (f32(-8), f32(2))                                        # amax from the negative end: inv = 2, a bin is 0.5 wide
    x = np.array([0, -0.0, 0.49, 0.5, -0.5, 1.0, 7.99, 8.0, -8.0, 9.0, 1e30, np.nan, np.inf, -np.inf], f32)
    b = K.bins_of(x, rng2, nb)
    assert b.dtype == np.uint64 and int(b.sum()) == 11              # NaN and +-inf are skipped
    assert (int(b[0]), int(b[1]), int(b[2]), int(b[15])) == (3, 2, 1, 5)      # exact multiples open their bin; amax and everything above: the last
    np.testing.assert_array_equal(K.bins_of(x, rng2, nb, into=b), 2 * b)
    for rng0 in ((f32(0), f32(0)), (f32(np.nan), f32(np.nan))):      # inv = +inf or NaN: the product is +inf or NaN, the cast never sees it
        z = K.bins_of(np.array([0, 1, -2], f32), rng0, nb)
        assert int(z[15]) == 3 and int(z.sum()) == 3
    e = K.bins_of(np.array([0, 1, -2], f32), (f32(np.inf), f32(-np.inf)), nb)      # a range over nothing finite: inv = 0
    assert int(e[0]) == 3


def test_scale_rule_at_its_edges():
    nb, rng2 = 16, (f32(-1), f32(4))
    before = f32(123)
    bins = np.zeros(nb, np.uint64)
    assert K.scale_from_hist(bins, rng2, 999900, before) == (before, [15, 0, 0, 0])                    # empty: the fallback
    bins[0] = 10
    s, st = K.scale_from_hist(bins, rng2, 1000000, before)                                            # all mass in bin 0
    assert st == [0, 10, 10, 10] and s == f32(f32(1) * f32(f32(4) / f32(16))) / f32(127)
    bins[:] = 0
    bins[:4] = (25, 25, 25, 25)
    assert K.scale_from_hist(bins, rng2, 500000, before)[1] == [1, 100, 50, 25]                        # exactly on a cumulative boundary
    assert K.scale_from_hist(bins, rng2, 500001, before)[1] == [2, 100, 75, 25]                        # one millionth past it
    assert K.scale_from_hist(bins, rng2, 1, before)[1] == [0, 100, 25, 25]
    bins[15] = 1
    s, st = K.scale_from_hist(bins, rng2, 1000000, before)
    assert st == [15, 101, 101, 1] and s == f32(4) / f32(127) == R.act_scale(*rng2)                    # the last bin: T is amax itself
    for degenerate in ((f32(0), f32(0)), (f32(3), f32(3)), (f32(np.inf), f32(-np.inf)), (f32(0), f32(1e-39))):
        assert K.scale_from_hist(bins, degenerate, 500000, before) == (before, [15, 101, 101, 1])
    bins[:] = 0
    bins[3] = 2 ** 40
    bins[9] = 1
    assert K.scale_from_hist(bins, rng2, 999999, before)[1] == [3, 2 ** 40 + 1, 2 ** 40, 2 ** 40]      # 64-bit counts


def test_keeping_everything_is_the_min_max_scale():
    rng = np.random.default_rng(3)
    for nb in (16, 2048, 8192):
        for scale in (1e-3, 1.0, 77.7):
            a, b = (scale * rng.standard_normal(500)).astype(f32), (scale * rng.uniform(0, 1, 300)).astype(f32)
            c = K.calibrate([a, b], 1000000, nb)
            assert c["bin"] == nb - 1 and c["kept"] == c["total"] == 800 and c["scale"] == R.act_scale_of(a, b)
            assert c["threshold"] == max(abs(c["min"]), abs(c["max"]))


@pytest.mark.parametrize("seed", range(5))
def test_a_percentile_clip_recovers_the_rows_beside_an_outlier(seed):
    """The whole static restatement of tests/qstatic_ref.py (activation codes, packed weight, integer product) on the outlier Linear, once
    with the min / max scale and once with the 99.9 % scale of 2 048 bins, against the float64 product on the rows without the outlier.
    Min / max: 1.00 of max |y| on every seed; percentile: 2.93e-2, 2.09e-2, 1.95e-2, 2.24e-2, 2.14e-2 -- factors 34.1, 47.8, 51.3, 44.6,
    46.7, all at least 30, so the bar is the per-channel test's 10."""
    x, w = K.outlier_layer(seed)
    c = K.calibrate([x], K.keep_ppm_of(99.9), 2048)
    s_minmax = R.act_scale_of(x)
    assert s_minmax == f32(1000) / f32(127) and c["max"] == f32(1000) and c["total"] == x.size
    assert c["threshold"] == f32(3.4179688) and c["bin"] == 6 and c["scale"] == f32(c["threshold"] / f32(127))
    e_minmax = K.clean_row_error(K.static_linear(x, w, s_minmax), x, w)
    e_pct = K.clean_row_error(K.static_linear(x, w, c["scale"]), x, w)
    print(f"seed {seed}: min/max {e_minmax:.3e}, percentile {e_pct:.3e}, factor {e_minmax / e_pct:.1f}")
    assert e_minmax / e_pct >= 10, (e_minmax, e_pct)
