"""Percentile calibration on the GPU: th_act_hist_update and th_act_scale_from_hist against the numpy restatement of
tests/qcalib_ref.py -- counters with assert_array_equal, scales on bits -- and Module.quantize_static_calibrated in every twin form
against the existing twins (percentile = 100) and the existing twin restatements fed its scales (percentile = 99)."""
import ctypes as C

import numpy as np
import pytest

from tests import qcalib_ref as K
from tests import qstatic_ref as R
from tests import test_gpu_qconv as TC
from tests import test_gpu_qlink as TK
from tests import test_gpu_qperchan as TP

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 32                            # 64-bit words on either side of the counters
GUARD_WORD = 0xA5A5A5A5C3C3C3C3
SCALE_BITS = 0x4A21C3E1               # what d_scale holds before a call: no scale a rule gives
_bits, _in_use, _pool_in_use = TC._bits, TC._in_use, TC._pool_in_use


def _b(v):
    """the bits of one f32 as an int"""
    return int(np.array(v, f32).reshape(1).view(np.uint32)[0])


CONVS, CHAIN, PER_CHANNEL, LINKS = 1, 2, 4, 16


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1: the counting pass
SIZES = (0, 1, 3, 63, 64, 255, 1025, 4101, 70001)      # nothing launched, under a wave, the scalar tail, one vector trip + a tail, several workgroups
DATA = ("normal", "relu", "nonfinite", "at_amax", "bin_edges", "above_range", "negative_end")


def _data(kind, n, nb, seed):
    """-> (x [n], range2): the range is what th_act_range_update would have found on x, except where the case says otherwise"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(f32)
    if kind == "relu":
        x = np.maximum(x, f32(0))                                   # half the mass in bin 0: the hot bin
    elif kind == "nonfinite" and n:
        x[0] = np.nan
        x[n // 2] = np.inf                                           # (n = 1: nothing finite at all, a range of {+inf, -inf})
        x[n - 1] = -np.inf
        x[n // 3::7] = np.nan
    elif kind == "at_amax" and n:
        x[::5] = f32(6.5)
        x[1::5] = f32(-6.5)
    elif kind == "bin_edges":                                        # amax = nb / 4: inv = 4 exactly, every element an exact multiple of the width
        x = (rng.integers(0, nb + 1, n) * rng.choice([-1, 1], n)).astype(f32) / f32(4)
        return x, (f32(-nb / 4), f32(nb / 4))
    elif kind == "negative_end" and n:
        x[n // 2] = f32(-7)
    rng2 = K.finite_range(x) if n else (f32(0), f32(1))
    if kind == "above_range" and n:                                  # a tensor the range pass never saw
        x[n // 3] = f32(3) * K.amax_of(rng2)
    return x, rng2


def _count(ctx, x, rng2, nb, off, bins=None):
    """one th_act_hist_update on x placed `off` floats behind a 16-byte boundary -> the guarded counter buffer"""
    if bins is None:
        bins = ctx.upload(np.concatenate([np.full(GUARD, GUARD_WORD, np.uint64), np.zeros(nb, np.uint64), np.full(GUARD, GUARD_WORD, np.uint64)]))
    dx = ctx.upload(np.concatenate([np.zeros(off, f32), x, np.full(4, 1e9, f32)]))      # (what follows x must not be counted)
    dr = ctx.upload(np.array(rng2, f32))
    before = _in_use(ctx)
    ctx.call("th_act_hist_update", dx.offset(4 * off), x.size, dr, nb, bins.offset(8 * GUARD))
    assert _in_use(ctx) == before
    return bins


def _counters(ctx, bins, nb):
    raw = ctx.download(bins, (nb + 2 * GUARD,), np.uint64)
    assert (raw[:GUARD] == GUARD_WORD).all() and (raw[GUARD + nb:] == GUARD_WORD).all(), "words around the counters were written"
    return raw[GUARD:GUARD + nb]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
@pytest.mark.parametrize("nb", [16, 128, 2048, 8192])
def test_counters_are_the_restatement(ctx, nb, off):
    for n in SIZES:
        for d, kind in enumerate(DATA):
            x, rng2 = _data(kind, n, nb, 1000 * d + n)
            ref = K.bins_of(x, rng2, nb)
            assert int(ref.sum()) == int(np.isfinite(x).sum())
            runs = [_counters(ctx, _count(ctx, x, rng2, nb, off), nb) for _ in range(2)]
            np.testing.assert_array_equal(runs[0], ref, err_msg=f"{kind} n={n}")
            np.testing.assert_array_equal(runs[1], runs[0], err_msg=f"{kind} n={n}: a second run")
            if kind == "above_range" and n:
                assert ref[nb - 1] >= 1 and np.abs(x).max() > K.amax_of(rng2)
            if kind == "negative_end" and n > 3:
                assert K.amax_of(rng2) == f32(7) and rng2[1] < f32(7)


@pytest.mark.parametrize("nb", [16, 2048])
def test_two_calls_accumulate_to_the_histogram_of_the_concatenation(ctx, nb):
    a, _ = _data("normal", 4101, nb, 1)
    b, _ = _data("relu", 70001, nb, 2)
    rng2 = K.finite_range(a, b)
    bins = _count(ctx, b, rng2, nb, 1, _count(ctx, a, rng2, nb, 0))
    np.testing.assert_array_equal(_counters(ctx, bins, nb), K.bins_of(np.concatenate([a, b]), rng2, nb))
    np.testing.assert_array_equal(K.bins_of(b, rng2, nb, into=K.bins_of(a, rng2, nb)), K.bins_of(np.concatenate([a, b]), rng2, nb))


def test_ranges_that_give_no_width(ctx):
    x = np.array([0, 1, -2, 0, np.nan], f32)
    for rng2, where in (((0, 0), 15), ((np.nan, np.nan), 15), ((np.inf, -np.inf), 0), ((0, 1e-42), 15)):
        got = _counters(ctx, _count(ctx, x, (f32(rng2[0]), f32(rng2[1])), 16, 0), 16)
        np.testing.assert_array_equal(got, K.bins_of(x, rng2, 16))
        assert got[where] == 4


# ---------------------------------------------------------------- 2: the scale
def _scale_call(ctx, bins, rng2, keep_ppm, dscale=None):
    """-> (scale bits after the call, stats4 as Python ints)"""
    nb = len(bins)
    db = ctx.upload(np.asarray(bins, np.uint64))
    dr = ctx.upload(np.array(rng2, f32))
    if dscale is None:
        dscale = ctx.upload(np.array([SCALE_BITS], np.uint32))
    ds = ctx.upload(np.full(4 + 2 * GUARD, GUARD_WORD, np.uint64))
    before = _in_use(ctx)
    ctx.call("th_act_scale_from_hist", db, nb, dr, keep_ppm, dscale, ds.offset(8 * GUARD))
    assert _in_use(ctx) == before
    raw = ctx.download(ds, (4 + 2 * GUARD,), np.uint64)
    assert (raw[:GUARD] == GUARD_WORD).all() and (raw[GUARD + 4:] == GUARD_WORD).all()
    np.testing.assert_array_equal(ctx.download(db, (nb,), np.uint64), np.asarray(bins, np.uint64))      # the counters are only read
    return int(ctx.download(dscale, (1,), np.uint32)[0]), [int(v) for v in raw[GUARD:GUARD + 4]]


def _hand_made():
    """(name, bins, range2, keep_ppm)"""
    out = []
    for nb in (16, 300, 8192):
        rng2 = (f32(-1.25), f32(4.75))
        z = np.zeros(nb, np.uint64)
        b = z.copy()
        b[0] = 12345
        out.append((f"all in bin 0 / {nb}", b, rng2, 999900))
        b = z.copy()
        b[[1, 5, nb // 2, nb - 3]] = (25, 25, 25, 25)
        out += [(f"on a boundary / {nb}", b, rng2, 500000), (f"one millionth past it / {nb}", b, rng2, 500001), (f"keep_ppm 1 / {nb}", b, rng2, 1),
                (f"everything / {nb}", b, rng2, 1000000)]
        short = b.copy()
        short[5], short[nb // 2] = 24, 26                                # the same target finds the boundary one count short: the next bin that holds any
        out.append((f"one count short of the boundary / {nb}", short, rng2, 500000))
        b = b.copy()
        b[nb - 1] = 3
        out.append((f"everything, to the last bin / {nb}", b, rng2, 1000000))
        out.append((f"empty / {nb}", z, rng2, 999900))
        b = z.copy()
        b[nb // 3], b[nb - 2] = 2 ** 40, 7
        out += [(f"2^40 in one bin / {nb}", b, rng2, 999999), (f"2^40 and the tail / {nb}", b, rng2, 1000000)]
        b = z.copy()
        b[:] = np.arange(1, nb + 1, dtype=np.uint64) * 3                # every lane of the scan owns non-empty bins
        out += [(f"ramp {ppm} / {nb}", b, rng2, ppm) for ppm in (1, 250000, 990000, 999999)]
        for name, deg in (("min == max == 0", (0, 0)), ("min == max == m", (2.5, 2.5)), ("nothing finite", (np.inf, -np.inf)), ("subnormal amax", (0, 1e-42)),
                          ("NaN range", (np.nan, np.nan))):
            out.append((f"{name} / {nb}", b, (f32(deg[0]), f32(deg[1])), 990000))
    return out


def test_scale_and_report_on_hand_made_histograms(ctx):
    before_scale = np.array([SCALE_BITS], np.uint32).view(f32)[0]
    for name, bins, rng2, ppm in _hand_made():
        ref_scale, ref_stats = K.scale_from_hist(bins, rng2, ppm, before_scale)
        got_bits, got_stats = _scale_call(ctx, bins, rng2, ppm)
        assert got_stats == ref_stats, (name, got_stats, ref_stats)
        assert got_bits == _b(ref_scale), (name, hex(got_bits))
        fallback = any(s in name for s in ("empty", "min == max", "nothing finite", "subnormal", "NaN"))
        assert (got_bits == SCALE_BITS) == fallback, name              # d_scale untouched exactly where the range rule stands
        k, total, kept, count = got_stats
        if not fallback:
            assert kept * 10 ** 6 >= total * ppm > (kept - count) * 10 ** 6 and count > 0, name
            assert total >= 2 ** 40 or "2^40" not in name


@pytest.mark.parametrize("case", ["normal", "zeros", "constant"])
@pytest.mark.parametrize("nb", [16, 2048, 8192])
def test_keeping_everything_reproduces_the_range_scale_bit_for_bit(ctx, case, nb):
    rng = np.random.default_rng(nb)
    tensors = {"normal": [(0.37 * rng.standard_normal(5000)).astype(f32), rng.uniform(-3, 1, 777).astype(f32)],
               "zeros": [np.zeros(100, f32)], "constant": [np.full(100, -2.5, f32)]}[case]
    drange = ctx.upload(np.zeros(3, f32))
    for i, t in enumerate(tensors):
        ctx.call("th_act_range_update", ctx.upload(t), t.size, 1 if i == 0 else 0, drange, drange.offset(8))
    mn, mx, scale = ctx.download(drange, (3,))
    assert _b(scale) == _b(R.act_scale_of(*tensors)) and (mn, mx) == K.finite_range(*tensors)
    bins = None
    for t in tensors:
        bins = _count(ctx, t, (mn, mx), nb, 0, bins)
    counters = _counters(ctx, bins, nb)
    got_bits, stats = _scale_call(ctx, counters, (mn, mx), 1000000, dscale=drange.offset(8))
    assert got_bits == _b(scale) and stats[0] == nb - 1 and stats[1] == stats[2] == sum(t.size for t in tensors)
    ref = K.calibrate(tensors, 1000000, nb)
    assert _b(ref["scale"]) == got_bits and stats == [ref["bin"], ref["total"], ref["kept"], ref["bin_count"]]


def test_kernel_refusals_name_the_call_and_the_next_call_succeeds(ctx):
    hip = TC._lib()
    x = np.arange(100, dtype=f32)
    dx, dr, db = ctx.upload(x), ctx.upload(np.array([0, 99], f32)), ctx.upload(np.zeros(16, np.uint64))
    dsc, dst = ctx.upload(np.array([SCALE_BITS], np.uint32)), ctx.upload(np.zeros(4, np.uint64))
    X, Rg, Bn, Sc, St = int(dx), int(dr), int(db), int(dsc), int(dst)
    before = _in_use(ctx)
    for args, what in (((None, 100, Rg, 16, Bn), "null"), ((X, 100, None, 16, Bn), "null"), ((X, 100, Rg, 16, None), "null"), ((X, -1, Rg, 16, Bn), "negative"),
                       ((X, 100, Rg, 15, Bn), "num_bins"), ((X, 100, Rg, 8193, Bn), "num_bins"), ((X, 1 << 40, Rg, 16, Bn), "2^32")):
        assert hip.th_act_hist_update(ctx.h, *args) != 0, args
        assert hip.th_last_error().decode().startswith("th_act_hist_update: ") and what in hip.th_last_error().decode(), args
    for args, what in (((None, 16, Rg, 5, Sc, St), "null"), ((Bn, 16, None, 5, Sc, St), "null"), ((Bn, 16, Rg, 5, None, St), "null"), ((Bn, 16, Rg, 5, Sc, None), "null"),
                       ((Bn, 15, Rg, 5, Sc, St), "num_bins"), ((Bn, 8193, Rg, 5, Sc, St), "num_bins"), ((Bn, 16, Rg, 0, Sc, St), "keep_ppm"),
                       ((Bn, 16, Rg, 1000001, Sc, St), "keep_ppm")):
        assert hip.th_act_scale_from_hist(ctx.h, *args) != 0, args
        assert hip.th_last_error().decode().startswith("th_act_scale_from_hist: ") and what in hip.th_last_error().decode(), args
    assert _in_use(ctx) == before
    assert not ctx.download(db, (16,), np.uint64).any() and ctx.download(dsc, (1,), np.uint32)[0] == SCALE_BITS      # a refused call writes nothing
    assert hip.th_act_hist_update(ctx.h, None, 0, Rg, 16, Bn) == 0                                                   # n == 0: nothing to read
    assert hip.th_act_hist_update(ctx.h, X, 100, Rg, 16, Bn) == 0 and hip.th_act_scale_from_hist(ctx.h, Bn, 16, Rg, 500000, Sc, St) == 0
    np.testing.assert_array_equal(ctx.download(db, (16,), np.uint64), K.bins_of(x, (0, 99), 16))
    assert [int(v) for v in ctx.download(dst, (4,), np.uint64)] == K.scale_from_hist(K.bins_of(x, (0, 99), 16), (0, 99), 500000, 0)[1]


def test_both_calls_can_be_captured_and_replayed(ctx):
    nb, x = 128, _data("relu", 70001, 128, 5)[0]
    rng2 = K.finite_range(x)
    dx, dr, db = ctx.upload(x), ctx.upload(np.array(rng2, f32)), ctx.upload(np.full(nb, 9, np.uint64))
    dsc, dst = ctx.upload(np.array([SCALE_BITS], np.uint32)), ctx.upload(np.zeros(4, np.uint64))
    ctx.sync()
    ctx.graph_begin()
    try:
        ctx.call("th_fill_f32", db, 0.0, 2 * nb)
        ctx.call("th_act_hist_update", dx, x.size, dr, nb, db)
        ctx.call("th_act_scale_from_hist", db, nb, dr, 990000, dsc, dst)
    finally:
        g = ctx.graph_end()
    try:
        ref_bins = K.bins_of(x, rng2, nb)
        ref_scale, ref_stats = K.scale_from_hist(ref_bins, rng2, 990000, 0)
        for _ in range(2):
            ctx.graph_launch(g)
            ctx.sync()
            np.testing.assert_array_equal(ctx.download(db, (nb,), np.uint64), ref_bins)
            assert [int(v) for v in ctx.download(dst, (4,), np.uint64)] == ref_stats
            assert int(ctx.download(dsc, (1,), np.uint32)[0]) == _b(ref_scale)
    finally:
        ctx.graph_destroy(g)


# ---------------------------------------------------------------- 3: the twins
def _old_twin(model, calib, flags):
    from taper_amd._lib import host
    return model._quantize_static(host.tp_module_quantize_static_ex, "quantize_static_ex", calib, flags)


def _new_twin(model, calib, flags, percentile, bins):
    return model.quantize_static_calibrated(calib, percentile=percentile, bins=bins, convs=bool(flags & CONVS), chain=bool(flags & CHAIN),
                                            per_channel=bool(flags & PER_CHANNEL), links=bool(flags & LINKS))


def _mlp():
    import taper_amd as T
    rng = np.random.default_rng(90)
    model = TK._randomize(T.Sequential([T.Linear(20, 12, True), T.ReLU(), T.Linear(12, 5, True)]), rng)
    calib = [rng.standard_normal((16, 20)).astype(f32), (2 * rng.standard_normal((9, 20))).astype(f32)]
    x = (1.5 * rng.standard_normal((7, 20))).astype(f32)
    return model, calib, x, [(20,), (12,)], None


def _cnn():
    rng = np.random.default_rng(91)
    model, layers, _ = TC._cnn(rng)
    calib = [rng.uniform(0, 1, TC.SHAPE).astype(f32), (1.5 * rng.standard_normal(TC.SHAPE)).astype(f32)]
    x = rng.standard_normal(TC.SHAPE).astype(f32)
    return model, calib, x, [(1, 12, 12), (4, 5, 5), (32,)], layers


MODELS = {"mlp": _mlp, "cnn": _cnn}
FLAGS = {"plain": 0, "convs": CONVS, "chain": CONVS | CHAIN, "per_channel": CONVS | CHAIN | PER_CHANNEL, "links": CONVS | CHAIN | LINKS}


def _tensors_of(arrays):
    import taper_amd as T
    return [T.Tensor(a, a.shape) for a in arrays]


@pytest.mark.parametrize("form", list(FLAGS))
@pytest.mark.parametrize("name", list(MODELS))
def test_percentile_100_is_the_existing_twin_bit_for_bit(name, form):
    import taper_amd as T
    model, calib, x, _, _ = MODELS[name]()
    ct, flags = _tensors_of(calib), FLAGS[form]
    T.Tape.reset()
    new, old = _new_twin(model, ct, flags, 100, 2048), _old_twin(model, ct, flags)
    assert T.Tape.len() == 0
    np.testing.assert_array_equal(_bits(new.act_scales()), _bits(old.act_scales()))
    TK._assert_same_tensors(new, old)
    assert new.chain_links() == old.chain_links() and new.storage_bytes() == old.storage_bytes()
    xt = T.Tensor(x, x.shape)
    np.testing.assert_array_equal(_bits(new(xt).data()), _bits(old(xt).data()))
    for rec, s in zip(new.calibration(), new.act_scales()):
        assert rec["bin"] == 2047 and rec["kept"] == rec["total"] > 0 and _b(rec["scale"]) == _b(s)
        assert rec["threshold"] == max(abs(rec["min"]), abs(rec["max"]))
    for rec, s in zip(old.calibration(), old.act_scales()):                # a min / max twin reports its range and no histogram
        assert (rec["bin"], rec["total"], rec["kept"], rec["bin_count"]) == (0, 0, 0, 0) and _b(rec["scale"]) == _b(s)
        assert rec["threshold"] == max(abs(rec["min"]), abs(rec["max"]))


def _reference_forward(name, form, q, x, layers):
    import taper_amd as T
    ts = [(k, c, np.asarray(p, f32) if np.ndim(p) == 2 else p) for k, c, p in q.tensors()]
    scales = q.act_scales()
    if name == "mlp":
        return TK._linear_ref(ts, scales, x, (True, False))
    if form == "plain":                                   # the convs stay weight-only: the weight-only twin of the front, then the one static Linear
        feat = T.Sequential(layers[:6]).quantize("int8").forward(T.Tensor(x, x.shape)).data()
        return TK._linear_ref(ts[4:], scales, feat, (False,))
    return TP._cnn_ref_chain(ts, scales, x) if form == "per_channel" else TC._ref_chain(ts, scales, x)


@pytest.mark.parametrize("name", list(MODELS))
def test_percentile_99_twins(name):
    import taper_amd as T
    model, calib, x, layer_inputs, layers = MODELS[name]()
    ct, bins, ppm = _tensors_of(calib), 128 if name == "mlp" else 2048, K.keep_ppm_of(99.0)
    images = sum(c.shape[0] for c in calib)
    xt = T.Tensor(x, x.shape)
    T.Tape.reset()
    before = _pool_in_use()
    old = _old_twin(model, ct, FLAGS["chain"])
    old_bytes = _pool_in_use() - before
    twins = {"chain": _new_twin(model, ct, FLAGS["chain"], 99.0, bins)}
    extra = _pool_in_use() - before - 2 * old_bytes
    assert 0 <= extra < 8 * bins, extra                                    # the report's integers stay, no histogram does
    assert twins["chain"].storage_bytes() == old.storage_bytes()
    del old
    twins.update({form: _new_twin(model, ct, flags, 99.0, bins) for form, flags in FLAGS.items() if form != "chain"})
    assert T.Tape.len() == 0
    held, outs = _pool_in_use(), {}
    first = K.calibrate(calib, ppm, bins)                                  # the first static layer sees the calibration tensors themselves
    as_bits = lambda rec: {k: (_b(v) if isinstance(v, f32) else v) for k, v in rec.items()}
    for form, q in twins.items():
        recs, scales = q.calibration(), q.act_scales()
        shapes = layer_inputs[-len(recs):]                                  # (without convs the CNN's Linear alone is static)
        assert len(recs) == len(scales) == (len(layer_inputs) if FLAGS[form] & CONVS or name == "mlp" else 1), form
        if len(recs) == len(layer_inputs):
            assert as_bits(recs[0]) == as_bits(first), (form, recs[0], first)
        for rec, s, shp in zip(recs, scales, shapes):
            assert rec["total"] == images * int(np.prod(shp)), (form, rec)                # every input is finite here
            assert rec["kept"] * 10 ** 6 >= rec["total"] * ppm > (rec["kept"] - rec["bin_count"]) * 10 ** 6, (form, rec)
            assert rec["threshold"] <= max(abs(rec["min"]), abs(rec["max"])) and rec["bin"] < bins
            assert _b(rec["scale"]) == _b(s) == _b(f32(rec["threshold"] / f32(127)))
            assert _b(rec["threshold"]) == _b(K.threshold_of(rec["bin"], (rec["min"], rec["max"]), bins))
        outs[form] = q(xt).data()
        np.testing.assert_array_equal(_bits(outs[form]), _bits(_reference_forward(name, form, q, x, layers)), err_msg=form)
    assert _pool_in_use() == held                                           # the forwards gave everything back
    np.testing.assert_array_equal(_bits(outs["chain"]), _bits(outs["convs"]))
    np.testing.assert_array_equal(_bits(outs["links"]), _bits(outs["chain"]))
    np.testing.assert_array_equal(_bits(twins["chain"].act_scales()), _bits(twins["convs"].act_scales()))
    assert any(r["bin"] < bins - 1 for r in twins["chain"].calibration())     # the clip is a clip somewhere
    del twins, q
    assert _pool_in_use() == before


@pytest.mark.parametrize("seed", range(5))
def test_the_outlier_linear_on_the_device(seed):
    """tests/test_qcalib_abi.py's construction as a model, calibrated on its own input: both twins give the restatement's bits, so the
    errors are the CPU test's (min / max 1.00 of max |y|; percentile 2.93e-2, 2.09e-2, 1.95e-2, 2.24e-2, 2.14e-2) and so is the factor."""
    import taper_amd as T
    x, w = K.outlier_layer(seed)
    model = T.Sequential([T.Linear(256, 40, False)])
    model.parameters()[0].set_data(w)
    xt = T.Tensor(x, x.shape)
    ref = K.calibrate([x], K.keep_ppm_of(99.9), 2048)
    errs = {}
    for name, twin, scale in (("min/max", model.quantize_static(xt), R.act_scale_of(x)),
                              ("percentile", model.quantize_static_calibrated(xt, percentile=99.9, bins=2048, convs=False, chain=False), ref["scale"])):
        assert _b(twin.act_scales()[0]) == _b(scale), name
        y = twin(xt).data()
        np.testing.assert_array_equal(_bits(y), _bits(K.static_linear(x, w, scale)), err_msg=name)
        errs[name] = K.clean_row_error(y, x, w)
    rec = twin.calibration()[0]
    assert (rec["bin"], rec["total"], rec["kept"], rec["bin_count"]) == (ref["bin"], ref["total"], ref["kept"], ref["bin_count"])
    T.Tape.reset()
    print(f"seed {seed}: min/max {errs['min/max']:.3e}, percentile {errs['percentile']:.3e}, factor {errs['min/max'] / errs['percentile']:.1f}")
    assert errs["min/max"] / errs["percentile"] >= 10, errs


# ---------------------------------------------------------------- 4: refusals
def _static_cal(model, tensors, flags, method, keep_ppm, num_bins):
    """tp_module_quantize_static_cal itself -> (return code, handle)"""
    from taper_amd._lib import host
    arr = (C.c_void_p * max(len(tensors), 1))(*[t._h if t is not None else None for t in tensors])
    h = C.c_void_p()
    return host.tp_module_quantize_static_cal(model._h, arr, len(tensors), flags, method, keep_ppm, num_bins, C.byref(h)), h


def test_refusals_allocate_nothing_and_the_next_call_succeeds():
    import taper_amd as T
    from taper_amd._lib import host
    model, calib, x, _, _ = _cnn()
    ct = _tensors_of(calib)
    dropout = T.Sequential([T.Conv2d(1, 4, (3, 3)), T.Dropout(0.5)])
    T.Device.sync()
    before = _pool_in_use()
    for kw, what in ((dict(percentile=0), "keep_ppm"), (dict(percentile=100.0001), "keep_ppm"), (dict(bins=15), "num_bins"), (dict(bins=8193), "num_bins")):
        with pytest.raises(T.TaperError, match="tp_module_quantize_static_cal: " + what):
            model.quantize_static_calibrated(ct, **kw)
    for args, what in (((0, 2, 999900, 2048), b"method"), ((CHAIN, 1, 999900, 2048), b"TP_QSTATIC_CHAIN"), ((8, 1, 999900, 2048), b"unknown"),
                       ((3, 1, 0, 2048), b"keep_ppm"), ((3, 1, 1000001, 2048), b"keep_ppm"), ((3, 1, 999900, 15), b"num_bins"), ((3, 1, 999900, 8193), b"num_bins")):
        rc, h = _static_cal(model, ct, *args)
        assert rc != 0 and not h.value and host.tp_last_error().startswith(b"tp_module_quantize_static_cal: ") and what in host.tp_last_error(), args
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static_calibrated(ct)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        model.quantize_static_calibrated([])
    with pytest.raises(T.TaperError, match="undefined calibration tensor"):
        model.quantize_static_calibrated([ct[0], None])
    assert _pool_in_use() == before
    q = model.quantize_static_calibrated(ct)                               # and the next valid call succeeds
    assert q.act_scales().shape == (3,) and q.chain_links() == 1 and q(T.Tensor(x, x.shape)).data().shape == (8, 10)
    rc, h = _static_cal(model, ct, 3, 0, 0, 0)                              # TP_CALIB_MINMAX reads neither number: tp_module_quantize_static_ex
    assert rc == 0
    same = T.QuantizedModule(h.value)
    np.testing.assert_array_equal(_bits(same.act_scales()), _bits(model.quantize_static_chain(ct).act_scales()))
    f, u = np.zeros(4, f32), np.zeros(4, np.uint64)
    for i in (-1, 3):
        assert host.tp_qmodule_calibration(q._h, i, f.ctypes.data, u.ctypes.data) != 0 and b"tp_qmodule_calibration: index" in host.tp_last_error()
    assert host.tp_qmodule_calibration(q._h, 0, None, u.ctypes.data) != 0 and b"tp_qmodule_calibration: null" in host.tp_last_error()
