"""Residual models through the static quantize calls on the GPU (TP_QBLOCKS): ResidualBlock and BottleneckBlock twins in every form
against the numpy restatement of tests/qres_ref.py, bit for bit; what the twins report; the exact convs as static convs; the refusals with
and without the flag; and the source model left as it was."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import qconv_ref as Q
from tests import qperchan_ref as P
from tests import qres_ref as S
from tests import qstatic_ref as R
from tests import test_gpu_qconv as TC

pytestmark = pytest.mark.gpu
f32 = np.float32
_bits, _pool_in_use = TC._bits, TC._pool_in_use
CONVS, CHAIN, PER_CHANNEL, LINKS, BLOCKS = 1, 2, 4, 16, 32
SHAPE = (3, 1, 12, 12)
CLASSES = 5

# name -> (first block: kind, constructor arguments, python constructor), the second block is an identity block of the same kind at the
# first's output width; the inner links of both with CHAIN (a ResidualBlock has one inner boundary, a BottleneckBlock two)
CONFIGS = {
    "res-4-4-s1": ("res", (4, 4, 1), "plain"),
    "res-4-8-s1": ("res", (4, 8, 1), "plain"),
    "res-4-8-s2-exact": ("res", (4, 8, 2), "exact"),
    "res-4-8-s2-pointwise": ("res", (4, 8, 2), "pointwise"),
    "neck-8-4-8-s1": ("neck", (8, 4, 8, 1), "plain"),
    "neck-4-4-8-s2": ("neck", (4, 4, 8, 2), "plain"),
}


def _build(name, rng):
    """-> (model, layers, [the two blocks' (kind, args, how)])"""
    import taper_amd as T
    kind, args, how = CONFIGS[name]
    c_in, c_out = args[0], args[-2]
    if kind == "res":
        make = {"plain": T.ResidualBlock, "exact": T.ResidualBlock.exact_stride, "pointwise": T.ResidualBlock.pointwise_shortcut}[how]
        first, second, second_args = make(*args, seed=11), T.ResidualBlock(c_out, c_out, 1, seed=21), (c_out, c_out, 1)
    else:
        first, second, second_args = T.BottleneckBlock(*args, seed=11), T.BottleneckBlock(c_out, 4, c_out, 1, seed=21), (c_out, 4, c_out, 1)
    layers = [T.Conv2dReLU(1, c_in, (3, 3), None, (1, 1), seed=5), first, T.MaxPool2d((2, 2), (2, 2)), second, T.AdaptiveAvgPool2d((1, 1)), T.Flatten(1),
              T.Linear(c_out, CLASSES, True, seed=6)]
    model = T.Sequential(layers)
    params = model.parameters()
    for i, p in enumerate(params):      # random weights and biases (the stem's and the Linear's), BatchNorm pairs of both signs below
        shape = p.data().shape
        if len(shape) == 4 or len(shape) == 2:
            p.set_data((rng.standard_normal(p.numel()) / np.sqrt(max(p.numel() // shape[0], 1))).astype(f32))
        elif i in (1, len(params) - 1):
            p.set_data((0.1 * rng.standard_normal(p.numel())).astype(f32))
    for blk in (first, second):
        ps = blk.parameters()
        for i in range(0, len(ps), 3):      # conv w, gamma, beta
            c = ps[i + 1].numel()
            ps[i + 1].set_data((rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32))
            ps[i + 2].set_data((0.1 * rng.standard_normal(c)).astype(f32))
    model.train()
    for _ in range(3):      # running pairs from three training-mode forwards; the model stays in training mode
        model.forward(T.Tensor(rng.standard_normal(SHAPE).astype(f32), SHAPE))
    T.Tape.reset()
    return model, layers, [(kind, args, how), (kind, second_args, "plain")]


def _ref_block(blk, spec):
    """the restatement's block from the float block's parameters and running pairs"""
    kind, args, how = spec
    ps, bufs = [p.data().reshape(-1) for p in blk.parameters()], [b.data().reshape(-1) for b in blk.buffers()]
    weights = [ps[i] for i in range(0, len(ps), 3)]
    bns = [S.bn_spec(ps[3 * i + 1], ps[3 * i + 2], bufs[2 * i], bufs[2 * i + 1]) for i in range(len(weights))]
    if kind == "res":
        return S.residual_block(weights, bns, *args, pointwise=how == "pointwise")
    return S.bottleneck_block(weights, bns, *args)


def _quantize(model, calib, flags, percentile=None):
    import taper_amd as T
    from taper_amd._lib import host
    arr = (C.c_void_p * len(calib))(*[t._h for t in calib])
    h = C.c_void_p()
    if percentile is None:
        rc = host.tp_module_quantize_static_ex(model._h, arr, len(calib), flags, C.byref(h))
    else:
        rc = host.tp_module_quantize_static_cal(model._h, arr, len(calib), flags, 1, int(round(percentile * 1e4)), 256, C.byref(h))
    if rc != 0:
        raise T.TaperError(host.tp_last_error().decode())
    return T.QuantizedModule(h.value)


def _features_ref(layers, specs, x, scales, pc):
    """the model up to the second block, restated: stem (Conv2dReLU with its bias) -> block -> max pool -> block"""
    w, b = (p.data().reshape(-1) for p in layers[0].parameters())
    c0 = specs[0][1][0]
    if pc:
        qw, wp = P.taper_pack_channels(w, c0, 1, (3, 3))
    else:
        qw, wp = R.pack(w)
    qb, bp = R.pack(b)
    conv = P.conv_q8q8_pc if pc else Q.conv_q8q8
    h = conv(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(np.asarray(qw).reshape(-1), c0, 1, (3, 3)), wp, qb, bp, (1, 1), (1, 1), True)
    b1, b2 = _ref_block(layers[1], specs[0]), _ref_block(layers[3], specs[1])
    n1 = len(S.block_convs(b1))
    h = S.block_twin(b1, h, scales[1:1 + n1], pc)
    h = Q.max_pool(h, (2, 2), (2, 2))
    return S.block_twin(b2, h, scales[1 + n1:1 + n1 + len(S.block_convs(b2))], pc), n1, len(S.block_convs(b2))


FORMS = {      # name -> (flags, percentile)
    "unchained": (CONVS | BLOCKS, None),
    "chained": (CONVS | BLOCKS | CHAIN, None),
    "chained-per-channel": (CONVS | BLOCKS | CHAIN | PER_CHANNEL, None),
    "chained-links": (CONVS | BLOCKS | CHAIN | LINKS, None),
    "percentile": (CONVS | BLOCKS | CHAIN, 99.0),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_block_twins_are_the_reference_bit_for_bit_in_every_form(name):
    import taper_amd as T
    rng = np.random.default_rng(sum(map(ord, name)))
    model, layers, specs = _build(name, rng)
    calib = [T.Tensor(a, SHAPE) for a in (rng.standard_normal(SHAPE).astype(f32), (1.5 * rng.standard_normal(SHAPE)).astype(f32))]
    x = rng.standard_normal(SHAPE).astype(f32)
    state = [_bits(t.data()).copy() for t in model.parameters() + model.buffers()]
    T.Tape.reset()
    twins = {f: _quantize(model, calib, *FORMS[f]) for f in FORMS}
    prefix_model = T.Sequential(layers[:4])      # shares the layers: the features in front of the average pool
    assert T.Tape.len() == 0
    for a, t in zip(state, model.parameters() + model.buffers()):
        np.testing.assert_array_equal(a, _bits(t.data()), err_msg="quantizing wrote to the source model")
    inner = [1 if s[0] == "res" else 2 for s in specs]
    outs = {}
    for f, q in twins.items():
        flags, pct = FORMS[f]
        pc = bool(flags & PER_CHANNEL)
        scales = q.act_scales()
        feats_ref, n1, n2 = _features_ref(layers, specs, x, scales, pc)
        assert scales.shape == (1 + n1 + n2 + 1,), f
        # conv1 and the projection observed the same tensor: the same scale, bit for bit, under both calibration methods
        for at, spec, n in ((1, specs[0], n1), (1 + n1, specs[1], n2)):
            if n > (2 if spec[0] == "res" else 3):
                assert _bits(scales[at]) == _bits(scales[at + n - 1]), (f, "conv1's scale differs from the projection's")
        assert q.chain_links() == ((2 + sum(inner)) if flags & CHAIN else 0), f
        # the features of the same flags on the prefix (the same scales: calibration sees the same tensors), against the restatement
        before = _pool_in_use()
        qp = _quantize(prefix_model, calib, flags & ~LINKS, pct)
        np.testing.assert_array_equal(_bits(qp.act_scales()), _bits(scales[:-1]))
        feats = qp(T.Tensor(x, SHAPE)).data()
        assert np.isfinite(feats_ref).all() and np.abs(feats_ref).max() > 0
        np.testing.assert_array_equal(_bits(feats), _bits(feats_ref), err_msg=f"{name} {f}: features")
        # the classifier on the float pool of those features
        pooled = layers[5].forward(layers[4].forward(T.Tensor(feats, feats.shape))).data()
        T.Tape.reset()
        (_, lw, lwp), (_, lb, lbp) = q.tensors()[-2:]
        lin = P.linear_q8q8_pc if pc else R.linear_q8q8
        ref = lin(R.quantize_act(pooled, scales[-1])[0], scales[-1], lw.reshape(CLASSES, -1), lwp, lb, lbp)
        y = q(T.Tensor(x, SHAPE).requires_grad())
        assert T.Tape.len() == 0 and y.tape_node() == 0
        outs[f] = y.data()
        del y, qp
        assert _pool_in_use() == before, f
        np.testing.assert_array_equal(_bits(outs[f]), _bits(ref), err_msg=f"{name} {f}: logits")
    for f in ("chained", "chained-links"):      # only the launches differ
        np.testing.assert_array_equal(_bits(outs[f]), _bits(outs["unchained"]), err_msg=f)
        np.testing.assert_array_equal(_bits(twins[f].act_scales()), _bits(twins["unchained"].act_scales()))
        assert twins[f].storage_bytes() == twins["unchained"].storage_bytes()
    assert not np.array_equal(outs["chained-per-channel"], outs["chained"])


@pytest.mark.parametrize("name", ["res-4-8-s2-pointwise", "neck-4-4-8-s2"])
def test_what_the_twins_report(name):
    import taper_amd as T
    rng = np.random.default_rng(7)
    model, layers, specs = _build(name, rng)
    calib = [T.Tensor(rng.standard_normal(SHAPE).astype(f32), SHAPE)]
    params = [p.data().reshape(-1) for p in model.parameters()]
    packed = params[:2] + params[2:-2:3] + params[-2:]      # parameters() without the BatchNorm pairs (a block's: conv w, gamma, beta in turn)
    for flags in (CONVS | BLOCKS, CONVS | BLOCKS | CHAIN | PER_CHANNEL):
        q = _quantize(model, calib, flags)
        ts = q.tensors()
        assert len(ts) == len(packed)      # parameters() without the BatchNorm pairs: stem w b, conv1, conv2, [conv3], [projection] twice, Linear w b
        blocks = [_ref_block(layers[1], specs[0]), _ref_block(layers[3], specs[1])]
        convs = [cv for b in blocks for cv, _ in S.block_convs(b)]
        for (kind, codes, pairs), v, cv in zip(ts[2:-2], packed[2:-2], convs):
            assert kind == "int8"
            if flags & PER_CHANNEL:
                ref_q, ref_p = P.taper_pack_channels(v, cv["c_out"], cv["c_in"], cv["k"])
                np.testing.assert_array_equal(_bits(pairs), _bits(ref_p))
            else:
                ref_q, ref_p = R.pack(v)
                np.testing.assert_array_equal(_bits(np.array(pairs, f32)), _bits(np.array(ref_p, f32)))
            np.testing.assert_array_equal(codes, np.asarray(ref_q).reshape(-1))
        # affines(): bn1, bn2, [bn3], [the shortcut's] of each block, th_fold_batchnorm2d on the running pairs
        folds = [S.N.fold(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"]) for b in blocks for _, bn in S.block_convs(b)]
        got = q.affines()
        assert len(got) == len(folds)
        for a, ref in zip(got, folds):
            np.testing.assert_array_equal(_bits(a), _bits(ref))
        n_pairs = sum(p.shape[0] if isinstance(p, np.ndarray) else 1 for _, _, p in ts)
        step = TC._lib().th_qlinear_i8_kstep()
        c_out = specs[0][1][-2]
        lin_pad = CLASSES * (-(-c_out // step) * step) - CLASSES * c_out
        assert q.storage_bytes() == sum(v.size for v in packed) + lin_pad + 8 * n_pairs + 4 * q.act_scales().size + 8 * sum(f.shape[0] for f in folds)
    # the stride-1 3x3 conv2 of the first block packs as the same buffer in a bare layer does through quantize_static_conv
    if specs[0][0] == "res":
        c = specs[0][1][1]
        bare = T.Conv2d(c, c, (3, 3), None, (1, 1), bias=False)
        bare.parameters()[0].set_data(layers[1].parameters()[3].data().reshape(-1))
        bq = bare.quantize_static_conv([T.Tensor(rng.standard_normal((1, c, 4, 4)).astype(f32), (1, c, 4, 4))])
        twin = _quantize(model, calib, CONVS | BLOCKS)
        np.testing.assert_array_equal(bq.tensors()[0][1], twin.tensors()[3][1])
        np.testing.assert_array_equal(_bits(np.array(bq.tensors()[0][2], f32)), _bits(np.array(twin.tensors()[3][2], f32)))
    T.Tape.reset()


def test_bare_exact_convs_are_static_with_the_flag():
    import taper_amd as T
    rng = np.random.default_rng(17)
    shape = (2, 4, 9, 9)
    layers = [T.Conv2d(4, 8, (3, 3), (2, 2), (1, 1), seed=3, exact_stride=True), T.ReLU(), T.Conv2d(8, 6, (1, 1), (2, 2), None, seed=4, exact_pointwise=True)]
    model = T.Sequential(layers)
    x = rng.standard_normal(shape).astype(f32)
    calib = [T.Tensor(x, shape)]
    for flags in (CONVS | BLOCKS, CONVS | BLOCKS | CHAIN, CONVS | BLOCKS | CHAIN | PER_CHANNEL):
        pc = bool(flags & PER_CHANNEL)
        q = _quantize(model, calib, flags)
        scales = q.act_scales()
        assert scales.shape == (2,) and q.chain_links() == (1 if flags & CHAIN else 0)
        (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2) = q.tensors()
        conv = P.conv_q8q8_pc if pc else Q.conv_q8q8
        h = conv(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 8, 4, (3, 3)), p1, b1, q1, (2, 2), (1, 1), True)
        ref = conv(Q.quantize_act_nchw(h, scales[1])[0], scales[1], Q.taper_weight(w2, 6, 8, (1, 1)), p2, b2, q2, (2, 2), (0, 0), False)
        assert ref.shape == (2, 6, 3, 3)
        np.testing.assert_array_equal(_bits(q(T.Tensor(x, shape)).data()), _bits(ref), err_msg=f"flags {flags}")
    # the calibrated scale of the second conv is the float model's own activation range: the exact conv ran in calibration
    fl = layers[1].forward(layers[0].forward(T.Tensor(x, shape))).data()
    T.Tape.reset()
    assert _bits(scales[1]) == _bits(R.act_scale_of(fl))


def test_refusals_with_and_without_the_flag():
    import taper_amd as T
    from taper_amd._lib import host
    rng = np.random.default_rng(19)
    shape = (2, 4, 8, 8)
    calib = [T.Tensor(rng.standard_normal(shape).astype(f32), shape)]
    default = T.Sequential([T.ResidualBlock(4, 8, 2, seed=1), T.Flatten(1)])      # the default strided paths: no convolutions
    good = T.Sequential([T.ResidualBlock.exact_stride(4, 8, 2, seed=1)])
    neck = T.Sequential([T.BottleneckBlock(4, 4, 8, 2, seed=1)])
    exact = T.Sequential([T.Conv2d(4, 8, (3, 3), (2, 2), (1, 1), exact_stride=True)])
    point = T.Sequential([T.Conv2d(4, 8, (1, 1), exact_pointwise=True)])
    T.Device.sync()
    before = _pool_in_use()
    for flags in (CONVS | BLOCKS, CONVS | BLOCKS | CHAIN | PER_CHANNEL | LINKS):
        with pytest.raises(T.TaperError, match=r"ResidualBlock: the block holds a default strided or 1x1 Conv2d.*no convolution \(SURVEY Q4 / Q9\).*exact_stride / pointwise_shortcut"):
            _quantize(default, calib, flags)
    assert _pool_in_use() == before
    # without the flag: today's refusals, today's messages
    for m in (default, good, neck):
        for call in (lambda: m.quantize("int8"), lambda: m.quantize_static(calib), lambda: m.quantize_static_conv(calib), lambda: m.quantize_static_chain(calib),
                     lambda: _quantize(m, calib, CONVS | CHAIN | PER_CHANNEL | LINKS)):
            with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
                call()
    for m, msg in ((exact, "exact-stride Conv2d: quantized twins are a follow-up"), (point, "exact-pointwise Conv2d: quantized twins are a follow-up")):
        for call in (lambda: m.quantize("int8"), lambda: m.quantize_static_conv(calib), lambda: _quantize(m, calib, CONVS | CHAIN)):
            with pytest.raises(T.TaperError, match=msg):
                call()
    # quantize() keeps the reference's refusal of the blocks whatever they are built from
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        good.quantize("float16")
    # the flag's own rules
    arr = (C.c_void_p * 1)(calib[0]._h)
    h = C.c_void_p()
    for flags, what in ((BLOCKS, b"TP_QBLOCKS needs TP_QSTATIC_CONVS"), (BLOCKS | PER_CHANNEL, b"TP_QBLOCKS needs TP_QSTATIC_CONVS"), (8 | CONVS | BLOCKS, b"unknown"),
                        (64 | CONVS, b"unknown"), (-1, b"unknown")):
        assert host.tp_module_quantize_static_ex(good._h, arr, 1, flags, C.byref(h)) != 0 and what in host.tp_last_error(), flags
        assert host.tp_module_quantize_static_cal(good._h, arr, 1, flags, 0, 0, 0, C.byref(h)) != 0 and what in host.tp_last_error(), flags
    assert _pool_in_use() == before
    q = good.quantize_static_residual(calib)
    assert q.chain_links() == 1 and q.act_scales().shape == (3,) and len(q.affines()) == 3 and len(q.tensors()) == 3
    assert _bits(q.act_scales()[0]) == _bits(q.act_scales()[2])


def test_the_source_model_still_trains_after_quantizing():
    import taper_amd as T
    rng = np.random.default_rng(23)
    model, layers, _ = _build("neck-4-4-8-s2", rng)
    calib = [T.Tensor(rng.standard_normal(SHAPE).astype(f32), SHAPE)]
    q = model.quantize_static_residual(calib, chain=True, per_channel=True, links=True, percentile=99.9, bins=256)
    x = rng.standard_normal(SHAPE).astype(f32)
    y0 = q(T.Tensor(x, SHAPE)).data()
    before = [p.data().copy() for p in model.parameters()]
    T.set_full_backward(True)
    try:
        T.Tape.reset()
        opt = T.Adam(model.parameters(), 1e-2)
        tr = T.Trainer(model, opt)
        loss = tr.train_step(T.Tensor(x, SHAPE), T.Tensor(rng.integers(0, CLASSES, SHAPE[0]).astype(f32), (SHAPE[0],)))[0]
        assert np.isfinite(loss)
        moved = [not np.array_equal(a, p.data()) for a, p in zip(before, model.parameters())]
        assert all(m for m, a in zip(moved, before) if a.ndim == 4), "a conv weight did not move"
        del tr, opt
    finally:
        T.set_full_backward(False)
        gc.collect()
        T.Tape.reset()
    np.testing.assert_array_equal(_bits(q(T.Tensor(x, SHAPE)).data()), _bits(y0))      # the twin is a snapshot
