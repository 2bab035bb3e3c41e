"""Post-training quantization on the GPU (src/nn.rs:14-23, the quantized twins of nn.rs:62-504, tensor.rs:2084-2108): the quantized
Linear kernels against the oracle's sgemm on dequantized weights, the packed codes against the oracle's codecs bit for bit, whole
quantized models against the oracle's Sequential run with the dequantized weights, sizes, the untouched source model, the refusals and
the example driver."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from oracle import train_extra as OX
from tests import backends

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RTOL = 1e-4


def _err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / max(1.0, float(np.abs(ref).max())))


def _deq(kind, codes, params):
    return OX.dequantize_int8(codes, params[1], -128, params[0]) if kind == "int8" else OX.f16_bits_to_f32(codes)


# ---------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.mark.parametrize("qtype", ["int8", "f16"])
@pytest.mark.parametrize("K,N", [(784, 128), (128, 10), (100, 52), (1000, 3), (4096, 4096)])
@pytest.mark.parametrize("B", [1, 2, 3, 7, 8, 16, 17, 64, 257])
def test_linear_q_kernel_matches_sgemm_on_dequantized_weights(ctx, qtype, K, N, B):
    rng = np.random.default_rng(B * 7919 + K * 31 + N)
    s = np.sqrt(2.0 / K)
    w = rng.uniform(-s, s, (N, K)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    x = rng.standard_normal((B, K)).astype(np.float32)
    if qtype == "int8":
        qw, ws, _, wm = OX.quantize_int8(w)
        qb, bs, _, bm = OX.quantize_int8(b)
        wdeq, bdeq = OX.dequantize_int8(qw, ws, -128, wm), OX.dequantize_int8(qb, bs, -128, bm)
        dw, db = ctx.upload(qw.view(np.uint8)), ctx.upload(qb.view(np.uint8))
        dwp, dbp = ctx.upload(np.array([wm, ws], np.float32)), ctx.upload(np.array([bm, bs], np.float32))
    else:
        hw, hb = OX.f32_to_f16_bits(w), OX.f32_to_f16_bits(b)
        wdeq, bdeq = OX.f16_bits_to_f32(hw).reshape(N, K), OX.f16_bits_to_f32(hb)
        dw, db = ctx.upload(hw), ctx.upload(hb)
    prod = O.sgemm_rowmajor(0, 1, B, N, K, 1.0, x, wdeq.reshape(N, K), 0.0, np.zeros((B, N), np.float32))
    dx, dy = ctx.upload(x), ctx.empty(B * N)
    for relu in (0, 1):
        for with_bias in (0, 1):
            ref = prod + bdeq[None, :] if with_bias else prod
            ref = np.where(ref > 0, ref, np.float32(0)) if relu else ref
            outs = []
            for _ in range(2):
                ctx.call("th_fill_f32", dy, float("nan"), B * N)
                if qtype == "int8":
                    ctx.call("th_linear_q8_fwd", dx, B, K, dw, N, dwp, db if with_bias else None, dbp if with_bias else None, relu, dy)
                else:
                    ctx.call("th_linear_h16_fwd", dx, B, K, dw, N, db if with_bias else None, relu, dy)
                outs.append(ctx.download(dy, (B, N)))
            assert np.isfinite(outs[0]).all()
            assert _err(outs[0], ref) <= RTOL, (relu, with_bias, _err(outs[0], ref))
            np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))   # bit-identical from run to run


def test_dequantize_multi_matches_the_codecs(ctx):
    rng = np.random.default_rng(4)
    a, b = (rng.standard_normal(1000) * 3).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    qa, sa, _, ma = OX.quantize_int8(a)
    hb = OX.f32_to_f16_bits(b)
    from taper_amd import hip as H
    ca, cb, pa = ctx.upload(qa.view(np.uint8)), ctx.upload(hb), ctx.upload(np.array([ma, sa], np.float32))
    oa, ob = ctx.empty(1000), ctx.empty(37)
    items = (H.QTensor * 2)(H.QTensor(int(ca), int(pa), int(oa), 1000, 0), H.QTensor(int(cb), None, int(ob), 37, 1))
    ctx.call("th_dequantize_multi", C.addressof(items), 2)
    np.testing.assert_array_equal(ctx.download(oa, (1000,)).view(np.uint32), OX.dequantize_int8(qa, sa, -128, ma).view(np.uint32))
    np.testing.assert_array_equal(ctx.download(ob, (37,)).view(np.uint32), OX.f16_bits_to_f32(hb).view(np.uint32))


# ---------------------------------------------------------------- models
def _grouped(rng):   # Conv2d(4, 8, 3x3, groups 2, pad 1) + ReLU, Flatten, Linear -- nn.rs:289-332
    bound = np.sqrt(2.0 / 18) * np.sqrt(3.0)
    return [dict(kind="conv2d", w=rng.uniform(-bound, bound, (8, 2, 3, 3)).astype(np.float32), b=np.zeros(8, np.float32), padding=(1, 1),
                 groups=2),
            dict(kind="relu"), dict(kind="flatten", start_dim=1), backends._lin(rng, 8 * 8 * 8, 10)]


def _no_bias(layer):
    layer["b"] = None
    return layer


def _mlp_nobias(rng):   # Linear layers built without a bias: the kernels' null bias pointers, one tensor a layer
    return [_no_bias(backends._lin(rng, 784, 100)), dict(kind="relu"), _no_bias(backends._lin(rng, 100, 10))]


def _cnn_nobias(rng):
    return [_no_bias(backends._conv(rng, 1, 8)), dict(kind="maxpool", kernel=(2, 2), stride=(2, 2)), _no_bias(backends._conv(rng, 8, 8, relu=False)),
            dict(kind="relu"), dict(kind="flatten", start_dim=1), _no_bias(backends._lin(rng, 8 * 4 * 4, 10))]


def _cnn_sigmoid_avg(rng):   # the pass-through twins no other model holds: Sigmoid, AvgPool2d, AdaptiveAvgPool2d
    return [backends._conv(rng, 1, 8, relu=False), dict(kind="sigmoid"), dict(kind="avgpool", kernel=(2, 2), stride=(2, 2)),
            backends._conv(rng, 8, 16), dict(kind="adaptive_avgpool", out=(1, 1)), dict(kind="flatten", start_dim=1), backends._lin(rng, 16, 10)]


def _nested(rng):   # a Sequential holding a Sequential that holds convs: the inner twin dequantizes its own convs, the outer one its own
    return [backends._conv(rng, 1, 4),
            dict(kind="sequential", layers=[backends._conv(rng, 4, 8), dict(kind="maxpool", kernel=(2, 2), stride=(2, 2)),
                                            dict(kind="sequential", layers=[backends._conv(rng, 8, 8, relu=False), dict(kind="relu")])]),
            dict(kind="flatten", start_dim=1), dict(kind="sequential", layers=[backends._lin(rng, 8 * 4 * 4, 32), dict(kind="relu")]),
            backends._lin(rng, 32, 10)]


def _conv17(rng):   # 17 convs = 34 conv tensors in one QSequential: two chunks of th_dequantize_multi (32 tensors a launch)
    return [backends._conv(rng, 2, 2) for _ in range(17)] + [dict(kind="flatten", start_dim=1), backends._lin(rng, 2 * 4 * 4, 10)]


MODELS = {"mlp_baseline": (backends.mlp_baseline, (784,)), "mlp_example": (backends.mlp_example, (784,)),
          "mlp_100_52": (backends.mlp_100_52, (784,)), "cnn_simple": (backends.cnn_simple, (1, 28, 28)),
          "cnn_reference": (backends.cnn_reference, (1, 28, 28)), "grouped": (_grouped, (4, 8, 8)),
          "mlp_nobias": (_mlp_nobias, (784,)), "cnn_nobias": (_cnn_nobias, (1, 8, 8)), "cnn_sigmoid_avg": (_cnn_sigmoid_avg, (1, 12, 12)),
          "nested": (_nested, (1, 8, 8)), "conv17": (_conv17, (2, 4, 4))}
MLPS = ("mlp_baseline", "mlp_example", "mlp_100_52")


def _flat(spec):
    """the layers of a spec in forward order, nested Sequentials opened (the same dicts: editing one edits the spec)"""
    out = []
    for s in spec:
        out += _flat(s["layers"]) if s["kind"] == "sequential" else [s]
    return out


def _max_batch():
    from taper_amd._lib import hip as H
    return int(H.th_qlinear_stream_max_batch())


def _hip_model(spec):
    import taper_amd as T
    if any(s["kind"] == "sequential" for s in spec):
        return T.Sequential([_hip_model(s["layers"]) if s["kind"] == "sequential" else backends.HipBackend().sequential([s]).layers[0] for s in spec])
    if any(s.get("groups", 1) > 1 for s in spec):
        layers = []
        for s in spec:
            if s["kind"] == "conv2d":
                co, cig, kh, kw = s["w"].shape
                l = T.Conv2d(cig * s["groups"], co, (kh, kw), (1, 1), s["padding"], None, s["groups"], True)
            elif s["kind"] == "relu":
                l = T.ReLU()
            elif s["kind"] == "flatten":
                l = T.Flatten(1)
            else:
                o, i = s["w"].shape
                l = T.Linear(i, o, True)
            if "w" in s:
                ps = l.parameters()
                ps[0].set_data(s["w"])
                ps[1].set_data(s["b"])
            layers.append(l)
        return T.Sequential(layers)
    return backends.HipBackend().sequential(spec)


def _reference_forward(spec, deq, x, shape):
    """the oracle's Sequential forward on the dequantized weights (the grouped convolution, which the oracle does not build, goes
    through the float HIP model holding the same weights; a nested Sequential computes what its layers in a row compute, so the oracle
    runs them flat)"""
    spec = [dict(s) for s in _flat(spec)]
    it = iter(deq)
    for s in spec:
        if "w" in s:
            s["w"] = next(it).reshape(s["w"].shape)
            if s.get("b") is not None:
                s["b"] = next(it)
    if any(s.get("groups", 1) > 1 for s in spec):
        import taper_amd as T
        return _hip_model(spec).forward(T.Tensor(x, (x.shape[0], *shape))).data()
    m = backends.OracleBackend().sequential(spec)
    return m.forward(O.Tensor(x, (x.shape[0], *shape))).data()


@pytest.mark.parametrize("mode", ["int8", "float16", "disabled"])
@pytest.mark.parametrize("name", list(MODELS))
def test_quantized_model_matches_oracle_on_dequantized_weights(name, mode):
    import taper_amd as T
    build, shape = MODELS[name]
    rng = np.random.default_rng(11)
    spec = build(rng)
    backends.nonzero_biases(_flat(spec), rng)
    model = _hip_model(spec)
    q = model.quantize("int8" if mode == "int8" else "float16") if mode != "disabled" else model.quantize("int4", enabled=False)
    ts = q.tensors()
    assert all(k == ("int8" if mode == "int8" else "float16") for k, _, _ in ts)
    assert len(ts) == sum(("w" in s) + (s.get("b") is not None) for s in _flat(spec))
    deq = [_deq(k, c, p) for k, c, p in ts]
    M = _max_batch()
    for B in (1, 64, 256) + ((M, M + 1, 2) if name in MLPS else ()):   # (the MLPs also on both sides of the switch between the Linear paths)
        x = rng.uniform(0, 1, (B, int(np.prod(shape)))).astype(np.float32)
        T.Tape.reset()
        xt = T.Tensor(x, (B, *shape)).requires_grad()
        y = q(xt)
        assert T.Tape.len() == 0 and y.tape_node() == 0   # inference: no tape node
        got = y.data()
        ref = np.asarray(_reference_forward(spec, deq, x, shape)).reshape(got.shape)
        assert _err(got, ref) <= RTOL, (B, _err(got, ref))


@pytest.mark.parametrize("mode", ["int8", "float16"])
@pytest.mark.parametrize("name", MLPS)
def test_quantized_mlp_across_the_switch_between_the_linear_paths(name, mode):
    """The same model on the same rows on both sides of th_qlinear_stream_max_batch(): the first max rows of a max + 1 batch (the
    dequantize workspace and th_linear_fwd) agree with the max batch (the streaming kernel) within RTOL, and the rows of the max batch
    are bit-identical to the rows sent one by one (each (weight row, batch row) accumulator of the streaming kernel is its own chain
    whose order depends on K and N only, layer after layer)."""
    import taper_amd as T
    build, shape = MODELS[name]
    rng = np.random.default_rng(13)
    model = _hip_model(backends.nonzero_biases(build(rng), rng))
    q = model.quantize(mode)
    M = _max_batch()
    x = rng.uniform(0, 1, (M + 1, 784)).astype(np.float32)

    def run(rows):
        return q(T.Tensor(rows, (rows.shape[0], *shape))).data()

    at_max, over = run(x[:M]), run(x)
    assert at_max.shape == (M, 10) and over.shape == (M + 1, 10) and np.isfinite(over).all()
    assert _err(over[:M], at_max) <= RTOL, _err(over[:M], at_max)
    for b in range(M):
        np.testing.assert_array_equal(run(x[b:b + 1])[0].view(np.uint32), at_max[b].view(np.uint32), err_msg=f"row {b} alone")


@pytest.mark.parametrize("name", ["mlp_baseline", "cnn_reference"])
def test_packed_codes_equal_the_oracle_codecs_bit_for_bit(name):
    build, _ = MODELS[name]
    spec = build(np.random.default_rng(3))      # the reference's zero biases: constant tensors
    model = _hip_model(spec)
    params = [p.data().reshape(-1) for p in model.parameters()]
    q8, q16 = model.quantize("int8"), model.quantize("float16")
    for p, (k, codes, (mn, scale)) in zip(params, q8.tensors()):
        rq, rs, rzp, rmn = OX.quantize_int8(p)
        assert k == "int8" and rzp == -128
        np.testing.assert_array_equal(codes, rq)
        assert np.float32(mn).view(np.uint32) == np.float32(rmn).view(np.uint32)
        assert np.float32(scale).view(np.uint32) == np.float32(rs).view(np.uint32)
        if not p.any():   # an all-zero bias: min == max, widened by 0.1 -- it dequantizes to ~3.9e-4, not 0 (tensor.rs:2127-2131)
            d = OX.dequantize_int8(codes, scale, -128, mn)
            assert (d != 0).all() and np.allclose(d, 3.9e-4, rtol=0.05), d[:4]
    assert any(not p.any() for p in params)
    for p, (k, codes, _) in zip(params, q16.tensors()):
        assert k == "float16"
        np.testing.assert_array_equal(codes, OX.f32_to_f16_bits(p))


@pytest.mark.parametrize("name", list(MODELS))
def test_storage_bytes_closed_form(name):
    build, _ = MODELS[name]
    model = _hip_model(build(np.random.default_rng(2)))
    ns = [p.numel() for p in model.parameters()]
    assert model.quantize("int8").storage_bytes() == sum(ns) + 8 * len(ns)
    assert model.quantize("float16").storage_bytes() == 2 * sum(ns)
    assert model.quantize("int8", enabled=False).storage_bytes() == 2 * sum(ns)


def test_source_model_keeps_training_bit_for_bit():
    import taper_amd as T
    spec = backends.nonzero_biases(backends.mlp_example(np.random.default_rng(8)), np.random.default_rng(9))
    x, y = backends.mnist_like(np.random.default_rng(10), 64)
    after = []
    for quantize_first in (False, True):
        model = _hip_model(spec)
        opt = T.Adam(model.parameters(), 1e-3)
        tr = T.Trainer(model, opt)
        if quantize_first:
            for kind in ("int8", "float16"):
                q = model.quantize(kind)
                q(T.Tensor(x, (64, 784))).data()
                del q
        tr.train_step(T.Tensor(x, (64, 784)), T.Tensor(y))
        after.append([p.data() for p in model.parameters()])
    for a, b in zip(*after):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _pool_in_use():
    import taper_amd as T
    from taper_amd._lib import hip as H
    r, u = C.c_size_t(), C.c_size_t()
    assert H.th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


def test_refusals_carry_the_reference_message_and_leak_nothing():
    import taper_amd as T
    model = T.Sequential([T.Linear(784, 128, True), T.ReLU(), T.Dropout(0.5), T.Linear(128, 10, True)])
    T.Device.sync()
    before = _pool_in_use()
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        model.quantize("int8")
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        T.Dropout(0.5).quantize("float16")
    assert _pool_in_use() == before
    plain = T.Sequential([T.Linear(784, 128, True), T.ReLU(), T.Linear(128, 10, True)])
    before_plain = _pool_in_use()
    for kind in ("int4", "bfloat16", "nf4"):
        with pytest.raises(T.TaperError, match="placeholder"):
            plain.quantize(kind)
    assert _pool_in_use() == before_plain
    q = model.layers[0].quantize("int8")   # the layers themselves still quantize
    assert q.storage_bytes() == 784 * 128 + 128 + 16


def test_ptq_example_prints_the_storage_sizes():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "examples")])
    out = subprocess.run([str(ROOT / "examples" / "_build" / "ptq_quantize"), "--data-dir", "/nonexistent", "--steps", "3", "--train-n", "256",
                          "--test-n", "128"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "Quantization Complete!" in out.stdout
    s8 = int(re.search(r"Int8 size: (\d+) bytes", out.stdout).group(1))
    s16 = int(re.search(r"Float16 size: (\d+) bytes", out.stdout).group(1))
    model = _hip_model(backends.cnn_reference(np.random.default_rng(0)))
    assert s8 == model.quantize("int8").storage_bytes()
    assert s16 == model.quantize("float16").storage_bytes()
    for line in ("Original model accuracy", "Int8 model accuracy", "Float16 model accuracy"):
        assert line in out.stdout
