"""The split form of th_mlp_tail's launch (mlp_tail_split_kernel) with an argument block of its own -- the first loads' pointers and the
counts in the block's first line, the rest fetched behind them -- and with gradient slots that may be null beside a fused update
(th_mlp_tail_drops_grads).  Against the 320-thread form of the SAME launch
(th_mlp_tail_set_split(ctx, 0)), whose kernel and arguments are untouched, through the C ABI on raw guarded buffers and ON BITS: loss, hit
count, dW1, db1, dW2, db2, every p / m / v, the step log.  Both forms run the same MFMA and FMA chains in the same order.

Shapes: the smallest at which each path can go wrong -- batch 16 (three pairs without rows), 48, 64; in_features 16 (no second tile
anywhere), 48 (only the last column group lacks its second tile), 80; hidden 32 / 64 / 128 (every instance of the split kernel); 1, 10 and 16
classes (the class mask at both ends); with and without b2; with and without the fused updates.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from taper_amd._lib import INCLUDE, hip as lib, parse_header
from taper_amd.hip import AdamFuse
from tests import backends
from tests.test_gpu_step_tails import BETAS
from tests.test_gpu_tail_helper import LRS, Guarded, same_bits, tail_data

GRADS = ("dw1", "db1")
REST = ("dw2", "db2", "loss", "nc", "metrics", "state")
STATE = ("w1", "mw", "vw", "b1", "mb", "vb")
TS = (5, 1000)                # W1's t, b1's t
# (batch, in_features, hidden): every value of each beside every value of the two others' pairs at least once
SHAPES = [(16, 16, 32), (16, 48, 64), (16, 80, 128), (48, 16, 64), (48, 48, 128), (48, 80, 32), (64, 16, 128), (64, 48, 32), (64, 80, 64)]
CLASSES = (1, 10, 16)


def test_the_query_is_in_the_header_and_refuses_a_null_ctx():
    assert "th_mlp_tail_drops_grads" in parse_header(INCLUDE / "taper_hip.h")
    assert lib.th_mlp_tail_drops_grads(None, 64, 784, 128) == 0


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def run(ctx, shape, fused, with_b2=True, null_slots=False, split=True):
    """one th_mlp_tail launch on fresh guarded buffers: everything it wrote, guards checked.  null_slots: no d_dw1 / d_db1"""
    batch, inf, hid, cls = shape
    d = tail_data(*shape)
    up = {k: ctx.upload(d[k]) for k in ("x", "h", "w2", "b2", "y")}
    nan = lambda n: np.full(n, np.nan, np.float32)
    g = dict(dw1=Guarded(ctx, nan(hid * inf)), db1=Guarded(ctx, nan(hid)), dw2=Guarded(ctx, nan(cls * hid)), db2=Guarded(ctx, nan(cls)),
             loss=Guarded(ctx, nan(1)), nc=Guarded(ctx, nan(1)), metrics=Guarded(ctx, np.full(16, -1.0, np.float32)),
             state=Guarded(ctx, np.array([5, (1 << 35) + 11], np.int64)),
             w1=Guarded(ctx, d["w1"]), mw=Guarded(ctx, d["mw"]), vw=Guarded(ctx, d["vw"]),
             b1=Guarded(ctx, d["b1"]), mb=Guarded(ctx, d["mb"]), vb=Guarded(ctx, d["vb"]),
             ticks=Guarded(ctx, np.array(TS, np.int32)), lrs=Guarded(ctx, np.array(LRS, np.float32)))
    wf = AdamFuse(g["w1"].ptr, g["mw"].ptr, g["vw"].ptr, g["ticks"].ptr, g["lrs"].ptr, *BETAS) if fused else None
    bf = AdamFuse(g["b1"].ptr, g["mb"].ptr, g["vb"].ptr, g["ticks"].ptr + 4, g["lrs"].ptr + 4, *BETAS) if fused else None
    try:
        ctx.call("th_mlp_tail_set_split", int(split))
        ctx.call("th_mlp_tail", up["x"], up["h"], up["w2"], up["b2"] if with_b2 else None, up["y"], batch, inf, hid, cls, g["loss"].ptr,
                 g["nc"].ptr, None if null_slots else g["dw1"].ptr, None if null_slots else g["db1"].ptr, g["dw2"].ptr, g["db2"].ptr, None, None,
                 g["metrics"].ptr, 4096, g["state"].ptr, batch, C.byref(wf) if wf else None, C.byref(bf) if bf else None)
    finally:
        ctx.call("th_mlp_tail_set_split", 1)
    out = {k: v.get(k) for k, v in g.items()}
    for k in GRADS:
        assert np.isnan(out[k]).all() if null_slots else not np.isnan(out[k]).any(), f"{k}: {'written without a slot' if null_slots else 'not every element was written'}"
    for k in ("dw2", "db2", "loss", "nc"):
        assert not np.isnan(out[k]).any(), f"{k}: not every element was written"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"c{c}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_split_form_equals_the_320_thread_form(ctx, shape, cls):
    for with_b2 in (True, False):
        for fused in (False, True):
            what = f"{shape} C={cls} b2={with_b2} fused={fused}"
            on, off = run(ctx, shape + (cls,), fused, with_b2), run(ctx, shape + (cls,), fused, with_b2, split=False)
            for k in GRADS + REST + STATE:
                same_bits(on[k], off[k], f"{what}: {k} differs between the split and the 320-thread form")
            assert on["state"].tolist() == [6, (1 << 35) + 11 + shape[0]]
            assert on["metrics"].reshape(8, 2)[5].tolist() == [on["loss"][0], on["nc"][0]]
            if fused:
                assert not np.array_equal(on["w1"], tail_data(*shape, cls)["w1"].ravel()), f"{what}: W1 did not move"


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"c{c}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_null_gradient_slots_change_nothing_else(ctx, shape, cls):
    """d_dw1 == d_db1 == NULL beside the fused updates: the same p / m / v and everything else as with the slots, whose gradients in turn
    are the 320-thread form's"""
    full = shape + (cls,)
    assert lib.th_mlp_tail_drops_grads(ctx.h, *shape) == 1
    for with_b2 in (True, False):
        kept, dropped, off = run(ctx, full, True, with_b2), run(ctx, full, True, with_b2, null_slots=True), run(ctx, full, True, with_b2, split=False)
        for k in REST + STATE:
            same_bits(dropped[k], kept[k], f"{full} b2={with_b2}: {k} differs without the gradient slots")
        for k in GRADS:
            same_bits(kept[k], off[k], f"{full} b2={with_b2}: {k} differs between the split and the 320-thread form")


@pytest.mark.gpu
def test_null_slots_are_refused_where_the_launch_would_store(ctx):
    """without the fused update the gradient has nowhere else to go; the 320-thread, the 8-wave and the hidden-256 launches always store"""
    assert lib.th_mlp_tail_drops_grads(ctx.h, 80, 48, 128) == 0 and lib.th_mlp_tail_drops_grads(ctx.h, 64, 48, 256) == 0
    assert lib.th_mlp_tail_drops_grads(ctx.h, 64, 50, 128) == 0
    with pytest.raises(Exception, match="d_dw1"):
        run(ctx, (64, 48, 128, 10), False, null_slots=True)
    with pytest.raises(Exception, match="d_dw1"):
        run(ctx, (64, 48, 128, 10), True, null_slots=True, split=False)
    with pytest.raises(Exception, match="d_dw1"):
        run(ctx, (80, 48, 128, 10), True, null_slots=True)
    try:
        ctx.call("th_mlp_tail_set_split", 0)
        assert lib.th_mlp_tail_drops_grads(ctx.h, 64, 48, 128) == 0
    finally:
        ctx.call("th_mlp_tail_set_split", 1)


@functools.lru_cache(maxsize=None)
def _trainer_run(chunk):
    import taper_amd as T
    rng = np.random.default_rng(96)
    spec = backends.mlp_baseline(rng)
    x, y = backends.mnist_like(rng, 96)
    model = backends.get("hip").sequential(spec)
    opt = T.Adam(model.parameters(), 1e-3, None, None, 1e-4)
    tr = T.Trainer(model, opt, **({"graph_chunk": chunk} if chunk else {}))
    ep = tr.run_epoch(T.DataLoader(T.MNISTDataset.from_host(x, y), 32, True, seed=7), T.Trainer.GRAPH, max_steps=3)
    return np.asarray(ep["losses"]), [p.data() for p in model.parameters()]


@pytest.mark.gpu
def test_three_trainer_steps_equal_a_graph_chunk_1_trainer():
    """784-128-10 at batch 32: the Trainer's fused step hands the launch no slot for dW1 / db1; losses and final parameters are those of a
    Trainer that enqueues step by step"""
    (losses, params), (ref_losses, ref_params) = _trainer_run(0), _trainer_run(1)
    assert len(losses) == 3 and np.isfinite(losses).all()
    np.testing.assert_array_equal(losses, ref_losses)
    for a, b in zip(params, ref_params):
        same_bits(np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel(), "final parameter")
