"""The helper wave of th_mlp_tail's whole-tile kernel (mlp_tail_exact_kernel, the 4-wave instances up to hidden 128): wave 4 forms the
step size of the workgroup's fused Adam update and, in the lead head workgroup, the step log, db2, loss and hit count; waves 0..3 read the
step size from LDS behind the final barrier.  Through the C ABI on raw buffers, every comparison on bits:

1. the gradients, loss, hit count, log entry and state words do not depend on which updates are fused;
2. the fused p / m / v of W1 and b1 are what a stand-alone th_adam_slices launch makes of the stored dW1 / db1 and the same starting
   p / m / v, t, lr -- W1 and b1 with DIFFERENT counters and learning rates, so a swapped or shared step size shows;
3. guard words around every buffer the launch may write stay as they were.

Shapes: the smallest at which the helper can go wrong (upper waves without rows, a dW1 group whose second tile is absent, one to sixteen
classes), and two instances WITHOUT a helper (8 waves; hidden 256) that guard the dispatch on the block size.
"""
import ctypes as C

import numpy as np
import pytest

from taper_amd.hip import AdamFuse, AdamSlice
from tests.test_gpu_step_tails import BETAS, LOG_STATES, MAX_SLICES

pytestmark = pytest.mark.gpu
G = 4                                       # guard words on either side (keeps the 16-byte alignment of what follows)
GUARD_F32 = np.uint32(0x7FC0BEEF)           # a NaN no arithmetic here produces
GUARD_I64 = np.int64(-0x0123456789ABCDEF)
LRS = (1e-3, 3e-2)                          # W1's, b1's


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


class Guarded:
    """a device buffer with guard words in front of and behind the part the launch is given"""

    def __init__(self, ctx, host):
        host = np.ascontiguousarray(host).ravel()
        self.ctx, self.n, self.dtype = ctx, host.size, host.dtype
        pad = np.full(G, GUARD_F32).view(np.float32) if host.dtype == np.float32 else np.full(G, GUARD_I64 if host.dtype == np.int64 else 0x5EEDBEE5, host.dtype)
        self.pad = pad
        self.buf = ctx.upload(np.concatenate([pad, host, pad]))
        self.ptr = int(self.buf) + G * host.dtype.itemsize

    def get(self, what):
        a = self.ctx.download(self.buf, (self.n + 2 * G,), self.dtype)
        u = np.uint32 if self.dtype.itemsize == 4 else np.uint64
        np.testing.assert_array_equal(a[:G].view(u), self.pad.view(u), err_msg=f"{what}: written in front of the buffer")
        np.testing.assert_array_equal(a[-G:].view(u), self.pad.view(u), err_msg=f"{what}: written behind the buffer")
        return a[G:-G]


_data = {}


def tail_data(batch, inf, hid, cls):
    """operands and starting p / m / v of one shape, made once"""
    key = (batch, inf, hid, cls)
    if key not in _data:
        rng = np.random.default_rng(batch * 1009 + inf * 31 + hid * 7 + cls)
        f = np.float32
        _data[key] = dict(
            x=rng.uniform(0, 1, (batch, inf)).astype(f), h=np.maximum(rng.standard_normal((batch, hid)), 0).astype(f),
            w2=rng.uniform(-0.3, 0.3, (cls, hid)).astype(f), b2=rng.uniform(-0.1, 0.1, cls).astype(f), y=rng.integers(0, cls, batch).astype(f),
            w1=(rng.uniform(-1, 1, (hid, inf)) * np.sqrt(2.0 / inf)).astype(f), b1=rng.uniform(-0.1, 0.1, hid).astype(f),
            mw=(rng.standard_normal(hid * inf) * 0.01).astype(f), vw=rng.uniform(0, 1e-4, hid * inf).astype(f),
            mb=(rng.standard_normal(hid) * 0.01).astype(f), vb=rng.uniform(0, 1e-4, hid).astype(f))
    return _data[key]


GRADS = ("dw1", "db1", "dw2", "db2", "loss", "nc", "metrics", "state")


def run_tail(ctx, shape, fuse_w, fuse_b, ts=(5, 1000), with_dx=False, capacity=4096, state0=5, slots=8):
    """one th_mlp_tail launch on fresh guarded buffers: everything it wrote (guards checked), and the buffers' starting values"""
    batch, inf, hid, cls = shape
    d = tail_data(*shape)
    up = {k: ctx.upload(d[k]) for k in ("x", "h", "w2", "b2", "y")}
    nan = lambda n: np.full(n, np.nan, np.float32)
    g = dict(dw1=Guarded(ctx, nan(hid * inf)), db1=Guarded(ctx, nan(hid)), dw2=Guarded(ctx, nan(cls * hid)), db2=Guarded(ctx, nan(cls)),
             loss=Guarded(ctx, nan(1)), nc=Guarded(ctx, nan(1)), metrics=Guarded(ctx, np.full(2 * slots, -1.0, np.float32)),
             state=Guarded(ctx, np.array([state0, (1 << 35) + 11], np.int64)),
             w1=Guarded(ctx, d["w1"]), mw=Guarded(ctx, d["mw"]), vw=Guarded(ctx, d["vw"]),
             b1=Guarded(ctx, d["b1"]), mb=Guarded(ctx, d["mb"]), vb=Guarded(ctx, d["vb"]),
             ticks=Guarded(ctx, np.array(ts, np.int32)), lrs=Guarded(ctx, np.array(LRS, np.float32)))
    if with_dx:
        g["dx"] = Guarded(ctx, nan(batch * inf))
    wf = AdamFuse(g["w1"].ptr, g["mw"].ptr, g["vw"].ptr, g["ticks"].ptr, g["lrs"].ptr, *BETAS) if fuse_w else None
    bf = AdamFuse(g["b1"].ptr, g["mb"].ptr, g["vb"].ptr, g["ticks"].ptr + 4, g["lrs"].ptr + 4, *BETAS) if fuse_b else None
    ctx.call("th_mlp_tail", up["x"], up["h"], up["w2"], up["b2"], up["y"], batch, inf, hid, cls, g["loss"].ptr, g["nc"].ptr, g["dw1"].ptr,
             g["db1"].ptr, g["dw2"].ptr, g["db2"].ptr, g["w1"].ptr if with_dx else None, g["dx"].ptr if with_dx else None, g["metrics"].ptr,
             capacity, g["state"].ptr, batch, C.byref(wf) if wf else None, C.byref(bf) if bf else None)
    out = {k: v.get(k) for k, v in g.items()}
    np.testing.assert_array_equal(out["ticks"], np.array(ts, np.int32))          # read, never written
    np.testing.assert_array_equal(out["lrs"].view(np.uint32), np.array(LRS, np.float32).view(np.uint32))
    for k in ("dw1", "db1", "dw2", "db2", "loss", "nc") + (("dx",) if with_dx else ()):
        assert not np.isnan(out[k]).any(), f"{k}: not every element was written"
    return out, d


def same_bits(got, want, what):
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=what)


def adam_alone(ctx, p, m, v, grad, t, lr):
    """th_adam_slices on copies: the stand-alone update of one tensor"""
    dp, dm, dv, dg = ctx.upload(p), ctx.upload(m), ctx.upload(v), ctx.upload(grad)
    tick, dlr = ctx.upload(np.array([t, 0], np.int32)), ctx.upload(np.array([lr], np.float32))
    arr = (AdamSlice * MAX_SLICES)()
    arr[0] = AdamSlice(int(dg), p.size, AdamFuse(int(dp), int(dm), int(dv), int(tick), int(dlr), *BETAS))
    ctx.call("th_adam_slices", arr, 1)
    return [ctx.download(b, (p.size,)) for b in (dp, dm, dv)]


def check_updates(ctx, out, d, fuse_w, fuse_b, ts, what):
    for fused, names, grad, t, lr in ((fuse_w, ("w1", "mw", "vw"), "dw1", ts[0], LRS[0]), (fuse_b, ("b1", "mb", "vb"), "db1", ts[1], LRS[1])):
        start = [d[k].ravel() for k in names]
        want = adam_alone(ctx, *start, out[grad], t, lr) if fused else start
        for k, w in zip(names, want):
            same_bits(out[k], w, f"{what}: {k} ({'fused' if fused else 'must stay untouched'})")
        if fused:
            assert not np.array_equal(out[names[0]], start[0]), f"{what}: {names[0]} did not move"


# (batch, in_features, hidden, classes)
HELPER_SHAPES = [(16, 16, 32, 10), (32, 16, 32, 10), (64, 16, 32, 10), (16, 48, 32, 10), (32, 48, 32, 10), (64, 48, 32, 10), (64, 48, 128, 10),
                 (16, 16, 32, 1), (64, 48, 32, 1), (32, 48, 32, 16), (64, 16, 32, 16), (64, 48, 128, 1), (64, 48, 128, 16)]
PLAIN_SHAPES = [(80, 48, 32, 10), (80, 48, 128, 16), (16, 48, 256, 10), (64, 16, 256, 1)]       # 8 waves; hidden 256: no helper wave
T_PAIRS = [(1, 2), (2, 1), (1000, 4097), (4097, (1 << 24) + 1), ((1 << 24) + 1, 1000)]             # (W1's t, b1's t)
FUSIONS = [(False, False), (True, False), (False, True), (True, True)]
CASES = [(s, (5, 1000)) for s in HELPER_SHAPES + PLAIN_SHAPES] + [(s, ts) for s in ((16, 16, 32, 10), (64, 48, 128, 10)) for ts in T_PAIRS]


@pytest.mark.parametrize("shape,ts", CASES, ids=lambda v: "x".join(map(str, v)))
def test_fused_updates_leave_the_gradients_alone_and_equal_the_stand_alone_update(ctx, shape, ts):
    ref = None
    for fuse_w, fuse_b in FUSIONS:
        what = f"{shape} t={ts} fuse_w={fuse_w} fuse_b={fuse_b}"
        out, d = run_tail(ctx, shape, fuse_w, fuse_b, ts)
        if ref is None:
            ref = out
            want = np.full((8, 2), -1.0, np.float32)
            want[5] = [out["loss"][0], out["nc"][0]]
            same_bits(out["metrics"], want.ravel(), f"{what}: log entry")
            assert out["state"].tolist() == [6, (1 << 35) + 11 + shape[0]]
        for k in GRADS:
            same_bits(out[k], ref[k], f"{what}: {k} differs from the launch without fused updates")
        check_updates(ctx, out, d, fuse_w, fuse_b, ts, what)


@pytest.mark.parametrize("batch,inf", [(16, 16), (64, 48), (80, 48)], ids=["b16", "b64", "b80_no_helper"])
def test_dx_role_with_the_helper_wave(ctx, batch, inf):
    """with d_dx the launch has a third role without barriers (the helper wave just leaves) and reads W1, whose update is deferred"""
    shape, ts = (batch, inf, 32, 10), (5, 1000)
    plain, _ = run_tail(ctx, shape, False, False, ts)
    ref, _ = run_tail(ctx, shape, False, False, ts, with_dx=True)
    out, d = run_tail(ctx, shape, False, True, ts, with_dx=True)
    for k in GRADS:
        same_bits(ref[k], plain[k], f"{k}: changed by the dX role")
    for k in GRADS + ("dx",):
        same_bits(out[k], ref[k], f"{k}: differs from the launch without the fused b1 update")
    check_updates(ctx, ref, d, False, False, ts, "dx, nothing fused")
    check_updates(ctx, out, d, False, True, ts, "dx, b1 fused")


@pytest.mark.parametrize("capacity,state0", LOG_STATES)
@pytest.mark.parametrize("shape", [(16, 16, 32, 10), (64, 48, 128, 10), (80, 48, 32, 10)], ids=["b16", "flagship_hidden", "b80_no_helper"])
def test_step_log_from_the_helper_wave(ctx, shape, capacity, state0):
    """the wrap branch, the 32-bit and the 64-bit remainder of the log slot; the capacity influences nothing else"""
    slots = min(capacity, 4096)
    slot = state0 if state0 < capacity else state0 % capacity
    assert slot < slots
    ref, _ = run_tail(ctx, shape, True, True)
    out, d = run_tail(ctx, shape, True, True, capacity=capacity, state0=state0, slots=slots)
    want = np.full((slots, 2), -1.0, np.float32)
    want[slot] = [ref["loss"][0], ref["nc"][0]]
    same_bits(out["metrics"], want.ravel(), "log entry")
    assert out["state"].tolist() == [state0 + 1, (1 << 35) + 11 + shape[0]]
    for k in ("dw1", "db1", "dw2", "db2", "loss", "nc", "w1", "mw", "vw", "b1", "mb", "vb"):
        same_bits(out[k], ref[k], k)
