"""Every kernel that applies Adam in its epilogue against the library's stand-alone path, BIT FOR BIT: one row per entry point and
kernel form that fuses the update (csrc/adam_dev.h states optim.rs:99-110 once, as adam_moments / adam_param; a site keeps its own loads
and stores around them, and five epilogues still write the lines out -- this file is what holds those to the same bits).

Each row: (1) the entry without fuse descriptors writes the gradient; (2) th_adam_slices applies that gradient to copies of p0 / m0 / v0
with the same pre-ticked counter: the expectation; (3) the entry with the descriptors runs on fresh copies; (4) p, m, v compared as
uint32.  The state exercises every term: m0 random and nonzero, v0 random and >= 0, weight decay 1e-4, the counter at t >= 2 (the
oracle comparisons elsewhere start from m = v = 0, which hides beta1 * m and beta2 * v)."""
import ctypes as C

import numpy as np
import pytest

from tests import sgemm_ref
from taper_amd.hip import AdamFuse, AdamSlice, Mlp3Gap, Mlp3Layer, RowSource, WideFuse

pytestmark = pytest.mark.gpu
LR, T0, B1, B2, EPS, WD = 1e-2, 3, 0.9, 0.999, 1e-8, 1e-4


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _lib():
    from taper_amd._lib import hip as lib
    return lib


class Param:
    """p0 / m0 / v0 of one parameter on the host; every dev() is a fresh copy on the device"""

    def __init__(self, rng, p0):
        self.p0 = np.ascontiguousarray(p0, np.float32).reshape(-1)
        self.n = self.p0.size
        self.m0 = (rng.standard_normal(self.n) * 0.01).astype(np.float32)
        self.m0[self.m0 == 0] = np.float32(0.01)
        self.v0 = ((rng.standard_normal(self.n) * 0.01) ** 2).astype(np.float32)

    def dev(self, ctx):
        return [ctx.upload(self.p0), ctx.upload(self.m0), ctx.upload(self.v0)]


def _fuse(bufs, tick, lr):
    return AdamFuse(int(bufs[0]), int(bufs[1]), int(bufs[2]), int(tick), int(lr), B1, B2, EPS, WD)


def _counter(ctx, t=T0, words=4):
    return ctx.upload(np.array([t] + [0] * (words - 1), np.int32)), ctx.upload(np.array([LR], np.float32))


def _bits(ctx, bufs, n):
    return [ctx.download(b, n).view(np.uint32) for b in bufs]


def _expect(ctx, par, grad, t):
    """th_adam_slices on copies of the state with this gradient (a device buffer) and the counter at t"""
    tick, lr = _counter(ctx, t)
    bufs = par.dev(ctx)
    sl = (AdamSlice * 1)(AdamSlice(int(grad), par.n, _fuse(bufs, tick, lr)))
    ctx.call("th_adam_slices", sl, 1)
    return _bits(ctx, bufs, par.n)


def _same(ctx, name, par, grad, fused_bufs, t=T0):
    want, got = _expect(ctx, par, grad, t), _bits(ctx, fused_bufs, par.n)
    assert np.any(want[0] != par.p0.view(np.uint32)), name        # the update moved something
    for what, w, g in zip("pmv", want, got):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what} differs from th_adam_slices on the same gradient")


# ------------------------------------------------------------------------------------------------------------------ th_linear_bwd_adam
def _linear_bwd(ctx, batch, inf, outf, with_dx):
    rng = np.random.default_rng(batch + inf + outf + with_dx)
    x = rng.uniform(0, 1, (batch, inf)).astype(np.float32)
    w = rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32)
    dy = (rng.standard_normal((batch, outf)) * 0.01).astype(np.float32)
    yact = np.maximum(rng.standard_normal((batch, outf)), 0).astype(np.float32)
    pw, pb = Param(rng, w), Param(rng, rng.uniform(-0.1, 0.1, outf))
    xd, dyd, yd = ctx.upload(x), ctx.upload(dy), ctx.upload(yact)
    dw, db = ctx.empty(w.size), ctx.empty(outf)
    dx = ctx.empty(x.size) if with_dx else None
    ctx.call("th_linear_bwd_adam", xd, ctx.upload(w), dyd, yd, dx, dw, db, batch, inf, outf, 0, None, None)
    tick, lr = _counter(ctx)
    bw, bb = pw.dev(ctx), pb.dev(ctx)
    fw, fb = _fuse(bw, tick, lr), _fuse(bb, tick, lr)
    dw2, db2 = ctx.empty(w.size), ctx.empty(outf)
    # with dX the kernel reads the weight it updates (the update is deferred behind the read); without, an untouched copy is the operand
    ctx.call("th_linear_bwd_adam", xd, bw[0] if with_dx else ctx.upload(w), dyd, yd, dx, dw2, db2, batch, inf, outf, 0, C.byref(fw), C.byref(fb))
    np.testing.assert_array_equal(ctx.download(dw2, w.size).view(np.uint32), ctx.download(dw, w.size).view(np.uint32), err_msg="dW: fused vs plain launch")
    _same(ctx, "W", pw, dw, bw)
    _same(ctx, "b", pb, db, bb)
    assert ctx.download(tick, 1, np.int32)[0] == T0


def _site_small16_epilogue_and_db_role(ctx):
    """batch 16, in 40, out 24 (ragged 16-tiles), no dX: W in sgemm_small16's epilogue, b in linear_bwd_small's db role"""
    assert _lib().th_linear_bwd_separate_products(16, 40, 24, 0, 1, 0) == 0
    _linear_bwd(ctx, 16, 40, 24, False)


def _site_w_deferred_to_a_slice_launch(ctx):
    """the same shape with dX: the launch reads W, so W's update runs behind it as a slice launch"""
    assert _lib().th_linear_bwd_separate_products(16, 40, 24, 1, 1, 0) == 0
    _linear_bwd(ctx, 16, 40, 24, True)


def _site_splitk_reduce(ctx, inf, outf):
    """batch 512, no dX: the one-launch form (th_linear_bwd_separate_products == 0) cuts dW = dY^T . X into batch / 256 = 2 K slices from
    512 rows on, and W's update rides in the reduce pass: splitk_reduce4 where mn % 4 == 0 (20 x 12; four elements per thread, the
    pool's buffers are 16-byte aligned), splitk_reduce otherwise (9 x 5: mn = 45).  th_debug_sgemm_plan does not describe this launch: it
    speaks for th_sgemm / the separate products"""
    assert _lib().th_linear_bwd_separate_products(512, inf, outf, 0, 1, 0) == 0
    _linear_bwd(ctx, 512, inf, outf, False)


def _site_sgemm_tile128_adam_epilogue(ctx):
    """batch 128, 1024 x 1024: the unsplit exact 128-tiles with the update in the tile epilogue"""
    p = sgemm_ref.plan(1, 0, 1024, 1024, 128)
    assert p["tile"] == 128 and p["form"] == sgemm_ref.EXACT and p["slices"] == 1 and p["reduce"] == sgemm_ref.NO_REDUCE, p
    assert _lib().th_linear_bwd_separate_products(128, 1024, 1024, 0, 1, 0) == 1
    _linear_bwd(ctx, 128, 1024, 1024, False)


# ------------------------------------------------------------------------------------------------------------------ classifier heads
def _site_linear_xent_head(ctx):
    """th_linear_xent_head at the smallest row of test_linear_xent_head: dW and db updates on the state requested at kernel entry"""
    batch, k, c = 1, 3, 2
    rng = np.random.default_rng(7)
    h = np.maximum(rng.standard_normal((batch, k)), 0).astype(np.float32) + np.float32(0.25)
    w = rng.uniform(-0.3, 0.3, (c, k)).astype(np.float32)
    pw, pb = Param(rng, w), Param(rng, rng.uniform(-0.1, 0.1, c))
    hd, yd = ctx.upload(h), ctx.upload(rng.integers(0, c, batch).astype(np.float32))
    dw, db, loss = ctx.empty(c * k), ctx.empty(c), ctx.empty(1)
    ctx.call("th_linear_xent_head", hd, ctx.upload(pw.p0), ctx.upload(pb.p0), yd, batch, k, c, None, loss, None, None, dw, db, None, 0, None, 0,
             None, None, None)
    tick, lr = _counter(ctx)
    bw, bb = pw.dev(ctx), pb.dev(ctx)
    fw, fb = _fuse(bw, tick, lr), _fuse(bb, tick, lr)
    ctx.call("th_linear_xent_head", hd, bw[0], bb[0], yd, batch, k, c, None, loss, None, None, ctx.empty(c * k), ctx.empty(c), None, 0, None, 0,
             None, C.byref(fw), C.byref(fb))
    _same(ctx, "W", pw, dw, bw)
    _same(ctx, "b", pb, db, bb)


def _site_linear_xent_wide_fused(ctx):
    """th_linear_xent_wide_fused at the smallest row of test_linear_xent_wide_fused_tail: W, b and the bias of the conv in front, the
    counter ticked in the launch (the updates run at t + 1); gradients from th_linear_xent_wide_ex + th_bias_from_colsum_adam"""
    batch, c_conv, hw, c = 40, 6, 50, 7
    k = c_conv * hw
    rng = np.random.default_rng(batch * 3 + k + c)
    h = np.maximum(rng.standard_normal((batch, k)), 0).astype(np.float32)
    pw = Param(rng, rng.uniform(-1, 1, (c, k)) * np.sqrt(2.0 / k))
    pb, pcb = Param(rng, rng.uniform(-0.1, 0.1, c)), Param(rng, rng.uniform(-0.3, 0.3, c_conv))
    hd, yd = ctx.upload(h), ctx.upload(rng.integers(0, c, batch).astype(np.float32))
    dw, db, cs, gcb, loss = ctx.empty(c * k), ctx.empty(c), ctx.empty(k), ctx.empty(c_conv), ctx.empty(1)
    ctx.call("th_linear_xent_wide_ex", hd, ctx.upload(pw.p0), ctx.upload(pb.p0), yd, batch, k, c, loss, None, None, dw, db, None, 0, None, 0, None, cs)
    ctx.call("th_bias_from_colsum_adam", cs, gcb, c_conv, hw, None, None, 0)
    tick, lr = _counter(ctx)
    bw, bb, bcb = pw.dev(ctx), pb.dev(ctx), pcb.dev(ctx)
    gcb2 = ctx.empty(c_conv)
    f = WideFuse(_fuse(bw, tick, lr), _fuse(bb, tick, lr), _fuse(bcb, tick, lr), int(gcb2), c_conv, hw)
    ctx.call("th_linear_xent_wide_fused", hd, bw[0], bb[0], yd, batch, k, c, loss, None, ctx.empty(c * k), ctx.empty(c), None, 0, None, 0, tick,
             ctx.empty(k), C.byref(f))
    np.testing.assert_array_equal(ctx.download(tick, 2, np.int32), [T0 + 1, 0])
    _same(ctx, "W", pw, dw, bw, T0 + 1)
    _same(ctx, "b", pb, db, bb, T0 + 1)
    _same(ctx, "conv bias", pcb, gcb, bcb, T0 + 1)


# ------------------------------------------------------------------------------------------------------------------ th_mlp_tail
def _tail(ctx, batch, inf, hid, c, comm=None):
    rng = np.random.default_rng(batch * 13 + inf + hid + c)
    x = rng.uniform(0, 1, (batch, inf)).astype(np.float32)
    w1 = rng.uniform(-1, 1, (hid, inf)).astype(np.float32) * np.float32(np.sqrt(2.0 / inf))
    b1 = rng.uniform(-0.1, 0.1, hid).astype(np.float32)
    h = np.maximum(x @ w1.T + b1, 0).astype(np.float32)
    pw, pb = Param(rng, w1), Param(rng, b1)
    xd, hd = ctx.upload(x), ctx.upload(h)
    w2d, b2d = ctx.upload(rng.uniform(-0.3, 0.3, (c, hid)).astype(np.float32)), ctx.upload(rng.uniform(-0.1, 0.1, c).astype(np.float32))
    yd = ctx.upload(rng.integers(0, c, batch).astype(np.float32))
    tick, lr = _counter(ctx)

    def launch(dw1, db1, fw, fb):
        common = (xd, hd, w2d, b2d, yd, batch, inf, hid, c, ctx.empty(1), None, dw1, db1, ctx.empty(c * hid), ctx.empty(c))
        if comm is None:
            ctx.call("th_mlp_tail", *common, None, None, None, 0, None, 0, fw, fb)
        else:
            from taper_amd._lib import th_check
            conv = [int(a) if hasattr(a, "ptr") else a for a in common]
            th_check(_lib().th_mlp_tail_dp(comm, ctx.h, *conv, None, 0, None, 0, fw, fb, int(tick)), "th_mlp_tail_dp")

    dw1, db1 = ctx.empty(hid * inf), ctx.empty(hid)
    launch(dw1, db1, None, None)          # (data parallel with the update fused: the reduced gradient is never written -- it comes from here)
    bw, bb = pw.dev(ctx), pb.dev(ctx)
    fw, fb = _fuse(bw, tick, lr), _fuse(bb, tick, lr)
    launch(ctx.empty(hid * inf), ctx.empty(hid), C.byref(fw), C.byref(fb))
    _same(ctx, "W1", pw, dw1, bw)
    _same(ctx, "b1", pb, db1, bb)
    assert ctx.download(tick, 1, np.int32)[0] == T0


# (1, 5, 4, 2): the smallest shape of test_gpu_mlp_tail.py, the general kernel; (16, 32, 64, 2): the smallest whole-tile shape with a
# data-parallel instance (hidden 64 / 128, batch and input whole 16-tiles), the whole-tile kernel
def _site_mlp_tail(ctx, *shape):
    assert _lib().th_mlp_tail_supported(*shape, 0) == 1
    _tail(ctx, *shape)


def _site_mlp_tail_dp_loopback(ctx):
    """th_mlp_tail_dp on a loopback communicator (this process as its own peer: (g + g) * 0.5 == g): the exchange's epilogues.  The general
    shape above has no data-parallel instance: the smallest whole-tile shape"""
    from taper_amd._lib import th_check
    lib, comm = _lib(), C.c_void_p()
    th_check(lib.th_comm_init_loopback(ctx.h, C.byref(comm)), "th_comm_init_loopback")
    try:
        assert lib.th_mlp_tail_dp_supported(comm, ctx.h, 16, 32, 64, 2) == 1
        _tail(ctx, 16, 32, 64, 2, comm)
        ctx.sync()
    finally:
        lib.th_comm_destroy(comm)


# ------------------------------------------------------------------------------------------------------------------ th_mlp2_xent, th_mlp3_xent
def _site_mlp2_xent(ctx, ksplit):
    """th_mlp2_xent at the smallest shape th_mlp2_xent_supported accepts: W1 in the finish launch's K-slice role (operands requested
    first), b1 / W2 / b2 through m2_apply; the launch ticks the counter, the updates run at t + 1"""
    batch, inf, hid, c = 32, 32 * ksplit, 4, 2      # (split by 3: three 32-wide k chunks, one per workgroup of a row block)
    lib = _lib()
    assert lib.th_mlp2_xent_supported(batch, inf, hid, c, batch) == 1
    assert lib.th_mlp2_xent_supported(batch - 1, inf, hid, c, batch) == 0 and lib.th_mlp2_xent_supported(batch, 28, hid, c, batch) == 0
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 1, (batch, inf)).astype(np.float32)
    par = dict(w1=Param(rng, rng.uniform(-1, 1, (hid, inf)) * np.sqrt(2.0 / inf)), b1=Param(rng, rng.uniform(-0.1, 0.1, hid)),
               w2=Param(rng, rng.uniform(-0.3, 0.3, (c, hid))), b2=Param(rng, rng.uniform(-0.1, 0.1, c)))
    names = ("w1", "b1", "w2", "b2")
    xd, yd = ctx.upload(x), ctx.upload(rng.integers(0, c, batch).astype(np.float32))
    src = RowSource(int(xd), int(yd), None, None, 0, batch)

    def launch(dev, grads, tick, fuses):
        ctx.call("th_mlp2_xent", C.byref(src), batch, inf, hid, c, *[dev[k] for k in names], *[grads[k] for k in names], ctx.empty(1), ctx.empty(1),
                 None, 0, None, 0, tick, *fuses)

    lib.th_debug_mlp2_ksplit(ksplit)
    try:
        grads = {k: ctx.empty(par[k].n) for k in names}
        launch({k: ctx.upload(par[k].p0) for k in names}, grads, None, [None] * 4)
        tick, lr = _counter(ctx)
        bufs = {k: par[k].dev(ctx) for k in names}
        fuses = [_fuse(bufs[k], tick, lr) for k in names]
        launch({k: bufs[k][0] for k in names}, {k: ctx.empty(par[k].n) for k in names}, tick, [C.byref(f) for f in fuses])
    finally:
        lib.th_debug_mlp2_ksplit(0)
    assert ctx.download(tick, 1, np.int32)[0] == T0 + 1
    for k in names:
        _same(ctx, k, par[k], grads[k], bufs[k], T0 + 1)


def _site_mlp3_layers_and_gap_bias(ctx):
    """th_mlp3_xent with a th_mlp3_gap (as test_mlp3_finishes_the_bias_of_the_conv_in_front) and every layer fused: in mlp3_grads_kernel the
    three W (small16_body's epilogue) and b (linear_db_role) updates, and the bias of the conv in front from the dX the first launch wrote"""
    B, in_f, h1, h2, c, hw = 256, 128, 128, 64, 10, 49
    rng = np.random.default_rng(12)
    dims = [(h1, in_f), (h2, h1), (c, h2)]
    net = [(Param(rng, rng.uniform(-1, 1, d) * np.sqrt(2.0 / d[1])), Param(rng, rng.uniform(-0.2, 0.2, d[0]))) for d in dims]
    xd, yd = ctx.upload(rng.uniform(0, 1, (B, in_f)).astype(np.float32)), ctx.upload(rng.integers(0, c, B).astype(np.float32))
    cnt = ctx.upload(rng.integers(0, hw + 1, (B, in_f)).astype(np.float32))
    pgb = Param(rng, rng.uniform(-0.2, 0.2, in_f))
    gx, loss = ctx.empty(B * in_f), ctx.empty(1)

    def launch(params, grads, fuses, gb, gap_fuse):
        ptr = lambda f: C.cast(C.pointer(f), C.c_void_p) if f is not None else None
        layers = (Mlp3Layer * 3)()
        for l in range(3):
            layers[l] = Mlp3Layer(int(params[l][0]), int(params[l][1]), int(grads[l][0]), int(grads[l][1]), ptr(fuses[l][0]), ptr(fuses[l][1]), dims[l][0])
        gap = Mlp3Gap(int(cnt), int(gb), hw, ptr(gap_fuse))
        ctx.call("th_mlp3_xent", xd, yd, B, in_f, C.cast(layers, C.c_void_p), gx, loss, None, None, 0, None, 0, None, C.cast(C.pointer(gap), C.c_void_p))

    new_grads = lambda: [(ctx.empty(w.n), ctx.empty(b.n)) for w, b in net]
    grads, gb = new_grads(), ctx.empty(in_f)
    launch([(ctx.upload(w.p0), ctx.upload(b.p0)) for w, b in net], grads, [(None, None)] * 3, gb, None)
    tick, lr = _counter(ctx)
    bufs, gbufs = [(w.dev(ctx), b.dev(ctx)) for w, b in net], pgb.dev(ctx)
    fuses = [(_fuse(bw, tick, lr), _fuse(bb, tick, lr)) for bw, bb in bufs]
    launch([(bw[0], bb[0]) for bw, bb in bufs], new_grads(), fuses, ctx.empty(in_f), _fuse(gbufs, tick, lr))
    for l, ((w, b), (bw, bb)) in enumerate(zip(net, bufs)):
        _same(ctx, f"W{l + 1}", w, grads[l][0], bw)
        _same(ctx, f"b{l + 1}", b, grads[l][1], bb)
    _same(ctx, "conv bias", pgb, gb, gbufs)
    assert ctx.download(tick, 1, np.int32)[0] == T0


def _site_wide_head_grads(ctx, n, k, classes, conv_c):
    """th_wide_head_grads (wide_grads_kernel, the launch behind the conv chain's classifier rows) on its own, at shapes of
    test_wide_head_grads_ragged_shapes: W in the dW epilogue on the state requested at entry, b and the last conv's bias from the column sums"""
    rng = np.random.default_rng(n + k + classes)
    x = ctx.upload(rng.standard_normal((n, k)).astype(np.float32))
    dl = np.zeros((n, 16), np.float32)
    dl[:, :classes] = (rng.standard_normal((n, classes)) / n).astype(np.float32)
    dl = ctx.upload(dl)
    rs = ctx.upload(np.stack([rng.uniform(0, 3, n), rng.integers(0, 2, n)], axis=1).astype(np.float32))
    cbp = ctx.upload(rng.standard_normal((n, conv_c)).astype(np.float32))
    pw, pb, pcb = Param(rng, rng.uniform(-0.3, 0.3, classes * k)), Param(rng, rng.uniform(-0.1, 0.1, classes)), Param(rng, rng.uniform(-0.3, 0.3, conv_c))
    dw, db, gcb, loss = ctx.empty(classes * k), ctx.empty(classes), ctx.empty(conv_c), ctx.empty(1)
    ctx.call("th_wide_head_grads", x, dl, rs, cbp, n, k, classes, conv_c, dw, db, gcb, loss, None, None, 0, None, 0, None, None, None)
    tick, lr = _counter(ctx)
    bw, bb, bcb = pw.dev(ctx), pb.dev(ctx), pcb.dev(ctx)
    fw, fb, fcb = _fuse(bw, tick, lr), _fuse(bb, tick, lr), _fuse(bcb, tick, lr)
    ctx.call("th_wide_head_grads", x, dl, rs, cbp, n, k, classes, conv_c, ctx.empty(classes * k), ctx.empty(classes), ctx.empty(conv_c), loss, None,
             None, 0, None, 0, C.byref(fw), C.byref(fb), C.byref(fcb))
    _same(ctx, "W", pw, dw, bw)
    _same(ctx, "b", pb, db, bb)
    _same(ctx, "conv bias", pcb, gcb, bcb)
    assert ctx.download(tick, 1, np.int32)[0] == T0


# ------------------------------------------------------------------------------------------------------------------ bias gradients of a conv
def _site_bias_grad_masked_adam(ctx, pooled_avg):
    n, c, hw = 6, 5, 9
    rng = np.random.default_rng(n + c + hw + pooled_avg)
    yp = ctx.upload(np.maximum(rng.standard_normal((n, c, hw)), 0).astype(np.float32))
    g = ctx.upload((rng.standard_normal((n, c) if pooled_avg else (n, c, hw)) * 0.01).astype(np.float32))
    par = Param(rng, rng.uniform(-0.1, 0.1, c))
    gb = ctx.empty(c)
    ctx.call("th_bias_grad_masked_adam", g, yp, gb, n, c, hw, pooled_avg, None, None, 0)
    tick, lr = _counter(ctx)
    bufs = par.dev(ctx)
    f = _fuse(bufs, tick, lr)
    ctx.call("th_bias_grad_masked_adam", g, yp, ctx.empty(c), n, c, hw, pooled_avg, C.byref(f), None, 0)
    _same(ctx, "bias", par, gb, bufs)


def _site_bias_from_colsum_adam(ctx, c, hw):
    rng = np.random.default_rng(c + hw)
    cs = ctx.upload((rng.standard_normal(c * hw) * 0.01).astype(np.float32))
    par = Param(rng, rng.uniform(-0.1, 0.1, c))
    gb = ctx.empty(c)
    ctx.call("th_bias_from_colsum_adam", cs, gb, c, hw, None, None, 0)
    tick, lr = _counter(ctx)
    bufs = par.dev(ctx)
    f = _fuse(bufs, tick, lr)
    ctx.call("th_bias_from_colsum_adam", cs, ctx.empty(c), c, hw, C.byref(f), None, 0)
    _same(ctx, "bias", par, gb, bufs)


def _site_bias_grad_counts_adam(ctx):
    n, c, hw = 6, 5, 9
    rng = np.random.default_rng(n + c + hw)
    g = ctx.upload((rng.standard_normal((n, c)) * 0.01).astype(np.float32))
    cnt = ctx.upload(rng.integers(0, hw + 1, (n, c)).astype(np.float32))
    par = Param(rng, rng.uniform(-0.1, 0.1, c))
    gb = ctx.empty(c)
    ctx.call("th_bias_grad_counts_adam", g, cnt, gb, n, c, hw, None, None, 0)
    tick, lr = _counter(ctx)
    bufs = par.dev(ctx)
    f = _fuse(bufs, tick, lr)
    ctx.call("th_bias_grad_counts_adam", g, cnt, ctx.empty(c), n, c, hw, C.byref(f), None, 0)
    _same(ctx, "bias", par, gb, bufs)


# ------------------------------------------------------------------------------------------------------------------ the optimizer's own kernels
def _site_adam_step_against_adam_slices(ctx, n, off):
    """th_adam_step (optim.hip's vector body and element tail) and th_adam_slices on the same inputs"""
    rng = np.random.default_rng(n)
    par = Param(rng, rng.uniform(-0.3, 0.3, n))
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    pad = np.zeros(off // 4, np.float32)
    up = lambda a: ctx.upload(np.concatenate([pad, a]))
    out = []
    for which in ("step", "slices"):
        tick, lr = _counter(ctx)
        bufs, gd = [up(par.p0), up(par.m0), up(par.v0)], up(g)
        ptr = [b.offset(off) for b in bufs]
        if which == "step":
            ctx.call("th_adam_step", ptr[0], gd.offset(off), ptr[1], ptr[2], ctx.upload(np.zeros(1, np.int64)), ctx.upload(np.ones(1, np.int32)), 1, n,
                     tick, lr, B1, B2, EPS, WD, 1)
        else:
            sl = (AdamSlice * 1)(AdamSlice(gd.offset(off), n, AdamFuse(ptr[0], ptr[1], ptr[2], int(tick), int(lr), B1, B2, EPS, WD)))
            ctx.call("th_adam_slices", sl, 1)
        out.append([ctx.download(p, n).view(np.uint32) for p in ptr])
        assert ctx.download(tick, 1, np.int32)[0] == T0
    assert np.any(out[0][0] != par.p0.view(np.uint32))
    for what, a, b in zip("pmv", *out):
        np.testing.assert_array_equal(a, b, err_msg=what)


def _site_allreduce_adam_one_rank(ctx):
    """th_allreduce_adam (comm.hip) on a one-rank peer-to-peer communicator connected to itself: the mean over one rank is the gradient.
    A tensor of 4099 elements; the exported arena holds whole quads, so it is 4100 floats long (the pad element is updated with the rest)"""
    from taper_amd._lib import th_check
    lib, comm = _lib(), C.c_void_p()
    n = 4100
    rng = np.random.default_rng(n)
    par = Param(rng, rng.uniform(-0.3, 0.3, n))
    g = ctx.upload((rng.standard_normal(n) * 0.01).astype(np.float32))
    th_check(lib.th_comm_init_p2p(ctx.h, 1, 0, C.byref(comm)), "th_comm_init_p2p")
    try:
        blob = (C.c_uint8 * 4096)()      # (TH_P2P_BLOB_BYTES is far below this)
        th_check(lib.th_comm_p2p_export(comm, int(g), n, blob), "th_comm_p2p_export")
        th_check(lib.th_comm_p2p_connect(comm, blob), "th_comm_p2p_connect")
        tick, lr = _counter(ctx)
        bufs = par.dev(ctx)
        th_check(lib.th_allreduce_adam(comm, ctx.h, int(g), n, 1.0, int(bufs[0]), int(bufs[1]), int(bufs[2]), int(ctx.upload(np.zeros(1, np.int64))),
                                       int(ctx.upload(np.ones(1, np.int32))), 1, int(tick), int(lr), B1, B2, EPS, WD, 1), "th_allreduce_adam")
        ctx.sync()
        _same(ctx, "arena", par, g, bufs)
    finally:
        lib.th_comm_destroy(comm)


ROWS = [
    ("small16_epilogue_and_db_role", _site_small16_epilogue_and_db_role, ()),
    ("w_deferred_to_a_slice_launch", _site_w_deferred_to_a_slice_launch, ()),
    ("splitk_reduce4", _site_splitk_reduce, (20, 12)),
    ("splitk_reduce", _site_splitk_reduce, (9, 5)),
    ("sgemm_tile128_adam_epilogue", _site_sgemm_tile128_adam_epilogue, ()),
    ("linear_xent_head", _site_linear_xent_head, ()),
    ("linear_xent_wide_fused", _site_linear_xent_wide_fused, ()),
    ("mlp_tail_general", _site_mlp_tail, (1, 5, 4, 2)),
    ("mlp_tail_whole_tiles", _site_mlp_tail, (16, 32, 64, 2)),
    ("mlp_tail_dp_loopback", _site_mlp_tail_dp_loopback, ()),
    ("mlp2_xent_ksplit_off", _site_mlp2_xent, (1,)),
    ("mlp2_xent_ksplit_3", _site_mlp2_xent, (3,)),
    ("mlp3_layers_and_gap_bias", _site_mlp3_layers_and_gap_bias, ()),
    ("wide_head_grads_smallest", _site_wide_head_grads, (1, 16, 1, 4)),
    ("wide_head_grads_ragged", _site_wide_head_grads, (37, 100, 7, 5)),
    ("allreduce_adam_one_rank", _site_allreduce_adam_one_rank, ()),
    ("bias_grad_masked_adam_nchw", _site_bias_grad_masked_adam, (0,)),
    ("bias_grad_masked_adam_pooled_avg", _site_bias_grad_masked_adam, (1,)),
    ("bias_from_colsum_adam_one_group", _site_bias_from_colsum_adam, (5, 9)),
    ("bias_from_colsum_adam_second_channel_group", _site_bias_from_colsum_adam, (70, 49)),
    ("bias_grad_counts_adam", _site_bias_grad_counts_adam, ()),
    ("adam_step_float4_body_and_tail", _site_adam_step_against_adam_slices, (4099, 0)),
    ("adam_step_4_bytes_off_a_16_byte_boundary", _site_adam_step_against_adam_slices, (1023, 4)),
]


@pytest.mark.parametrize("site,args", [pytest.param(f, a, id=i) for i, f, a in ROWS])
def test_fused_site_matches_standalone_adam(ctx, site, args):
    site(ctx, *args)
