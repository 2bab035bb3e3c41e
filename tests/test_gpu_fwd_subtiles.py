"""th_linear_fwd_ex's sub-tile forms (csrc/gemm.hip: a workgroup of the one-launch path owns an RM x RN sub-tile of a 16 x 16 MFMA tile)
against the 16 x 16 form: the same bits.  Every output element of v_mfma_f32_16x16x4_f32 is its own FMA chain over k, so H must not
change by a bit whichever rows share the MFMA -- against the same call with the context's switch off, against th_linear_fwd (the 16 x 16
kernel without the spare workgroup), and, on integer operands (tests/sgemm_ref.py: every sum exact), against numpy's float64 product.
WHICH instance a case takes is asserted through th_debug_linear_fwd_ex_plan, the host function the launch itself consumes."""
import ctypes as C

import numpy as np
import pytest

from taper_amd.hip import AdamFuse, AdamSlice
from tests import sgemm_ref as R

pytestmark = pytest.mark.gpu

# (batch, in, out, X's bytes off a 16-byte boundary): the smallest shapes at which each thing can go wrong
CASES = [
    (64, 784, 128, 0),    # the XCD map, all workgroups
    (128, 784, 128, 0),   # the batch-128 choice: the 16 x 16 form (nothing measured a gain there)
    (16, 256, 16, 0),     # one old tile cut into sub-tiles, whole chunks only
    (18, 784, 20, 0),     # a ragged last sub-tile in both directions
    (7, 260, 9, 0),       # fewer rows and columns than one sub-tile row; a last chunk of 4 k
    (5, 258, 10, 0),      # k % 4 != 0: element loads for both operands
    (18, 784, 20, 4),     # element loads for A only
]
IDS = ["x".join(map(str, c[:3])) + ("-xoff4" if c[3] else "") for c in CASES]
# the sub-tile instances th_linear_fwd_ex compiles: (rows, columns, waves, chunks per wave)
SUBTILE_INSTANCES = {(8, 8, 16, 1)}


def fwd_plan(batch, inf, outf, subtiles=1):
    from taper_amd._lib import hip
    out = (C.c_int * 8)()
    assert hip.th_debug_linear_fwd_ex_plan(batch, inf, outf, subtiles, out) == 0, hip.th_last_error()
    return dict(zip(("one_launch", "rm", "rn", "waves", "cpw", "grid_x", "grid_y", "xcd"), out))


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.call("th_linear_fwd_ex_set_subtiles", 1)
    c.close()


def test_every_subtile_instance_is_reached():
    reached = set()
    for b, i, o, _ in CASES:
        p = fwd_plan(b, i, o)
        assert p["one_launch"] == 1 and ((p["rm"], p["rn"]) != (16, 16)) == (b <= 64), (b, i, o, p)   # every case but batch 128 runs a sub-tile form ...
        q = fwd_plan(b, i, o, 0)
        assert (q["rm"], q["rn"], q["waves"], q["cpw"]) == (16, 16, 16, 1), (b, i, o, q)  # ... and the 16-wave 16 x 16 form with the switch off
        if (p["rm"], p["rn"]) != (16, 16):
            reached.add((p["rm"], p["rn"], p["waves"], p["cpw"]))
    assert reached == SUBTILE_INSTANCES
    assert fwd_plan(64, 784, 128)["xcd"] == 1


def _upload_x(ctx, x, off):
    """X on the device, `off` bytes past a 16-byte boundary (the pool's blocks are 16-byte aligned)"""
    buf = ctx.empty(x.size + 4)
    assert int(buf) % 16 == 0
    from taper_amd._lib import hip
    assert hip.th_memcpy_h2d(ctx.h, int(buf) + off, x.ctypes.data, x.nbytes) == 0
    return buf, int(buf) + off


def _three_ways(ctx, x, w, b, case, relu, slices=None, n_slices=0, tick=None):
    """H of th_linear_fwd_ex with the switch on (carrying `slices` and `tick`), of the same call with the switch off, and of th_linear_fwd"""
    batch, inf, outf, off = case
    keep, dx = _upload_x(ctx, np.ascontiguousarray(x), off)
    dw, db = ctx.upload(w), (ctx.upload(b) if b is not None else None)
    out = []
    for which in ("on", "off", "fwd"):
        y = ctx.upload(np.full(batch * outf, np.nan, np.float32))
        if which == "fwd":
            ctx.call("th_linear_fwd", dx, dw, db, y, batch, inf, outf, relu)
        else:
            ctx.call("th_linear_fwd_ex_set_subtiles", int(which == "on"))
            if which == "on":
                ctx.call("th_linear_fwd_ex", dx, dw, db, y, batch, inf, outf, relu, slices, n_slices, tick)
            else:
                ctx.call("th_linear_fwd_ex", dx, dw, db, y, batch, inf, outf, relu, None, 0, None)
        out.append(ctx.download(y, (batch, outf)))
    ctx.call("th_linear_fwd_ex_set_subtiles", 1)
    del keep
    return out


def _floats(case, seed):
    batch, inf, outf, _ = case
    rng = np.random.default_rng([seed, batch, inf, outf])
    return (rng.uniform(0, 1, (batch, inf)).astype(np.float32), rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32),
            rng.uniform(-0.1, 0.1, outf).astype(np.float32))


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("bias", [0, 1], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_h_is_bit_identical_without_the_tick(ctx, case, bias, relu):
    batch, inf, outf, _ = case
    x, w, b = _floats(case, 1)
    on, off, fwd = _three_ways(ctx, x, w, b if bias else None, case, relu)
    assert not np.isnan(on).any()
    assert on.tobytes() == off.tobytes(), f"{np.count_nonzero(on != off)} of {on.size} elements differ from the 16 x 16 launch"
    assert on.tobytes() == fwd.tobytes(), f"{np.count_nonzero(on != fwd)} of {on.size} elements differ from th_linear_fwd"
    # integer operands: exact in every summation order, so float64 gives the float32 bits
    sc = (0, 1, batch, outf, inf)
    a, bt, _, ib = R.operands(sc, seed=2)
    want = R.epilogue(R.product64(sc, a, bt), 1.0, 0.0, None, ib if bias else None, bool(relu))
    on, off, fwd = _three_ways(ctx, a, bt, ib if bias else None, case, relu)
    assert on.tobytes() == want.tobytes() and off.tobytes() == want.tobytes() and fwd.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_carried_slices_and_the_tick(ctx, case):
    """two carried Adam slices and the tick beside the sub-tiles: p / m / v as th_adam_slices leaves them, t one further, H unchanged"""
    batch, inf, outf, _ = case
    x, w, b = _floats(case, 3)
    rng = np.random.default_rng([4, batch, inf, outf])
    t = 7
    dlr = ctx.upload(np.array([1e-3], np.float32))
    ticks = [ctx.upload(np.array([t, 0], np.int32)) for _ in range(2)]
    sizes, host, bufs = (1280, 10), [], [[], []]
    for n in sizes:
        host.append([rng.uniform(-0.1, 0.1, n).astype(np.float32), (rng.standard_normal(n) * 1e-3).astype(np.float32),
                     rng.uniform(0, 1e-5, n).astype(np.float32), (rng.standard_normal(n) * 0.01).astype(np.float32)])
    sl = []
    for side in range(2):       # [0]: carried by the forward launch; [1]: th_adam_slices on copies, same counter value
        arr = (AdamSlice * 2)()
        for i, n in enumerate(sizes):
            d = [ctx.upload(a) for a in host[i]]
            bufs[side].append(d)
            arr[i] = AdamSlice(int(d[3]), n, AdamFuse(int(d[0]), int(d[1]), int(d[2]), int(ticks[side]), int(dlr), 0.9, 0.999, 1e-8, 1e-4))
        sl.append(arr)
    on, off, fwd = _three_ways(ctx, x, w, b, case, 1, sl[0], 2, ticks[0])
    assert on.tobytes() == off.tobytes() and on.tobytes() == fwd.tobytes()
    ctx.call("th_adam_slices", sl[1], 2)
    for i, n in enumerate(sizes):
        for j, name in enumerate("pmv"):
            got, want = ctx.download(bufs[0][i][j], (n,)), ctx.download(bufs[1][i][j], (n,))
            assert got.tobytes() == want.tobytes(), (name, i)
            assert got.tobytes() != host[i][j].tobytes(), (name, i)       # ... and the update did happen
    assert ctx.download(ticks[0], 2, np.int32)[0] == t + 1
    assert ctx.download(ticks[1], 2, np.int32)[0] == t
