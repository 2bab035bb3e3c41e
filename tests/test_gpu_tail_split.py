"""The split form of th_mlp_tail's whole-tile launch (mlp_tail_split_kernel: the instances with a helper wave -- batch <= 64, hidden <= 128,
no in-launch exchange -- run 576 threads: logit waves 0..3 park dlogits in LDS, operand waves 4..7 request everything the gradient products
need meanwhile and finish the tile, wave 8 is the helper) against the 320-thread form it replaces (th_mlp_tail_set_split(ctx, 0)).

Through the C ABI on raw guarded buffers, every comparison ON BITS and between the two forms of the SAME launch: dW1, db1, dW2, db2, loss,
hit count, the log entry, the state words, and p / m / v of W1 and b1 with the fused updates on and off, at t = 1 and t = 1000.  Both forms
run the same MFMA and FMA chains in the same order, so equality is exact.  Shapes: the smallest at which the split can go wrong.
"""
import pytest

from taper_amd._lib import INCLUDE, hip as lib, parse_header
from tests.test_gpu_tail_helper import GRADS, run_tail, same_bits

STATE = ("w1", "mw", "vw", "b1", "mb", "vb")
FUSIONS = [(False, False), (True, False), (False, True), (True, True)]
T_PAIRS = [(1, 1000), (1000, 1)]            # (W1's t, b1's t): both counters at both values
# (batch, in_features, hidden, classes)
SPLIT_SHAPES = [
    (16, 16, 32, 10),     # three pairs without rows
    (48, 48, 64, 10),     # one pair without rows; a last column group whose second tile is absent (48 = 32 + 16, as 784 = 24 x 32 + 16)
    (64, 48, 128, 10),    # the flagship's hidden width and wave count
    (64, 32, 128, 3),     # the class mask at both ends
    (64, 32, 128, 16),
]
EIGHT_WAVES = (80, 48, 128, 10)             # the 8-wave instance: the switch changes nothing


def test_switch_is_in_the_header_and_refuses_a_null_ctx():
    assert "th_mlp_tail_set_split" in parse_header(INCLUDE / "taper_hip.h")
    assert lib.th_mlp_tail_set_split(None, 1) != 0 and b"th_mlp_tail_set_split" in lib.th_last_error()
    assert lib.th_mlp_tail_set_split(None, 0) != 0


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def both_forms(ctx, *args, **kw):
    """the same launch on fresh buffers with the switch off and on; the context is left as it was made (on)"""
    try:
        ctx.call("th_mlp_tail_set_split", 0)
        off, _ = run_tail(ctx, *args, **kw)
    finally:
        ctx.call("th_mlp_tail_set_split", 1)
    on, _ = run_tail(ctx, *args, **kw)
    return on, off


def assert_same(on, off, keys, what):
    for k in keys:
        same_bits(on[k], off[k], f"{what}: {k} differs between the split and the 320-thread form")


@pytest.mark.gpu
@pytest.mark.parametrize("ts", T_PAIRS, ids=lambda v: "t" + "_".join(map(str, v)))
@pytest.mark.parametrize("shape", SPLIT_SHAPES + [EIGHT_WAVES], ids=lambda v: "x".join(map(str, v)))
def test_split_form_equals_the_320_thread_form(ctx, shape, ts):
    for fuse_w, fuse_b in FUSIONS:
        on, off = both_forms(ctx, shape, fuse_w, fuse_b, ts)
        assert_same(on, off, GRADS + STATE, f"{shape} t={ts} fuse_w={fuse_w} fuse_b={fuse_b}")
        assert on["state"].tolist() == [6, (1 << 35) + 11 + shape[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("ts", T_PAIRS, ids=lambda v: "t" + "_".join(map(str, v)))
def test_dx_role_beside_nine_wave_workgroups(ctx, ts):
    """with d_dx the launch has a third role without barriers: its logit waves work, its operand waves and helper leave; W1's update is deferred"""
    shape = (32, 16, 64, 10)
    for fuse_b in (False, True):
        on, off = both_forms(ctx, shape, False, fuse_b, ts, with_dx=True)
        assert_same(on, off, GRADS + STATE + ("dx",), f"{shape} with d_dx t={ts} fuse_b={fuse_b}")


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,state0", [(4096, 5000), ((1 << 33) + 1, (1 << 34) + 7)], ids=["wrap", "rem64"])
def test_step_log_in_the_split_form(ctx, capacity, state0):
    """the helper wave beside eight waves: the wrap branch and the 64-bit remainder of the log slot"""
    shape, slots = (64, 48, 128, 10), 4096
    on, off = both_forms(ctx, shape, True, True, capacity=capacity, state0=state0, slots=slots)
    assert_same(on, off, GRADS + STATE, f"{shape} capacity={capacity} state0={state0}")
    slot = state0 % capacity
    assert slot < slots and on["state"].tolist() == [state0 + 1, (1 << 35) + 11 + shape[0]]
    assert on["metrics"].reshape(slots, 2)[slot].tolist() == [on["loss"][0], on["nc"][0]]
