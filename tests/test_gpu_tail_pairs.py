"""The wave pairs of th_mlp_tail's split launch (mlp_tail_split_kernel) behind their barriers: in a dW1 workgroup operand wave 4 + j finishes
element j of tile 0 and logit wave j the same element of tile 1 (the cross-wave sum in wave order, the dW1 store, the fused Adam update from
the p / m / v words the wave requested itself); in the lead head workgroup logit wave j sums its own sixteen rows of dlogits, NLL and hit
flags behind barrier 1 and hands them to the helper wave.  Against the 320-thread form of the SAME launch (th_mlp_tail_set_split(ctx, 0)).

Through the C ABI on raw guarded buffers, every comparison ON BITS: dW1, db1, dW2, db2, loss, hit count, the log entry, the state words,
and p / m / v of W1 and b1, with the four combinations of fused updates and t in {1, 1000} on both counters.  No arithmetic moved and no sum
changed its order, so equality is exact.  Shapes: the smallest at which the pairs can go wrong.
"""
import pytest

from tests.test_gpu_tail_helper import GRADS, run_tail, same_bits

pytestmark = pytest.mark.gpu
STATE = ("w1", "mw", "vw", "b1", "mb", "vb")
FUSIONS = [(False, False), (True, False), (False, True), (True, True)]
T_PAIRS = [(1, 1000), (1000, 1)]            # (W1's t, b1's t): both counters at both values
# (batch, in_features, hidden, classes)
PAIR_SHAPES = [
    (16, 16, 32, 10),     # no second tile anywhere; three pairs without rows, whose logit waves still write the lead's zeros
    (16, 32, 32, 10),     # one group with both tiles: logit waves without rows finish tile 1, Adam included
    (48, 80, 64, 10),     # 80 = 32 + 32 + 16: groups with and without a second tile in one launch, one pair without rows
    (64, 32, 128, 3),     # the flagship's hidden width; the class mask at both ends of the lead's db2 sums
    (64, 32, 128, 16),
    (64, 48, 128, 10),    # the flagship's instance with its last group short
]


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


@pytest.mark.parametrize("ts", T_PAIRS, ids=lambda v: "t" + "_".join(map(str, v)))
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_pairs_finish_what_the_320_thread_form_finishes(ctx, shape, ts):
    for fuse_w, fuse_b in FUSIONS:
        what = f"{shape} t={ts} fuse_w={fuse_w} fuse_b={fuse_b}"
        on, off = both_forms(ctx, shape, fuse_w, fuse_b, ts)
        assert_same(on, off, GRADS + STATE, what)
        assert on["state"].tolist() == [6, (1 << 35) + 11 + shape[0]], what
        assert on["metrics"].reshape(-1, 2)[5].tolist() == [on["loss"][0], on["nc"][0]], what


@pytest.mark.parametrize("ts", T_PAIRS, ids=lambda v: "t" + "_".join(map(str, v)))
def test_dx_role_beside_the_changed_roles(ctx, ts):
    """with d_dx the launch has a third role without barriers beside the two changed ones; W1's update is deferred, so the logit waves of
    the dW1 workgroups finish tile 1 without Adam"""
    shape = (32, 16, 64, 10)
    for fuse_b in (False, True):
        on, off = both_forms(ctx, shape, False, fuse_b, ts, with_dx=True)
        assert_same(on, off, GRADS + STATE + ("dx",), f"{shape} with d_dx t={ts} fuse_b={fuse_b}")
