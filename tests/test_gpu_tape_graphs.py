"""The eager tape on graphs that are no chains (tests/tape_graphs_ref.py): tensors with several consumers, tied weights, the same tensor
on both sides of an op, every differentiable op over an empty and over a held gradient slot, roots that are no lone loss -- the host
code that picks write or accumulate, applies a ReLU mask or trusts its consumer to have, and takes a bias gradient from sums someone
left behind.  Every graph runs on taper_amd and is held to the float64 tape first, to the CPU oracle second; a graph with a Linear runs
once spelled in primitives and once through Tensor.linear, the fused node every Linear module records.

Bounds, of the tensor's scale (max |reference|): twice the worst margin observed against float64 on an MI355X (profiles/tape_graphs_parity_margins.json,
written by tests/margins.py), never looser than the project's 1e-4.  Against the oracle the bound is that plus the oracle's own distance
from float64 (tests/test_tape_graphs_oracle.py: the triangle inequality, nothing measured on this side)."""
import numpy as np
import pytest

from tests import margins
from tests import tape_graphs_ref as G
from tests.test_tape_graphs_oracle import BOUND as ORACLE_BOUND

pytestmark = pytest.mark.gpu

CONTRACT = 1e-4
BOUND = dict(      # vs float64: 2 x the worst margin observed on MI355X (profiles/tape_graphs_parity_margins.json)
    graph1=3.2e-7,        # observed 1.57e-7 (b1)
    graph2=1.3e-6,        # observed 6.35e-7 (x, two heads); fused against primitive spelling 8.63e-7
    graph2_tile=1.2e-6,   # observed 5.98e-7 (Wa); fused against primitive spelling 3.99e-7
    graph3=4.9e-7,        # observed 2.45e-7 (x, global average pool recorded last)
    graph4=2.8e-7,        # observed 1.39e-7 (the root of x + x)
    graph5=3.2e-7,        # observed 1.58e-7 (log_softmax over a held slot)
    graph6=1.9e-6,        # observed 9.39e-7 (the root of the constant-operand graph, a sum of 40 signed terms: the oracle's own figure there)
)
# the Trainer's three steps over the tied layer against the oracle's loop, worst of the four variants (observed: 1.0e-7, 7.6e-7, 4.4e-7, 7.9e-4)
BOUND_TIED_LOSS, BOUND_TIED_M, BOUND_TIED_V, BOUND_TIED_WEIGHT_OVER_LR = 2.1e-7, 1.6e-6, 8.8e-7, 1.6e-3
assert all(b <= CONTRACT for b in list(BOUND.values()) + [BOUND_TIED_LOSS, BOUND_TIED_M, BOUND_TIED_V])

_REF = {}


@pytest.fixture(scope="module")
def H():
    return G.face("hip")


def refs(key, build, d, sentinel=None):
    """the float64 tape's and the oracle's run of a graph, computed once per key and left unchanged"""
    if key not in _REF:
        r64 = G.run(G.face("np64"), build, d, sentinel)
        ro = None if d.get("_name") in G.ORACLE_LACKS else G.run(G.face("oracle"), build, d, sentinel)
        _REF[key] = (r64, ro)
    return _REF[key]


def hold(family, tag, got, r64, ro, scale=None):
    """root value, None-for-None and every leaf's gradient: to float64 within BOUND[family], to the oracle within that plus its own"""
    (v, g, _, _), (v64, g64, _, _) = got, r64
    shift = (lambda k: 0.0) if scale is None else (lambda k: scale[k])   # (x / x: both sides moved by the cancelled term, so its size is the scale)
    margins.check(f"{tag}/root_vs_f64", v, v64, BOUND[family])
    for k in g64:
        assert (g[k] is None) == (g64[k] is None), f"{tag}/{k}: taper_amd has {'no ' if g[k] is None else 'a '}gradient, float64 the opposite"
        if g64[k] is not None:
            margins.check(f"{tag}/{k}_vs_f64", np.asarray(g[k], np.float64) + shift(k), g64[k] + shift(k), BOUND[family])
    if ro is not None:
        vo, go = ro[0], ro[1]
        margins.check(f"{tag}/root_vs_oracle", v, vo, BOUND[family] + ORACLE_BOUND[family])
        for k in go:
            assert (g[k] is None) == (go[k] is None), f"{tag}/{k}: gradient None-ness differs from the oracle's"
            if go[k] is not None:
                margins.check(f"{tag}/{k}_vs_oracle", np.asarray(g[k], np.float64) + shift(k), np.asarray(go[k], np.float64) + shift(k),
                              BOUND[family] + ORACLE_BOUND[family])


def spellings_agree(family, tag, fused, prim):
    for k in prim[1]:
        if prim[1][k] is not None:
            margins.check(f"{tag}/{k}_fused_vs_primitive", fused[1][k], prim[1][k], BOUND[family])


def same_bits(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=f"{k}: the two recording orders add the same terms in the same order")


# ---------------------------------------------------------------- graph 1
@pytest.mark.parametrize("sentinel", [False, True])
def test_graph1_shared_hidden_tied_weights(H, sentinel):
    d = G.data_graph1()
    got = {}
    for order in (0, 1):
        r64, ro = refs(("g1", order, sentinel), G.graph1(order), d, sentinel)
        for fused in (False, True):
            got[order, fused] = G.run(H, G.graph1(order, fused), d, sentinel)
            hold("graph1", f"order{order}", got[order, fused], r64, ro)
        spellings_agree("graph1", f"order{order}", got[order, True], got[order, False])
    for fused in (False, True):   # the tied branch hangs off h alone: which consumer of h was recorded first changes no sum in it
        same_bits(got[0, fused], got[1, fused], ("W2", "b2"))


# ---------------------------------------------------------------- graph 2
def _graph2(H, family, d, cases, shape):
    from taper_amd._lib import hip as lib
    assert lib.th_linear_bwd_dx_epilogue_rows(*shape) > 0, f"{shape}: the head's dX product no longer hands over a masked gradient"
    got = {}
    for variant, order in cases:
        r64, ro = refs((family, variant, order), G.graph2(variant, order), d)
        for fused in (True, False):
            got[variant, order, fused] = G.run(H, G.graph2(variant, order, fused), d)
            hold(family, f"{variant}{order}", got[variant, order, fused], r64, ro)
        spellings_agree(family, f"{variant}{order}", got[variant, order, True], got[variant, order, False])
    return got


def test_graph2_thin_head_hands_over_masked_gradient(H):
    """h[512, 2048] = relu(x W1^T + b1) feeds two heads 2048 -> 10 (or one head and h * h): the head that replays first leaves h's
    gradient masked, with the column partials of the bias gradient beside it; the second consumer adds an unmasked term, so the producer
    has to mask again and must not take its bias gradient from the stale partials.  "one": the control, where it does take them."""
    got = _graph2(H, "graph2", G.data_graph2(), [("two", 0), ("two", 1), ("square", 0), ("square", 1), ("one", 0)], (512, 2048, 10))
    for fused in (True, False):   # both heads see the same upstream gradient whichever was recorded first
        same_bits(got["two", 0, fused], got["two", 1, fused], ("Wa", "ba", "Wb", "bb"))
        same_bits(got["square", 0, fused], got["square", 1, fused], ("Wa", "ba"))


def test_graph2_tile128_head_hands_over_masked_gradient(H):
    _graph2(H, "graph2_tile", G.data_graph2(1024, 16, 1024, 256), [("two", 0)], (1024, 1024, 256))


# ---------------------------------------------------------------- graph 3
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("pool", ["max", "avg"])
def test_graph3_conv_relu_two_consumers(H, pool, full):
    d = G.data_graph3()
    for order in (0, 1):
        r64, ro = refs(("g3", pool, order, full), G.graph3(pool, order, full), d)
        got = G.run(H, G.graph3(pool, order, full), d)
        hold("graph3", f"{pool}{order}", got, r64, ro)
        assert (got[1]["w"] is None) == (not full) and (got[1]["x"] is None) == (not full) and got[1]["b"] is not None   # Q2


@pytest.mark.parametrize("full", [True, False])
def test_graph3_tied_conv_matrix_core_shapes(H, full):
    d = G.data_graph3(8, 16, seed=3)
    r64, ro = refs(("g3t", full), G.graph3_tied(full), d)
    hold("graph3", "tied", G.run(H, G.graph3_tied(full), d), r64, ro)


# ---------------------------------------------------------------- graph 4
@pytest.mark.parametrize("op", G.GRAPH4_OPS)
def test_graph4_same_tensor_both_sides(H, op):
    d = G.data_graph4()
    r64, ro = refs(("g4", op), G.graph4(op), d)
    got = G.run(H, G.graph4(op), d)
    term = None if G.graph4_scale(op, d) is None else dict(x=d["w"].astype(np.float64) / d["x"])
    hold("graph4", op, got, r64, ro, scale=term)
    assert got[2] == r64[2] == ro[2], "tape lengths differ"
    if op in ("add", "sub"):     # g + g and g - g: one IEEE operation per element on every side
        np.testing.assert_array_equal(got[1]["x"], r64[1]["x"].astype(np.float32))
    if op in ("add", "sub", "div", "div_view"):   # the same IEEE operations in the same order as the oracle's loop
        np.testing.assert_array_equal(got[1]["x"], ro[1]["x"])


# ---------------------------------------------------------------- graph 5
@pytest.mark.parametrize("name", sorted(G.OPS))
def test_graph5_every_op_on_empty_and_held_slot(H, name):
    d = G.data_graph5(name)
    for order in (0, 1):
        r64, ro = refs(("g5", name, order), G.graph5(name, order), d)
        hold("graph5", f"{name}/order{order}", G.run(H, G.graph5(name, order), d), r64, ro)


@pytest.mark.parametrize("name", G.RESHAPE_FAMILY)
def test_graph5_reshape_family_alone_is_exact(H, name):
    d = G.data_graph5(name)
    got = G.run(H, G.graph5(name, 0, solo=True), d)
    np.testing.assert_array_equal(got[1]["x"].reshape(-1), G.graph5_solo_weight(name, d["x"].shape, d["x"].size).reshape(-1))


# ---------------------------------------------------------------- graph 6
@pytest.mark.parametrize("sentinel", [False, True])
@pytest.mark.parametrize("kind", G.GRAPH6_KINDS)
def test_graph6_roots_and_repetition(H, kind, sentinel):
    """backward() twice without zero_grad (the adopted cross-entropy gradient, the shared [1.0] of a scalar root, private storage on the
    first write through it), zero_grad and a third backward; a non-scalar root, a seeded slot, a loss that is no root, a constant operand.
    (leaf_logits: the third backward used to adopt the forward kernel's buffer a second time, after the second had accumulated into it --
    twice the gradient.)"""
    d = G.data_graph6()
    for fused in ((False, True) if kind == "linear_logits" else (False,)):
        # Tensor.linear is one node: the product and the pre-activation have no slots that keep a gradient from one backward() to the
        # next, so from the second backward on the fused spelling is a different function -- judged by the float64 tape's fused node
        key = ("g6", kind, sentinel, fused)
        if key not in _REF:
            _REF[key] = (G.run_repeated(G.face("np64"), G.graph6(kind, fused), d, sentinel),
                         None if fused else G.run_repeated(G.face("oracle"), G.graph6(kind), d, sentinel))
        (v64, s64), ro = _REF[key]
        v, s = G.run_repeated(H, G.graph6(kind, fused), d, sentinel)
        tag = f"{kind}{'_fused' if fused else ''}"
        margins.check(f"{tag}/root_vs_f64", v, v64, BOUND["graph6"])
        for i, (a, b) in enumerate(zip(s, s64)):
            for k in b:
                assert (a[k] is None) == (b[k] is None), f"{tag}/{k} after backward {i + 1}: gradient None-ness differs"
                if b[k] is not None:
                    margins.check(f"{tag}/{k}_backward{i + 1}_vs_f64", a[k], b[k], BOUND["graph6"])
                if ro is not None:
                    c = ro[1][i]
                    assert (a[k] is None) == (c[k] is None), f"{tag}/{k} after backward {i + 1}: gradient None-ness differs from the oracle's"
                    if c[k] is not None:
                        margins.check(f"{tag}/{k}_backward{i + 1}_vs_oracle", a[k], c[k], BOUND["graph6"] + ORACLE_BOUND["graph6"])
    assert H.Tape.len() == 0


@pytest.mark.parametrize("sentinel", [False, True])
def test_graph6_root_is_node0(H, sentinel):
    """Q1: compat mode takes a root that is the tape's first node for a tensor without one, like the reference; the default does not"""
    d = G.data_graph6()
    r64, ro = refs(("g6n0", sentinel), G.graph_root_is_node0(), d, sentinel)
    got = G.run(H, G.graph_root_is_node0(), d, sentinel)
    hold("graph6", "node0", got, r64, ro)
    assert (got[1]["x"] is None) == sentinel


# ---------------------------------------------------------------- graph 7
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_trainer_tied_layer(H, fuse_adam, graph):
    """Sequential[Linear(784,32), ReLU, L, ReLU, L, ReLU, Linear(32,10)] with the SAME L twice, batch 8, three Adam steps, eager and as a
    captured graph: losses, parameters and both moments are those of the oracle's hand-written loop over the six distinct parameters.
    (Before Trainer::has_shared_parameter the captured step with fused Adam updates applied L's update in the node of its later use, on
    that use's share of the gradient: losses 1.7e-4 of their scale off, a thousand times the figure of the other three variants.)"""
    T, d, lr = H.m, G.data_graph7(), 1e-3
    G.reset(H)
    l0, L, l3 = T.Linear(784, 32), T.Linear(32, 32), T.Linear(32, 10)
    for layer, (w, b) in zip((l0, L, l3), (("W0", "b0"), ("WL", "bL"), ("W3", "b3"))):
        ps = layer.parameters()
        ps[0].set_data(d[w])
        ps[1].set_data(d[b])
    model = T.Sequential([l0, T.ReLU(), L, T.ReLU(), L, T.ReLU(), l3])
    params = l0.parameters() + L.parameters() + l3.parameters()   # the six distinct parameters
    opt = T.Adam(params, lr)
    tr = T.Trainer(model, opt, fuse_adam=fuse_adam)
    if graph:
        loader = T.DataLoader(T.MNISTDataset.from_host(d["xs"].reshape(-1, 784), d["ys"].reshape(-1)), d["xs"].shape[1], False)
        losses = tr.train_epoch_graph(loader)["losses"]
    else:
        losses = [tr.train_step(T.Tensor(x), T.Tensor(y))[0] for x, y in zip(d["xs"], d["ys"])]
    o_losses, o_params, o_m, o_v = G.oracle_tied_training(d, lr)
    assert opt.t() == len(o_losses)
    margins.check("losses", np.asarray(losses), np.asarray(o_losses), BOUND_TIED_LOSS)
    m, v = opt.moments()
    off = 0
    for i, p in enumerate(params):
        n = p.numel()
        margins.check(f"m{i}", m[off:off + n], o_m[i], BOUND_TIED_M)
        margins.check(f"v{i}", v[off:off + n], o_v[i], BOUND_TIED_V)
        margins.check_adam_weights(f"param{i}", p.data(), o_params[i], o_v[i], lr, len(o_losses), BOUND_TIED_WEIGHT_OVER_LR)
        off += n
    G.reset(H)
