"""Which graphs a train_epoch_graph call records and which it replays (StepGraphs in csrc/host/taper.h), read from
Trainer.last_replays().  Every expected record is derived by hand from the policy: the binary ladder behind one eager step, at most four
exact remainders, at most four whole-call graphs and those only where a step graph of that length exists.  Notation: r = the state reset
on its own, E = steps enqueued eagerly, C / R = a step graph captured / replayed, CW / RW = a whole-call graph; the number is the steps.

Baseline MLP 784-128-10, batch 32.  In every case the losses and the final parameters are bit-identical to a graph_chunk=1 Trainer's on the
same data and calls: the op list is the same whatever replays it."""
import functools
import re

import numpy as np
import pytest

from tests import backends

pytestmark = pytest.mark.gpu

BATCH = 32
KINDS = {"r": 0, "E": 1, "C": 2, "R": 3, "CW": 4, "RW": 5}


def rec(text):
    """'r E1 C16 RW20' -> [(0, 0), (1, 1), (2, 16), (5, 20)]"""
    out = []
    for tok in text.split():
        m = re.fullmatch(r"(r|CW|RW|E|C|R)(\d*)", tok)
        out.append((KINDS[m[1]], int(m[2] or 0)))
    return out


@functools.lru_cache(maxsize=None)
def _data(rows):
    rng = np.random.default_rng(rows)
    spec = backends.mlp_baseline(rng)
    x, y = backends.mnist_like(rng, rows)
    return spec, x, y


def _run(chunk, rows, calls):
    """calls: (loader index, max_steps) each -> (the record of every call, all losses, the final parameters)"""
    import taper_amd as T
    spec, x, y = _data(rows)
    model = backends.get("hip").sequential(spec)
    opt = T.Adam(model.parameters(), 1e-3, None, None, 1e-4)
    tr = T.Trainer(model, opt, graph_chunk=chunk)
    ds = T.MNISTDataset.from_host(x, y)
    loaders = [T.DataLoader(ds, BATCH, True, seed=7 + i) for i in range(1 + max(i for i, _ in calls))]
    records, losses = [], []
    for i, k in calls:
        ep = tr.run_epoch(loaders[i], T.Trainer.GRAPH, max_steps=k)
        records.append(tr.last_replays())
        losses += list(ep["losses"])
    return records, np.asarray(losses), [p.data() for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _reference(rows, calls):
    return _run(1, rows, calls)[1:]


def _check(chunk, rows, calls, expected):
    calls = tuple(calls)
    records, losses, params = _run(chunk, rows, calls)
    for i, (got, want) in enumerate(zip(records, expected)):
        assert got == rec(want), f"call {i + 1}: {got} is not {want}"
    assert len(records) == len(expected)
    ref_losses, ref_params = _reference(rows, calls)
    np.testing.assert_array_equal(losses, ref_losses)
    for a, b in zip(params, ref_params):
        np.testing.assert_array_equal(a, b)


CALL_1_OF_20 = "r E1 C16 C8 C4 C2 C1 C19 R19"


def test_the_20_step_cache_is_complete_on_the_third_call():
    """three epochs of 20 steps, default chunk: the ladder and the 19-step remainder behind the eager step, then the 20-step graph and the
    whole-call graph around it, then ONE replay with no separate reset -- and so every later call"""
    _check(128, 640, [(0, 0)] * 5, [CALL_1_OF_20, "r C20 CW20 RW20", "RW20", "RW20", "RW20"])


def test_the_benchmark_shape_in_small():
    """a short warm-up, a top-up that completes the ladder, one untimed call of K steps, then the timed call: one replay"""
    _check(8, 640, [(0, 5), (0, 17), (0, 6), (0, 6)], ["r E1 C4 C2 C1 R4", "r E1 C8 R8 R8", "r C6 CW6 RW6", "RW6"])


def test_a_partial_batch_is_eager_and_keeps_whole_call_graphs_out():
    """677 rows = 21 full steps + 5 rows: the last batch is a trailing eager step of every call, and no call is a whole-call graph"""
    _check(8, 677, [(0, 0)] * 3, ["r E1 C8 C4 C2 C1 R8 R8 R4 E1", "r C5 R8 R8 R5 E1", "r R8 R8 R5 E1"])


def test_the_two_caps_of_four():
    """four exact remainders and four whole-call graphs are recorded; a fifth length gets neither and replays from the ladder"""
    calls = [(0, 33), (0, 3), (0, 5), (0, 6), (0, 7), (0, 9), (0, 3)]
    expected = ["r E1 C16 C8 C4 C2 C1 R16 R16"] + [f"r C{k} CW{k} RW{k}" for k in (3, 5, 6, 7)] + ["r R8 R1", "RW3"]
    _check(16, 1280, calls, expected)


def test_another_loader_drops_everything():
    """a second DataLoader over the same dataset has index storage of its own, which the captured steps bake in: its first call records as
    the very first call did"""
    _check(128, 640, [(0, 0)] * 3 + [(1, 0)], [CALL_1_OF_20, "r C20 CW20 RW20", "RW20", CALL_1_OF_20])


def test_no_graph_is_eager_and_latches(monkeypatch):
    """TAPER_NO_GRAPH=1: every step enqueued eagerly; the Trainer that saw it stays eager after the variable is gone, a fresh one records"""
    import taper_amd as T
    spec, x, y = _data(640)
    eager = "r E1 E1 E1 E1 E1"

    def trainer():
        model = backends.get("hip").sequential(spec)
        tr = T.Trainer(model, T.Adam(model.parameters(), 1e-3, None, None, 1e-4))
        return model, tr, T.DataLoader(T.MNISTDataset.from_host(x, y), BATCH, True, seed=7)

    model, tr, loader = trainer()
    monkeypatch.setenv("TAPER_NO_GRAPH", "1")
    losses = list(tr.run_epoch(loader, T.Trainer.GRAPH, max_steps=5)["losses"])
    assert tr.last_replays() == rec(eager)
    monkeypatch.delenv("TAPER_NO_GRAPH")
    losses += list(tr.run_epoch(loader, T.Trainer.GRAPH, max_steps=5)["losses"])
    assert tr.last_replays() == rec(eager)
    ref_losses, ref_params = _reference(640, ((0, 5), (0, 5)))
    np.testing.assert_array_equal(np.asarray(losses), ref_losses)
    for a, b in zip([p.data() for p in model.parameters()], ref_params):
        np.testing.assert_array_equal(a, b)

    _, fresh, loader = trainer()
    first = fresh.run_epoch(loader, T.Trainer.GRAPH, max_steps=5)["losses"]
    assert fresh.last_replays() == rec("r E1 C4 C2 C1 R4")
    np.testing.assert_array_equal(first, ref_losses[:5])
