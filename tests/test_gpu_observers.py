"""The quantization observers on the GPU (src/quantization/observers.rs; csrc/observers.hip) against the numpy restatement of
tests/observers_ref.py.  Every comparison is exact: integer equality for bins and counts, bit equality for edges, min / max and stats
(+0 == -0, and a NaN equals a NaN whatever its payload: observers_ref.same_bits says why).  Every case runs once."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import observers_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32


def _cap():
    from taper_amd._lib import hip
    return hip.th_obs_hist_lds_max_bins()


def _pool_in_use():
    import taper_amd as T
    from taper_amd._lib import hip as H
    T.Device.sync()
    r, u = C.c_size_t(), C.c_size_t()
    assert H.th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


def _same_stats(got, ref):
    assert set(got) == set(ref)
    for k, v in ref.items():
        if isinstance(v, (np.floating, float)):
            assert R.same_bits(got[k], v), (k, got[k], v)
        else:
            assert int(got[k]) == int(v), (k, got[k], v)


def _check_hist(obs, ref):
    bins, edges = obs.bins(), obs.bin_edges()
    assert bins.dtype == np.uint64 and np.array_equal(bins, ref.bins), np.flatnonzero(bins != ref.bins)[:8]
    assert R.same_bits(edges, ref.edges)
    assert obs.num_observations() == ref.num_observations
    _same_stats(obs.get_stats(), ref.stats())


def _run_hist(num_bins, observations):
    import taper_amd as T
    obs, ref = T.HistogramObserver(num_bins), R.Histogram(num_bins)
    for a in observations:
        a = np.asarray(a, F)
        obs.observe(T.Tensor(a))
        ref.observe(a)
    _check_hist(obs, ref)
    return obs, ref


def _check_minmax(obs, ref):
    assert R.same_bits(obs.min_values(), ref.min_values) and R.same_bits(obs.max_values(), ref.max_values)
    assert obs.num_observations() == ref.num_observations
    _same_stats(obs.get_stats(), ref.stats())
    assert R.same_bits(obs.global_min(), ref.stats()["global_min"]) and R.same_bits(obs.global_max(), ref.stats()["global_max"])


# ---- the reference's own unit tests (observers.rs:351-387), as they stand ----
def test_minmax_observer():
    import taper_amd as T
    observer = T.MinMaxObserver()
    observer.observe(T.Tensor([1.0, 2.0, 3.0, 4.0], (2, 2)))
    assert observer.num_observations() == 1
    assert observer.global_min() == 1.0
    assert observer.global_max() == 4.0


def test_histogram_observer():
    import taper_amd as T
    observer = T.HistogramObserver(10)
    observer.observe(T.Tensor([1.0, 2.0, 3.0, 4.0], (2, 2)))
    assert observer.num_observations() == 1
    assert len(observer.bins()) == 10


def test_observer_manager():
    import taper_amd as T
    manager = T.ObserverManager()
    manager.add_minmax_observer("test")
    manager.observe_minmax("test", T.Tensor([1.0, 2.0, 3.0], (3,)))
    stats = manager.get_minmax_stats("test")
    assert stats["num_observations"] == 1
    assert stats["global_min"] == 1.0
    assert stats["global_max"] == 3.0


# ---- MinMax ----
def test_minmax_before_any_observation():
    import taper_amd as T
    _check_minmax(T.MinMaxObserver(), R.MinMax())


@pytest.mark.parametrize("n", [1, 3, 4099, 1_000_003])
def test_minmax_over_observations_longer_shorter_nan_and_infinity(n):
    import taper_amd as T
    rng = np.random.default_rng(n)
    obs, ref = T.MinMaxObserver(), R.MinMax()

    def see(a):
        a = np.asarray(a, F)
        obs.observe(T.Tensor(a))
        ref.observe(a)
        _check_minmax(obs, ref)

    first = rng.standard_normal(n).astype(F)
    first[::7] = np.nan                        # NaNs in the state ...
    first[n // 2] = -0.0
    see(first)
    for k in range(3):
        a = (rng.standard_normal(n) * (k + 1)).astype(F)
        a[k::5] = np.nan                       # ... and in the data: some meet a NaN (stays NaN), some a number (the number wins)
        see(a)
    longer = (rng.standard_normal(2 * n + 5) * 10).astype(F)   # the tail past the vectors' length is ignored
    see(longer)
    shorter = (rng.standard_normal(max(n // 3, 1)) * 100).astype(F)
    see(shorter)
    inf = rng.standard_normal(n).astype(F)
    inf[0], inf[-1] = np.inf, -np.inf          # infinities take part in min / max and in the global folds
    see(inf)
    assert (n == 1 or ref.stats()["global_max"] == np.inf) and ref.stats()["global_min"] == -np.inf and obs.min_values().size == n
    see(np.full(n, np.nan, F))                 # changes nothing
    obs.set_enabled(False)
    ref.enabled = False
    see(np.full(n, 1e30, F))                   # disabled: not observed, not counted
    obs.set_enabled(True)
    ref.enabled = True
    obs.reset()
    ref.reset()
    _check_minmax(obs, ref)
    see(np.full(5, np.nan, F))                 # a first observation again, of another length; all NaN: the folds stay at their seeds
    assert obs.global_min() == np.inf and obs.global_max() == -np.inf and obs.min_values().size == 5


def test_minmax_kernels_on_unaligned_pointers():
    import taper_amd as T
    from taper_amd import hip
    ctx = hip.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(5)
    n = 10_007
    x0, x1 = rng.standard_normal(n + 1).astype(F), rng.standard_normal(n + 1).astype(F)
    x1[3::11] = np.nan
    d0, d1, lo, hi, out = ctx.upload(x0), ctx.upload(x1), ctx.empty(n + 1), ctx.empty(n + 1), ctx.empty(2)
    ctx.call("th_obs_minmax_first", d0.offset(4), lo.offset(4), hi.offset(4), n)     # every pointer 4 bytes off a 16-byte boundary
    ctx.call("th_obs_minmax_update", d1.offset(4), lo.offset(4), hi.offset(4), n)
    ctx.call("th_obs_fold", lo.offset(4), hi.offset(4), n, out)
    ref = R.MinMax()
    ref.observe(x0[1:])
    ref.observe(x1[1:])
    assert R.same_bits(ctx.download(lo.offset(4), n), ref.min_values) and R.same_bits(ctx.download(hi.offset(4), n), ref.max_values)
    got = ctx.download(out, 2)
    assert R.same_bits(got[0], ref.stats()["global_min"]) and R.same_bits(got[1], ref.stats()["global_max"])


# ---- Histogram ----
def _bins_list():
    return [1, 2, 10, 255, 2048, 65536, _cap() + 1]


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("which", range(7))
def test_histogram_normal_data_then_outside_edges_and_specials(which, scale):
    nb = _bins_list()[which]
    rng = np.random.default_rng(1000 * which + int(np.log10(scale)) + 3)
    first = (rng.standard_normal(200_003) * scale).astype(F)
    edges = R.make_edges(first, nb)
    assert np.all(np.isfinite(edges))
    far = (rng.standard_normal(50_001) * scale * 50).astype(F)                 # reaching far outside the first observation's range
    on_edges = np.concatenate([edges, np.nextafter(edges, F(np.inf)), np.nextafter(edges, F(-np.inf)), edges[::-1]]).astype(F)
    special = (rng.standard_normal(4097) * scale).astype(F)
    special[::3] = np.nan
    special[1::17] = np.inf
    special[2::19] = -np.inf
    obs, ref = _run_hist(nb, [first, far, on_edges, special])
    assert ref.num_observations == 4 and int(ref.bins.sum()) == first.size + far.size + on_edges.size + special.size


@pytest.mark.parametrize("nb", [1, 2, 256, 2048, 65536])
def test_histogram_post_relu(nb):
    rng = np.random.default_rng(nb)
    a = np.maximum(rng.standard_normal(1_000_003).astype(F), 0)               # half the elements are the minimum: bin 0
    b = np.maximum(rng.standard_normal(300_001).astype(F) * 2, 0)
    obs, ref = _run_hist(nb, [a, b])
    assert int(ref.bins[0]) >= (a.size + b.size) // 3


@pytest.mark.parametrize("nb", [1, 7, 2048, 65536])
def test_histogram_constant_first_observation(nb):
    c = np.full(10_001, 0.75, F)                                               # bin_width 0: all edges equal
    later = np.array([0.75, 0.5, -1e9, 1.0, 1e9, np.nan, np.inf, -np.inf, np.nextafter(F(0.75), F(1)), np.nextafter(F(0.75), F(0))] * 13, F)
    obs, ref = _run_hist(nb, [c, later])
    assert np.all(ref.edges == F(0.75)) and int(ref.bins[0]) >= c.size


@pytest.mark.parametrize("n", [1, 3, 1_000_003, (1 << 24) + 3])
def test_histogram_lengths_that_are_not_multiples_of_four(n):
    rng = np.random.default_rng(n % 1000)
    a = rng.standard_normal(n).astype(F)
    _run_hist(2048, [a, a[: n // 2 + 1] * F(1.5)])


def test_histogram_duplicate_edges_where_the_width_is_below_the_spacing():
    rng = np.random.default_rng(9)
    a = (1000.0 + rng.random(100_003) * 1e-3).astype(F)                        # ~16 distinct floats in the range, 2048 and 65 536 bins
    for nb in (2048, 65536):
        obs, ref = _run_hist(nb, [a, a[::-1].copy()])
        assert np.unique(ref.edges).size < nb // 8


def test_histogram_last_edge_below_the_first_observations_maximum():
    found = None
    for seed in range(2000):                                                   # constructed on the CPU: 10 bins, the last edge rounds down
        a = np.random.default_rng(seed).standard_normal(64).astype(F)
        e = R.make_edges(a, 10)
        if e[-1] < a.max():
            found = (a, e)
            break
    assert found is not None, "no such first observation among the seeds tried"
    a, e = found
    assert e[10] < a.max()                                                     # it IS such a case: the maximum goes to the last bin by overflow
    assert R.find_bins_scan(a[[int(a.argmax())]], e, 10).tolist() == [9]
    _run_hist(10, [a, a])


@pytest.mark.parametrize("first", [[1.0, 2.0, np.inf, -3.0, np.nan], [1.0, -np.inf, 4.0], [-np.inf, np.inf, 0.0], [np.nan, np.nan], [np.inf, np.inf],
                                   [3.0e38, -3.0e38, 1.0]])
def test_histogram_non_finite_first_observation_is_the_literal_scan(first):
    later = [0.0, -1.0, 5.0, np.nan, np.inf, -np.inf, 1e30, -1e30]
    for nb in (1, 4, 9):
        obs, ref = _run_hist(nb, [first, later])
        assert not np.all(np.isfinite(ref.edges))


def test_histogram_disabled_reset_and_new_edges():
    import taper_amd as T
    rng = np.random.default_rng(11)
    obs, ref = T.HistogramObserver(255), R.Histogram(255)

    def see(a):
        a = np.asarray(a, F)
        obs.observe(T.Tensor(a))
        ref.observe(a)
        _check_hist(obs, ref)

    _check_hist(obs, ref)
    see(rng.standard_normal(30_001))
    obs.set_enabled(False)
    ref.enabled = False
    assert not obs.is_enabled()
    see(rng.standard_normal(999) * 7)            # not observed, not counted
    obs.set_enabled(True)
    ref.enabled = True
    see(rng.standard_normal(12_345) * 3)
    old = ref.edges.copy()
    obs.reset()
    ref.reset()
    _check_hist(obs, ref)
    assert obs.bin_edges().size == 0 and obs.bins().sum() == 0
    see(rng.standard_normal(5_003) * 40 + 100)   # a first observation again: new edges
    assert not R.same_bits(old, ref.edges)


def test_histogram_same_sequence_twice_gives_identical_bins():
    rng = np.random.default_rng(13)
    seq = [rng.standard_normal(3_000_001).astype(F), np.maximum(rng.standard_normal(2_000_003), 0).astype(F) * 3, rng.standard_normal(77).astype(F)]
    for nb in (2048, _cap() + 1):
        one, ref = _run_hist(nb, seq)
        two, _ = _run_hist(nb, seq)
        assert np.array_equal(one.bins(), two.bins()) and R.same_bits(one.bin_edges(), two.bin_edges())
        assert one.get_stats() == two.get_stats()


def test_histogram_count_kernel_on_an_unaligned_pointer():
    import taper_amd as T
    from taper_amd import hip
    ctx = hip.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(17)
    x = rng.standard_normal(70_002).astype(F)
    for nb in (64, _cap() + 1):
        d, edges, bins, out = ctx.upload(x), ctx.empty(nb + 1), ctx.upload(np.zeros(nb, np.uint64)), ctx.empty(3, np.uint64)
        ctx.call("th_obs_hist_edges", d.offset(4), x.size - 1, nb, edges)
        ctx.call("th_obs_hist_count", d.offset(4), x.size - 1, edges, nb, bins)
        ctx.call("th_obs_hist_stats", bins, nb, out)
        ref = R.Histogram(nb)
        ref.observe(x[1:])
        assert R.same_bits(ctx.download(edges, nb + 1), ref.edges) and np.array_equal(ctx.download(bins, nb, np.uint64), ref.bins)
        got = ctx.download(out, 3, np.uint64)
        assert int(got[0]) == ref.stats()["total_count"] and int(got[2]) == ref.stats()["max_bin_count"]
        assert int(got[1]) == sum(i * int(c) for i, c in enumerate(ref.bins))


# ---- buffers ----
def test_pooled_bytes_return_after_reset_and_after_the_objects_die():
    import taper_amd as T
    rng = np.random.default_rng(19)
    t = T.Tensor(rng.standard_normal(100_000).astype(F))
    before = _pool_in_use()
    mm, h, big, m = T.MinMaxObserver(), T.HistogramObserver(2048), T.HistogramObserver(_cap() + 1), T.ObserverManager()
    m.add_minmax_observer("a")
    m.add_histogram_observer("a", 16)
    for _ in range(2):
        mm.observe(t)
        h.observe(t)
        big.observe(t)
        m.observe_minmax("a", t)
        m.observe_histogram("a", t)
    assert _pool_in_use() >= before + 2 * 100_000 * 4 + 2048 * 12
    mm.get_stats(), h.get_stats(), big.get_stats(), m.get_minmax_stats("a"), m.get_histogram_stats("a")   # (their temporaries are returned)
    mm.reset()
    h.reset()
    big.reset()
    m.reset_all()
    assert _pool_in_use() == before
    mm.observe(t)
    h.observe(t)
    big.observe(t)
    m.observe_minmax("a", t)
    m.observe_histogram("a", t)
    m.add_minmax_observer("a")                   # the replaced observer's buffers go back too
    m.add_histogram_observer("a", 16)
    m.observe_histogram("a", t)
    assert _pool_in_use() > before
    del mm, h, big, m
    assert _pool_in_use() == before


# ---- manager ----
def test_manager_replace_unknown_names_and_order():
    import taper_amd as T
    rng = np.random.default_rng(23)
    a, b = rng.standard_normal(1000).astype(F), (rng.standard_normal(1000) * 3).astype(F)
    m = T.ObserverManager()
    m.add_minmax_observer("y")
    m.add_histogram_observer("y", 10)            # a name may be in both maps
    m.add_histogram_observer("x", 4)
    m.add_minmax_observer("b")
    assert m.get_observer_names() == ["b", "y", "x", "y"]
    m.observe_minmax("nobody", T.Tensor(a))      # unknown names: nothing happens, nothing is found
    m.observe_histogram("b", T.Tensor(a))        # "b" is a minmax observer only
    assert m.get_minmax_stats("nobody") is None and m.get_histogram_stats("b") is None
    assert m.get_minmax_stats("b")["num_observations"] == 0
    rm, rh = R.MinMax(), R.Histogram(10)
    for v in (a, b):
        m.observe_minmax("y", T.Tensor(v))
        m.observe_histogram("y", T.Tensor(v))
        rm.observe(v)
        rh.observe(v)
    _same_stats(m.get_minmax_stats("y"), rm.stats())
    _same_stats(m.get_histogram_stats("y"), rh.stats())
    m.add_histogram_observer("y", 3)             # replaced by a fresh one, with its own bin count
    assert m.get_histogram_stats("y") == dict(num_observations=0, total_count=0, mean_bin=F(0), max_bin_count=0)
    _same_stats(m.get_minmax_stats("y"), rm.stats())
    rh3 = R.Histogram(3)
    m.observe_histogram("y", T.Tensor(b))
    rh3.observe(b)
    _same_stats(m.get_histogram_stats("y"), rh3.stats())
    m.reset_all()
    assert m.get_minmax_stats("y")["num_observations"] == 0 and m.get_minmax_stats("y")["global_min"] == np.inf
    assert m.get_histogram_stats("y")["total_count"] == 0 and m.get_observer_names() == ["b", "y", "x", "y"]


# ---- example ----
def test_observe_calibration_example_prints_a_line_per_observer():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "examples")])
    out = subprocess.run([str(ROOT / "examples" / "_build" / "observe_calibration"), "--data-dir", "/nonexistent", "--steps", "3", "--train-n",
                          "512", "--calib", "2", "--bins", "32"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("observer ")]
    names = [ln.split()[1] for ln in lines]
    assert names == ["linear1.out", "relu.out", "linear2.out", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]
    counts = {ln.split()[1]: int(ln.split("count ")[1].split()[0]) for ln in lines}
    assert counts["linear1.weight"] == 784 * 128 and counts["linear2.bias"] == 10 and counts["relu.out"] == 2 * 64 * 128
    assert "Observers: 14 names" in out.stdout
