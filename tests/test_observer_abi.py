"""The quantization observers' boundary without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h), their exports, the
Python face (MinMaxObserver, HistogramObserver, ObserverManager) and what is decided before anything touches the device.  Also the numpy
restatement the GPU tests compare against (tests/observers_ref.py): its search agrees with its literal scan, and the quirks the issue
names are there."""
import ctypes as C

import numpy as np
import pytest

from tests import observers_ref as R

TH = (("th_obs_minmax_first", 5), ("th_obs_minmax_update", 5), ("th_obs_fold", 5), ("th_obs_hist_edges", 5), ("th_obs_hist_count", 6),
      ("th_obs_hist_lds_max_bins", 0), ("th_obs_hist_stats", 4))
TP = (("tp_observer_new", 3), ("tp_observer_free", 1), ("tp_observer_set_enabled", 2), ("tp_observer_is_enabled", 2), ("tp_observer_observe", 2),
      ("tp_observer_num_observations", 2), ("tp_observer_reset", 1), ("tp_observer_minmax_len", 2), ("tp_observer_minmax_values", 3),
      ("tp_observer_minmax_stats", 5), ("tp_observer_hist_num_bins", 2), ("tp_observer_hist_bins", 2), ("tp_observer_hist_num_edges", 2),
      ("tp_observer_hist_edges", 2), ("tp_observer_hist_stats", 5), ("tp_observer_manager_new", 1), ("tp_observer_manager_free", 1),
      ("tp_observer_manager_add_minmax", 2), ("tp_observer_manager_add_histogram", 3), ("tp_observer_manager_observe_minmax", 3),
      ("tp_observer_manager_observe_histogram", 3), ("tp_observer_manager_minmax_stats", 7), ("tp_observer_manager_histogram_stats", 7),
      ("tp_observer_manager_reset_all", 1), ("tp_observer_manager_names", 5))


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, hip
    for name, nargs in TH:
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert getattr(hip, name)
    assert {n for n in HIP_PROTOS if n.startswith("th_obs_")} == {n for n, _ in TH}
    assert HIP_PROTOS["th_obs_hist_count"][1][2] is C.c_int64 and HIP_PROTOS["th_obs_hist_count"][1][4] is C.c_int   # (ctx first)


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, host
    for name, nargs in TP:
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name)
    assert {n for n in HOST_PROTOS if n.startswith("tp_observer")} == {n for n, _ in TP}


def test_lds_cap_leaves_two_workgroups_per_cu():
    from taper_amd._lib import hip
    cap = hip.th_obs_hist_lds_max_bins()
    assert cap >= 2048 and 2 * (2 * cap + 1) * 4 <= 160 * 1024   # edges + 32-bit counters of two workgroups in a CU's 160 KiB


def test_python_face():
    import taper_amd as T
    for cls in (T.MinMaxObserver, T.HistogramObserver):
        for meth in ("set_enabled", "is_enabled", "observe", "num_observations", "reset", "get_stats", "stats"):
            assert callable(getattr(cls, meth)), (cls, meth)
    for meth in ("min_values", "max_values", "global_min", "global_max"):
        assert callable(getattr(T.MinMaxObserver, meth))
    for meth in ("bins", "bin_edges", "edges"):
        assert callable(getattr(T.HistogramObserver, meth))
    for meth in ("add_minmax_observer", "add_histogram_observer", "observe_minmax", "observe_histogram", "get_minmax_stats",
                 "get_histogram_stats", "reset_all", "get_observer_names"):
        assert callable(getattr(T.ObserverManager, meth))
    assert {"MinMaxObserver", "HistogramObserver", "ObserverManager"} <= set(T.__all__)


def test_zero_bins_are_refused_before_the_device_is_touched():
    # on a machine without a GPU nothing that needs the device could have succeeded: the refusal and its message come from the host
    import taper_amd as T
    from taper_amd._lib import host
    with pytest.raises(T.TaperError, match="num_bins must be at least 1"):
        T.HistogramObserver(0)
    out = C.c_void_p()
    assert host.tp_observer_new(1, 0, C.byref(out)) != 0 and out.value is None
    assert "num_bins must be at least 1" in host.tp_last_error().decode()
    assert host.tp_observer_new(7, 4, C.byref(out)) != 0 and out.value is None
    m = T.ObserverManager()
    with pytest.raises(T.TaperError, match="num_bins must be at least 1"):
        m.add_histogram_observer("h", 0)
    mh = C.c_void_p()
    assert host.tp_observer_manager_new(C.byref(mh)) == 0
    assert host.tp_observer_manager_add_histogram(mh, b"h", 0) != 0 and "num_bins must be at least 1" in host.tp_last_error().decode()
    assert host.tp_observer_manager_free(mh) == 0


def test_state_before_any_observation_needs_no_device():
    import taper_amd as T
    mm = T.MinMaxObserver()
    st = mm.get_stats()
    assert st["num_observations"] == 0 and st["global_min"] == np.inf and st["global_max"] == -np.inf and st["range"] == -np.inf
    assert mm.global_min() == np.inf and mm.global_max() == -np.inf
    assert mm.min_values().size == 0 and mm.max_values().size == 0 and mm.is_enabled()
    mm.set_enabled(False)
    assert not mm.is_enabled()
    mm.reset()
    h = T.HistogramObserver(10)
    assert h.bins().dtype == np.uint64 and h.bins().tolist() == [0] * 10 and h.bin_edges().size == 0
    assert h.get_stats() == dict(num_observations=0, total_count=0, mean_bin=np.float32(0.0), max_bin_count=0)
    h.reset()
    assert h.num_observations() == 0
    from taper_amd._lib import host
    with pytest.raises(T.TaperError, match="not a Histogram observer"):
        from taper_amd._lib import tp_check
        tp_check(host.tp_observer_hist_bins(mm._h, None), "bins of a MinMax observer")


def test_manager_rules_without_a_device():
    import taper_amd as T
    m = T.ObserverManager()
    assert m.get_observer_names() == []
    m.add_minmax_observer("zeta")
    m.add_histogram_observer("mid", 4)
    m.add_minmax_observer("alpha")
    m.add_histogram_observer("alpha", 8)
    m.add_minmax_observer("zeta")
    assert m.get_observer_names() == ["alpha", "zeta", "alpha", "mid"]      # minmax names, then histogram names, each sorted
    assert m.get_minmax_stats("nobody") is None and m.get_histogram_stats("zeta") is None and m.get_minmax_stats("mid") is None
    assert m.get_minmax_stats("alpha")["num_observations"] == 0 and m.get_histogram_stats("alpha")["total_count"] == 0
    m.reset_all()


# ---- the restatement itself ----
def test_reference_search_equals_its_literal_scan():
    rng = np.random.default_rng(0)
    for nb in (1, 2, 3, 10, 255, 2048):
        for scale in (1e-3, 1.0, 1e3):
            first = (rng.standard_normal(4096) * scale).astype(np.float32)
            e = R.make_edges(first, nb)
            v = np.concatenate([first, e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)),
                                (rng.standard_normal(512) * scale * 10).astype(np.float32),
                                np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)]).astype(np.float32)
            assert np.array_equal(R.find_bins_scan(v, e, nb), R.find_bins_search(v, e, nb)), (nb, scale)
    e = R.make_edges(np.full(5, 2.5, np.float32), 7)     # a constant first observation: all edges equal
    assert np.all(e == np.float32(2.5))
    v = np.array([2.5, 2.0, 3.0, np.nan], np.float32)
    assert R.find_bins_scan(v, e, 7).tolist() == [0, 0, 6, 6] == R.find_bins_search(v, e, 7).tolist()


def test_reference_quirks():
    mm = R.MinMax()
    mm.observe([1.0, np.nan, 3.0])
    mm.observe([np.nan, np.nan, 2.0, 9.0])       # a NaN loses to a number, NaN when both are; the fourth element is ignored
    assert R.same_bits(mm.min_values, [1.0, np.nan, 2.0]) and R.same_bits(mm.max_values, [1.0, np.nan, 3.0])
    assert mm.stats()["global_min"] == 1.0 and mm.stats()["global_max"] == 3.0
    h = R.Histogram(4)
    h.observe([0.0, 1.0, 2.0, 4.0, np.nan])      # edges 0 1 2 3 4: bin k is (edge[k], edge[k + 1]], bin 0 also takes <= edge[0]; NaN -> last
    assert h.bins.tolist() == [2, 1, 0, 2]
    assert R.same_bits([0.0, np.nan], [-0.0, np.nan]) and not R.same_bits([1.0], [np.nextafter(np.float32(1), np.float32(2))])
