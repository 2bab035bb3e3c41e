"""src/quantization/observers.rs restated in numpy, for the GPU tests to compare against bit for bit: the per-element MinMax observer, the
histogram observer with find_bin as the LITERAL linear scan, and their statistics.  Every float operation is an np.float32 operation
rounded once, in the reference's order.  No GPU, no library of the project: a plain module."""
import numpy as np

F = np.float32


def rust_min(a, b):
    """f32::min elementwise: a NaN operand loses to a number, NaN only when both are (np.fmin)"""
    return np.fmin(a, b)


def rust_max(a, b):
    return np.fmax(a, b)


def fold_min(v):
    """data.iter().copied().fold(f32::INFINITY, f32::min)"""
    v = np.asarray(v, F).ravel()
    return F(np.fmin.reduce(v, initial=F(np.inf))) if v.size else F(np.inf)


def fold_max(v):
    v = np.asarray(v, F).ravel()
    return F(np.fmax.reduce(v, initial=F(-np.inf))) if v.size else F(-np.inf)


class MinMax:
    def __init__(self):
        self.min_values = np.empty(0, F)
        self.max_values = np.empty(0, F)
        self.num_observations = 0
        self.enabled = True

    def observe(self, data):
        if not self.enabled:
            return
        d = np.asarray(data, F).ravel()
        if self.min_values.size == 0:
            self.min_values, self.max_values = d.copy(), d.copy()
        else:
            k = min(d.size, self.min_values.size)
            self.min_values[:k] = rust_min(self.min_values[:k], d[:k])
            self.max_values[:k] = rust_max(self.max_values[:k], d[:k])
        self.num_observations += 1

    def reset(self):
        self.__init__()

    def stats(self):
        with np.errstate(invalid="ignore"):
            lo, hi = fold_min(self.min_values), fold_max(self.max_values)
            return dict(num_observations=self.num_observations, global_min=lo, global_max=hi, range=F(hi - lo))


def make_edges(data, num_bins):
    """observers.rs:170-178: one division, then a multiply and an add per edge"""
    with np.errstate(all="ignore"):
        lo, hi = fold_min(data), fold_max(data)
        width = F(F(hi - lo) / F(num_bins))
        i = np.arange(num_bins + 1, dtype=np.int64).astype(F)
        return (lo + (i * width).astype(F)).astype(F)


def find_bins_scan(values, edges, num_bins):
    """find_bin for every value by the literal scan (observers.rs:194-201), vectorised over the VALUES only: walk the edges in order and
    let each value keep the first edge with val <= edge; no edge (a NaN, or past the last one) -> the last bin"""
    v = np.asarray(values, F).ravel()
    first = np.full(v.size, -1, np.int64)
    with np.errstate(invalid="ignore"):
        for i, e in enumerate(edges):
            hit = (first < 0) & (v <= e)
            first[hit] = i
    return np.where(first < 0, num_bins - 1, np.maximum(first - 1, 0))


def find_bins_search(values, edges, num_bins):
    """the same bins by a search -- only for finite (hence non-decreasing) edges; the tests check it against the scan where both run"""
    v = np.asarray(values, F).ravel()
    assert np.all(np.isfinite(edges)) and np.all(np.diff(edges.astype(np.float64)) >= 0)
    i = np.searchsorted(edges, v, "left")            # first i with v <= edges[i]; NaN sorts past the end
    return np.where(i > num_bins, num_bins - 1, np.maximum(i - 1, 0))


class Histogram:
    def __init__(self, num_bins, scan_limit=1 << 22):
        assert num_bins >= 1
        self.num_bins = num_bins
        self.bins = np.zeros(num_bins, np.uint64)
        self.edges = np.empty(0, F)
        self.num_observations = 0
        self.enabled = True
        self.scan_limit = scan_limit    # values * edges up to which the literal scan runs; above it the search (finite edges only)

    def observe(self, data):
        if not self.enabled:
            return
        d = np.asarray(data, F).ravel()
        if self.edges.size == 0:
            self.edges = make_edges(d, self.num_bins)
        if d.size * (self.num_bins + 1) <= self.scan_limit or not np.all(np.isfinite(self.edges)):
            k = find_bins_scan(d, self.edges, self.num_bins)
        else:
            k = find_bins_search(d, self.edges, self.num_bins)
        self.bins += np.bincount(k, minlength=self.num_bins).astype(np.uint64)
        self.num_observations += 1

    def reset(self):
        self.bins[:] = 0
        self.edges = np.empty(0, F)
        self.num_observations = 0

    def stats(self):
        total = int(self.bins.sum(dtype=np.uint64))
        weighted = sum(int(i) * int(c) for i, c in enumerate(self.bins) if c) & ((1 << 64) - 1)
        mean = F(F(weighted) / F(total)) if total else F(0.0)      # `as f32` of a u64 rounds to nearest, as np.float32(int) does
        return dict(num_observations=self.num_observations, total_count=total, mean_bin=mean,
                    max_bin_count=int(self.bins.max()) if self.num_bins else 0)


def same_bits(a, b):
    """bit equality of two f32 arrays, except that +0 and -0 are equal (the sign of a zero min / max is unspecified in Rust) and that a
    NaN equals a NaN: the sign and payload of a NaN that arithmetic PRODUCES (0 * inf, inf - inf: the edges after an infinite first
    observation) are unspecified in IEEE 754 and in Rust, and do differ between this host (x86: 0xffc00000) and the device (0x7fc00000)"""
    a, b = np.atleast_1d(np.asarray(a, F)), np.atleast_1d(np.asarray(b, F))
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    return bool(np.all((ua == ub) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))))
