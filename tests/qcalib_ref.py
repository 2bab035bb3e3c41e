"""Numpy restatement of percentile calibration (csrc/qcalib.hip), exact to the bit: f32 operations one at a time, integer counts.

    amax = max(|min|, |max|)                        of the finite range th_act_range_update keeps (tests/qstatic_ref.py's act_scale_of)
    inv  = (float)num_bins / amax
    bin  = min((int)(|v| * inv), num_bins - 1)      every finite v; a product that is +inf or NaN takes the last bin; NaN, +-inf skipped
    k    = the first bin with cum[k] * 10^6 >= total * keep_ppm
    T    = (float)(k + 1) * (amax / (float)num_bins), exactly amax at k = num_bins - 1;  scale = T / 127
    fallback (min == max, amax not a normal number, total == 0): the scale stays, k = num_bins - 1"""
import numpy as np

from tests import qstatic_ref as R

f32 = np.float32
MAX_BINS, MIN_BINS = 8192, 16
TINY = np.finfo(f32).tiny


def finite_range(*tensors):
    """{finite min, finite max} over every tensor, as th_act_range_update leaves it ({+inf, -inf} over nothing finite)"""
    fin = np.concatenate([np.asarray(t, f32).reshape(-1) for t in tensors])
    fin = fin[np.isfinite(fin)]
    return (f32(fin.min()), f32(fin.max())) if fin.size else (f32(np.inf), f32(-np.inf))


def amax_of(range2):
    return f32(np.fmax(np.abs(f32(range2[0])), np.abs(f32(range2[1]))))      # fmaxf: a NaN loses to a number


def bins_of(x, range2, num_bins, into=None):
    """th_act_hist_update: -> uint64 counters [num_bins] (added to `into`)"""
    assert MIN_BINS <= num_bins <= MAX_BINS
    v = np.asarray(x, f32).reshape(-1)
    v = np.abs(v[np.isfinite(v)])
    with np.errstate(all="ignore"):
        inv = f32(f32(num_bins) / amax_of(range2))
        t = (v * inv).astype(f32)
    k = np.where(np.isnan(t), f32(num_bins - 1), np.minimum(t, f32(num_bins - 1))).astype(np.int64)
    out = np.bincount(k, minlength=num_bins).astype(np.uint64)
    return out if into is None else (np.asarray(into, np.uint64) + out).astype(np.uint64)


def threshold_of(k, range2, num_bins):
    amax = amax_of(range2)
    return amax if k == num_bins - 1 else f32(f32(k + 1) * f32(amax / f32(num_bins)))


def scale_from_hist(bins, range2, keep_ppm, scale_before):
    """th_act_scale_from_hist: -> (scale f32, stats4 = [k, total, cum[k], bins[k]] as Python ints)"""
    bins = [int(b) for b in np.asarray(bins, np.uint64)]
    nb = len(bins)
    assert MIN_BINS <= nb <= MAX_BINS and 1 <= keep_ppm <= 1000000
    total, amax = sum(bins), amax_of(range2)
    normal = bool(np.isfinite(amax)) and amax >= TINY
    if f32(range2[0]) == f32(range2[1]) or not normal or total == 0:
        return f32(scale_before), [nb - 1, total, total, bins[nb - 1]]
    assert total < 2 ** 43
    cum = 0
    for k, b in enumerate(bins):
        cum += b
        if cum * 1000000 >= total * keep_ppm:
            break
    return f32(threshold_of(k, range2, nb) / f32(127)), [k, total, cum, bins[k]]


def calibrate(tensors, keep_ppm, num_bins):
    """what quantize_static's percentile method does for one layer whose float inputs are `tensors`:
    -> dict(min, max, threshold, scale, bin, total, kept, bin_count)"""
    rng2 = finite_range(*tensors)
    with np.errstate(all="ignore"):
        before = R.act_scale(*rng2)
    bins = None
    for t in tensors:
        bins = bins_of(t, rng2, num_bins, bins)
    scale, (k, total, kept, count) = scale_from_hist(bins, rng2, keep_ppm, before)
    return dict(min=rng2[0], max=rng2[1], threshold=threshold_of(k, rng2, num_bins), scale=scale, bin=k, total=total, kept=kept, bin_count=count)


def keep_ppm_of(percentile):
    return int(round(float(percentile) * 1e4))


# ---------------------------------------------------------------- the outlier Linear
OUTLIER_SHAPE = (64, 256, 40)      # batch, in_features, out_features


def outlier_layer(seed):
    """x ~ N(0, 1) [64, 256] with x[0, 5] = 1000, w ~ N(0, 1) / 16 [40, 256]"""
    B, K, N = OUTLIER_SHAPE
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, K)).astype(f32)
    x[0, 5] = f32(1000)
    w = (rng.standard_normal((N, K)) / 16).astype(f32)
    return x, w


def static_linear(x, w, sx):
    """tests/qstatic_ref.py's whole static layer without a bias: activation codes with sx, the packed weight, the integer product"""
    qw, wp = R.pack(w)
    return R.linear_q8q8(R.quantize_act(x, sx)[0], sx, qw, wp)


def clean_row_error(y, x, w):
    """the worst error of the rows that hold no outlier (1 ..) against the float64 product, over their max |y|"""
    y64 = x.astype(np.float64)[1:] @ w.astype(np.float64).T
    return float(np.abs(np.asarray(y, np.float64)[1:] - y64).max() / np.abs(y64).max())
