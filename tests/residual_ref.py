"""The residual tail in float64 numpy: y = relu?(bn(x) + r) and its backward, built on tests/batchnorm_ref.py (the formulas of
include/taper_hip.h: th_bn_residual_fwd / th_bn_residual_bwd).  tests/golden/make_golden_residual.py pins this file against torch on the
CPU, and the GPU tests compare the layer against it.  x, r, y, gy: [n, c, h, w]; per-channel vectors: [c]."""
import numpy as np

from tests import batchnorm_ref as R

F64 = np.float64


def forward(x, r, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, training=True, relu=False):
    """-> batchnorm_ref.forward's dict with y = bn(x) + r, then max(y, 0) with relu (the ReLU comes after the add)"""
    f = R.forward(x, gamma, beta, running_mean, running_var, eps, momentum, training, False)
    y = f["y"] + np.asarray(r, F64)
    f["y"] = np.maximum(y, 0.0) if relu else y
    return f


def backward(gy, x, gamma, save_mean, save_invstd, y=None, batch_stats=True):
    """-> (gx, gr, ggamma, gbeta); y given: gy is masked by y > 0 first, and the residual's gradient is that masked gy"""
    gx, gg, gb = R.backward(gy, x, gamma, save_mean, save_invstd, y, batch_stats)
    gr = np.asarray(gy, F64) if y is None else np.where(np.asarray(y) > 0, np.asarray(gy, F64), 0.0)
    return gx, gr, gg, gb
