"""BatchNorm2d in float64 numpy: the formulas of include/taper_hip.h (th_batchnorm2d_fwd / th_batchnorm2d_bwd), which are
torch.nn.BatchNorm2d's -- tests/golden/make_golden_batchnorm.py pins this file against torch on the CPU, and the GPU tests compare the
kernels against it.  x, y, gy: [n, c, h, w]; per-channel vectors: [c]."""
import numpy as np

F64 = np.float64
AX = (0, 2, 3)


def _bc(v):
    return np.asarray(v, F64).reshape(1, -1, 1, 1)


def forward(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, training=True, relu=False):
    """-> dict(y, save_mean, save_invstd, var, running_mean, running_var): the statistics the forward normalised with (the batch's in
    training mode, the running pair otherwise) and the running pair afterwards (unchanged in eval mode)."""
    x = np.asarray(x, F64)
    rm, rv = np.asarray(running_mean, F64).copy(), np.asarray(running_var, F64).copy()
    m = x.shape[0] * x.shape[2] * x.shape[3]
    if training:
        if m == 1:
            raise ValueError("Expected more than 1 value per channel when training")
        mean = x.mean(axis=AX)
        var = ((x - _bc(mean)) ** 2).mean(axis=AX)          # biased
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * (var * m / (m - 1))   # unbiased
    else:
        mean, var = rm.copy(), rv.copy()
    invstd = 1.0 / np.sqrt(var + eps)
    y = (x - _bc(mean)) * _bc(invstd * np.asarray(gamma, F64)) + _bc(beta)
    if relu:
        y = np.maximum(y, 0.0)
    return dict(y=y, save_mean=mean, save_invstd=invstd, var=var, running_mean=rm, running_var=rv)


def backward(gy, x, gamma, save_mean, save_invstd, y=None, batch_stats=True):
    """-> (gx, ggamma, gbeta); y given: gy is masked by y > 0 first (the fused ReLU)"""
    gy, x = np.asarray(gy, F64), np.asarray(x, F64)
    if y is not None:
        gy = np.where(np.asarray(y) > 0, gy, 0.0)
    m = x.shape[0] * x.shape[2] * x.shape[3]
    xh = (x - _bc(save_mean)) * _bc(save_invstd)
    gbeta = gy.sum(axis=AX)
    ggamma = (gy * xh).sum(axis=AX)
    a = _bc(np.asarray(gamma, F64) * np.asarray(save_invstd, F64))
    gx = a * (gy - _bc(gbeta) / m - xh * _bc(ggamma) / m) if batch_stats else a * gy
    return gx, ggamma, gbeta


def softmax_xent(logits, labels):
    """mean cross-entropy of [B, C] logits against integer labels, and its gradient"""
    z = np.asarray(logits, F64)
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    b = z.shape[0]
    idx = np.asarray(labels).astype(np.int64)
    loss = -logp[np.arange(b), idx].mean()
    g = np.exp(logp)
    g[np.arange(b), idx] -= 1.0
    return loss, g / b
