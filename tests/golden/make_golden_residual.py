"""Writes tests/golden/residual_tail_*.npz: relu?(batch_norm(x) + r) with autograd on the CPU in float64 (torch.nn.functional.batch_norm,
an add and a relu), seeded, in training and eval mode, with and without the ReLU -- the fixtures that pin tests/residual_ref.py
(tests/test_residual_abi.py).

    python tests/golden/make_golden_residual.py
"""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
torch.set_default_dtype(torch.float64)
EPS, MOM = 1e-5, 0.1


def tail(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x0 = torch.randn(shape, generator=g) * (torch.rand(1, c, 1, 1, generator=g) * 1.5 + 0.5) + (torch.rand(1, c, 1, 1, generator=g) * 2 - 1)
    r0 = torch.randn(shape, generator=g) * 0.8
    gy = torch.randn(shape, generator=g) + 0.5
    gamma0, beta0 = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm0, rv0 = torch.rand(c, generator=g) * 2 - 1, torch.rand(c, generator=g) * 1.5 + 0.5
    out = dict(x=x0.numpy().copy(), r=r0.numpy().copy(), gy=gy.numpy().copy(), gamma=gamma0.numpy().copy(), beta=beta0.numpy().copy(),
               rm0=rm0.numpy().copy(), rv0=rv0.numpy().copy())
    for mode, training in (("t", True), ("e", False)):
        for tag, relu in (("p", False), ("r", True)):
            x, r = x0.clone().requires_grad_(), r0.clone().requires_grad_()
            gamma, beta = gamma0.clone().requires_grad_(), beta0.clone().requires_grad_()
            rm, rv = rm0.clone(), rv0.clone()
            y = F.batch_norm(x, rm, rv, gamma, beta, training, MOM, EPS) + r
            if relu:
                y = torch.relu(y)
            y.backward(gy)
            k = f"{mode}{tag}"
            out[f"y_{k}"] = y.detach().numpy().copy()
            out[f"gx_{k}"], out[f"gr_{k}"] = x.grad.numpy().copy(), r.grad.numpy().copy()
            out[f"gg_{k}"], out[f"gb_{k}"] = gamma.grad.numpy().copy(), beta.grad.numpy().copy()
            out[f"rm_{k}"], out[f"rv_{k}"] = rm.numpy().copy(), rv.numpy().copy()
    return out


if __name__ == "__main__":
    np.savez(HERE / "residual_tail_2x5x3x3.npz", **tail((2, 5, 3, 3), 11))
    np.savez(HERE / "residual_tail_4x3x1x1.npz", **tail((4, 3, 1, 1), 12))
