"""Writes tests/golden/batchnorm_*.npz: torch.nn.BatchNorm2d on the CPU in float64, seeded -- the fixtures that pin tests/batchnorm_ref.py
(tests/test_batchnorm_abi.py) and the five-step trajectory the GPU test replays (tests/test_gpu_batchnorm.py).

    python tests/golden/make_golden_batchnorm.py
"""
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
torch.set_default_dtype(torch.float64)


def single(shape, seed):
    """three training forwards in a row (running statistics after each), an eval forward, a backward with and without the ReLU"""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    out = {}
    bn = torch.nn.BatchNorm2d(c, eps=1e-5, momentum=0.1)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g))
    out["gamma"], out["beta"] = bn.weight.detach().numpy().copy(), bn.bias.detach().numpy().copy()
    bn.train()
    for k in range(3):
        x = torch.randn(shape, generator=g) * (torch.rand(1, c, 1, 1, generator=g) * 1.5 + 0.5) + (torch.rand(1, c, 1, 1, generator=g) * 2 - 1)
        y = bn(x)
        out[f"x{k}"], out[f"y{k}"] = x.numpy().copy(), y.detach().numpy().copy()
        out[f"rm{k}"], out[f"rv{k}"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    bn.eval()
    xe = torch.randn(shape, generator=g)
    out["xe"], out["ye"] = xe.numpy().copy(), bn(xe).detach().numpy().copy()
    bn.train()
    for relu in (False, True):
        bn.zero_grad()
        x = (torch.randn(shape, generator=g) * 1.3 + 0.2).requires_grad_()
        gy = torch.randn(shape, generator=g) + 0.5
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        y = bn(x)
        if relu:
            y = torch.relu(y)
        y.backward(gy)
        with torch.no_grad():   # (the backward case does not count as a running update in the fixture)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
        tag = "r" if relu else "p"
        out[f"bx_{tag}"], out[f"bgy_{tag}"], out[f"by_{tag}"] = x.detach().numpy().copy(), gy.numpy().copy(), y.detach().numpy().copy()
        out[f"gx_{tag}"], out[f"gg_{tag}"], out[f"gb_{tag}"] = x.grad.numpy().copy(), bn.weight.grad.numpy().copy(), bn.bias.grad.numpy().copy()
    if n * h * w > 1:   # eval-mode layer that still trains its affine pair
        bn.eval()
        bn.zero_grad()
        x = torch.randn(shape, generator=g).requires_grad_()
        gy = torch.randn(shape, generator=g) + 0.5
        bn(x).backward(gy)
        out["bx_e"], out["bgy_e"] = x.detach().numpy().copy(), gy.numpy().copy()
        out["gx_e"], out["gg_e"], out["gb_e"] = x.grad.numpy().copy(), bn.weight.grad.numpy().copy(), bn.bias.grad.numpy().copy()
        out["rm_e"], out["rv_e"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    return out


def trajectory(seed=7):
    """five Adam steps (lr 1e-2) of BatchNorm2d(3) -> ReLU -> Flatten -> Linear(48, 5) -> cross-entropy on one fixed batch [8, 3, 4, 4]"""
    g = torch.Generator().manual_seed(seed)
    bn, lin = torch.nn.BatchNorm2d(3), torch.nn.Linear(48, 5)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(3, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(3, generator=g) * 0.1)
        lin.weight.copy_(torch.randn(5, 48, generator=g) * 0.2)
        lin.bias.copy_(torch.randn(5, generator=g) * 0.1)
    x = torch.randn(8, 3, 4, 4, generator=g) * 1.5 + 0.3
    labels = torch.randint(0, 5, (8,), generator=g)
    out = dict(x=x.numpy().copy(), labels=labels.numpy().astype(np.float64), gamma0=bn.weight.detach().numpy().copy(),
               beta0=bn.bias.detach().numpy().copy(), w0=lin.weight.detach().numpy().copy(), b0=lin.bias.detach().numpy().copy())
    opt = torch.optim.Adam(list(bn.parameters()) + list(lin.parameters()), lr=1e-2)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(lin(torch.relu(bn(x)).flatten(1)), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out.update(losses=np.array(losses), gamma=bn.weight.detach().numpy().copy(), beta=bn.bias.detach().numpy().copy(),
               w=lin.weight.detach().numpy().copy(), b=lin.bias.detach().numpy().copy(), running_mean=bn.running_mean.numpy().copy(),
               running_var=bn.running_var.numpy().copy(), lr=np.array(1e-2))
    return out


if __name__ == "__main__":
    np.savez(HERE / "batchnorm_2x5x3x3.npz", **single((2, 5, 3, 3), 1))
    np.savez(HERE / "batchnorm_4x3x1x1.npz", **single((4, 3, 1, 1), 2))
    np.savez(HERE / "batchnorm_trajectory.npz", **trajectory())
