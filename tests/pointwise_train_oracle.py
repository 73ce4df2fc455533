"""Truth, yardstick and inputs of the f-15 tests (tests/test_pointwise_train.py): the train-mode Conv1d(k=1) -> BatchNorm1d -> ReLU.

Truth: the same computation in fp64 torch on the CPU -- `autograd_run` (F.linear, F.batch_norm(training=True), relu, autograd) for
the small cases, `closed_form` (the formulas of include/pointdsc_hip.h written out) for the large ones, where the ReLU mask is
taken from the device's own Z > 0; a CPU test holds the two to 1e-12 of each other.  Error measure and bound are the project's
(tests/train_oracle.py errors / bound): err(X) = max|X - X64| / max|X64| per tensor, db -- zero in exact arithmetic -- on dW's scale;
yardstick e32 = the maximum of that measure for torch's fp32 modules on the device; bound = max(4 e32, 128 2^-24).

ReLU kinks: a pre-activation gamma xh + beta that changes sign between precisions flips a mask bit and moves a gradient by O(1).
The small cases use generator seeds (SEEDS, found on the CPU) whose fp64 truth keeps every pre-activation at least MARGIN_FLOOR away
from zero; the GPU tests assert that this margin exceeds 8 x the larger absolute pre-activation error of the device and the yardstick."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_oracle as TO  # noqa: E402

SHAPES = ((128, 128), (128, 64), (64, 64))          # (Cin, Cout)
MOMENTUM, EPS = 0.1, 1e-5
MARGIN_FLOOR = 3e-5
TENSORS = ("z", "running_mean", "running_var", "dx", "dw", "db", "dgamma", "dbeta")
OFFSET, OFFSET_CHANNELS = 30.0, (3, 17, 40, 64, 77, 90, 101, 127)

# (M, Cin, Cout, offset) -> generator seed whose fp64 truth has min |gamma xh + beta| > MARGIN_FLOOR (test_seed_margins)
SEEDS = {
    (258, 128, 128, False): 30, (258, 128, 64, False): 1, (258, 64, 64, False): 4, (258, 128, 128, True): 30,
    (2, 128, 64, False): 1, (63, 128, 64, False): 1, (64, 128, 64, False): 1, (65, 128, 64, False): 2,
}
bound = TO.bound


def make_case(m: int, cin: int, cout: int, seed: int, offset: bool = False) -> dict:
    """fp32 CPU inputs: x, w, b, gamma in [0.5, 1.5], beta, non-trivial starting running statistics, dz."""
    gen = torch.Generator().manual_seed(seed)
    c = {
        "x": torch.randn(m, cin, generator=gen),
        "w": torch.randn(cout, cin, generator=gen) / cin ** 0.5,
        "b": 0.5 * torch.randn(cout, generator=gen),
        "gamma": 0.5 + torch.rand(cout, generator=gen),
        "beta": 0.5 * torch.randn(cout, generator=gen),
        "running_mean": 0.3 * torch.randn(cout, generator=gen),
        "running_var": 0.5 + torch.rand(cout, generator=gen),
        "dz": torch.randn(m, cout, generator=gen),
    }
    if offset:
        c["b"][list(OFFSET_CHANNELS)] = OFFSET
    return c


@functools.lru_cache(maxsize=None)
def seeded_case(m: int, cin: int, cout: int, offset: bool = False) -> dict:
    return make_case(m, cin, cout, SEEDS[(m, cin, cout, offset)], offset)


def to(case: dict, dtype=None, device=None) -> dict:
    return {k: v.to(dtype=dtype, device=device).clone() for k, v in case.items()}


def autograd_run(c: dict) -> dict:
    """torch's own modules' arithmetic (F.linear, F.batch_norm with batch statistics, relu) and autograd, in the dtype and on the
    device of `c` -> the TENSORS and 'pre' (the pre-activation gamma xh + beta)."""
    x, w, b, gamma, beta = (c[k].detach().clone().requires_grad_(True) for k in ("x", "w", "b", "gamma", "beta"))
    rm, rv = c["running_mean"].clone(), c["running_var"].clone()
    pre = F.batch_norm(F.linear(x, w, b), rm, rv, gamma, beta, True, MOMENTUM, EPS)
    z = F.relu(pre)
    dx, dw, db, dgamma, dbeta = torch.autograd.grad(z, (x, w, b, gamma, beta), c["dz"])
    return {"z": z.detach(), "pre": pre.detach(), "running_mean": rm, "running_var": rv, "dx": dx, "dw": dw, "db": db,
            "dgamma": dgamma, "dbeta": dbeta}


def closed_form(c: dict, mask=None) -> dict:
    """The formulas of the header, line by line, in the dtype of `c`; mask [M,Cout] bool = Z > 0 (None: this forward's own)."""
    x, w, b, gamma, beta, dz = c["x"], c["w"], c["b"], c["gamma"], c["beta"], c["dz"]
    m = x.shape[0]
    y = x @ w.T + b
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    xh = (y - mean) * invstd
    pre = gamma * xh + beta
    if mask is None:
        mask = pre > 0
    g = torch.where(mask, dz, torch.zeros_like(dz))
    dbeta = g.sum(0)
    dgamma = (g * xh).sum(0)
    dy = gamma * invstd * (g - dbeta / m - xh * dgamma / m)
    return {"z": torch.relu(pre), "pre": pre,
            "running_mean": (1 - MOMENTUM) * c["running_mean"] + MOMENTUM * mean,
            "running_var": (1 - MOMENTUM) * c["running_var"] + MOMENTUM * var * m / (m - 1),
            "dx": dy @ w, "dw": dy.T @ x, "db": dy.sum(0), "dgamma": dgamma, "dbeta": dbeta}


def errors(got: dict, ref64: dict) -> dict:
    """err(X) = max|X - X64| / max|X64| per tensor of TENSORS; db on dW's scale."""
    out = {}
    for name in TENSORS:
        scale = ref64["dw" if name == "db" else name].abs().max()
        out[name] = float((got[name].detach().to(torch.float64).cpu() - ref64[name]).abs().max() / scale)
    return out


def margin(ref64: dict) -> float:
    return float(ref64["pre"].abs().min())


def pre_error(got: dict, ref64: dict) -> float:
    return float((got["pre"].detach().to(torch.float64).cpu() - ref64["pre"]).abs().max())


@functools.lru_cache(maxsize=None)
def truth(m: int, cin: int, cout: int, offset: bool = False) -> dict:
    """fp64 autograd on the CPU of the seeded case; computed once, shared, never modified."""
    return autograd_run(to(seeded_case(m, cin, cout, offset), torch.float64))
