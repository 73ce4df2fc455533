#!/usr/bin/env python3
"""Time of the spatial-consistency attention, forward and forward + backward (f-12), next to the reference's three lines in torch
on the same device (materialised bs x N x N scores, autograd) at the training shape (bs 16, N 1000) and at (bs 1, N 5000).

The method of tools/loss_bench.py: device events around a window of back-to-back calls that fills `--window` seconds after
`--warmup` calls of the same shape; the two sides of a row alternate inside one process (`--rounds` rounds, the median round is
printed with the spread).  These are CALL times (wrapper, allocations and every launch of the call), not kernel times.  The torch
side is the comparison, never the code under test.  Flop: 4 C N^2 bs for the forward, 18 C N^2 bs for forward + backward (the
backward's 14 C N^2: both kernels recompute S and dP, 8, and accumulate dQ, dK, dV, 6)."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from pointdsc_amd import ops, training  # noqa: E402
from loss_bench import timed  # noqa: E402

C = 128


def torch_lines(q, k, v, compat):
    feat_attention = torch.matmul(q, k.transpose(1, 2)) / C ** 0.5
    return torch.matmul(torch.softmax(compat * feat_attention, dim=-1), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attention_backward_bench needs the GPU: a CPU run gives no time"
    dev = "cuda:0"
    for bs, n in ((16, 1000), (1, 5000)):
        gen = torch.Generator().manual_seed(bs * n)
        q, k, v, dO = (torch.randn(bs, n, C, generator=gen).to(dev) for _ in range(4))
        compat = training._pad_compat(torch.clamp(torch.rand(bs, n, n, generator=gen) * 1.5 - 0.5, 0, 1), n).to(dev)
        cn = compat[..., :n].contiguous()
        qkv = torch.cat((q * training.Q_SCALE, k, v), dim=-1).reshape(bs * n, 3 * C).contiguous()
        dmsg = dO.reshape(bs * n, C).contiguous()
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))

        def device_fb():
            msg, lse = ops.sc_attention_lse(qkv, compat, bs, n)
            return ops.sc_attention_backward(qkv, compat, msg, lse, dmsg, bs, n)

        def wrapper_fb():
            return torch.autograd.grad(training.sc_attention(qg, kg, vg, compat), (qg, kg, vg), dO)

        def torch_fb():
            return torch.autograd.grad(torch_lines(qg, kg, vg, cn), (qg, kg, vg), dO)

        rows = [
            ("forward", 4, lambda: ops.sc_attention_lse(qkv, compat, bs, n), lambda: torch_lines(q, k, v, cn)),
            ("forward + backward", 18, device_fb, torch_fb),
            ("forward + backward, autograd wrapper", 18, wrapper_fb, torch_fb),
        ]
        print(f"bs={bs} N={n}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
        for name, flop_c, ours, theirs in rows:
            flop = flop_c * C * n * n * bs
            t_ours, t_theirs = [], []
            for _ in range(a.rounds):                     # alternate the two sides
                t_ours.append(timed(ours, a.warmup, a.window)[0])
                t_theirs.append(timed(theirs, a.warmup, a.window)[0])
            mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
            print(f"  {name:38s} device {mo:9.1f} ({min(t_ours):.1f} .. {max(t_ours):.1f}) {flop / mo * 1e-6:6.1f} Tflop/s   "
                  f"torch {mt:9.1f} ({min(t_theirs):.1f} .. {max(t_theirs):.1f}) {flop / mt * 1e-6:6.1f} Tflop/s   "
                  f"torch / device {mt / mo:6.2f}")


if __name__ == "__main__":
    main()
