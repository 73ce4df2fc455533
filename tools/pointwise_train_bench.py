#!/usr/bin/env python3
"""Time of the fused train-mode point-wise layer (pointdsc_amd.conv_bn_relu) next to torch's modules.

For the model's three (Cin, Cout) shapes at M = bs * N rows (16 x 1000 by default): the forward alone (no graph kept) and forward +
backward (gradients for x and the five parameters) of ``conv_bn_relu`` against the same Conv1d(k=1) -> BatchNorm1d -> ReLU as
``training._train_encoder`` builds it by default: F.linear, the BatchNorm1d module in train() mode, F.relu, torch's autograd.

The method of tools/train_step_bench.py: device events around a window of back-to-back calls that fills `--window` seconds after
`--warmup` calls; the two sides alternate inside one process; the median of `--rounds` windows is printed with min .. max.  These
are CALL times, host work (torch's dispatch, the ctypes calls, the allocations of the outputs) included."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=16000, help="M = bs * N")
    a = ap.parse_args()

    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from loss_bench import timed
    from pointdsc_amd import conv_bn_relu, ops
    assert torch.cuda.is_available(), "pointwise_train_bench needs the GPU: a CPU run gives no time"
    dev, m = "cuda:0", a.rows

    def spread(ts):
        return f"{statistics.median(ts):8.1f} ({min(ts):.1f} .. {max(ts):.1f})"

    def compare(name, ours, theirs):
        t_ours, t_theirs = [], []
        for _ in range(a.rounds):                         # alternate the two sides
            t_ours.append(timed(ours, a.warmup, a.window)[0])
            t_theirs.append(timed(theirs, a.warmup, a.window)[0])
        mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
        print(f"  {name:34s} device {spread(t_ours)}   torch {spread(t_theirs)}   torch / device {mt / mo:5.2f}")

    print(f"M={m}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
    for cin, cout in ops.POINTWISE_TRAIN_SHAPES:
        gen = torch.Generator().manual_seed(cin * 1000 + cout)
        conv, bn = nn.Conv1d(cin, cout, 1).to(dev), nn.BatchNorm1d(cout).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(0.5 + torch.rand(cout, generator=gen))
            bn.bias.copy_(0.5 * torch.randn(cout, generator=gen))
        x = torch.randn(m, cin, generator=gen).to(dev).requires_grad_(True)
        dz = torch.randn(m, cout, generator=gen).to(dev)
        leaves = (x, conv.weight, conv.bias, bn.weight, bn.bias)

        def ours():
            return conv_bn_relu(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)

        def theirs():
            return F.relu(bn(F.linear(x, conv.weight[:, :, 0], conv.bias)))

        def no_graph(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def with_backward(fn):
            return lambda: torch.autograd.grad(fn(), leaves, dz)
        compare(f"({cin:3d},{cout:3d}) forward", no_graph(ours), no_graph(theirs))
        compare(f"({cin:3d},{cout:3d}) forward + backward", with_backward(ours), with_backward(theirs))


if __name__ == "__main__":
    main()
