#!/usr/bin/env python3
"""Time of the train path's plain linears on the device (pointdsc_amd.linear_rows, qkv_projection, classification_head; DESIGN.md
section 8 f-16) next to the torch lines each of them replaces in ``training._train_encoder`` / ``train_forward``.

At M = bs * N rows (16 x 1000 by default), forward alone (no graph kept) and forward + backward (gradients for the input, where the
model needs one, and every parameter):

  layer0 (6,128)                 linear_rows(x, w, b)                   F.linear(x, w[:, :, 0], b); x carries no gradient
  fc_message.6 (64,128) + feat   linear_rows(h, w, b, feat)             feat + F.linear(h, w[:, :, 0], b)
  q|k|v (128, 3 x 128)           qkv_projection(x, wq, bq, ...)         torch.cat of the three weights (q's times Q_SCALE) and of
                                                                        the three biases, one F.linear
  head (128, 32, 32, 1)          classification_head(feat, w0, ...)     three F.linear with two F.relu between them

The method of tools/pointwise_train_bench.py: device events around a window of back-to-back calls that fills `--window` seconds
after `--warmup` calls; the two sides alternate inside one process; the median of `--rounds` windows is printed with min .. max.
These are CALL times, host work (torch's dispatch, the ctypes calls, the allocations of the outputs) included."""
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
    from pointdsc_amd import classification_head, linear_rows, qkv_projection, training
    assert torch.cuda.is_available(), "linear_train_bench needs the GPU: a CPU run gives no time"
    dev, m = "cuda:0", a.rows
    gen = torch.Generator().manual_seed(m)

    def spread(ts):
        return f"{statistics.median(ts):8.1f} ({min(ts):.1f} .. {max(ts):.1f})"

    def compare(name, ours, theirs):
        t_ours, t_theirs = [], []
        for _ in range(a.rounds):                         # alternate the two sides
            t_ours.append(timed(ours, a.warmup, a.window)[0])
            t_theirs.append(timed(theirs, a.warmup, a.window)[0])
        mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
        print(f"  {name:44s} device {spread(t_ours)}   torch {spread(t_theirs)}   torch / device {mt / mo:5.2f}")

    def no_graph(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def both(name, ours, theirs, leaves, dy):
        compare(f"{name} forward", no_graph(ours), no_graph(theirs))
        compare(f"{name} forward + backward", lambda: torch.autograd.grad(ours(), leaves, dy), lambda: torch.autograd.grad(theirs(), leaves, dy))

    def rows(c, grad=True):
        return torch.randn(m, c, generator=gen).to(dev).requires_grad_(grad)

    print(f"M={m}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
    conv = nn.Conv1d(6, 128, 1).to(dev)
    x, dy = rows(6, grad=False), rows(128, grad=False)
    both("layer0 (6,128)", lambda: linear_rows(x, conv.weight, conv.bias), lambda: F.linear(x, conv.weight[:, :, 0], conv.bias),
         (conv.weight, conv.bias), dy)

    fc6 = nn.Conv1d(64, 128, 1).to(dev)
    h, feat = rows(64), rows(128)
    both("fc_message.6 (64,128) + residual", lambda: linear_rows(h, fc6.weight, fc6.bias, feat),
         lambda: feat + F.linear(h, fc6.weight[:, :, 0], fc6.bias), (h, feat, fc6.weight, fc6.bias), dy)

    q, k, v = (nn.Conv1d(128, 128, 1).to(dev) for _ in range(3))
    xq, dqkv = rows(128), rows(384, grad=False)

    def torch_qkv():
        w = torch.cat((q.weight[:, :, 0] * training.Q_SCALE, k.weight[:, :, 0], v.weight[:, :, 0]))
        b = torch.cat((q.bias * training.Q_SCALE, k.bias, v.bias))
        return F.linear(xq, w, b)
    both("q|k|v (128, 3 x 128)", lambda: qkv_projection(xq, q.weight, q.bias, k.weight, k.bias, v.weight, v.bias), torch_qkv,
         (xq, q.weight, q.bias, k.weight, k.bias, v.weight, v.bias), dqkv)

    c0, c1, c2 = nn.Conv1d(128, 32, 1).to(dev), nn.Conv1d(32, 32, 1).to(dev), nn.Conv1d(32, 1, 1).to(dev)
    xf, dl = rows(128), torch.randn(m, generator=gen).to(dev)

    def torch_head():
        return F.linear(F.relu(F.linear(F.relu(F.linear(xf, c0.weight[:, :, 0], c0.bias)), c1.weight[:, :, 0], c1.bias)),
                        c2.weight[:, :, 0], c2.bias).reshape(-1)
    both("head (128, 32, 32, 1)", lambda: classification_head(xf, c0.weight, c0.bias, c1.weight, c1.bias, c2.weight, c2.bias), torch_head,
         (xf, c0.weight, c0.bias, c1.weight, c1.bias, c2.weight, c2.bias), dl)


if __name__ == "__main__":
    main()
