#!/usr/bin/env python3
"""Time of the differentiable per-seed solver (f-14) at the training shape (bs 16, N 1000, S 100 seeds, k 40), next to torch on the
same device, and of the training step with a transformation weight.

  kernel      training.seed_solve forward + backward for a DENSE upstream gradient (every seed) and for a SPARSE one (one seed per
              pair: what the vote's winner gives in training), against torch's autograd of the same formulas on the device
              (tests/seed_solve_oracle.chain: [bs*S, k, k] matrices for every iterate, the 3x3 SVD on the host as in the reference);
              the forward alone is printed too, so that the backward's share can be read off.
  whole step  the step of tools/train_step_bench.py (zero_grad, train()-mode forward, losses, backward, Adam; 12 layers) with
              weights (1, 1, 1) on TrainablePointDSC(differentiable_trans=True) against weights (1, 1, 0) on the plain module --
              the parent's step.

The method of tools/attention_backward_bench.py: device events around a window of back-to-back calls that fills `--window` seconds
after `--warmup` calls; the sides alternate inside one process; the median of `--rounds` windows is printed with the spread.
These are CALL times, host work included.  If the sparse call is not clearly cheaper than the dense one, the skip of the seeds
without a gradient is not working."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import seed_solve_oracle as SO
    from loss_bench import timed
    from pointdsc_amd import ClassificationLoss, PointDSC, SpectralMatchingLoss, TransformationLoss, ops, synthetic, training
    assert torch.cuda.is_available(), "seed_solve_backward_bench needs the GPU: a CPU run gives no time"
    dev, bs, n, S, k, iters = "cuda:0", a.bs, a.n, a.seeds, a.k, 10

    def spread(ts):
        return f"{statistics.median(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f})"

    def measure(fns):
        ts = [[] for _ in fns]
        for _ in range(a.rounds):                             # alternate the sides
            for t, fn in zip(ts, fns):
                t.append(timed(fn, a.warmup, a.window)[0])
        return ts

    print(f"bs={bs} N={n} S={S} k={k}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
    gen = torch.Generator().manual_seed(bs * n)
    normed = F.normalize(0.35 * torch.randn(bs, n, 128, generator=gen) + torch.randn(bs, 1, 128, generator=gen), dim=-1).to(dev)
    batch = {key: v.to(dev) for key, v in synthetic.make_batch(bs, n, seed=100, inlier_ratio=0.3).items()}
    src, tgt = batch["src_keypts"], batch["tgt_keypts"]
    seeds = ops.rank_select(torch.randn(bs, n, generator=gen).to(dev), S)
    knn = ops.knn_seeds(normed, seeds, k, form="matrix")
    sigma, sigma_spat = torch.tensor([1.5], device=dev, requires_grad=True), torch.tensor([0.1], device=dev)
    nd = normed.clone().requires_grad_(True)
    dense = torch.randn(bs, S, 4, 4, generator=gen).to(dev)
    dense[:, :, 3] = 0
    sparse = torch.zeros_like(dense)
    sparse[torch.arange(bs), torch.randint(S, (bs,), generator=gen)] = dense[:, 0]
    knn_long = knn.long()

    def ours(g):
        return lambda: torch.autograd.grad(training.seed_solve(nd, src, tgt, knn, sigma, sigma_spat, iters), (nd, sigma), g)

    def theirs(g):
        return lambda: torch.autograd.grad(SO.chain(nd, sigma, src, tgt, knn_long, sigma_spat, iters), (nd, sigma), g[:, :, :3])

    def forward_only():
        with torch.no_grad():
            return training.seed_solve(nd, src, tgt, knn, sigma, sigma_spat, iters)

    t_fwd, t_dense, t_sparse, t_torch, t_torch_sparse = measure([forward_only, ours(dense), ours(sparse), theirs(dense), theirs(sparse)])
    md, ms = statistics.median(t_dense), statistics.median(t_sparse)
    print(f"  seed_solve forward only                       device {spread(t_fwd)}")
    print(f"  forward + backward, dense upstream gradient   device {spread(t_dense)}   torch {spread(t_torch)}   "
          f"torch / device {statistics.median(t_torch) / md:6.2f}")
    print(f"  forward + backward, one seed per pair         device {spread(t_sparse)}   torch {spread(t_torch_sparse)}   "
          f"torch / device {statistics.median(t_torch_sparse) / ms:6.2f}   dense / sparse {md / ms:6.2f}")

    state = synthetic.make_state_dict(PointDSC(num_layers=a.layers).state_dict(), seed=1)
    data = {key: batch[key] for key in ("corr_pos", "src_keypts", "tgt_keypts")}
    gt = batch["gt_labels"]
    cls_fn, sm_fn, tr_fn = ClassificationLoss(False), SpectralMatchingLoss(False), TransformationLoss()

    def make_step(with_trans):
        model = training.TrainablePointDSC(num_layers=a.layers, differentiable_trans=with_trans)
        model.load_state_dict(state, strict=True)
        model = model.to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-6)

        def step():
            opt.zero_grad()
            res = model(data)
            loss = cls_fn(res["final_labels"], gt, device_stats=True)["loss"] + sm_fn(res["M"], gt)
            if with_trans:
                loss = loss + tr_fn(res["final_trans"], batch["gt_trans"], src, tgt, res["final_labels"], device_stats=True)[0]
            loss.backward()
            opt.step()
            return loss
        return step

    t_on, t_off = measure([make_step(True), make_step(False)])
    print(f"bs={bs} N={n} layers={a.layers}: training step (forward, losses, backward, Adam)")
    print(f"  weights (1, 1, 1), differentiable final_trans  device {spread(t_on)}")
    print(f"  weights (1, 1, 0), the parent's step           device {spread(t_off)}   "
          f"(1,1,1) / (1,1,0) {statistics.median(t_on) / statistics.median(t_off):6.3f}")


if __name__ == "__main__":
    main()
