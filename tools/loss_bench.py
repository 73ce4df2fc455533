#!/usr/bin/env python3
"""Time of every loss call of pointdsc_amd.losses (f-11) next to the same formulas written in torch on the same device -- what a
user of the reference's libs/loss.py gets today -- at (bs 16, N 1000) and (bs 1, N 5000).

Device events around a window of back-to-back calls that fills `--window` seconds (0.3 s by default: 300 to 15 000 calls) after
`--warmup` calls of the same shape; the two sides of a row alternate inside one process (`--rounds` rounds, the median round is
printed with the spread).  These are CALL times (wrapper, allocations and every launch of the call), not kernel times.  The torch side is the comparison, never the code
under test.  Bytes: the features form reads bs N 512 B (plus L2-resident re-reads of the column tiles); the torch path writes and
reads at least six N x N fp32 arrays per pair."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from pointdsc_amd import losses, ops, synthetic  # noqa: E402


def timed(fn, warmup, window_s):
    """microseconds per call: device events around enough back-to-back calls to fill `window_s` seconds (counted from a first
    window of 20 calls), after `warmup` calls of the same shape."""
    def window(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    iters = max(20, int(window_s * 1e6 / window(20)))
    return window(iters), iters


# ---- the reference's formulas in torch, on the device (libs/loss.py without the host round trips of sklearn) -----------------
def torch_sm_matrix(M, gt, balanced):
    gt_M = ((gt[:, None, :] + gt[:, :, None]) == 2).float()
    gt_M = gt_M * (1 - torch.eye(gt.shape[1], device=gt.device))[None]
    if balanced:
        p = ((M - 1) ** 2 * gt_M).sum(-1).sum(-1) / (torch.relu(gt_M.sum(-1).sum(-1) - 1.0) + 1.0)
        q = (M ** 2 * (1 - gt_M)).sum(-1).sum(-1) / (torch.relu((1 - gt_M).sum(-1).sum(-1) - 1.0) + 1.0)
        return torch.mean(p * 0.5 + q * 0.5)
    return torch.nn.functional.mse_loss(M, gt_M)


def torch_feature_matrix(normed, sigma):
    M = torch.matmul(normed, normed.transpose(1, 2))
    M = torch.clamp(1 - (1 - M) / sigma ** 2, min=0, max=1)
    return M * (1 - torch.eye(M.shape[1], device=M.device))[None]


def torch_classification(pred, gt, balanced):
    num_pos = torch.relu(gt.sum() - 1) + 1
    num_neg = torch.relu((1 - gt).sum() - 1) + 1
    pw = num_neg / num_pos if balanced else None
    return torch.nn.functional.binary_cross_entropy_with_logits(pred, gt, pos_weight=pw)


def torch_transformation(trans, gt_trans, src, tgt, probs):
    out = []
    for i in range(trans.shape[0]):
        warp = src[i] @ trans[i, :3, :3].T + trans[i, :3, 3]
        out.append(((warp - tgt) ** 2).sum(-1).mean() + torch.norm(warp - tgt, dim=-1).mean())
    return torch.stack(out).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "loss_bench needs the GPU: a CPU run gives no time"
    dev = "cuda:0"
    for bs, n in ((16, 1000), (1, 5000)):
        batch = synthetic.make_batch(bs, n, seed=5, inlier_ratio=0.3)
        gt, src, tgt, gt_trans = (batch[k].to(dev) for k in ("gt_labels", "src_keypts", "tgt_keypts", "gt_trans"))
        g = torch.Generator().manual_seed(bs * n)
        f = torch.randn(bs, n, 128, generator=g)
        f[..., 0] += 3.0 * batch["gt_labels"]
        normed = torch.nn.functional.normalize(f, dim=-1).to(dev).reshape(bs * n, 128).contiguous()
        normed3 = normed.view(bs, n, 128)
        sigma = torch.tensor([1.0], device=dev)
        pred = (torch.randn(bs, n, generator=g) * 4).to(dev)
        M = ops.feature_compat(normed, sigma, bs, n)
        normed_g, sigma_g = normed3.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
        M_g, pred_g = M.clone().requires_grad_(True), pred.clone().requires_grad_(True)

        def torch_features_fb():
            loss = torch_sm_matrix(torch_feature_matrix(normed_g, sigma_g), gt, True)
            return torch.autograd.grad(loss, (normed_g, sigma_g))

        def torch_matrix_fb():
            return torch.autograd.grad(torch_sm_matrix(M_g, gt, True), M_g)

        def torch_cls_fb():
            return torch.autograd.grad(torch_classification(pred_g, gt, True), pred_g)

        rows = [
            ("sm features, forward", lambda: losses.sm_loss_features_raw(normed, sigma, gt, True),
             lambda: torch_sm_matrix(torch_feature_matrix(normed3, sigma), gt, True)),
            ("sm features, forward + backward", lambda: losses.sm_loss_features_raw(normed, sigma, gt, True, True, True), torch_features_fb),
            ("sm matrix, forward", lambda: losses.sm_loss_matrix_raw(M, gt, True), lambda: torch_sm_matrix(M, gt, True)),
            ("sm matrix, forward + backward", lambda: losses.sm_loss_matrix_raw(M, gt, True, True), torch_matrix_fb),
            ("classification, forward", lambda: losses.classification_loss_raw(pred, gt, None, True), lambda: torch_classification(pred, gt, True)),
            ("classification, forward + backward", lambda: losses.classification_loss_raw(pred, gt, None, True, True), torch_cls_fb),
            ("transformation", lambda: losses.transformation_loss_raw(gt_trans, gt_trans, src, tgt, pred),
             lambda: torch_transformation(gt_trans, gt_trans, src, tgt, pred)),
        ]
        print(f"bs={bs} N={n}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
        for name, ours, theirs in rows:
            t_ours, t_theirs = [], []
            for _ in range(a.rounds):                     # alternate the two sides
                t_ours.append(timed(ours, a.warmup, a.window)[0])
                t_theirs.append(timed(theirs, a.warmup, a.window)[0])
            mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
            print(f"  {name:36s} device {mo:9.1f} ({min(t_ours):.1f} .. {max(t_ours):.1f})   torch {mt:9.1f} "
                  f"({min(t_theirs):.1f} .. {max(t_theirs):.1f})   torch / device {mt / mo:6.2f}")


if __name__ == "__main__":
    main()
