"""Truth, yardstick and inputs of the f-15 tests (tests/test_tail_fp64.py): the forward's tail -- per-seed solver, early-exit fix-up,
scoring, selection, refinement -- against fp64.

Truth: seed_solve_oracle.truth_trans (fp64, CPU, per pair) on the device's own discrete choices -- knn_idx and the iterate count
T = seed_solve_oracle.chosen_T(the pair's mask word); the same fp64 pointdsc_oracle.seed_matrices and the power iteration with that fixed
count give the truth of M, of the chosen iterate and of the weights.
Yardstick e32: `parts`, seed_solve_oracle.chain cut into its pieces (matrices, iterate, weights, Procrustes), in fp32 torch on the CPU;
test_parts_are_chain holds it to chain bit for bit.  Never the code under test.
Measure and bound are f-12..f-14's: err(X) = max|X - X64| / max|X64|, bound max(4 e32, 128 2^-24), per tensor and case."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_solve_oracle as SO  # noqa: E402

from oracle import pointdsc_oracle as O  # noqa: E402

BS, N, S, SIGMA, SIGMA_SPAT = 3, 200, 100, 1.5, 0.1
RATIOS = (0.8, 0.2, 0.8)
TENSORS = ("M", "iterate", "weights", "trans")
bound, err = SO.bound, SO.err


def direct_inputs(seed=40):
    """bs 3 x N 200 by seed_solve_oracle.make_inputs' recipe: features normalize(0.35 randn + one common randn vector per pair),
    pairs synthetic.make_pair(200, seed + i, inlier_ratio 0.8 / 0.2 / 0.8), seeds (7 i) mod 200 for i < 100 (cut to [:S'] for fewer)."""
    from pointdsc_amd import synthetic
    gen = torch.Generator().manual_seed(1000 + seed)
    normed = torch.nn.functional.normalize(0.35 * torch.randn(BS, N, 128, generator=gen) + torch.randn(BS, 1, 128, generator=gen), dim=-1)
    pairs = [synthetic.make_pair(N, seed=seed + i, inlier_ratio=r) for i, r in enumerate(RATIOS)]
    seeds = ((7 * torch.arange(S)) % N).to(torch.int32)[None].repeat(BS, 1).contiguous()
    return {"normed": normed.contiguous(), "src": torch.cat([p["src_keypts"] for p in pairs]).contiguous(),
            "tgt": torch.cat([p["tgt_keypts"] for p in pairs]).contiguous(), "seeds": seeds,
            "sigma": torch.tensor([SIGMA]), "sigma_spat": torch.tensor([SIGMA_SPAT])}


# ---- the yardstick's pieces: seed_solve_oracle.chain, line by line, for ONE pair (normed [N,128], knn_idx [S,k] long) ----------------
def matrices(normed, sigma, src, tgt, knn_idx, sigma_spat):
    f, a, b = normed[knn_idx], src[knn_idx], tgt[knn_idx]
    fm = torch.clamp(1 - (1 - f @ f.transpose(-1, -2)) / sigma.reshape(()) ** 2, min=0)
    da = ((a[..., :, None, :] - a[..., None, :, :]) ** 2).sum(-1) ** 0.5
    db = ((b[..., :, None, :] - b[..., None, :, :]) ** 2).sum(-1) ** 0.5
    M = fm * torch.clamp(1 - (da - db) ** 2 / sigma_spat.reshape(()) ** 2, min=0)
    k = M.shape[-1]
    return M * (1 - torch.eye(k, dtype=M.dtype, device=M.device))


def iterate(M, T):
    """The iterate after T steps of the power iteration from v = 1 (T = 0: the ones)."""
    v = torch.ones_like(M[:, :, 0])
    for _ in range(T):
        v = torch.einsum("sij,sj->si", M, v)
        v = v / (torch.sqrt((v * v).sum(-1, keepdim=True)) + 1e-6)
    return v


def weights(v):
    return v / (v.sum(-1, keepdim=True) + 1e-6)


def procrustes(a, b, w):
    """a, b [S,k,3], w [S,k] -> [S,4,4]; the 3x3 SVD on the host, as in the reference."""
    den = w.sum(-1)[:, None, None] + 1e-6
    cA, cB = (a * w[:, :, None]).sum(1, keepdim=True) / den, (b * w[:, :, None]).sum(1, keepdim=True) / den
    H = (a - cA).transpose(1, 2) @ (w[:, :, None] * (b - cB))
    U, _, Vh = torch.linalg.svd(H.cpu())
    U, V = U.to(H.device), Vh.transpose(1, 2).to(H.device)
    X = V @ U.transpose(1, 2)
    det = (X[:, 0] * torch.linalg.cross(X[:, 1], X[:, 2])).sum(-1)
    D = torch.diag_embed(torch.stack([torch.ones_like(det), torch.ones_like(det), det], -1))
    R = V @ D @ U.transpose(1, 2)
    t = cB.transpose(1, 2) - R @ cA.transpose(1, 2)
    last = torch.zeros(R.shape[0], 1, 4, dtype=R.dtype, device=R.device)
    last[:, 0, 3] = 1
    return torch.cat([torch.cat([R, t], dim=-1), last], dim=1)


def parts(inp, knn_idx, Ts, dtype=torch.float32):
    """The yardstick: per pair b the chain's pieces at that pair's T -> dict(M [bs,S,k,k], iterate, weights [bs,S,k], trans [bs,S,4,4])."""
    out = {n: [] for n in TENSORS}
    c = lambda t: t.to(dtype)
    for b in range(knn_idx.shape[0]):
        idx = knn_idx[b].long().cpu()
        M = matrices(c(inp["normed"][b]), c(inp["sigma"]), c(inp["src"][b]), c(inp["tgt"][b]), idx, c(inp["sigma_spat"]))
        v = iterate(M, Ts[b])
        w = weights(v)
        out["M"].append(M)
        out["iterate"].append(v)
        out["weights"].append(w)
        out["trans"].append(procrustes(c(inp["src"][b])[idx], c(inp["tgt"][b])[idx], w))
    return {n: torch.stack(v) for n, v in out.items()}


def truth(inp, knn_idx, Ts):
    """fp64 on the CPU, per pair at that pair's T -> dict(M, iterate, weights, trans, cond [bs,S]): trans and cond are
    seed_solve_oracle.truth_trans's, M is pointdsc_oracle.seed_matrices', the iterate is `iterate` of it."""
    d = lambda t: t.double().cpu()
    out = {n: [] for n in TENSORS + ("cond",)}
    for b in range(knn_idx.shape[0]):
        idx = knn_idx[b:b + 1].long().cpu()
        trans, cond = SO.truth_trans(d(inp["normed"][b:b + 1]), d(inp["sigma"]), d(inp["src"][b:b + 1]), d(inp["tgt"][b:b + 1]), idx,
                                     d(inp["sigma_spat"]), Ts[b])
        M = O.seed_matrices(d(inp["normed"][b]), d(inp["src"][b]), d(inp["tgt"][b]), idx[0], d(inp["sigma"]), d(inp["sigma_spat"])).double()
        v = iterate(M, Ts[b])
        out["M"].append(M)
        out["iterate"].append(v)
        out["weights"].append(weights(v))
        out["trans"].append(trans[0])
        out["cond"].append(cond[0])
    return {n: torch.stack(v) for n, v in out.items()}


def fp64_check(label, got, ref, e32, pairs, names=TENSORS):
    """Prints one line per tensor (error, torch fp32's error, bound) over the pairs `pairs`, then -> the list of the lines that miss
    the bound.  got / ref / e32: dicts of [bs, S, ...] tensors."""
    misses = []
    for name in names:
        x64 = ref[name][pairs]
        e = err(got[name].cpu()[pairs], x64)
        y = err(e32[name][pairs], x64)
        line = f"f15 {label}: {name:8s} err {e:.3e}  torch fp32 {y:.3e}  bound {bound(y):.3e}"
        print(line)
        if not e <= bound(y):
            misses.append(line)
    return misses


def mask_from_iterates(iters, k, num_iter):
    """Host replay of the convergence mask on the device's own iterates [bs,S,num_iter,64] in fp64: bit i of a pair's word is set iff
    every seed and lane < k has |v_i - v_(i-1)| <= 1e-8 + 1e-5 |v_(i-1)| (v_(-1) = 1).  -> (must_be_set, may_be_set) words per pair:
    a bit may go either way only where some entry lies within a factor 1 +- 2^-20 of its threshold (fp32 rounding of the threshold)."""
    v = iters.double().cpu()[:, :, :num_iter, :k]
    last = torch.cat([torch.ones_like(v[:, :, :1]), v[:, :, :-1]], dim=2)
    lhs, thr = (v - last).abs(), 1e-8 + 1e-5 * last.abs()
    must = (lhs <= thr * (1 - 2.0 ** -20)).all(dim=3).all(dim=1)             # [bs, num_iter]
    may = (lhs <= thr * (1 + 2.0 ** -20)).all(dim=3).all(dim=1)
    word = lambda bits: sum(1 << i for i, on in enumerate(bits.tolist()) if on)
    return [word(r) for r in must], [word(r) for r in may]
