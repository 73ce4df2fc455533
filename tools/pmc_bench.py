#!/usr/bin/env python3
"""Per-stage time, clique size, proof status and nodes expanded of the PMC baseline (pointdsc_amd.baselines.PMC, csrc/pmc.hip).

    python tools/pmc_bench.py [--max-nodes K] [--reps 3] [--json] [--lds-words W] [--instances [NAME ...]]

Cases: the four fixtures of tests/test_pmc.py, make_pair(5000, inlier_ratio=0.1, seed=0), and the hard instance
make_pair(1000, inlier_ratio=0.5, seed=5) (500 inliers whose subgraph is ~90 % dense: a CPU branch and bound does not finish it in
ten minutes), all at threshold 0.10 and the default budget unless --max-nodes is given.  Stage times are event times on the stream
(pdsc_pmc_baseline_stages): adjacency | ordering, greedy cliques and bound | search | labels and Procrustes; the fastest of --reps
calls after one warm-up call is printed.

--instances runs the search instances of tests/pmc_oracle.py (RECIPES: dense "ball" graphs and noisy inlier sets whose greedy clique
is not a maximum clique) in place of the cases above, all of them or the named ones; --lds-words W restricts the LDS pool of the first
search pass (pdsc_pmc_baseline_ex), which moves roots to the slab pass.  profiles/f10_pmc_search_instances.txt is
    --instances --max-nodes 4194304,  the same with --lds-words 1 | 128 | 256 | 384 on B3 B4 B5,  and
    --instances B2 B4 B5 Z2 --max-nodes 1 | 8 | 64 | 512 | 4096.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import baselines, synthetic  # noqa: E402

CASES = [(70, 0.3, 1), (257, 0.2, 2), (600, 0.2, 3), (1000, 0.1, 4), (5000, 0.1, 0), (1000, 0.5, 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-nodes", type=int, default=baselines.PMC_DEFAULT_MAX_NODES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--lds-words", type=int, default=0, help="words of the LDS pool for the first search pass (0 = all 6144)")
    ap.add_argument("--instances", nargs="*", default=None, metavar="NAME", help="the instances of tests/pmc_oracle.py (none named = all)")
    a = ap.parse_args()
    if a.instances is None:
        cases = [(f"{n}", dict(num_corr=n, inlier_ratio=ratio, seed=seed)) for n, ratio, seed in CASES]
    else:
        sys.path.insert(0, str(ROOT / "tests"))
        import pmc_oracle
        cases = [(name, pmc_oracle.RECIPES[name]) for name in (a.instances or pmc_oracle.RECIPES)]
    rows = []
    for name, recipe in cases:
        p = synthetic.make_pair(**recipe)
        n, ratio, seed = recipe["num_corr"], recipe["inlier_ratio"], recipe["seed"]
        args = (p["corr_pos"].cuda(), p["src_keypts"].cuda(), p["tgt_keypts"].cuda(), 0.10, a.max_nodes)
        baselines.pmc_run(*args, lds_words=a.lds_words)           # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        best = None
        for _ in range(max(1, a.reps)):
            r = baselines.pmc_run(*args, stages=True, lds_words=a.lds_words)
            if best is None or sum(r["stage_ms"]) < sum(best["stage_ms"]):
                best = r
        cnt = best["counters"][0].tolist()
        inl = int((best["pred_labels"][0].cpu() * p["gt_labels"][0]).sum())
        rows.append({"name": name, "N": n, "inlier_ratio": ratio, "seed": seed, "max_nodes": a.max_nodes, "lds_words": a.lds_words or 6144,
                     "stage_ms": [round(x, 4) for x in best["stage_ms"]],
                     "total_ms": round(sum(best["stage_ms"]), 4), "clique_size": int(best["clique_size"][0]), "proven": int(best["proven"][0]),
                     "nodes": cnt[0], "roots_branched": cnt[1], "roots_not_exhausted": cnt[2], "greedy_bound": cnt[3],
                     "true_inliers_in_clique": inl})
    if a.json:
        print(json.dumps(rows))
        return
    print(f"max_nodes {a.max_nodes} per root, LDS pool {a.lds_words or 6144} words; times in ms (fastest of {a.reps})")
    print(f"{'name':>5s} {'N':>5s} {'ratio':>5s} {'seed':>4s} {'adjacency':>9s} {'order+bnd':>9s} {'search':>9s} {'procrust':>9s} {'total':>9s} "
          f"{'clique':>6s} {'proven':>6s} {'greedy':>6s} {'nodes':>10s} {'roots':>6s} {'open':>5s}")
    for r in rows:
        s = r["stage_ms"]
        print(f"{r['name']:>5s} {r['N']:5d} {r['inlier_ratio']:5.2f} {r['seed']:4d} {s[0]:9.3f} {s[1]:9.3f} {s[2]:9.3f} {s[3]:9.3f} {r['total_ms']:9.3f} "
              f"{r['clique_size']:6d} {r['proven']:6d} {r['greedy_bound']:6d} {r['nodes']:10d} {r['roots_branched']:6d} {r['roots_not_exhausted']:5d}")


if __name__ == "__main__":
    main()
