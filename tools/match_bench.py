#!/usr/bin/env python3
"""Timing of the correspondence construction (csrc/match.hip) at the sizes of the hot path's inputs.

--batch P: P pairs of the first shape (N = 5000, D = 32) through ONE build_correspondences_batch call (csrc/match_batch.hip, f-19)
beside the same pairs through build_correspondences in a loop, alternating the two: medians and min .. max over --rounds rounds,
each round ending in a device synchronise (host clock: what a caller waits for, launches and host plumbing included).
--loop-only times the per-pair loop alone (for a library that has no batched entry)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pointdsc_amd import correspondences  # noqa: E402


def unit(rs, n, d):
    a = rs.randn(n, d).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def batch(p, rounds, loop_only, n=5000, d=32, dev="cuda:0"):
    rs = np.random.RandomState(0)
    desc = [torch.from_numpy(unit(rs, n, d)).to(dev) for _ in range(2 * p)]
    kp = [torch.rand(n, 3, device=dev) for _ in range(2 * p)]
    pairs = [(2 * i, 2 * i + 1) for i in range(p)]

    def loop(mutual):
        for s, t in pairs:
            correspondences.build_correspondences(desc[s], desc[t], kp[s], kp[t], use_mutual=mutual)

    def batched(mutual):
        correspondences.build_correspondences_batch(pool, None, pairs, use_mutual=mutual)

    def timed(fn, mutual):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(mutual)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pool = None if loop_only else correspondences.CorrPool(desc, kp)
    for mutual in (False, True):
        names = ["loop"] if loop_only else ["loop", "batch"]
        fns = {"loop": loop, "batch": batched}
        for nm in names:
            for _ in range(3):
                timed(fns[nm], mutual)
        ms = {nm: [] for nm in names}
        for _ in range(rounds):
            for nm in names:
                ms[nm].append(timed(fns[nm], mutual))
        line = f"batch P={p} N={n} D={d} mutual={mutual}:"
        for nm in names:
            v = np.array(ms[nm])
            line += f"  {nm} median {np.median(v):8.3f} ms (min {v.min():8.3f} max {v.max():8.3f}, {rounds} rounds)"
        if not loop_only:
            line += f"  batch / loop = {np.median(ms['batch']) / np.median(ms['loop']):.3f}"
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0, help="time P pairs through one batched call beside the per-pair loop")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--loop-only", action="store_true", help="with --batch: the per-pair loop alone")
    a = ap.parse_args()
    if a.batch > 0:
        return batch(a.batch, a.rounds, a.loop_only)
    dev = "cuda:0"
    for n, d in ((5000, 32), (5000, 33), (10000, 32), (20000, 32)):
        rs = np.random.RandomState(0)
        a = rs.randn(n, d).astype(np.float32); a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = rs.randn(n, d).astype(np.float32); b /= np.linalg.norm(b, axis=1, keepdims=True)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        kp = torch.rand(n, 3, device=dev)
        for mutual in (False, True):
            for _ in range(3):
                correspondences.build_correspondences(ta, tb, kp, kp, use_mutual=mutual)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                correspondences.build_correspondences(ta, tb, kp, kp, use_mutual=mutual)
            e1.record()
            torch.cuda.synchronize()
            gpu_us = e0.elapsed_time(e1) / 20 * 1e3
            # one call at a time, waited for (what a per-pair evaluation loop sees: launch count matters here, not in the back-to-back loops)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                correspondences.build_correspondences(ta, tb, kp, kp, use_mutual=mutual)
                torch.cuda.synchronize()
            lat_us = (time.perf_counter() - t0) / 50 * 1e6
            t0 = time.perf_counter()
            dist = np.sqrt(2 - 2 * (a @ b.T) + 1e-6)
            idx = np.argmin(dist, axis=1)
            if mutual:
                np.argmin(dist, axis=0)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            flops = 2.0 * n * n * d * (2 if mutual else 1)
            print(f"N={n} D={d} mutual={mutual}: GPU {gpu_us:8.1f} us ({flops / gpu_us / 1e6:6.2f} TFLOP/s; one call at a time, waited for: {lat_us:7.1f} us)   numpy on the host {cpu_ms:8.1f} ms")


if __name__ == "__main__":
    main()
