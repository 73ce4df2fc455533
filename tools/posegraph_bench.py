#!/usr/bin/env python3
"""Device time of the pose-graph optimisation (pointdsc_amd.multiway.global_optimization, csrc/posegraph.hip).

    python tools/posegraph_bench.py [--nodes 57] [--graphs 1 4] [--steps 20] [--warmup 3] [--json]

Cases: one graph of --nodes fragments with dense loop closures (a seeded chain of 25 deg / 0.4 m motions, true closures on every
other pair, two gross false ones: 1 596 edges at 57 nodes) and a batch of four such graphs (different seeds).  The one launch of
pdsc_global_optimization on pre-allocated buffers is timed with device events (median over --steps).  The split between assembly
and factorisation comes from the kernel's own clock readings (the optional `ticks` output: constant 100 MHz clock, read by the
graph's workgroup around its residual + assembly phases and around its solves), of the first graph of the batch.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import multiway  # noqa: E402

TICK_US = 0.01          # wall_clock64: 100 MHz


def motion(rs, deg, metres):
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    d = rs.standard_normal(3)
    T[:3, 3] = d / np.linalg.norm(d) * metres
    return T


def dense_graph(F, seed, dev):
    """Every pair is an edge: odometry (1 deg / 1 cm noise, certain), loop closures (0.3 deg / 3 mm, uncertain), two of them gross."""
    rs = np.random.RandomState(seed)
    truth = [np.eye(4)]
    for _ in range(F - 1):
        truth.append(truth[-1] @ motion(rs, 25.0, 0.4))
    pairs = [(s, t) for s in range(F) for t in range(s + 1, F)]
    closures = [i for i, (s, t) in enumerate(pairs) if t > s + 1]
    false = set(rs.choice(closures, min(2, len(closures)), replace=False).tolist())
    X, info = [], []
    for i, (s, t) in enumerate(pairs):
        exact = np.linalg.inv(truth[t]) @ truth[s]
        noise = motion(rs, 1.0, 0.01) if t == s + 1 else (motion(rs, 80.0, 1.0) if i in false else motion(rs, 0.3, 0.003))
        X.append(noise @ exact)
        q = rs.uniform(-1.5, 1.5, (300, 3))
        G = np.zeros((300, 3, 6))
        G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = q[:, 2], -q[:, 1], -q[:, 2], q[:, 0], q[:, 1], -q[:, 0]
        G[:, :, 3:] = np.eye(3)
        info.append(np.einsum("nra,nrb->ab", G, G))
    edges = {"source": torch.tensor([p[0] for p in pairs], dtype=torch.int32).to(dev),
             "target": torch.tensor([p[1] for p in pairs], dtype=torch.int32).to(dev),
             "transformation": torch.from_numpy(np.array(X)).to(dev), "information": torch.from_numpy(np.array(info)).to(dev),
             "uncertain": torch.tensor([t > s + 1 for s, t in pairs]).to(dev)}
    return multiway.pose_graph_nodes(edges, F), edges


def bench(F, graphs, steps, warmup):
    dev = torch.device("cuda:0")
    gs = [dense_graph(F, 100 + i, dev) for i in range(graphs)]
    call = multiway._posegraph_call([g[0] for g in gs], [g[1] for g in gs], None, multiway.EDGE_DISTANCE, 0.25, 20.0, 0, ticks=True)
    for _ in range(warmup):
        multiway._posegraph_launch(call)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        multiway._posegraph_launch(call)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    rec, ticks = call["record"].cpu().numpy(), call["ticks"].cpu().numpy()
    return {"graphs": graphs, "nodes": F, "edges": int(rec[0, 9]), "edges_out": int(rec[0, 11]), "status": int(rec[:, 0].max()),
            "iterations": [int(rec[0, 1]), int(rec[0, 5])], "solves": [int(rec[0, 2]), int(rec[0, 6])],
            "launch_us": float(np.median(times)), "assembly_us": float(ticks[0, 0] * TICK_US), "solve_us": float(ticks[0, 1] * TICK_US),
            "graph_us": float(ticks[0, 2] * TICK_US)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=57)
    ap.add_argument("--graphs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rows = [bench(a.nodes, g, a.steps, a.warmup) for g in a.graphs]
    if a.json:
        print(json.dumps(rows))
        return
    for r in rows:
        s = sum(r["solves"])
        print(f"{r['graphs']} graph(s) of {r['nodes']} nodes, {r['edges']} -> {r['edges_out']} edges, iterations {r['iterations']}, solves "
              f"{r['solves']}: launch {r['launch_us']:.0f} us (median); first graph {r['graph_us']:.0f} us = residuals + assembly "
              f"{r['assembly_us']:.0f} us + {s} solves {r['solve_us']:.0f} us ({r['solve_us'] / max(s, 1):.0f} us each) + rest")


if __name__ == "__main__":
    main()
