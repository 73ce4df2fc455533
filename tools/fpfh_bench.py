#!/usr/bin/env python3
"""Per-stage device time of the FPFH path (pointdsc_amd.features, csrc/fpfh.hip).

    python tools/fpfh_bench.py [--clouds 1 32] [--steps 20] [--warmup 3] [--json]

Cases: 1 and 32 clouds of the demo fixture (tests/golden/demo_clouds_vox005.npz, cloud_bin_0 and cloud_bin_1 alternating: a ragged
batch) with the parameters of misc/cal_fpfh.py:21-26 at voxel 0.05.  Every stage is called through its own library entry on
pre-allocated buffers and timed with device events (median over --steps); "whole" is one pdsc_fpfh call.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import _lib  # noqa: E402
from pointdsc_amd import features as F  # noqa: E402

VOXEL = 0.05


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def bench(bs, steps, warmup):
    lib = _lib.load()
    d = np.load(ROOT / "tests" / "golden" / "demo_clouds_vox005.npz")
    clouds = [d["cloud_bin_0"] if i % 2 == 0 else d["cloud_bin_1"] for i in range(bs)]
    n = max(len(c) for c in clouds)
    dev = torch.device("cuda:0")
    pts = torch.zeros(bs, n, 3, device=dev)
    for i, c in enumerate(clouds):
        pts[i, :len(c)] = torch.from_numpy(c).to(dev)
    counts = torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=dev)
    rn, kn, rf, kf = F.NORMAL_RADIUS_VOXELS * VOXEL, F.NORMAL_MAX_NN, F.FEATURE_RADIUS_VOXELS * VOXEL, F.FEATURE_MAX_NN
    new = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)  # noqa: E731
    idx_n, cnt_n = new(bs, n, kn, dtype=torch.int32), new(bs, n, dtype=torch.int32)
    idx_f, d2_f, cnt_f = new(bs, n, kf, dtype=torch.int32), new(bs, n, kf), new(bs, n, dtype=torch.int32)
    normals, spfh, fpfh, desc = new(bs, n, 3), new(bs, n, 33), new(bs, n, 33), new(bs, n, 33, dtype=torch.float32)
    ws_nb = new(int(lib.pdsc_hybrid_neighbours_workspace_bytes(bs, n)), dtype=torch.uint8)
    ws = new(int(lib.pdsc_fpfh_workspace_bytes(bs, n, kn, kf)), dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def ok(rc):
        if rc != 0:
            raise RuntimeError(_lib.last_error())

    stages = {
        "neighbours_r0.10_k30": lambda: ok(lib.pdsc_hybrid_neighbours(p(pts), p(counts), rn, kn, p(idx_n), None, p(cnt_n), p(ws_nb),
                                                                      ws_nb.numel(), bs, n, st)),
        "normals": lambda: ok(lib.pdsc_estimate_normals(p(pts), p(counts), p(idx_n), p(cnt_n), kn, None, p(normals), bs, n, st)),
        "neighbours_r0.25_k100": lambda: ok(lib.pdsc_hybrid_neighbours(p(pts), p(counts), rf, kf, p(idx_f), p(d2_f), p(cnt_f), p(ws_nb),
                                                                       ws_nb.numel(), bs, n, st)),
        "spfh": lambda: ok(lib.pdsc_spfh(p(pts), p(counts), p(normals), p(idx_f), p(cnt_f), kf, p(spfh), bs, n, st)),
        "fpfh": lambda: ok(lib.pdsc_fpfh_from_spfh(p(spfh), p(counts), p(idx_f), p(d2_f), p(cnt_f), kf, p(fpfh), p(desc), bs, n, st)),
        "whole": lambda: ok(lib.pdsc_fpfh(p(pts), p(counts), rn, kn, rf, kf, None, p(fpfh), p(desc), None, p(ws), ws.numel(), bs, n, st)),
    }
    return {"clouds": bs, "points": int(counts.sum()), **{k + "_us": timed(fn, steps, warmup) for k, fn in stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rows = [bench(bs, a.steps, a.warmup) for bs in a.clouds]
    if a.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['clouds']} clouds, {r['points']} points: " + "  ".join(f"{k[:-3]} {v:.0f} us" for k, v in r.items() if k.endswith("_us")))


if __name__ == "__main__":
    main()
