#!/usr/bin/env python3
"""Per-stage device time of the FPFH path (pointdsc_amd.features, csrc/fpfh.hip).

    python tools/fpfh_bench.py [--clouds 1 32] [--steps 20] [--warmup 3] [--json]

Cases: 1 and 32 clouds of the demo fixture (tests/golden/demo_clouds_vox005.npz, cloud_bin_0 and cloud_bin_1 alternating: a ragged
batch) with the parameters of misc/cal_fpfh.py:21-26 at voxel 0.05.  Every stage is called through its own library entry on
pre-allocated buffers and timed with device events (median over --steps); "whole" is one pdsc_fpfh call.

    python tools/fpfh_bench.py --raw [--clouds 1 4] [--copies 48] [--repeats 3] [--json]

The demo's recipe from RAW clouds, stage by stage, with the one-workgroup kernels (path 1) and the
many-workgroups kernels (path 2) in front of the descriptor.  The raw demo clouds are not in the repository, so the cloud is
SYNTHETIC: --copies (48) seeded copies of every point of cloud_bin_0 of the fixture, each jittered uniformly within a voxel-sized cube
around it -- about 256 k points with the raw cloud's DENSITY but not its SURFACE (the real scan is a thin sheet on a regular grid; here
a voxel is filled in depth, which if anything raises the search's candidate count).  Every figure is the median of --steps; the
measurement is repeated --repeats times and the lowest and highest median are printed (their difference is the run-to-run spread).
"baseline" is what --pcd1 / --pcd2 cost before f-9: harness.voxel_down_sample on the host (wall clock) plus device_fpfh.
"""
import argparse
import ctypes as C
import json
import sys
import time
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


def synthetic_raw(copies, seed):
    base = np.load(ROOT / "tests" / "golden" / "demo_clouds_vox005.npz")["cloud_bin_0"].astype(np.float64)
    rs = np.random.RandomState(seed)
    pts = base[:, None, :] + rs.uniform(-0.5 * VOXEL, 0.5 * VOXEL, (len(base), copies, 3))
    return np.ascontiguousarray(rs.permutation(pts.reshape(-1, 3)), dtype=np.float32)


def bench_raw(bs, copies, path, steps, warmup, repeats):
    """Per-stage medians (lowest, highest over `repeats`) of the demo's recipe on bs synthetic raw clouds with path 1 or 2."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    clouds = [synthetic_raw(copies, 100 + i) for i in range(bs)]
    n = len(clouds[0])
    pts = torch.stack([torch.from_numpy(c) for c in clouds]).to(dev)
    rn, kn, rf, kf = F.NORMAL_RADIUS_VOXELS * VOXEL, F.NORMAL_MAX_NN, F.FEATURE_RADIUS_VOXELS * VOXEL, F.FEATURE_MAX_NN
    new = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def ok(rc):
        if rc != 0:
            raise RuntimeError(_lib.last_error())

    idx_n, cnt_n, normals = new(bs, n, kn, dtype=torch.int32), new(bs, n, dtype=torch.int32), new(bs, n, 3)
    ws_nb = new(int(lib.pdsc_hybrid_neighbours_workspace_bytes(bs, n)), dtype=torch.uint8)
    ws_v = new(int(lib.pdsc_cloud_voxel_workspace_bytes(bs, n)), dtype=torch.uint8)
    keys = new(bs, n, dtype=torch.int64)
    state = {}

    def sort():
        sk, pm = torch.sort(keys, dim=1, stable=True)
        state["sk"], state["pm"] = sk.contiguous(), pm.contiguous()

    ok(lib.pdsc_cloud_voxel_keys(p(pts), None, VOXEL, p(keys), p(ws_v), ws_v.numel(), bs, n, path, st))
    sort()
    heads = (state["sk"][:, 1:] != state["sk"][:, :-1]).sum(dim=1) + 1
    cap = int(heads.max().item())
    dpts, dnrm, dcnt = new(bs, cap, 3, dtype=torch.float32), new(bs, cap, 3), new(bs, dtype=torch.int32)
    idx_f, d2_f, cnt_f = new(bs, cap, kf, dtype=torch.int32), new(bs, cap, kf), new(bs, cap, dtype=torch.int32)
    spfh, fpfh, desc = new(bs, cap, 33), new(bs, cap, 33), new(bs, cap, 33, dtype=torch.float32)
    ws_f = new(int(lib.pdsc_hybrid_neighbours_workspace_bytes(bs, cap)), dtype=torch.uint8)
    stages = {
        "neighbours_raw_r0.10_k30": lambda: ok(lib.pdsc_cloud_neighbours(p(pts), None, rn, kn, p(idx_n), None, p(cnt_n), p(ws_nb),
                                                                         ws_nb.numel(), bs, n, path, st)),
        "normals_raw": lambda: ok(lib.pdsc_estimate_normals(p(pts), None, p(idx_n), p(cnt_n), kn, None, p(normals), bs, n, st)),
        "voxel_keys": lambda: ok(lib.pdsc_cloud_voxel_keys(p(pts), None, VOXEL, p(keys), p(ws_v), ws_v.numel(), bs, n, path, st)),
        "torch_sort": sort,
        "voxel_means": lambda: ok(lib.pdsc_cloud_voxel_means(p(pts), p(normals), p(state["sk"]), p(state["pm"]), p(dpts), p(dnrm), p(dcnt),
                                                             cap, 0, p(ws_v), ws_v.numel(), bs, n, path, st)),
        "neighbours_down_r0.25_k100": lambda: ok(lib.pdsc_cloud_neighbours(p(dpts), p(dcnt), rf, kf, p(idx_f), p(d2_f), p(cnt_f), p(ws_f),
                                                                           ws_f.numel(), bs, cap, path, st)),
        "spfh": lambda: ok(lib.pdsc_spfh(p(dpts), p(dcnt), p(dnrm), p(idx_f), p(cnt_f), kf, p(spfh), bs, cap, st)),
        "fpfh": lambda: ok(lib.pdsc_fpfh_from_spfh(p(spfh), p(dcnt), p(idx_f), p(d2_f), p(cnt_f), kf, p(fpfh), p(desc), bs, cap, st)),
        "extract_fpfh_features": lambda: F.extract_fpfh_features(pts, VOXEL, capacity=cap, path={1: "one", 2: "many"}[path]),
    }
    row = {"clouds": bs, "points_per_cloud": n, "voxels": cap, "path": path}
    for k, fn in stages.items():
        med = [timed(fn, steps, warmup) for _ in range(repeats)]
        row[k + "_us"] = [min(med), max(med)]
    return row


def bench_raw_baseline(copies, steps, warmup):
    """What a raw cloud cost before f-9: the host's voxel_down_sample (wall clock, one cloud) and device_fpfh on its result."""
    from pointdsc_amd import harness
    raw = synthetic_raw(copies, 100)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        down = harness.voxel_down_sample(raw, VOXEL)
        host.append((time.perf_counter() - t0) * 1e6)
    return {"points_per_cloud": len(raw), "voxels": len(down), "host_voxel_down_sample_us": float(np.median(host)),
            "device_fpfh_us": timed(lambda: harness.device_fpfh(down, VOXEL), steps, warmup)}


def main_raw(a):
    clouds = a.clouds or [1, 4]
    out = {"baseline": [bench_raw_baseline(c, a.steps, a.warmup) for c in a.copies],
           "rows": [bench_raw(bs, c, path, a.steps, a.warmup, a.repeats) for c in a.copies for bs in clouds for path in (1, 2)]}
    if a.json:
        print(json.dumps(out))
        return
    for r in out["baseline"]:
        print(f"baseline, 1 synthetic cloud of {r['points_per_cloud']} points -> {r['voxels']} voxels: host voxel_down_sample "
              f"{r['host_voxel_down_sample_us']:.0f} us (wall clock)  device_fpfh {r['device_fpfh_us']:.0f} us")
    for r in out["rows"]:
        print(f"{r['clouds']} synthetic clouds of {r['points_per_cloud']} points -> {r['voxels']} voxels, path {r['path']}: "
              + "  ".join(f"{k[:-3]} {v[0]:.0f}..{v[1]:.0f} us" for k, v in r.items() if k.endswith("_us")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=None, help="default: 1 32 (with --raw: 1 4)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--raw", action="store_true", help="the demo's recipe from synthetic raw clouds, paths 1 and 2 (f-9)")
    ap.add_argument("--copies", type=int, nargs="+", default=[48], help="--raw: copies of every fixture point (48: about 256 k points)")
    ap.add_argument("--repeats", type=int, default=3, help="--raw: repetitions of every median (their range is the spread)")
    a = ap.parse_args()
    if a.raw:
        return main_raw(a)
    rows = [bench(bs, a.steps, a.warmup) for bs in (a.clouds or [1, 32])]
    if a.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['clouds']} clouds, {r['points']} points: " + "  ".join(f"{k[:-3]} {v:.0f} us" for k, v in r.items() if k.endswith("_us")))


if __name__ == "__main__":
    main()
