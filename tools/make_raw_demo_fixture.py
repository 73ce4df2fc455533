#!/usr/bin/env python3
"""Crops of the RAW demo clouds and the fp64 oracle's results on them (build container only: reads
/root/reference/demo_data/*.ply).

    python tools/make_raw_demo_fixture.py      # writes tests/golden/demo_raw_crop.npz

The demo (demo_registration.py:37-44) estimates normals on the raw clouds (258 342 and 268 977 vertices) before it down-samples them;
DESIGN.md section 8 f-9 does the same on the device.  The raw clouds are far too large for a fixture, so this one holds, per cloud,
the CROP_POINTS raw vertices nearest to the cloud's coordinate-wise median (in file order, fp32: the raw cloud's density on a patch
of its surface) and what the oracle of tests/test_fpfh_raw.py computes from them: the (2 voxel, 30) neighbour lists, the normals,
the down-sampled points and averaged normals (VOXEL_NORMAL_RULE), fpfh and desc.  Data only.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
REFERENCE_DEMO = Path("/root/reference/demo_data")
CROP_POINTS = 6000
NAMES = ("cloud_bin_0", "cloud_bin_1")


def crop(raw: np.ndarray, n: int = CROP_POINTS) -> np.ndarray:
    """The n vertices nearest to the coordinate-wise median (fp64 squared distance, ties by file order), in file order."""
    p = np.asarray(raw, np.float32).astype(np.float64)
    d = p - np.median(p, axis=0)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = np.sort(np.argsort(d2, kind="stable")[:n])
    return np.ascontiguousarray(raw[keep], dtype=np.float32)


def reference_crop(name: str) -> np.ndarray:
    from pointdsc_amd import harness
    return crop(harness.read_ply_xyz(REFERENCE_DEMO / f"{name}.ply"))


def fixture_arrays(name: str, points: np.ndarray, o: dict) -> dict:
    """What the fixture stores of the oracle's result `o` (tests/test_fpfh_raw.raw_oracle) on `points`."""
    assert o["idx_n"].max() < 32768
    return {f"{name}_points": points, f"{name}_idx": o["idx_n"].astype(np.int16), f"{name}_count": o["count_n"].astype(np.int16),
            f"{name}_normals": o["normals"], f"{name}_down_points": o["down_points"], f"{name}_down_normals": o["down_normals"],
            f"{name}_fpfh": o["fpfh"], f"{name}_desc": o["desc"]}


def main():
    from test_fpfh_raw import raw_oracle_of
    out = {}
    for name in NAMES:
        pts = reference_crop(name)
        o = raw_oracle_of(pts)
        print(f"{name}: {len(pts)} raw vertices -> {len(o['down_points'])} occupied voxels; margins "
              + " ".join(f"{k}={v:.2e}" for k, v in o["margins"].items()))
        out.update(fixture_arrays(name, pts, o))
    path = ROOT / "tests" / "golden" / "demo_raw_crop.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
