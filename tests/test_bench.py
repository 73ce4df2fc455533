"""bench.py's plain run (the headline only) and --dump-outputs; the legs behind --full are exercised by tests/test_sharding_gloo.py."""
import hashlib
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench_module(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_full_legs_and_dumps_are_opt_in(monkeypatch):
    bench = _bench_module("bench_opts")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "out"


def test_dump_outputs_writes_float32_within_the_cap(tmp_path, monkeypatch):
    """What a caller of the timed path receives, as float32 .npy files; an array over its share of the cap is a seeded sample of
    its rows, the same one every run."""
    bench = _bench_module("bench_dump")
    g = torch.Generator().manual_seed(0)
    res = {"final_trans": torch.randn(6, 4, 4, generator=g), "final_labels": (torch.rand(6, 50, generator=g) > 0.5).float()}
    bench.dump_outputs(tmp_path / "a", res, gathered_trans=torch.randn(12, 4, 4, generator=g))
    for name, want in (("final_trans", res["final_trans"]), ("final_labels", res["final_labels"])):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert np.load(tmp_path / "a" / "gathered_final_trans.npy").shape == (12, 4, 4)
    assert not list((tmp_path / "a").glob("*_rows.npy"))
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 2400)               # 600 B per array: final_labels (6 x 200 B) is sampled
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, res)
    rows = np.load(tmp_path / "b" / "final_labels_rows.npy")
    got = np.load(tmp_path / "b" / "final_labels.npy")
    assert rows.shape == (3,) and got.shape == (3, 50) and np.array_equal(got, res["final_labels"].numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "c" / "final_labels_rows.npy"))
    assert sum(p.stat().st_size for p in (tmp_path / "b").iterdir()) < 2400 + 3 * 128         # (+ the .npy headers)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_its_last_step(tmp_path):
    """`bench.py --steps K` without --full: the headline fields, K timed steps, none of the --full legs, and --dump-outputs holds
    exactly the poses of the last timed step (the line's own fingerprint of them)."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-seconds", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "pairs/s"
    assert abs(line["value"] - line["config"]["global_batch"] * 1e3 / line["ms_per_step"]) < 1e-2 * line["value"]
    for k in ("check", "roofline", "sustained", "single_stream", "extra", "cpu_baseline"):
        assert k not in line, k
    B, N = line["config"]["pairs_per_gpu"], line["config"]["num_corr"]
    trans, labels = np.load(out / "final_trans.npy"), np.load(out / "final_labels.npy")
    assert trans.dtype == np.float32 and trans.shape == (B, 4, 4) and labels.dtype == np.float32 and labels.shape == (B, N)
    assert np.isfinite(trans).all() and set(np.unique(labels).tolist()) <= {0.0, 1.0}
    assert hashlib.sha256(trans.tobytes()).hexdigest()[:16] == line["config"]["gathered_poses_sha256_16"]
