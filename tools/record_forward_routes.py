#!/usr/bin/env python3
"""Record tests/golden/forward_routes.json: the sha256 of every output of every route into the library's whole-path call -- uniform
and ragged testing forward, validation forward, both testing batches through pipeline.InFlight on two streams, and the range probe
-- from the library as it is built now, on the GPU.  Only the module's public API is used, so the same file runs on any commit: run
it on the commit whose results are the reference (the parent of a refactor), never to make a failing tests/test_forward_routes.py
pass.

    python tools/record_forward_routes.py [--out tests/golden/forward_routes.json]
"""
import argparse
import hashlib
import json
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from pointdsc_amd import PointDSC, synthetic  # noqa: E402
from pointdsc_amd.pipeline import InFlight  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "forward_routes.json"
SIZES = (320, 288)          # 10 and 9 key tiles, 32 and 28 seeds, k = 40: one ragged launch (PointDSC._ragged_groups)
KEYS = ("corr_pos", "src_keypts", "tgt_keypts")


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_model(device="cuda:0") -> PointDSC:
    model = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10, sigma_d=0.10,
                     k=40, nms_radius=0.10)
    model.load_state_dict(synthetic.make_state_dict(model.state_dict(), seed=6))
    return model.eval().to(device)


def make_inputs(device="cuda:0"):
    """(uniform, ragged): two pairs of SIZES[0] correspondences as one tensor batch; the first of them and a pair of SIZES[1] as lists."""
    a, b, short = (synthetic.make_pair(n, inlier_ratio=0.3, seed=s) for n, s in ((SIZES[0], 41), (SIZES[0], 42), (SIZES[1], 43)))
    uniform = {k: torch.cat([a[k], b[k]], 0).to(device) for k in KEYS}
    ragged = {k: [a[k][0].to(device), short[k][0].to(device)] for k in KEYS}
    return uniform, ragged


def record(device="cuda:0") -> dict:
    model = make_model(device)
    uniform, ragged = make_inputs(device)
    out = {}

    def put(route, res, names=("final_trans", "final_labels")):
        for name in names:
            ts = res[name] if isinstance(res[name], (list, tuple)) else [res[name]]
            for i, t in enumerate(ts):
                out[f"{route}/{name}" + (f"[{i}]" if len(ts) > 1 else "")] = _sha(t)

    with torch.no_grad():
        first = model(dict(uniform, testing=True))
        assert bool(torch.isfinite(first["final_trans"]).all()) and float(first["final_labels"].sum(1).min()) >= 32, "a registration, not a degenerate case"
        put("uniform", first)
        probe = model.last_range_probe          # taken by the first forward after the weights were packed
        out["probe/absmax"] = hashlib.sha256(b"".join(struct.pack("<d", probe[k]) for k in model.RANGE_KINDS)).hexdigest()
        put("ragged", model(dict(ragged, testing=True)))
        put("validation", model(dict(uniform)), ("final_trans", "final_labels", "M"))
        runner = InFlight(model, depth=2, tail_streams=True, graphs=False)
        res = [runner(dict(uniform, testing=True)), runner(dict(ragged, testing=True))]
        runner.synchronize()
        put("inflight uniform", res[0])
        put("inflight ragged", res[1])
        runner.close()
    torch.cuda.synchronize()
    assert model.range_fallbacks == 0 and model.attention_precision == "fp16x3" and model.layer_gemm == "h3", "the default arithmetic must have run"
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=Path, default=GOLDEN)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "recording needs the GPU"
    out = record()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for k, v in sorted(out.items()):
        print(f"{k}: {v[:16]}")
    print(f"{args.out}: {len(out)} digests")


if __name__ == "__main__":
    main()
