#!/usr/bin/env python3
"""sha256 of every input and output tensor of the train path's kernels (pointwise_train.hip, linear_train.hip, train_tile.h) on the
oracle cases: what a change that must not move a bit is held to.

    python tools/train_kernel_bits.py [--m 2 65 258 16451] [--json FILE]
    POINTDSC_HIP_LIB=<another build> python tools/train_kernel_bits.py        # the same table from that library

One line per tensor: ``M<rows> <case> <pass> <tensor> <in|out> <sha256 of its raw bytes>``.  Inputs come from the fixed-seed CPU
generators of tests/pointwise_train_oracle.py (seed 7, as the large cases of tests/test_pointwise_train.py) and
tests/linear_train_oracle.py.  Cases: conv + BN + ReLU at (Cin, Cout) = (128,128), (128,64), (64,64); linear at Cin = 6, 16 and 64
with the residual; q|k|v; the head with its pre-activations.  Every backward runs in its three compiled forms (dX and parameters,
dX only, parameters only); the running statistics are hashed before and after the forward.  tests/test_train_kernel_bits.py
compares `table(m)` with tests/golden/train_kernel_bits.json."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SIZES = (2, 65, 258, 16451)
POINTWISE_SEED = 7
LINEAR_SHAPES = ((6, False), (16, False), (64, True))
FORMS = (("all", True, True), ("dx_only", True, False), ("params_only", False, True))      # (name, dX, parameters)
DEV = "cuda:0"


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def inputs(m: int) -> dict:
    """{case: its fp32 CPU tensors} for M = m rows."""
    import linear_train_oracle as LO
    import pointwise_train_oracle as PO
    cases = {f"pointwise_{cin}x{cout}": PO.make_case(m, cin, cout, POINTWISE_SEED) for cin, cout in PO.SHAPES}
    cases.update({f"linear_{cin}{'_residual' if residual else ''}": LO.linear_case(m, cin, residual) for cin, residual in LINEAR_SHAPES})
    cases["qkv"], cases["head"] = LO.qkv_case(m), LO.head_case(m)
    return cases


def input_hashes(m: int) -> dict:
    return {f"{case} forward {name} in": sha(t) for case, c in inputs(m).items() for name, t in c.items()}


def table(m: int) -> dict:
    """{"<case> <pass> <tensor> <in|out>": sha256} for M = m rows: the inputs, then the outputs in the order they are made."""
    import linear_train_oracle as LO
    import pointwise_train_oracle as PO
    from pointdsc_amd import ops
    cases, out = inputs(m), input_hashes(m)

    def note(case, step, kind, tensors):
        for name, t in tensors.items():
            if t is not None:
                out[f"{case} {step} {name} {kind}"] = sha(t)

    for cin, cout in PO.SHAPES:
        case = f"pointwise_{cin}x{cout}"
        d = PO.to(cases[case], device=DEV)
        z, y, mean, invstd = ops.pointwise_train_forward(d["x"], d["w"], d["b"], d["gamma"], d["beta"], d["running_mean"], d["running_var"],
                                                         PO.MOMENTUM, PO.EPS)
        note(case, "forward", "out", {"z": z, "y": y, "mean": mean, "invstd": invstd, "running_mean": d["running_mean"],
                                      "running_var": d["running_var"]})
        for form, dx, par in FORMS:
            g = ops.pointwise_train_backward(d["x"], d["w"], d["gamma"], d["beta"], y, mean, invstd, d["dz"], dx, par, par, par, par)
            note(case, "backward_" + form, "out", dict(zip(("dx", "dw", "db", "dgamma", "dbeta"), g)))

    for cin, residual in LINEAR_SHAPES:
        case = f"linear_{cin}{'_residual' if residual else ''}"
        d = LO.to(cases[case], device=DEV)
        note(case, "forward", "out", {"y": ops.linear_train_forward(d["x"], d["w"], d["b"], d.get("r"))})
        for form, dx, par in FORMS:
            note(case, "backward_" + form, "out", dict(zip(("dx", "dw", "db"), ops.linear_train_backward(d["x"], d["w"], d["dy"], dx, par, par))))

    d = LO.to(cases["qkv"], device=DEV)
    note("qkv", "forward", "out", {"qkv": ops.qkv_train_forward(d["x"], d["wq"], d["bq"], d["wk"], d["bk"], d["wv"], d["bv"], LO.Q_SCALE)})
    for form, dx, par in FORMS:
        g = ops.qkv_train_backward(d["x"], d["wq"], d["wk"], d["wv"], LO.Q_SCALE, d["dqkv"], (dx,) + (par,) * 6)
        note("qkv", "backward_" + form, "out", dict(zip(LO.QKV_TENSORS[1:], g)))

    d = LO.to(cases["head"], device=DEV)
    logits, pre = ops.head_train_forward(d["feat"], *(d[k] for k in LO.HEAD_PARAMS), want_pre=True)
    note("head", "forward", "out", {"logits": logits, "pre": pre})
    for form, dx, par in FORMS:
        g = ops.head_train_backward(d["feat"], *(d[k] for k in LO.HEAD_PARAMS[:5]), d["dl"], (dx,) + (par,) * 6)
        note("head", "backward_" + form, "out", dict(zip(LO.HEAD_TENSORS[1:], g)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--json", default=None, help="also write {M: table} to this file")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "train_kernel_bits needs the GPU"
    tables = {}
    for m in a.m:
        tables[str(m)] = table(m)
        for key, digest in tables[str(m)].items():
            print(f"M{m} {key} {digest}")
    if a.json:
        Path(a.json).write_text(json.dumps(tables, indent=0, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
