"""The train path's kernels give the bits that were recorded before they were rewritten on one shared tile (train_tile.h; DESIGN.md
section 8 f-17): tools/train_kernel_bits.py's table of sha256 digests -- every input and output tensor of the conv + BN + ReLU, linear,
q|k|v and head cases, each backward in its three compiled forms -- against tests/golden/train_kernel_bits.json, which was recorded
from the library of the commit before the rewrite.  M = 2 (the fewest rows batch statistics take), 65 (a full tile and one row), 258
(the other tests' size), 16451 (258 tiles: a persistent workgroup walks two, the merge adds 256 partials).

The inputs come from torch's CPU generator; if THEIR digests differ the kernels are not to blame and the failure says so."""
import json
import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, str(ROOT / "tools"))
import train_kernel_bits as TB  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "train_kernel_bits.json").read_text())
INPUTS_DIFFER = "the INPUTS differ from the recorded ones (torch's CPU generator), not the kernels: "


def test_fixture_covers_the_cases_and_the_inputs_are_the_recorded_ones():
    assert sorted(GOLDEN, key=int) == [str(m) for m in TB.SIZES]
    for m in TB.SIZES:
        rec = GOLDEN[str(m)]
        assert all(len(v) == 64 for v in rec.values())
        cases = {k.split()[0] for k in rec}
        assert cases == {"pointwise_128x128", "pointwise_128x64", "pointwise_64x64", "linear_6", "linear_16", "linear_64_residual",
                         "qkv", "head"}
        for case in cases:
            steps = {k.split()[1] for k in rec if k.split()[0] == case}
            assert steps == {"forward"} | {"backward_" + f[0] for f in TB.FORMS}, case
        for before in ("running_mean in", "running_var in"):
            assert f"pointwise_64x64 forward {before}" in rec and f"pointwise_64x64 forward {before[:-2]}out" in rec
        got = TB.input_hashes(m)
        bad = [k for k in got if rec.get(k) != got[k]]
        assert not bad and len(got) == len([k for k in rec if k.endswith(" in")]), INPUTS_DIFFER + f"M={m} {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("m", TB.SIZES)
def test_bits_equal_the_recorded_table(m):
    rec, got = GOLDEN[str(m)], TB.table(m)
    bad_inputs = [k for k in rec if k.endswith(" in") and got.get(k) != rec[k]]
    assert not bad_inputs, INPUTS_DIFFER + str(bad_inputs)
    assert sorted(got) == sorted(rec)
    bad = [k for k in rec if got[k] != rec[k]]
    print(f"M={m}: {len(rec)} tensors, {len(bad)} differ")
    assert not bad, f"M={m}: these tensors' bits differ from the recorded ones: {bad}"
