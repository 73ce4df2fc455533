"""The routes into pdsc_forward (include/pointdsc_hip.h: one call struct for the testing forward -- uniform, ragged, on two streams
--, the validation forward and the range probe) compute, bit for bit, what the five entry points they replaced computed:
tests/golden/forward_routes.json holds the sha256 of every output of every route, written by tools/record_forward_routes.py from
the library of the commit BEFORE the entry points became one (the recorder uses the module's public API only, so it ran there
unchanged).  And the one argument rule of the call that needs the HIP runtime: range_report must be pinned, device-mapped host memory.
bs = 2, N = 320 (10 key tiles, 32 seeds, k = 40) and 288."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("record_forward_routes", ROOT / "tools" / "record_forward_routes.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_route_reproduces_the_recorded_digests():
    rec = _recorder()
    want = json.loads(rec.GOLDEN.read_text())
    # the ragged case is ONE library call over both pairs, not one call per pair
    assert rec.make_model()._ragged_groups(list(rec.SIZES)) == [[0, 1]]
    got = rec.record()
    assert sorted(got) == sorted(want) and len(want) == 14
    assert got == want, sorted(k for k in want if got[k] != want[k])


def test_range_report_in_device_memory_is_rejected_before_any_launch():
    """A testing forward whose range_report points at ordinary device memory returns PDSC_ERR_ARG and has enqueued nothing: the
    pre-filled outputs are untouched once the stream has drained.  The module's own call on the same inputs (range_guard = "sync",
    which hands the library a pinned buffer) still returns what it returned before."""
    from pointdsc_amd import _lib
    rec = _recorder()
    lib = _lib.load()
    model = rec.make_model()
    uniform, _ = rec.make_inputs()
    data = dict(uniform, testing=True)
    with torch.no_grad():
        plain = model(data)
    assert model.range_guard == "sync" and model._report_ok
    bs, n = uniform["corr_pos"].shape[:2]
    cfg, S = model._config(), int(n * model.ratio)
    ws = torch.empty(int(lib.pdsc_workspace_bytes(C.byref(cfg), bs, n, S)), dtype=torch.uint8, device="cuda:0")
    trans, labels = torch.full((bs, 4, 4), 7.0, device="cuda:0"), torch.full((bs, n), 7.0, device="cuda:0")
    words = torch.zeros(bs, dtype=torch.int32, device="cuda:0")
    call = model._forward_call(cfg, model.packed_weights(), model.split_weights(), tuple(uniform[k] for k in rec.KEYS), bs, n, S, ws)
    call.mode, call.final_trans, call.final_labels = _lib.FORWARD_TESTING, trans.data_ptr(), labels.data_ptr()
    call.range_report = words.data_ptr()
    torch.cuda.synchronize()
    rc = lib.pdsc_forward(C.byref(call), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG and "pdsc_forward(testing): range_report" in _lib.last_error() and "not pinned" in _lib.last_error()
    torch.cuda.current_stream().synchronize()
    assert bool((trans == 7.0).all()) and bool((labels == 7.0).all()) and int(words.abs().sum()) == 0
    with torch.no_grad():
        again = model(data)
    assert model._report_ok and model.range_fallbacks == 0
    assert torch.equal(again["final_trans"], plain["final_trans"]) and torch.equal(again["final_labels"], plain["final_labels"])
    # and the same call without the report buffer is accepted and gives the module's result
    call.range_report = None
    assert lib.pdsc_forward(C.byref(call), torch.cuda.current_stream().cuda_stream) == 0, _lib.last_error()
    torch.cuda.current_stream().synchronize()
    assert torch.equal(trans, plain["final_trans"]) and torch.equal(labels, plain["final_labels"])
