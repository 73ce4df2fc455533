#!/usr/bin/env python3
"""Times pdsc_layer_run alone on fragment streams (merge of the attention partials + tail + head, the forward's output set) at the
bench's size, interleaving variants given as ENV=value lists inside one process.

    python tools/layer_bench.py --bs 32 --variants PDSC_LAYER_GEMM=0 PDSC_LAYER_GEMM=1 PDSC_LAYER_GEMM=1,PDSC_LAYER_H3_EXP=2
"""
import argparse
import ctypes as C
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import os as _os
_os.environ.setdefault("POINTDSC_HIP_LIB", str(__import__("pathlib").Path(__file__).resolve().parents[1] / "pointdsc_amd" / "libpointdsc_hip_exp.so"))   # PDSC_* knobs / traces: experiments library (python -m pointdsc_amd.build --experiments)
from pointdsc_amd import _lib, ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=5000)
ap.add_argument("--bs", type=int, default=32)
ap.add_argument("--variants", nargs="+", default=["PDSC_LAYER_GEMM=0", "PDSC_LAYER_GEMM=1"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--pf", action="store_true", help="hand-offs in point-fragment order (pdsc_layer_call.io_flags, H3 only)")
a = ap.parse_args()
lib = _lib.load()
n, bs, dev = a.n, a.bs, "cuda:0"
gen = torch.Generator().manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)  # noqa: E731
m = n * bs
batch = synthetic.make_batch(bs, n, seed=1)
compat = ops.spatial_compat(batch["src_keypts"].to(dev), batch["tgt_keypts"].to(dev), torch.tensor([0.1], device=dev))
qs, kv = ops.pack_qkv_split(rnd(m, 384) * 0.3, bs, n)
scratch, nsplit = ops.sc_attention_split(qs, kv, compat, bs, n, merge=False, layout="pf" if a.pf else "rows")
del compat
npad = (n + 255) // 256 * 256
res = rnd(m, 128)
tail_w = [rnd(64, 128) / 11, rnd(64), rnd(64, 64) / 8, rnd(64), rnd(128, 64) / 8, rnd(128)]
head_w = [rnd(128, 128) / 11, rnd(128), rnd(384, 128) / 11, rnd(384)]
streams = {g: (ops.frag_weights_tail(tail_w, g), ops.frag_weights_head(head_w, g)) for g in ("f32", "h3")}
featB = torch.empty(bs * ops.pf_rows(n), 128, device=dev)
if a.pf:
    res = ops.rows_to_pf(res, bs, n)
part_o = scratch.data_ptr()
base = dict(part_o=part_o, part_ml=part_o + bs * nsplit * npad * 128 * 4, nsplit=nsplit, Npad=npad, res=res.data_ptr(),
            featB_out=featB.data_ptr(), q_split=qs.data_ptr(), kv_tiles=kv.data_ptr(), io_flags=7 if a.pf else 0, bs=bs, N=n)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call():
    gemm = int(os.environ.get("PDSC_LAYER_GEMM", "0"))
    wt, wh = streams["h3" if gemm else "f32"]
    c = _lib.PdscLayerCall(wfrag_tail=wt.data_ptr(), wfrag_head=wh.data_ptr(), gemm_format=gemm, **base)
    _lib.check(lib.pdsc_layer_run(C.byref(c), stream), "pdsc_layer_run")


def apply(v):
    for kvp in v.split(","):
        k, val = kvp.split("=")
        os.environ[k] = val


times = {v: [] for v in a.variants}
for v in a.variants:
    apply(v)
    for _ in range(3):
        call()
torch.cuda.synchronize()
for _ in range(a.rounds):
    for v in a.variants:
        apply(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        times[v].append(e0.elapsed_time(e1) / a.calls * 1e3)
for v in a.variants:
    print(f"N={n} bs={bs} nsplit={nsplit}  {v:60s} median {statistics.median(times[v]):7.1f} us  min {min(times[v]):7.1f}")
