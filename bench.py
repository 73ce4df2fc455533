#!/usr/bin/env python3
"""Throughput bench of the PointDSC outlier-rejection hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config NAME]      (N>1: under torch.distributed.run, or plain: it re-executes itself
                                                                        under torch.distributed.run --nproc-per-node N)

Metric (BASELINE.json): point-cloud pairs/sec at N=5000 correspondences.  One "step" = one pass of the whole
hot path (pdsc_forward_testing: compat build, 12 SCNonlocal layers, seeds, per-seed solver, scoring,
refinement) over one batch of synthetic correspondence sets sharded over the GPUs, inputs already resident in
HBM.  Pairs are independent units: every rank processes its own shard and the only collective is the final
all_gather of the poses (RCCL), which is inside the timed region.

--config selects a BASELINE.json configuration (pointdsc_amd/workloads.py); the default n5000_b32 is configs[2], the
one the metric is quoted on (32 pairs at N=5000: 32 / N per GPU = strong scaling; --pairs-per-gpu fixes the
per-GPU batch instead).  n1000_b1, kitti_n5000_b16 and lomatch_n10000_b8 are configs[1], [3], [4].

Rank 0 prints ONE JSON line.  A plain run does only what that line's headline needs: set-up, the W warm-up steps and the
untimed --settle-seconds load, the K timed steps, and the line (metric, value, unit, higher_is_better, dtype, ms_per_step and
the configuration).  --dump-outputs DIR writes what the last timed step returned (rank 0's final_trans and final_labels, plus
the gathered poses with N > 1) as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared output for
output.  With --full the line also carries every leg and figure below (each needs runs of its own):
  roofline        -- the dominant kernel (sc_attention_split_kernel, MFMA-bound: every fp32 product as three f16
                     MFMAs, fp32 accumulate): algorithmic flops per launch / average launch duration measured with
                     hipEvents on the launch stream over the timed region (pdsc_profile_* in include/pointdsc_hip.h);
  roofline_layer, roofline_compat -- the fused point-wise layer launch (matrix-pipe cycles) and the compat-matrix
                     build (HBM-write-bound), the kernel north_star names;
  check           -- parity of THIS run's outputs -- the LAST forward of the timed region, i.e. produced with the schedule
                     `value` was measured with (forwards in flight): every pair of rank 0's shard against the outputs
                     of the unmodified reference on the same pairs (tests/golden/census_<config>.npz, written by
                     oracle/make_census_goldens.py), bitwise against the single-stream leg's result, and the first pairs
                     against the CPU oracle run in the cpu_baseline leg;
  sustained       -- the same step repeated for >= --sustain-seconds after the timed region (the K timed steps of
                     the default invocation last a fraction of a second on a power-managed chip);
  power           -- socket power / shader clock of rank 0's GPU sampled from its hwmon during the sustained leg, the
                     board's cap, joules per pair: at frac_of_cap ~ 1 the step is bounded by the board's power budget
                     (tools/forward_power.py is the stand-alone record; null where no sensor is readable);
  cpu_baseline    -- the reference's CPU path timed on this host's cores on a bounded sample of the same workload
                     (rank 0, N=1 only): the unmodified reference when /root/reference is importable (kind
                     "reference"), else the CPU oracle in its timing mode (kind "port").
--backend gloo runs the N>1 path with CPU-tensor collectives and all ranks on the visible GPU(s) round-robin: the
rehearsal of the multi-GPU code path on a one-GPU box (not a scaling measurement).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import glob
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense BF16/FP16 MFMA peak (one row of the guide)
PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: dense fp32-input MFMA peak
PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E peak (6.3 TB/s achievable)
MAX_CLOCK_GHZ = 2.4               # MI355X_MICROARCH.md: max shader clock
ORACLE_KEYS = ("num_layers", "num_channels", "num_iterations", "ratio", "inlier_threshold", "k", "nms_radius")
REFERENCE_DIR = Path("/root/reference")      # exists in the build container only, never on the GPU box


def log(msg):
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


_T0 = time.perf_counter()


class PowerSampler(threading.Thread):
    """Socket power and shader clock of this rank's GPU, read from the amdgpu hwmon files every 50 ms while a leg runs.

    A box may expose more GPUs in sysfs than the process sees: the sensor is the one whose PCI address equals the device's
    (torch's pci_*_id properties against the /sys/class/drm/card*/device link); failing that, with one rank on the box, the
    sensor with the highest mean reading (the loaded GPU).  Everything here is best effort: no sensor -> `power` is null."""

    def __init__(self, device_index: int, period: float = 0.05):
        super().__init__(daemon=True)
        self.period, self.stop_flag = period, False
        self.sensors = []
        for hw in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            for name in ("power1_average", "power1_input"):
                if os.path.exists(os.path.join(hw, name)):
                    self.sensors.append({"dir": hw, "power": os.path.join(hw, name), "pw": [], "ck": []})
                    break
        self.want_pci = None
        try:
            pr = torch.cuda.get_device_properties(device_index)
            self.want_pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}."
        except Exception:       # noqa: BLE001
            pass

    @staticmethod
    def _read(path):
        try:
            return int(open(path).read())
        except Exception:       # noqa: BLE001
            return None

    def run(self):
        while not self.stop_flag:
            for sn in self.sensors:
                v = self._read(sn["power"])
                if v is not None:
                    sn["pw"].append(v * 1e-6)
                c = self._read(os.path.join(sn["dir"], "freq1_input"))
                if c is not None:
                    sn["ck"].append(c * 1e-6)
            time.sleep(self.period)

    def finish(self, seconds: float, pairs: int, solo: bool):
        self.stop_flag = True
        self.join()
        live = [sn for sn in self.sensors if sn["pw"]]
        if not live:
            return None
        chosen, how = None, None
        if self.want_pci:
            for sn in live:
                try:
                    if os.path.basename(os.path.realpath(os.path.join(sn["dir"], "..", ".."))).lower().startswith(self.want_pci):
                        chosen, how = sn, "pci address"
                except Exception:       # noqa: BLE001
                    pass
        if chosen is None and solo:
            chosen, how = max(live, key=lambda sn: sum(sn["pw"]) / len(sn["pw"])), "highest mean reading on the box"
        if chosen is None:
            return None
        pw = chosen["pw"][len(chosen["pw"]) // 4:]                  # drop the first quarter: the sensor averages over a window
        ck = chosen["ck"][len(chosen["ck"]) // 4:]
        cap = self._read(os.path.join(chosen["dir"], "power1_cap"))
        mean = sum(pw) / len(pw)
        return {"leg": "sustained", "mean_w": round(mean, 1), "max_w": round(max(pw), 1), "cap_w": None if cap is None else round(cap * 1e-6, 1),
                "frac_of_cap": None if not cap else round(mean / (cap * 1e-6), 4), "mean_sclk_mhz": round(sum(ck) / len(ck), 0) if ck else None,
                "joule_per_pair": round(mean * seconds / pairs, 4), "samples": len(pw), "sensor": chosen["dir"], "sensor_matched_by": how,
                "note": "this rank's GPU only; value x joule_per_pair = mean_w: at frac_of_cap ~ 1 the step is bounded by the board's power, not by a kernel's schedule"}


def cpu_baseline_worker(config: str, pairs: int, threads: int, check_pairs: int, force_port: bool = False) -> None:
    """Child process: time the reference's CPU path on `pairs` pairs of the bench workload, then (untimed) run the exact
    oracle on `check_pairs` pairs for the parity check; prints one JSON line."""
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import pointdsc_oracle as O
    from pointdsc_amd import PointDSC, workloads
    torch.set_num_threads(threads)
    w = workloads.WORKLOADS[config]
    kw = dict(w["model"])
    sd = workloads.state_dict(config, PointDSC(**kw).state_dict())
    batch = workloads.batch(config, 0, max(pairs, check_pairs, 1))
    okw = {k: kw[k] for k in ORACLE_KEYS}
    kind, run = "port", None
    if (REFERENCE_DIR / "models" / "PointDSC.py").exists() and not force_port:
        try:
            sys.path.insert(0, str(REFERENCE_DIR))
            from models.PointDSC import PointDSC as RefPointDSC     # the unmodified reference (build container only)
            ref = RefPointDSC(**kw).eval()
            ref.load_state_dict(sd, strict=True)
            kind = "reference"

            def run(i):
                return ref({"corr_pos": batch["corr_pos"][i:i + 1], "src_keypts": batch["src_keypts"][i:i + 1],
                            "tgt_keypts": batch["tgt_keypts"][i:i + 1], "testing": True})
        except Exception:       # noqa: BLE001
            kind, run = "port", None
    if run is None:
        O.set_timing_mode(True)

        def run(i):
            return O.forward_testing(sd, batch["corr_pos"][i:i + 1], batch["src_keypts"][i:i + 1], batch["tgt_keypts"][i:i + 1], **okw)
    with torch.no_grad():
        run(0)                                                   # warm-up
        t1 = time.perf_counter()
        for i in range(pairs):
            run(i % batch["corr_pos"].shape[0])
        dt = time.perf_counter() - t1
        O.set_timing_mode(False)
        chk = [O.forward_testing(sd, batch["corr_pos"][i:i + 1], batch["src_keypts"][i:i + 1], batch["tgt_keypts"][i:i + 1], **okw)
               for i in range(check_pairs)]
    print(json.dumps({"pairs_per_s": pairs / dt, "seconds": dt, "threads": threads, "kind": kind,
                      "oracle_trans": [c["final_trans"][0].tolist() for c in chk],
                      "oracle_labels": [torch.nonzero(c["final_labels"][0] > 0).flatten().tolist() for c in chk]}), flush=True)


def reference_check(config, first_pair, B, N, res, dec, census_mod, w, kw, batch):
    """Parity of one forward's outputs against the unmodified reference's outputs on the same pairs (tests/golden/census_<config>.npz:
    its fp32 and its fp64 run; bench_<config>.npz for the large-N workloads): the contract of BASELINE.json, no looser tolerance for any
    pair -- labels bit-exact and R/t within 1e-4 of the fp32 output; a pair outside it passes only with the reference's fp64 output
    under the same contract or a NAMED rule of tools/parity_census.py:explain with its bounded check (same rule as test_parity_census).
    Returns the fields of the line's `check` object."""
    check = {}
    gold = ROOT / "tests" / "golden" / f"census_{config}.npz"
    gold_first = ROOT / "tests" / "golden" / f"bench_{config}.npz"
    if not gold.exists() and gold_first.exists() and first_pair == 0:
        # workloads without a census (the large-N ones): the reference's outputs on the FIRST pairs (oracle/make_bench_goldens.py)
        import numpy as np
        fxb = np.load(gold_first, allow_pickle=False)
        g = min(B, fxb["ref_final_trans"].shape[0])
        lab = torch.from_numpy(np.unpackbits(fxb["ref_final_labels_bits"][:g], axis=1)[:, :N].astype(np.float32))
        dTb = (res["final_trans"][:g].cpu().double() - torch.from_numpy(fxb["ref_final_trans"][:g]).double()).abs().amax(dim=(1, 2))
        flb = (res["final_labels"][:g].cpu() != lab).sum(dim=1)
        check.update(pairs_vs_reference=g, max_abs_dT_vs_reference=float(dTb.max()), max_abs_dT_vs_reference_fp32=float(dTb.max()),
                     pairs_failing_vs_reference=[int(i) for i in torch.nonzero(~((dTb < 1e-4) & (flb == 0))).flatten()],
                     label_flips_vs_reference=int(flb.sum()),
                     reference_outputs="tests/golden/bench_%s.npz (unmodified reference, first %d pair(s), oracle/make_bench_goldens.py)" % (config, g))
    if gold.exists():
        import numpy as np
        fx = np.load(gold, allow_pickle=False)
        f0 = first_pair
        g = max(0, min(B, fx["ref32_final_trans"].shape[0] - f0))
        fx = {k: (fx[k][f0:f0 + g] if getattr(fx[k], "ndim", 0) >= 1 and fx[k].shape[0] == fx["ref32_final_trans"].shape[0] else fx[k]) for k in fx.files}
        got_T, got_lab = res["final_trans"][:g].cpu().double(), res["final_labels"][:g].cpu()
        per = {}
        for tag in ("ref32", "ref64"):
            lab = torch.from_numpy(np.unpackbits(fx[tag + "_final_labels_bits"][:g], axis=1)[:, :N].astype(np.float32))
            per[tag] = ((got_T - torch.from_numpy(fx[tag + "_final_trans"][:g]).double()).abs().amax(dim=(1, 2)), (got_lab != lab).sum(dim=1))
        ok32 = (per["ref32"][0] < 1e-4) & (per["ref32"][1] == 0)
        # the rule of tests/test_gpu_parity.py::test_parity_census: a pair outside the contract against the reference's fp32 output needs
        # the reference's fp64 output under the same contract (where its two runs differ) or a NAMED rule checked against the
        # decisions recorded in tests/golden/census_internals_<config>.npz / census_refine_<config>.npz (tools/parity_census.py)
        ref_self = np.abs(fx["ref32_final_trans"][:g].astype(np.float64) - fx["ref64_final_trans"][:g]).max(axis=(1, 2))
        ill = (ref_self >= 1e-4) | (fx["ref32_final_labels_bits"][:g] != fx["ref64_final_labels_bits"][:g]).any(axis=1)
        ixp = ROOT / "tests" / "golden" / f"census_internals_{config}.npz"
        outside, failing = [], []
        ok64 = (per["ref64"][0] < 1e-4) & (per["ref64"][1] == 0)
        finite = torch.isfinite(res["final_trans"][:g].cpu()).flatten(1).all(dim=1) & torch.isfinite(got_lab).all(dim=1)
        for i in [int(i) for i in torch.nonzero(~ok32).flatten()]:
            #  a pair on which the reference does not reproduce itself is NOT excused by that alone: the result must
            # still be finite and either equal the reference's fp64 output under the same contract or match a decision the
            # reference recorded (explain below) -- garbage on such a pair fails the run
            why = "equals the reference's fp64 output (its fp32 run differs from it)" if bool(ill[i] and ok64[i]) else "no decision record"
            excused = bool(ill[i] and ok64[i] and finite[i])
            if dec is not None and ixp.exists():
                try:
                    ix = np.load(ixp, allow_pickle=False)
                    rxp = ROOT / "tests" / "golden" / f"census_refine_{config}.npz"
                    rx = np.load(rxp, allow_pickle=False) if rxp.exists() else None
                    l32 = np.unpackbits(fx["ref32_final_labels_bits"][i])[:N]
                    flipped = np.flatnonzero((got_lab[i].numpy() > 0) != (l32 > 0))
                    okx, why = census_mod.explain(f0 + i, {k: v[i] for k, v in dec.items()}, ix,
                                                  {k: batch[k][i] for k in ("src_keypts", "tgt_keypts")}, float(kw["inlier_threshold"]),
                                                  float(w["pair"]["scale"]), flipped if float(per["ref32"][0][i]) < 1e-4 else None,
                                                  nms_radius=float(kw["nms_radius"]), rx=rx, T_here=res["final_trans"][i].cpu().numpy(),
                                                  T_ref=fx["ref32_final_trans"][i], label_flips=int(per["ref32"][1][i]))
                    excused = (excused or bool(okx)) and bool(finite[i])
                except Exception as e:  # noqa: BLE001
                    why = f"explain failed: {e!r}"
            outside.append({"pair": f0 + i, "dT_vs_ref_fp32": float(per["ref32"][0][i]), "label_flips": int(per["ref32"][1][i]),
                            "reference_not_self_consistent": bool(ill[i]), "excused": excused, "why": why})
            if not excused:
                failing.append(f0 + i)
        # (a one-pair shard whose pair sits outside with a recorded cause has NO pair inside: the maximum over the inside set is
        #  then 0 by convention and the explicit list decides -- r05: multiway_n20000_b1 pair 0, knn-tie)
        n_in = int(ok32.sum())
        check.update(pairs_vs_reference=g, pairs_inside_fp32_contract=n_in,
                     max_abs_dT_vs_reference=float(per["ref32"][0][ok32].max()) if n_in else 0.0,
                     max_abs_dT_vs_reference_fp32=float(per["ref32"][0].max()),
                     pairs_outside_fp32_contract=outside, pairs_failing_vs_reference=failing,
                     outputs_finite=bool(finite.all()),
                     label_flips_vs_reference=int(per["ref32"][1][ok32].sum()) if n_in else 0,
                     reference_outputs="tests/golden/census_%s.npz (unmodified reference, fp32 and fp64 runs, "
                                       "oracle/make_census_goldens.py) + census_internals_%s.npz (its recorded decisions)"
                                       % (config, config))

    return check


def extra_leg(config, over, what, args, dev, lib, census_mod, use_tail):
    """One short leg of another line: its own module, pairs, timed region (two forwards in flight, like the headline) and parity check
    (reference_check on the last forward of ITS timed region).  Returns the object printed under `extra`."""
    from pointdsc_amd import PointDSC, workloads
    from pointdsc_amd.pipeline import InFlight
    w = workloads.WORKLOADS[config]
    kw = dict(w["model"])
    B, N = w["global_batch"], w["num_corr"]
    model = PointDSC(**kw)
    model.load_state_dict(workloads.state_dict(config, model.state_dict()))
    model = model.eval().to(dev)
    for k, v in over.items():
        setattr(model, k, v)
    batch = workloads.batch(config, 0, B)
    data = {k: batch[k].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["testing"] = True
    run2, run1 = InFlight(model, depth=2, tail_streams=use_tail), InFlight(model, depth=1)
    for _ in range(3):
        res = run2(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        run2(data)
    torch.cuda.synchronize()
    steps = max(8, min(2000, int(math.ceil(args.extra_seconds / max((time.perf_counter() - t0) / 4, 1e-5)))))
    t0 = time.perf_counter()
    for _ in range(steps):
        res = run2(data)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"what": what, "value": round(B * steps / dt, 3), "unit": "pairs/s", "ms_per_step": round(dt / steps * 1e3, 4), "steps": steps,
           "pairs_per_step": B, "in_flight": 2, "compat_format": model.compat_format, "layer_gemm": model.layer_gemm,
           "attention_precision": model.attention_precision,
           "weights": "trained-like (tests/golden/%s.npz)" % w["weights"] if "weights" in w else "seeded random"}
    last = {k: res[k].clone() for k in ("final_trans", "final_labels")}
    dec = census_mod.decisions(model, B, N) if census_mod is not None else None
    chk = reference_check(config, 0, B, N, last, dec, census_mod, w, kw, batch)
    chk["ok"] = bool(chk.get("max_abs_dT_vs_reference") is not None and chk["max_abs_dT_vs_reference"] < 1e-4 and
                     chk.get("label_flips_vs_reference") == 0 and not chk.get("pairs_failing_vs_reference") and chk.get("outputs_finite", True))
    out["check"] = chk
    if model.compat_format != "f32":
        del run2, run1, model
        torch.cuda.empty_cache()
        return out
    # the fp32-format compat build on one stream, hipEvents around the launch (same recorder as the headline's roofline objects)
    n_ev = 6
    _lib_check = __import__("pointdsc_amd._lib", fromlist=["check"]).check
    _lib_check(lib.pdsc_profile_enable(n_ev + 4), "pdsc_profile_enable")
    _lib_check(lib.pdsc_profile_reset(), "pdsc_profile_reset")
    for _ in range(n_ev):
        run1(data)
    torch.cuda.synchronize()
    ms, n = C.c_double(0), C.c_int(0)
    _lib_check(lib.pdsc_profile_read(1, C.byref(ms), C.byref(n)), "pdsc_profile_read")
    _lib_check(lib.pdsc_profile_enable(0), "pdsc_profile_enable(0)")
    if n.value:
        c16 = model.compat_format == "u16"
        nbytes = ((2.0 if c16 else 4.0) * N * N + 24.0 * N) * B
        avg = ms.value / n.value * 1e-3
        out["roofline_compat"] = {"kernel": "compat_sym_u16_kernel" if c16 else "compat_sym_kernel", "bound": "hbm", "achieved": round(nbytes / avg / 1e9, 1),
                                  "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(nbytes / avg / 1e9 / PEAK_HBM_GBS, 4), "launches": n.value,
                                  "avg_launch_ms": round(avg * 1e3, 4), "bytes_per_launch": nbytes}
    del run2, run1, model
    torch.cuda.empty_cache()
    return out


DUMP_CAP_BYTES = 64 * 10**6      # --dump-outputs: at most 64 MB in all


def dump_outputs(path, res, gathered_trans=None):
    """--dump-outputs: what the last timed step returned, as <path>/<name>.npy in float32 -- final_trans [B, 4, 4] and final_labels
    [B, N] of this rank's shard, and with N > 1 ranks the gathered poses of all ranks.  An array larger than its share of the cap
    is stored as a fixed, seeded sample of its rows (the row indices next to it as <name>_rows.npy)."""
    import numpy as np
    arrays = {k: res[k] for k in ("final_trans", "final_labels")}
    if gathered_trans is not None:
        arrays["gathered_final_trans"] = gathered_trans
    out = Path(path)
    out.mkdir(parents=True, exist_ok=True)
    share = DUMP_CAP_BYTES // (2 * len(arrays))       # (room for the row indices of a sampled array)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        row_bytes = max(a[0].nbytes if a.shape[0] else 1, 1)
        if a.nbytes > share:
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], size=max(1, share // row_bytes), replace=False))
            a = a[rows]
            np.save(out / f"{name}_rows.npy", rows.astype(np.float64))
        np.save(out / f"{name}.npy", np.ascontiguousarray(a, dtype=np.float32))
    log(f"outputs of the last timed step written to {out}: {', '.join(sorted(arrays))}")


def parse():
    from pointdsc_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other leg of the line: parity check, sustained leg and power, single-stream "
                         "leg with the roofline events, extra legs, CPU baseline (off: the headline figure only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--config", choices=sorted(workloads.WORKLOADS), default=workloads.DEFAULT,
                    help="BASELINE.json configuration (default: configs[2], the one the metric is quoted on)")
    ap.add_argument("--global-batch", type=int, default=0, help="override the configuration's pairs per step over ALL GPUs")
    ap.add_argument("--pairs-per-gpu", type=int, default=0,
                    help="override: fixed batch per GPU per step (weak scaling); 0 = global-batch / gpus")
    ap.add_argument("--attention-precision", choices=["fp16x3", "fp32"], default="fp16x3",
                    help="arithmetic of the attention contractions: split-precision f16 MFMA, fp16 hi+lo operand pairs (default) or exact fp32 MFMA")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl = RCCL, one GPU per rank; gloo = rehearsal of the N>1 path with CPU-tensor collectives")
    ap.add_argument("--att-leaves", default=None,
                    help="summation tree of the attention's key dimension (enum pdsc_att_leaves): canonical (a pair's bits do not depend on "
                         "its batch) | per_launch | an int 2..8 (default: the module's)")
    ap.add_argument("--latency", action="store_true",
                    help="the number an UNCHANGED caller sees (evaluation/test_3DMatch.py:53-64): one forward at a time on the current stream, "
                         "its pose and labels copied to the host before the next call (forces --in-flight 1, no graphs)")
    ap.add_argument("--range-guard", choices=["sync", "lazy", "off"], default=None,
                    help="--latency: the module's fp16 range guard for the plain calls (default: the module's own, 'sync': the call waits for the "
                         "forward and reads the range words the last launch left in pinned host memory; 'lazy': the call returns at once)")
    ap.add_argument("--no-check", action="store_true", help="--full: skip the parity check of this run's outputs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--sustain-seconds", type=float, default=2.0, help="--full: extra measured leg after the timed region (0 = off)")
    ap.add_argument("--in-flight", type=int, default=0,
                    help="forwards in flight: consecutive steps alternate between this many HIP streams (pointdsc_amd/pipeline.py); "
                         "1 = every step on the current stream; 0 = 2, or 6 captured hipGraphs (zero-copy replays) when a step is one small problem (<= 4096 "
                         "correspondences: its ~45 launches are latency- and host-bound).  The single-stream rate is measured and reported either way")
    ap.add_argument("--tail-streams", choices=["on", "off"], default="on",
                    help="with forwards in flight: enqueue each forward's latency-bound tail on a high-priority companion stream "
                         "(pdsc_forward_testing_streams; profiles/r03_h_inflight_ab.txt, r03_i_inflight_ab.txt: -2.6 %% per step at 32 "
                         "pairs of N=5000, -6 %% at 4 pairs, -13 %% for one pair of N=10000; not used on the hipGraph path)")
    ap.add_argument("--graphs", choices=["auto", "on", "off"], default="auto",
                    help="replay each in-flight slot's forward as a captured hipGraph (auto: only when a step is one small problem)")
    ap.add_argument("--zero-copy", choices=["on", "off"], default="off",
                    help="with --graphs, on: capture each slot's graph on the resident input tensors and hand out the graph's own output "
                         "tensors (pipeline.InFlight(zero_copy=True): no staging copies / clones around a replay -- a STRICTER contract than the "
                         "module call: results are overwritten `depth` calls later and the inputs must not change while a replay runs); "
                         "off (default, ADVICE r04): staged copies in, clones out, the drop-in call's contract")
    ap.add_argument("--settle-seconds", type=float, default=0.5,
                    help="untimed load before the timed region so that it does not sit on the clock ramp (0 = exactly W warm-up steps)")
    ap.add_argument("--cpu-pairs", type=int, default=0, help="pairs timed on the CPU baseline (0 = sized for ~10-20 s)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads for the CPU baseline (0 = min(host cores, 32))")
    ap.add_argument("--cpu-timeout", type=float, default=240.0, help="wall-clock cap for the CPU baseline leg")
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--force-port", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--check-pairs", type=int, default=2, help=argparse.SUPPRESS)
    ap.add_argument("--extra", choices=["auto", "on", "off"], default="auto",
                    help="--full: after the headline, short legs (<= 3 s each) of the lines the headline does not show, each with its own parity "
                         "check, printed under `extra`: the trained-like checkpoint of the same configuration and the headline workload with the "
                         "bit-exact fp32 spatial-consistency matrix (auto: on for the default --full invocation -- one GPU, default config, no --latency)")
    ap.add_argument("--extra-seconds", type=float, default=1.5, help="timed length of each extra leg")
    ap.add_argument("--first-pair", type=int, default=0,
                    help="start the workload's pair list at this pair (default 0 = the configuration as BASELINE.json quotes it); e.g. "
                         "--config kitti_n5000_b16 --global-batch 2 --first-pair 60 times and checks the census pair the parity "
                         "section of DESIGN.md discusses")
    return ap.parse_args()


def attention_plan(lib, B, N, leaves):
    """(key split = workgroups per query block, partials per query the layer kernel merges) of the attention launches of this run."""
    mode = {"per_launch": 0, "canonical": 1}.get(leaves, leaves)
    if mode == 0:
        ns = int(lib.pdsc_attention_split_default_split(B, N))
        return {"key_split": ns, "leaves": ns, "form": "key split planned per launch (bits depend on the batch)"}
    ns, nl = C.c_int(), C.c_int()
    lib.pdsc_attention_leaf_plan(B, N, int(mode), C.byref(ns), C.byref(nl))
    return {"key_split": ns.value, "leaves": nl.value, "form": "leaves that depend on N alone (bits independent of the batch)"}


def fp32_att(args):
    return args.attention_precision == "fp32"


def main():
    args = parse()
    full = args.full
    if args.cpu_baseline_worker:
        cpu_baseline_worker(args.config, args.cpu_pairs, args.cpu_threads or (os.cpu_count() or 1), args.check_pairs, args.force_port)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            # plain `python bench.py --gpus N`: launch ourselves, one process per GPU, exactly as the driver's
            # torch.distributed.run line would (rendezvous on 127.0.0.1, a free port); the ranks' output is ours
            import socket
            import subprocess
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                port = so.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
                   "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
            log("--gpus %d without a launcher: re-executing under torch.distributed.run (%s)" % (args.gpus, " ".join(cmd[1:8])))
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            sys.exit(subprocess.run(cmd, env=env).returncode)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run for N>1")
    if args.backend == "gloo":
        local_rank %= max(torch.cuda.device_count(), 1)          # rehearsal: ranks share the visible GPU(s)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    # launched by torch.distributed.run with ONE rank (tests/test_gpu_parity.py: the RCCL bring-up -- init with device_id=, barrier,
    # all_gather -- exercised on the one-GPU box): the process group exists, the data path is the world-1 one
    solo_pg = world == 1 and args.backend == "nccl" and "RANK" in os.environ and "MASTER_PORT" in os.environ
    if world > 1 or solo_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend="gloo")

    from pointdsc_amd import PointDSC, _lib, sharding, workloads
    lib = _lib.load()
    w = workloads.WORKLOADS[args.config]
    global_batch = args.global_batch or w["global_batch"]
    if args.pairs_per_gpu > 0:
        B, scaling = args.pairs_per_gpu, "weak"
    else:
        if global_batch % world:
            raise SystemExit(f"global batch {global_batch} is not divisible by {world} GPUs")
        B, scaling = global_batch // world, "strong"
    N = w["num_corr"]
    kw = dict(w["model"])
    model = PointDSC(**kw)
    sd = workloads.state_dict(args.config, model.state_dict())
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    model.attention_precision = args.attention_precision
    if args.att_leaves is not None:
        model.att_leaves = int(args.att_leaves) if args.att_leaves.lstrip("-").isdigit() else args.att_leaves
    if args.latency:
        args.in_flight, args.graphs = 1, "off"
        model.freeze_weights()          # the evaluation loop never edits the weights between calls: no per-call fingerprint walk
        if args.range_guard:
            model.range_guard = args.range_guard
    # each rank owns its shard of the global batch: pairs [rank*B, (rank+1)*B) of the workload's pair list
    batch = workloads.batch(args.config, args.first_pair + rank * B, B)
    data = {k: batch[k].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["testing"] = True
    total_pairs = B * world
    last = {}

    from pointdsc_amd.pipeline import InFlight
    small = B * N <= 4096                      # one small problem per step: its ~45 launches are latency- and host-bound
    # small steps are host / queue bound: depth sweep r04 (profiles/r04_w_inflight_depth_n1000.txt; sustained pairs/s at depth
    # 2 / 3 / 4 / 5 / 6 / 8: 4650 / 6530 / 4730 / 5630 / 6520 / 5990; timed K = 20 region 2550 / 2890 / 3490 / 4770 / 5160 / 4940)
    in_flight = args.in_flight if args.in_flight > 0 else (6 if small else 2)
    use_graphs = in_flight > 1 and (args.graphs == "on" or (args.graphs == "auto" and small))
    use_tail = args.tail_streams == "on"
    # captured forwards read the bench's resident input tensors in place and hand out the graphs' own output tensors
    zero_copy = use_graphs and args.zero_copy == "on"
    runners = {d: InFlight(model, depth=d, graphs=use_graphs and d > 1, tail_streams=use_tail, zero_copy=zero_copy and d > 1)
               for d in sorted({1, in_flight})}
    depth = {"d": in_flight}

    def gather(res):
        # the pose gather rides behind its forward on the forward's stream: off the critical path of the next step
        if args.backend == "gloo" and world > 1:                 # CPU-tensor all_gather of the 64 B poses
            return sharding.gather_results(res["final_trans"].cpu(), None, total_pairs)
        return sharding.gather_results(res["final_trans"], None, total_pairs)

    def step():
        if args.latency:
            # the UNCHANGED caller's call: the plain module call with the module's default range guard ("sync": the range words are
            # read back before the call returns), not a pipeline slot
            with torch.no_grad():
                res = model(data)
            res["post"] = gather(res)
        else:
            res = runners[depth["d"]](data, post=gather)
        last["res"] = res
        if args.latency:
            # what the reference's evaluation loop does with every result before it asks for the next one
            # (evaluation/test_3DMatch.py:54,64: pred_labels.detach().cpu().numpy(), the pose for the metrics)
            last["host"] = (res["final_trans"].cpu(), res["final_labels"].cpu())
        return res["post"]

    def fence():
        torch.cuda.synchronize()
        if world > 1 or solo_pg:
            dist.barrier()
        torch.cuda.synchronize()

    log(f"rank {rank}: {args.config}: model + {B} pairs (N={N}) resident on {dev}; warm-up x{args.warmup}")
    for _ in range(args.warmup):
        out = step()
    torch.cuda.synchronize()
    # The chip is power-managed: it leaves its idle clocks only after tens of milliseconds of load, so W = 3-5 warm-up steps
    # of a 2 ms step (the per-GPU share of an 8-GPU run) would leave the timed K steps on the ramp (measured r03: 1707 pairs/s
    # on the ramp, 1891 sustained, same code).  Keep stepping, untimed, until the GPU has been busy for --settle-seconds in all
    # (same step count on every rank: decided by rank 0); the count is reported as warmup_settle_steps.
    settle = 0
    if args.settle_seconds > 0:
        t_s = time.perf_counter()
        probe = 0
        while probe < 4:
            step()
            probe += 1
        torch.cuda.synchronize()
        per_step = max((time.perf_counter() - t_s) / 4, 1e-5)
        settle = min(5000, max(0, int(math.ceil(args.settle_seconds / per_step)) - 4))
        if world > 1:
            t = torch.tensor([settle], dtype=torch.int64, device=dev if args.backend == "nccl" else "cpu")
            dist.broadcast(t, src=0)
            settle = int(t.item())
        for _ in range(settle):
            step()
        torch.cuda.synchronize()
        settle += 4
    log(f"warm-up done ({args.warmup} + {settle} settle steps); timing")

    n_layers = kw["num_layers"]

    def events_on():
        # hipEvents around ONE attention launch and ONE fused layer launch per forward (of 12 / 11 that do identical work) and
        # around the compat build: bracketing all 24 cost the stream ~50 event records per forward = 8 % of a 2 ms step
        _lib.check(lib.pdsc_profile_enable(args.steps + 8), "pdsc_profile_enable")
        _lib.check(lib.pdsc_profile_set_stride(0, n_layers), "pdsc_profile_set_stride")
        _lib.check(lib.pdsc_profile_set_stride(2, max(n_layers - 1, 1)), "pdsc_profile_set_stride")
        _lib.check(lib.pdsc_profile_reset(), "pdsc_profile_reset")

    # With several forwards in flight the kernels of two streams share the chip, so a kernel's event-to-event time is no longer
    # its own duration: the roofline events are then recorded during the single-stream K steps that follow the timed region
    # (same run, same data); with --in-flight 1 they are recorded during the timed region itself.  (--full only)
    if full and depth["d"] == 1:
        events_on()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    elapsed = time.perf_counter() - t0
    log(f"timed region done: {elapsed:.3f}s for {args.steps} steps")
    # the parity check below judges THIS result: the last forward of the timed region, produced with the schedule `value` was
    # measured with (forwards in flight, tail streams / replayed hipGraphs); the single-stream leg's result is compared with it
    timed_res = {k: last["res"][k].clone() for k in ("final_trans", "final_labels")}
    # fingerprint of the GATHERED poses of that step (all pairs of all ranks, in pair order): with att_leaves = "canonical" a run
    # sharded over 8 GPUs must print the same fingerprint as the one-GPU run of the same pairs (tests/test_sharding_gloo.py)
    import hashlib
    poses_sha = hashlib.sha256(out["final_trans"].detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16] if isinstance(out, dict) else None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_res, out["final_trans"] if world > 1 else None)
    # ... and (--full) the discrete decisions of that forward (seeds, votes, chosen hypothesis, refinement trace, neighbour sets), read
    # from its workspace before the next leg overwrites it: what tools/parity_census.py:explain needs should a pair leave the contract
    timed_dec, census_mod = None, None
    if full:
        try:
            import importlib.util
            _spec = importlib.util.spec_from_file_location("parity_census", ROOT / "tools" / "parity_census.py")
            census_mod = importlib.util.module_from_spec(_spec)
            _spec.loader.exec_module(census_mod)
            if not (runners[in_flight].graphs and runners[in_flight]._captured):
                timed_dec = census_mod.decisions(model, B, N)
        except Exception as e:  # noqa: BLE001
            log(f"decisions of the timed forward not available: {e!r}")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- roofline of the dominant kernels, from the recorded events ----
    def read(kind):
        ms, n = C.c_double(0), C.c_int(0)
        _lib.check(lib.pdsc_profile_read(kind, C.byref(ms), C.byref(n)), "pdsc_profile_read")
        return ms.value, n.value

    if full and depth["d"] == 1:
        (att_ms, att_n), (cmp_ms, cmp_n), (lay_ms, lay_n) = read(0), read(1), read(2)
        _lib.check(lib.pdsc_profile_enable(0), "pdsc_profile_enable(0)")

    # ---- sustained leg: the same step for >= sustain_seconds (same step count on every rank) ----
    sustained = None
    power = None
    if full and args.sustain_seconds > 0:
        n_sus = max(args.steps, min(2000, int(math.ceil(args.sustain_seconds / max(elapsed / args.steps, 1e-6)))))
        fence()
        sampler = None
        if rank == 0:
            try:
                sampler = PowerSampler(dev.index if hasattr(dev, "index") and dev.index is not None else 0)
                sampler.start()
            except Exception as e:  # noqa: BLE001
                log(f"power sampler not started: {e!r}")
                sampler = None
        t0 = time.perf_counter()
        for _ in range(n_sus):
            out = step()
        fence()
        sus = time.perf_counter() - t0
        if sampler is not None:
            try:
                power = sampler.finish(sus, B * n_sus, solo=(world == 1))
            except Exception as e:  # noqa: BLE001
                log(f"power sampler failed: {e!r}")
        if world > 1:
            t = torch.tensor([sus], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            sus = float(t.item())
        sustained = {"steps": n_sus, "seconds": round(sus, 3), "value": round(total_pairs * n_sus / sus, 3), "unit": "pairs/s"}
        log(f"sustained leg done: {sus:.3f}s for {n_sus} steps")

    # ---- the same K steps with every forward on ONE stream (no forwards in flight): reported next to `value` ----
    single = None
    if full and depth["d"] > 1:
        depth["d"] = 1
        for _ in range(3):
            step()
        events_on()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        fence()
        one = time.perf_counter() - t0
        (att_ms, att_n), (cmp_ms, cmp_n), (lay_ms, lay_n) = read(0), read(1), read(2)
        _lib.check(lib.pdsc_profile_enable(0), "pdsc_profile_enable(0)")
        if world > 1:
            t = torch.tensor([one], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            one = float(t.item())
        single = {"value": round(total_pairs * args.steps / one, 3), "unit": "pairs/s", "ms_per_step": round(one / args.steps * 1e3, 4),
                  "steps": args.steps}
        depth["d"] = in_flight

    rccl_probe = None
    if full and solo_pg:
        # one all_gather of the pose payload through RCCL with world size 1 (gather_results itself short-circuits at world 1)
        payload = last["res"]["final_trans"].reshape(-1, 16).contiguous()
        flat = torch.empty_like(payload)
        dist.all_gather_into_tensor(flat, payload)
        torch.cuda.synchronize()
        rccl_probe = {"backend": dist.get_backend(), "world": dist.get_world_size(), "all_gather_bitwise_equal": bool(torch.equal(flat, payload))}
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    # what `dtype` names: the H3 GEMMs of the layer launch and the unorm16 spatial-consistency matrix
    lay_h3 = (not fp32_att(args)) and model.layer_gemm == "h3"      # (since r03 the H3 arithmetic has its own kernels at every size)
    c16 = (not fp32_att(args)) and model.compat_format == "u16"
    fp32 = args.attention_precision == "fp32"

    value = total_pairs * args.steps / elapsed
    line = {
        "metric": "point-cloud pairs/sec @ N=%d corr" % N,
        "value": round(value, 3), "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "warmup_settle_steps": settle,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": scaling,
        "vs_baseline": None,
        "dtype": "f32" if fp32 else ("f32 (attention products as fp16x3 split (fp16 hi+lo operand pairs, three f16 MFMAs per product), f32 accumulate" +
                                      ("; fc_message / PointCN products as fp16 hi+lo split" if lay_h3 else "") +
                                      ("; spatial-consistency matrix stored as unorm16" if c16 else "") + ")"),
        "data": "synthetic",
        "config": {"workload": "%s: N=%d corr, %d pairs per step sharded over %d GPU(s) = %d per GPU, 12-layer PointDSC, "
                               "%s weights" % (w["label"], N, total_pairs, world, B,
                                               "trained-like (tests/golden/%s.npz)" % w["weights"] if "weights" in w else "seeded random"),
                   "name": args.config, "num_corr": N, "pairs_per_gpu": B, "global_batch": total_pairs,
                   "sigma_d": kw["sigma_d"], "inlier_threshold": kw["inlier_threshold"],
                   "compat_format": "f32" if fp32 else model.compat_format, "layer_gemm": model.layer_gemm,
                   "att_leaves": None if fp32 else model.att_leaves,
                   "attention_plan": None if fp32 else attention_plan(lib, B, N, model.att_leaves),
                   "latency_mode": bool(args.latency), "range_guard": model.range_guard if args.latency else "lazy (pipeline)",
                   "gathered_poses_sha256_16": poses_sha,
                   "collective": ("none (single process, no process group)" if not (world > 1 or solo_pg) else
                                  "all_gather_into_tensor of the 64-byte poses, %s, world %d" % ("RCCL" if args.backend == "nccl" else "gloo (rehearsal)", world)),
                   "parallelism": "pairs sharded over %d GPU(s), %s; %d forward(s) in flight per GPU "
                                  "(consecutive steps alternate between HIP streams%s)"
                                  % (world, ("no collective (single process)" if not (world > 1 or solo_pg) else
                                             "one all_gather of poses (%s)" % ("RCCL" if args.backend == "nccl" else "gloo rehearsal, ranks share the GPU")), depth["d"],
                                     ", each replayed as a captured hipGraph" if (runners[in_flight].graphs and runners[in_flight]._captured) else "")},
    }
    if full:
        # fused layer launch (tail of layer i + head of layer i+1).  With layer_gemm = "h3" on the wavefront-resident kernel (the
        # shipped default wherever pdsc_layer_prefers_block is 0) it is reported against HBM (`lay_bytes` below); the matrix-pipe
        # figure (600 fp32 MFMAs x 64 + 288 f16 MFMAs x 32 cycles per 32-point tile) is only reported for layer_gemm = "f32" /
        # the workgroup-per-tile kernel.  2 flop/MAC x (128*64 + 64*64 + 64*128 + 128*128 + 128*384) MACs per point
        lay_flops = 2.0 * 86016 * N * B
        lay_avg = lay_ms / max(lay_n, 1) * 1e-3
        lay_pipe_cycles = (600 * 64 + 288 * 32) * math.ceil(N / 32) * B / 1024.0      # per SIMD (256 CUs x 4)
        lay_ghz = lay_pipe_cycles / lay_avg / 1e9 if lay_n else None
        # with the H3 GEMMs (model.layer_gemm = "h3", wavefront-resident kernel) the launch needs 16 k matrix-pipe cycles per tile
        # and is bound by HBM: per point it reads the key-split partials (ns x (512 + 8) B) and the residual row (512 B) and
        # writes featB (512 B), the Q rows (512 B) and its share of the K/V tile image (32 KiB / 32)
        # (leaf form: one partial per LEAF)
        lay_ns = int(lib.pdsc_attention_split_default_split(B, N))
        if lay_h3 and model.att_leaves != "per_launch":
            lay_ns = attention_plan(lib, B, N, model.att_leaves)["leaves"]
        # r06: `bytes_per_launch` is the MINIMAL traffic of the fused launch, fixed by the algorithm and independent
        # of how the attention split its keys: per point ONE message row in (512 B) + the residual row in (512 B), featB (512 B), the Q
        # rows (fp16 hi|lo, 512 B) and the point's share of the K/V tile image (32 KiB / 32 = 1024 B) out = 3072 B.  What this
        # implementation moves on top (one 520-byte partial per LEAF instead of one merged message) is reported as `moved_bytes`.
        lay_bytes = 3072.0 * N * B
        lay_moved = (520.0 * lay_ns + 512 + 512 + 512 + 32768 / 32.0) * N * B
        lay_gbs = lay_bytes / lay_avg / 1e9 if lay_n else None
        att_flops = 4.0 * 128 * float(N) * float(N) * B           # 2 GEMMs x 2 flop/MAC x C x N^2 per pair, per launch
        att_avg = att_ms / max(att_n, 1) * 1e-3
        att_tflops = att_flops / att_avg / 1e12 if att_n else None
        # compat write + keypoint reads; the matrix is stored as unorm16 (2 B per entry) unless
        # model.compat_format = "f32" 
        cmp_bytes = ((2.0 if c16 else 4.0) * N * N + 24.0 * N) * B
        cmp_avg = cmp_ms / max(cmp_n, 1) * 1e-3
        cmp_gbs = cmp_bytes / cmp_avg / 1e9 if cmp_n else None
        att_peak = PEAK_FP32_MFMA_TFLOPS if fp32 else PEAK_F16_MFMA_TFLOPS
        roof = {"kernel": "sc_attention_kernel" if fp32 else "sc_attention_split_kernel", "bound": "mfma",
                "achieved": None if att_tflops is None else round(att_tflops, 2), "peak": att_peak, "unit": "TFLOP/s",
                "frac": None if att_tflops is None else round(att_tflops / att_peak, 4),
                "traffic": None, "launches": att_n, "launches_per_forward": n_layers, "avg_launch_ms": round(att_avg * 1e3, 4),
                "flops_per_launch": att_flops,
                "timing": "hipEvents on the launch stream around one launch per forward (the %d launches of a forward do identical work), "
                          "recorded during %s" % (n_layers, "the timed region" if depth["d"] == 1 else
                                                  "the single-stream K steps right after the timed region (with forwards in flight the "
                                                  "kernels of two streams overlap and an event pair no longer times one kernel)")}
        if not fp32:
            # `achieved` counts ALGORITHMIC flops (4 C N^2 per pair per launch) against the dense BF16/FP16 MFMA peak (one row of the guide); the kernel
            # executes 3 f16 MFMAs per algorithmic product (hi*hi, hi*lo, lo*hi): its matrix-pipe share is 3 x frac.
            roof["executed_tflops"] = None if att_tflops is None else round(3 * att_tflops, 2)
            roof["executed_frac"] = None if att_tflops is None else round(3 * att_tflops / att_peak, 4)
        line.update({
            "roofline": roof,
            # H3 kernel: algorithmic HBM bytes per launch / its duration against 8 TB/s; otherwise matrix-pipe issue cycles the
            # launch needs per SIMD / its duration, against a pipe that is busy every cycle at the maximum clock
            "roofline_layer": ({"kernel": "layer_h3_coop_kernel" if lib.pdsc_layer_h3_uses_coop(B, N) else "layer_h3_kernel", "bound": "hbm",
                                "achieved": None if lay_gbs is None else round(lay_gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                "frac": None if lay_gbs is None else round(lay_gbs / PEAK_HBM_GBS, 4),
                                "traffic": None, "launches": lay_n, "avg_launch_ms": round(lay_avg * 1e3, 4),
                                "bytes_per_launch": lay_bytes, "bytes_per_point": 3072, "moved_bytes": lay_moved,
                                "moved_bytes_per_point": 520 * lay_ns + 2560, "partials_read_per_point": lay_ns,
                                "moved_frac": None if not lay_n else round(lay_moved / lay_avg / 1e9 / PEAK_HBM_GBS, 4),
                                "flops_per_launch": lay_flops} if lay_h3 else
                               {"kernel": "layer_wave_kernel" if not lib.pdsc_layer_prefers_block(B, N) else "layer_fused_kernel",
                                "bound": "mfma", "achieved": None if lay_ghz is None else round(lay_ghz, 4), "peak": MAX_CLOCK_GHZ,
                                "unit": "G matrix-pipe cycles/s per SIMD",
                                "frac": None if lay_ghz is None else round(lay_ghz / MAX_CLOCK_GHZ, 4),
                                "traffic": None, "launches": lay_n, "avg_launch_ms": round(lay_avg * 1e3, 4),
                                "flops_per_launch": lay_flops}),
            "roofline_compat": {"kernel": "compat_sym_u16_kernel" if c16 else "compat_sym_kernel", "bound": "hbm",
                                "achieved": None if cmp_gbs is None else round(cmp_gbs, 1), "peak": PEAK_HBM_GBS,
                                "unit": "GB/s", "frac": None if cmp_gbs is None else round(cmp_gbs / PEAK_HBM_GBS, 4),
                                "traffic": None, "launches": cmp_n, "avg_launch_ms": round(cmp_avg * 1e3, 4),
                                "bytes_per_launch": cmp_bytes},
        })
        if sustained is not None:
            line["sustained"] = sustained
        line["power"] = power
    line["in_flight"] = depth["d"]
    if rccl_probe is not None:
        line["rccl_world1_probe"] = rccl_probe
    line["hip_graphs"] = bool(runners[in_flight].graphs and runners[in_flight]._captured)
    line["tail_streams"] = bool(runners[in_flight].tail_streams)
    line["zero_copy_graphs"] = bool(runners[in_flight].zero_copy and line["hip_graphs"])
    if single is not None:
        line["single_stream"] = single
    if full:
        # PMC-derived HBM bytes per launch (tools/traffic_from_pmc.py writes profiles/traffic.json with the digest of the library sources it
        # was collected on): used only when that digest is THIS library's -- a figure from another build is not this run's traffic (r05's
        # line carried r04's number this way)
        traffic_file = ROOT / "profiles" / "traffic.json"
        line["traffic_source"] = None
        if traffic_file.exists():
            try:
                from pointdsc_amd import build as _build
                tj = json.loads(traffic_file.read_text())
                key = f"{args.config}_B{B}" + ("_u16" if c16 else "")
                digest = _build.source_digest()
                if tj.get("_library_source_sha256") != digest:
                    line["traffic_source"] = "profiles/traffic.json ignored: collected on library sources %s, this run's are %s" % (
                        str(tj.get("_library_source_sha256"))[:12], digest[:12])
                elif key in tj:
                    line["roofline"]["traffic"] = tj[key].get(line["roofline"]["kernel"])
                    line["roofline_compat"]["traffic"] = tj[key].get(line["roofline_compat"]["kernel"])
                    line["roofline_layer"]["traffic"] = tj[key].get(line["roofline_layer"]["kernel"])
                    line["traffic_source"] = "profiles/traffic.json (%s; library sources %s = this build)" % (tj.get("_collected", "rocprofv3 --pmc"), digest[:12])
            except Exception as e:  # noqa: BLE001
                line["traffic_source"] = "profiles/traffic.json unreadable: %r" % (e,)

    # ---- parity of this run's outputs, part 1: EVERY pair of rank 0's shard against the unmodified reference's outputs on
    #      the same pairs (tests/golden/census_<config>.npz: its fp32 and its fp64 run, oracle/make_census_goldens.py).  The
    #      contract of BASELINE.json, no looser tolerance for any pair: labels bit-exact and R/t within 1e-4 of the fp32
    #      output; a pair outside it passes only with a recorded discrete cause (same rule as test_parity_census).
    res = timed_res
    check = None
    if full and not args.no_check:
        check = {"result_judged": "last forward of the timed region (%d forward(s) in flight)" % depth["d"]}
        if single is not None:
            # the single-stream leg ran the same pairs on one stream afterwards: the schedule must not change a bit of the result
            check["timed_result_equals_single_stream_result_bitwise"] = bool(
                torch.equal(timed_res["final_trans"], last["res"]["final_trans"]) and torch.equal(timed_res["final_labels"], last["res"]["final_labels"]))
        check.update(reference_check(args.config, args.first_pair, B, N, res, timed_dec if rank == 0 else None, census_mod, w, kw, batch))

    # ---- extra legs: the lines a default invocation would otherwise never show ----
    want_extra = full and (args.extra == "on" or (args.extra == "auto" and world == 1 and args.config == workloads.DEFAULT and not args.latency
                                                  and not fp32 and not args.global_batch and not args.pairs_per_gpu and not args.first_pair))
    if want_extra and world == 1:
        line["extra"] = {}
        legs = []
        if ("trained_" + args.config) in workloads.WORKLOADS:
            legs.append(("trained_" + args.config, {}, "the same configuration on the trained-like checkpoint"))
        if model.compat_format != "f32":
            legs.append((args.config, {"compat_format": "f32"}, "the headline workload with the spatial-consistency matrix stored as the "
                                                                 "reference's fp32 values, bit for bit (compat_format = 'f32')"))
        for cfg, over, what in legs:
            try:
                line["extra"][cfg + "".join("_%s_%s" % kv for kv in sorted(over.items()))] = extra_leg(
                    cfg, over, what, args, dev, lib, census_mod, use_tail)
            except Exception as e:  # noqa: BLE001
                line["extra"][cfg] = {"error": repr(e), "ok": False}
        c32 = next((v.get("roofline_compat") for v in line["extra"].values()
                    if isinstance(v, dict) and (v.get("roofline_compat") or {}).get("kernel") == "compat_sym_kernel"), None)
        if c32 is not None:
            line["roofline_compat"]["f32_format"] = c32

    # ---- CPU baseline: the reference's CPU path on this host's cores, bounded sample (rank 0, N=1 only), in a child
    #      process with a wall-clock cap so the bench always finishes; the same child runs the exact oracle on the
    #      first pairs for part 2 of the check ----
    if full and world == 1 and not args.no_cpu_baseline:
        import subprocess
        # 32 intra-op threads is the fastest setting measured on the 256-core GPU box (16: 0.42, 32: 0.59, 64: 0.33,
        # 128: 0.19 pairs/s; 256 threads did not finish 3 pairs in 240 s), so that is what the baseline gets
        cores = args.cpu_threads or min(os.cpu_count() or 1, 32)
        n_cpu = args.cpu_pairs or {1000: 64, 5000: 6, 10000: 2}.get(N, 1 if N > 10000 else 4)
        n_chk = 0 if (args.no_check or args.first_pair) else min(B, args.check_pairs if N <= 5000 else 1)      # (the oracle leg runs the workload's first pairs)
        log(f"CPU baseline: {n_cpu} pair(s), {cores} threads (cap {args.cpu_timeout:.0f}s); exact oracle on {n_chk} pair(s) for the check")
        cmd = [sys.executable, str(Path(__file__).resolve()), "--cpu-baseline-worker", "--config", args.config,
               "--cpu-pairs", str(n_cpu), "--cpu-threads", str(cores), "--check-pairs", str(n_chk)]
        sample = "%d pair(s) of the same workload (%s, N=%d, bs=1 loop) after 1 warm-up, %d intra-op threads" % (n_cpu, args.config, N, cores)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.cpu_timeout)
            cj = json.loads(r.stdout.strip().splitlines()[-1])
            what = ("unmodified reference imported from /root/reference" if cj["kind"] == "reference"
                    else "torch-CPU oracle (oracle/pointdsc_oracle.py, timing mode = the reference's own ops)")
            ratio_file = ROOT / "profiles" / "cpu_baseline_ratio.json"
            if cj["kind"] == "port" and ratio_file.exists():
                try:
                    rj = json.loads(ratio_file.read_text())
                    what += ("; measured against the unmodified reference in the build container (%s, %d threads): reference %.3f, this "
                             "port %.3f pairs/s = %.2f x the reference's rate" % (rj["config"], rj["threads"], rj["reference"], rj["port"],
                                                                                  rj["port_over_reference"]))
                except Exception:       # noqa: BLE001
                    pass
            line["cpu_baseline"] = {"value": round(cj["pairs_per_s"], 4), "unit": "pairs/s", "cores": cores,
                                    "kind": cj["kind"], "sample": sample + ", " + what}
            if check is not None and n_chk:
                dT, flips = 0.0, 0
                for i in range(n_chk):
                    dT = max(dT, float((res["final_trans"][i].cpu() - torch.tensor(cj["oracle_trans"][i])).abs().max()))
                    lab = torch.zeros(N)
                    lab[torch.tensor(cj["oracle_labels"][i], dtype=torch.long)] = 1.0
                    flips += int((res["final_labels"][i].cpu() != lab).sum())
                check.update(pairs_vs_oracle=n_chk, max_abs_dT_vs_oracle=dT, label_flips_vs_oracle=flips)
        except subprocess.TimeoutExpired:
            line["cpu_baseline"] = {"value": None, "unit": "pairs/s", "cores": cores, "kind": "port",
                                    "sample": sample + " -- did not finish within %.0fs" % args.cpu_timeout}
        except Exception as e:  # noqa: BLE001
            line["cpu_baseline"] = {"value": None, "unit": "pairs/s", "cores": cores, "kind": "port",
                                    "sample": sample + " -- failed: %r" % (e,)}
        log("CPU baseline done")
    if check is not None:
        # The unmodified reference's outputs (fixtures generated in the build container) decide; the oracle leg -- the port, re-run on
        # THIS host's cores, whose BLAS summation order is not pinned -- is reported next to it and decides only when the
        # configuration has no reference fixture (on a near-tie pair the port itself moves with the thread count: N = 20000 pair 0
        # measured 2e-4 between the port here and the port in the build container, both within 5e-7 ... 2e-4 of the reference)
        has_ref = check.get("max_abs_dT_vs_reference") is not None
        dts = [check[k] for k in (("max_abs_dT_vs_reference",) if has_ref else ("max_abs_dT_vs_oracle",)) if check.get(k) is not None]
        fl = [check[k] for k in (("label_flips_vs_reference",) if has_ref else ("label_flips_vs_oracle",)) if k in check]
        # north_star: masks bit-exact, R/t within 1e-4 (None: neither the reference fixture nor the oracle leg was available)
        # (with a census fixture `max_abs_dT_vs_reference` / `label_flips_vs_reference` cover the pairs INSIDE the fp32 contract and are
        #  informational; what decides is the explicit list: every pair outside needs a recorded cause AND a bounded, finite result)
        check["ok"] = (max(dts) < 1e-4 and sum(fl) == 0 and not check.get("pairs_failing_vs_reference") and
                       check.get("outputs_finite", True) and
                       check.get("timed_result_equals_single_stream_result_bitwise", True)) if dts else None
        if check["ok"] and line.get("extra"):
            # an extra leg that misses the contract fails the run like the headline would
            check["extra_legs_ok"] = all(bool(v.get("check", {}).get("ok")) for v in line["extra"].values())
            check["ok"] = bool(check["extra_legs_ok"])
        line["check"] = check
    print(json.dumps(line), flush=True)
    if world > 1 or solo_pg:
        dist.destroy_process_group()
    if check is not None and check["ok"] is False:
        # a throughput figure next to outputs that miss the parity contract is not a result: fail the run
        print("[bench] PARITY CHECK FAILED: %s" % json.dumps(check), file=sys.stderr, flush=True)
        sys.exit(3)


if __name__ == "__main__":
    main()
