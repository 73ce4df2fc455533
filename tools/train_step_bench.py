#!/usr/bin/env python3
"""Time of the training path's f-13 pieces at the training shape (bs 16, N 1000, 12 layers), next to torch on the same device.

  kernel      training.feature_similarity forward + backward against torch's autograd of the reference's three formula lines
              (models/PointDSC.py:160-163), for a given dM;
  whole step  zero_grad, train()-mode forward, classification + spectral-matching loss, backward, Adam: TrainablePointDSC with
              the device losses against the pure-torch model of the tests (tests/train_oracle.TorchPointDSC: formula attention,
              formula M, torch losses; it has NO tail -- no seeds, kNN, power iteration, Procrustes or vote -- so the comparison
              favours it) with the same weights on the same batch.

The method of tools/attention_backward_bench.py: device events around a window of back-to-back calls that fills `--window` seconds
after `--warmup` calls; the two sides alternate inside one process; the median of `--rounds` windows is printed with the spread.
These are CALL times, host work included.

    --fused-layers       (f-15) the whole step of TrainablePointDSC(fused_layers=True) next to the default model's instead (same
                         weights, same batch, same method); with --profile-steps the profiled model is the fused one
    --fused-linears      (f-16) the whole step of TrainablePointDSC(fused_layers=True, fused_linears=True) next to
                         TrainablePointDSC(fused_layers=True) -- the step as it was before the flag existed -- likewise; with
                         --profile-steps the profiled model has both flags set
    --device-optimizer   (f-25) the whole step of TrainablePointDSC(fused_layers=True, fused_linears=True) with pointdsc_amd.DeviceAdam
                         (guard, update and skip decision on the device, nothing read back) next to the same model with
                         torch.optim.Adam and the trainer's guard line exactly as harness.train_epoch has it (one boolean read per
                         step), and next to torch.optim.Adam with no guard; with --profile-steps the profiled step is DeviceAdam's,
                         or with --torch-guard the guarded torch.optim.Adam step it replaces
    --profile-steps K    run K device steps and exit: the program of the one `rocprofv3 --kernel-trace --stats` run
    --breakdown FILE     group the per-kernel table tools/rocpd_kernel_stats.py made of that run into the step's parts (GROUPS)"""
import argparse
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

GROUPS = [      # first match wins
    ("attention forward", r"sc_attention_kernel|attention_combine_kernel"),
    ("attention backward", r"att_bwd_"),
    ("M forward + backward", r"gram_rows_kernel<2|feature_compat_backward"),
    ("losses", r"pdsc::(cls_|sm_loss_|trans_partial|trans_finish)"),
    ("optimiser (guard check, update, finish)", r"pdsc::optim_"),
    ("parameter-gradient merge (train_tile.h, both below)", r"pdsc::tt_merge_"),
    ("plain linears (layer0, q|k|v, fc_message.6, head)", r"pdsc::lth?_"),
    ("fused point-wise layers (conv + BN + ReLU)", r"pdsc::pwt_"),
    ("tail and compat (the library's other kernels)", r"pdsc::"),
    ("torch (GEMMs, batch-norm, point-wise, optimiser)", r"."),
]


def breakdown(path):
    totals, calls, total = {g: 0.0 for g, _ in GROUPS}, {g: 0 for g, _ in GROUPS}, 0.0
    for line in Path(path).read_text().splitlines():
        m = re.match(r"^(.{64}) +(\d+) +([0-9.]+) ", line)
        if not m or line.startswith("kernel "):
            continue
        name, n, us = m.group(1), int(m.group(2)), float(m.group(3))
        group = next(g for g, pat in GROUPS if re.search(pat, name))
        totals[group] += us
        calls[group] += n
        total += us
    print(f"# {path}: kernel time by part of the step, total {total / 1e3:.3f} ms")
    print(f"{'part':52s} {'launches':>9s} {'total_us':>11s} {'%':>6s}")
    for g, _ in GROUPS:
        print(f"{g:52s} {calls[g]:9d} {totals[g]:11.1f} {100 * totals[g] / total:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--breakdown", default=None)
    ap.add_argument("--fused-layers", action="store_true")
    ap.add_argument("--fused-linears", action="store_true")
    ap.add_argument("--device-optimizer", action="store_true")
    ap.add_argument("--torch-guard", action="store_true", help="with --device-optimizer --profile-steps: profile the torch side")
    a = ap.parse_args()
    if a.breakdown:
        return breakdown(a.breakdown)

    import torch
    import torch.nn.functional as F
    import train_oracle as TO
    from loss_bench import timed, torch_sm_matrix
    from pointdsc_amd import ClassificationLoss, DeviceAdam, PointDSC, SpectralMatchingLoss, synthetic, training
    assert torch.cuda.is_available(), "train_step_bench needs the GPU: a CPU run gives no time"
    dev, bs, n = "cuda:0", a.bs, a.n

    def spread(ts):
        return f"{statistics.median(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f})"

    def compare(name, ours, theirs):
        t_ours, t_theirs = [], []
        for _ in range(a.rounds):                         # alternate the two sides
            t_ours.append(timed(ours, a.warmup, a.window)[0])
            t_theirs.append(timed(theirs, a.warmup, a.window)[0])
        mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
        print(f"  {name:42s} device {spread(t_ours)}   torch {spread(t_theirs)}   torch / device {mt / mo:6.2f}")

    state = synthetic.make_state_dict(PointDSC(num_layers=a.layers).state_dict(), seed=1)
    batch = {k: v.to(dev) for k, v in synthetic.make_batch(bs, n, seed=100, inlier_ratio=0.3).items()}
    data = {k: batch[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    gt = batch["gt_labels"]
    cls_fn, sm_fn = ClassificationLoss(False), SpectralMatchingLoss(False)

    def make_step(fused, fused_linears=False, optimizer="torch", guard=False):
        model = training.TrainablePointDSC(num_layers=a.layers, fused_layers=fused, fused_linears=fused_linears)
        model.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
        model = model.to(dev).train()
        cls = DeviceAdam if optimizer == "device" else torch.optim.Adam
        opt = cls(model.parameters(), lr=1e-4, weight_decay=1e-6)
        params = [p for p in model.parameters() if p.requires_grad]

        def step():
            opt.zero_grad()
            res = model(data)
            loss = cls_fn(res["final_labels"], gt, device_stats=True)["loss"] + sm_fn(res["M"], gt)
            loss.backward()
            if guard:          # harness.train_epoch's lines for an optimiser without a guard of its own
                grads = [p.grad for p in params if p.grad is not None]
                if bool(torch.stack([torch.isfinite(g).all() for g in grads]).all()):
                    opt.step()
            else:
                opt.step()
            return loss
        return step
    if a.device_optimizer:
        device_step = make_step(True, True, "torch", True) if a.torch_guard else make_step(True, True, "device")
    else:
        device_step = make_step(a.fused_layers or a.fused_linears, a.fused_linears)

    if a.profile_steps:
        for _ in range(a.profile_steps):
            device_step()
        torch.cuda.synchronize()
        return

    print(f"bs={bs} N={n} layers={a.layers}: microseconds per call, median of {a.rounds} windows of {a.window} s (min .. max)")
    if a.device_optimizer:
        guarded_step, plain_step = make_step(True, True, "torch", True), make_step(True, True, "torch", False)
        t_dev, t_guard, t_plain = [], [], []
        for _ in range(a.rounds):                         # alternate the three steps
            t_dev.append(timed(device_step, a.warmup, a.window)[0])
            t_guard.append(timed(guarded_step, a.warmup, a.window)[0])
            t_plain.append(timed(plain_step, a.warmup, a.window)[0])
        md, mg = statistics.median(t_dev), statistics.median(t_guard)
        print(f"  training step (forward, 2 losses, backward, guard, Adam), fused_layers=True, fused_linears=True:")
        print(f"    DeviceAdam (guard on the device)            {spread(t_dev)}")
        print(f"    torch.optim.Adam + the trainer's guard line {spread(t_guard)}   guarded torch / DeviceAdam {mg / md:6.3f}")
        print(f"    torch.optim.Adam, no guard                  {spread(t_plain)}")
        room = (max(t_dev) - min(t_dev)) + (max(t_guard) - min(t_guard))
        print(f"    DeviceAdam median - guarded torch median = {md - mg:+.1f} us; the two sides' min..max spreads add up to {room:.1f} us: "
              f"{'not above' if md - mg <= room else 'ABOVE'} the parent's behaviour by more than the spread")
        return
    if a.fused_linears:
        layers_step = make_step(True)
        t_both, t_layers = [], []
        for _ in range(a.rounds):                         # alternate the two models
            t_both.append(timed(device_step, a.warmup, a.window)[0])
            t_layers.append(timed(layers_step, a.warmup, a.window)[0])
        mb, ml = statistics.median(t_both), statistics.median(t_layers)
        print(f"  {'training step (forward, 2 losses, backward, Adam)':42s} fused_layers=True, fused_linears=True {spread(t_both)}   "
              f"fused_layers=True {spread(t_layers)}   without / with fused_linears {ml / mb:6.2f}")
        return
    if a.fused_layers:
        torch_layers_step = make_step(False)
        t_fused, t_plain = [], []
        for _ in range(a.rounds):                         # alternate the two models
            t_fused.append(timed(device_step, a.warmup, a.window)[0])
            t_plain.append(timed(torch_layers_step, a.warmup, a.window)[0])
        mf, mp = statistics.median(t_fused), statistics.median(t_plain)
        print(f"  {'training step (forward, 2 losses, backward, Adam)':42s} fused_layers=True {spread(t_fused)}   "
              f"fused_layers=False {spread(t_plain)}   False / True {mp / mf:6.2f}")
        return
    gen = torch.Generator().manual_seed(bs * n)
    normed = F.normalize(torch.randn(bs, n, 128, generator=gen), dim=-1).to(dev).requires_grad_(True)
    sigma = torch.tensor([1.0], device=dev, requires_grad=True)
    dM = torch.randn(bs, n, n, generator=gen).to(dev)
    compare("feature_similarity forward + backward",
            lambda: torch.autograd.grad(training.feature_similarity(normed, sigma), (normed, sigma), dM),
            lambda: torch.autograd.grad(TO.formula_lines(normed, sigma), (normed, sigma), dM))

    ref = TO.TorchPointDSC(num_layers=a.layers)
    ref.load_state_dict(state, strict=True)
    ref = ref.to(dev).train()
    ref_opt = torch.optim.Adam(ref.parameters(), lr=1e-4, weight_decay=1e-6)

    def torch_step():
        ref_opt.zero_grad()
        logits, M, _ = ref(data["corr_pos"], data["src_keypts"], data["tgt_keypts"])
        loss = F.binary_cross_entropy_with_logits(logits, gt) + torch_sm_matrix(M, gt, False)
        loss.backward()
        ref_opt.step()
        return loss

    compare("training step (forward, 2 losses, backward, Adam)", device_step, torch_step)


if __name__ == "__main__":
    main()
