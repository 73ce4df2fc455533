"""The backward of the per-seed solver (pdsc_seed_solve_backward, ops.seed_solve_backward, training.seed_solve).

Truth, yardstick, inputs, error measure and bound: tests/seed_solve_oracle.py (fp64 autograd through the oracle's functions on the
device's own knn_idx and iterate T; e32 = the same formulas in torch fp32 on the device; bound max(4 e32, 128 2^-24)).  Every figure is
printed before it is asserted.  k = 17 (a partial second block of 16), 40 (the default), 64 (every lane) at inlier ratio 0.8 and
k = 40 at 0.2; conditioning min (s'_i + s'_j) / s_1 >= 0.03 is asserted for every seed on the truth."""
import ctypes as C
import functools
import os
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_solve_oracle as SO  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("pdsc_seed_solve_backward", "pdsc_seed_solve_backward_workspace_bytes", "pdsc_transformation_loss_grad")


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_names_exist_in_the_package_the_header_and_the_library():
    import pointdsc_amd
    from pointdsc_amd import _lib, ops, training
    assert pointdsc_amd.seed_solve is training.seed_solve and "seed_solve" in pointdsc_amd.__all__
    assert callable(ops.seed_solve_backward)
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
        assert hasattr(lib, name)
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    q = lib.pdsc_seed_solve_backward_workspace_bytes
    assert q(2, 129, 12, 40) >= 2 * 12 * (40 * 128 * 4 + 8) and q(0, 129, 12, 40) == 0 and q(2, 129, 12, 65) == 0 and q(2, 129, 0, 40) == 0


def test_entry_point_rejects_bad_arguments_before_any_hip_call():
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)         # never dereferenced: every call below must return before it enqueues anything
    big = 1 << 30

    def call(normed=p, dn=p, ds=p, ws=p, nbytes=big, bs=2, n=129, s=12, k=40, it=10):
        return lib.pdsc_seed_solve_backward(normed, p, p, p, p, p, p, p, dn, ds, ws, nbytes, bs, n, s, k, it, None)
    assert call(normed=None) == -1 and b"null pointer" in lib.pdsc_last_error()
    assert call(dn=None, ds=None) == -1 and b"neither gradient" in lib.pdsc_last_error()
    assert call(k=65) == -1 and b"k=65" in lib.pdsc_last_error()
    assert call(k=0) == -1
    assert call(it=33) == -1 and b"num_iterations=33" in lib.pdsc_last_error()
    assert call(it=-1) == -1
    assert call(bs=0) == -1 and call(s=0) == -1 and call(n=0) == -1
    assert call(ws=None) == -1
    assert call(nbytes=16) == -2 and b"workspace" in lib.pdsc_last_error()
    assert lib.pdsc_transformation_loss_grad(None, p, p, p, p, p, big, 2, 129, None) == -1 and b"null pointer" in lib.pdsc_last_error()
    assert lib.pdsc_transformation_loss_grad(p, p, p, p, p, p, 8, 2, 129, None) == -2


def test_seed_solve_refuses_what_it_cannot_do():
    from pointdsc_amd import seed_solve
    inp = SO.make_inputs()
    knn = torch.zeros(SO.BS, SO.S, 40, dtype=torch.int32)
    args = [inp["normed"], inp["src"], inp["tgt"], knn, inp["sigma"], inp["sigma_spat"], 10]
    with pytest.raises(RuntimeError, match="no CPU path"):
        seed_solve(*args)
    for i, name in ((1, "src"), (2, "tgt"), (5, "sigma_spat")):
        bad = list(args)
        bad[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} gets no gradient"):
            seed_solve(*bad)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def g(t):
    return t.to("cuda:0")


def device_forward(inp, k, num_iter):
    """The forward's stage ops as train_forward chains them -> (knn_idx, mask, seed_trans)."""
    from pointdsc_amd import _lib, ops
    nd, src, tgt = g(inp["normed"]), g(inp["src"]), g(inp["tgt"])
    knn = ops.knn_seeds(nd, g(inp["seeds"]), k, form="matrix")
    iters, mask, _ = ops.seed_power_iteration(nd, src, tgt, knn, g(inp["sigma"]), g(inp["sigma_spat"]), num_iter)
    _lib.check(_lib.load().pdsc_conv_mask_all_pairs(ops._p(mask), SO.BS, ops._stream()), "pdsc_conv_mask_all_pairs")
    trans, _ = ops.seed_transforms(src, tgt, knn, iters, mask, num_iter)
    return knn, mask, trans


def device_backward(inp, knn, mask, num_iter, dtrans=None):
    from pointdsc_amd import ops
    return ops.seed_solve_backward(g(inp["normed"]), g(inp["src"]), g(inp["tgt"]), knn, g(inp["sigma"]), g(inp["sigma_spat"]), mask,
                                   num_iter, g(inp["dtrans"] if dtrans is None else dtrans))


@functools.lru_cache(maxsize=None)
def case(ratio, k, num_iter=SO.NUM_ITER):
    """One (inputs, device forward, truth, yardstick) per configuration, shared by the tests below and left unchanged."""
    inp = SO.make_inputs(ratios=ratio) if isinstance(ratio, tuple) else SO.make_inputs(ratio)
    knn, mask, trans = device_forward(inp, k, num_iter)
    words = mask.cpu().tolist()
    assert len(set(words)) == 1                              # AND-ed over the pairs
    T = SO.chosen_T(words[0], num_iter)
    return {"inp": inp, "knn": knn, "mask": mask, "trans": trans, "T": T, "truth": SO.truth(inp, knn, T), "e32": SO.yardstick(inp, knn, T)}


def check(label, got_dn, got_ds, ref, e32):
    e_dn, e_ds = SO.err(got_dn, ref["dnormed"]), SO.err(got_ds, ref["dsigma"])
    y_dn, y_ds = SO.err(e32["dnormed"], ref["dnormed"]), SO.err(e32["dsigma"], ref["dsigma"])
    print(f"{label}: dnormed {e_dn:.3e} (torch fp32 {y_dn:.3e}, bound {SO.bound(y_dn):.3e})  dsigma {e_ds:.3e} (torch fp32 {y_ds:.3e}, "
          f"bound {SO.bound(y_ds):.3e})  conditioning >= {float(ref['cond'].min()):.3f}")
    assert float(ref["cond"].min()) >= 0.03
    assert e_dn <= SO.bound(y_dn), (label, e_dn, SO.bound(y_dn))
    assert e_ds <= SO.bound(y_ds), (label, e_ds, SO.bound(y_ds))


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,k", [(0.8, 17), (0.8, 40), (0.8, 64), (0.2, 40)])
def test_gradients_against_fp64_autograd(ratio, k):
    c = case(ratio, k)
    dn, ds = device_backward(c["inp"], c["knn"], c["mask"], SO.NUM_ITER)
    assert dn.shape == (SO.BS, SO.N, 128) and dn.dtype == torch.float32 and ds.shape == (1,) and ds.dtype == torch.float64
    assert float((c["trans"].double().cpu() - c["truth"]["trans"]).abs().max()) <= 1e-4          # same T, same hypotheses
    check(f"r {ratio} k {k} T {c['T']}", dn, ds, c["truth"], c["e32"])


@pytest.mark.gpu
def test_early_exit_is_replayed():
    c = case(0.8, 40)
    print(f"r 0.8 k 40: the device stopped at iterate {c['T']} of {SO.NUM_ITER}")
    assert 1 <= c["T"] < SO.NUM_ITER
    mixed = case((0.8, 0.2), 40)                             # the exit is AND-ed over the pairs: the r = 0.2 pair keeps both running
    print(f"r (0.8, 0.2) k 40: iterate {mixed['T']} of {SO.NUM_ITER}")
    assert mixed["T"] == SO.NUM_ITER
    dn, ds = device_backward(mixed["inp"], mixed["knn"], mixed["mask"], SO.NUM_ITER)
    check("r (0.8, 0.2) k 40 T 10", dn, ds, mixed["truth"], mixed["e32"])


@pytest.mark.gpu
def test_one_iteration_and_none():
    c = case(0.8, 40, 1)
    assert c["T"] == 1
    dn, ds = device_backward(c["inp"], c["knn"], c["mask"], 1)
    check("r 0.8 k 40 num_iterations 1", dn, ds, c["truth"], c["e32"])
    z = case(0.8, 40, 0)
    assert z["T"] == 0
    dn, ds = device_backward(z["inp"], z["knn"], z["mask"], 0)
    assert float(dn.abs().max()) == 0.0 and float(ds.abs().max()) == 0.0          # v = 1: no path to the features, exact zeros
    assert float((z["trans"].double().cpu() - z["truth"]["trans"]).abs().max()) <= 1e-4


@pytest.mark.gpu
def test_sparse_upstream_gradient_and_determinism():
    c = case(0.8, 40)
    inp = c["inp"]
    sparse = torch.zeros_like(inp["dtrans"])
    for b, s in enumerate((3, 10)):                          # one seed per pair, as the vote's winner in training
        sparse[b, s] = inp["dtrans"][b, s]
    dn, ds = device_backward(inp, c["knn"], c["mask"], SO.NUM_ITER, sparse)
    check("sparse (one seed per pair)", dn, ds, SO.truth(inp, c["knn"], c["T"], sparse), SO.yardstick(inp, c["knn"], c["T"], sparse))
    named = torch.zeros(SO.BS, SO.N, dtype=torch.bool)
    for b, s in enumerate((3, 10)):
        named[b, c["knn"][b, s].cpu().long()] = True
    # rows no active seed names are exact zeros (a named row may be one too: a neighbour whose spatial term is 0 against all others)
    assert float(dn.cpu()[~named].abs().max()) == 0.0 and int((dn.cpu()[named].abs().amax(-1) > 0).sum()) > int(named.sum()) // 2
    dn2, ds2 = device_backward(inp, c["knn"], c["mask"], SO.NUM_ITER, sparse)
    assert torch.equal(dn, dn2) and torch.equal(ds, ds2)
    dense = [device_backward(inp, c["knn"], c["mask"], SO.NUM_ITER) for _ in range(2)]
    assert torch.equal(dense[0][0], dense[1][0]) and torch.equal(dense[0][1], dense[1][1])


@pytest.mark.gpu
def test_seeds_that_share_their_rows_add():
    c = case(0.8, 40)
    inp = c["inp"]
    knn = c["knn"].clone()
    knn[:, 5] = knn[:, 2].flip(-1)                           # seed 5 gets seed 2's row set (in another order)
    dn, ds = device_backward(inp, knn, c["mask"], SO.NUM_ITER)
    check("shared rows", dn, ds, SO.truth(inp, knn, c["T"]), SO.yardstick(inp, knn, c["T"]))


@pytest.mark.gpu
def test_an_index_out_of_range_poisons_its_seed_only():
    c = case(0.8, 40)
    inp = c["inp"]
    two = torch.zeros_like(inp["dtrans"])
    two[0, 3], two[0, 10] = inp["dtrans"][0, 3], inp["dtrans"][0, 10]
    good = two.clone()
    good[0, 10] = 0
    for bad_value in (SO.N, -1, 2 ** 31 - 1):
        knn = c["knn"].clone()
        knn[0, 10, 7] = bad_value
        knn[1, 4, 0] = bad_value                             # a seed without a gradient: never looked at
        dn, ds = device_backward(inp, knn, c["mask"], SO.NUM_ITER, two)
        ref_dn, _ = device_backward(inp, c["knn"], c["mask"], SO.NUM_ITER, good)
        rows10 = torch.zeros(SO.N, dtype=torch.bool)
        rows10[c["knn"][0, 10].cpu().long()[torch.arange(40) != 7]] = True
        dn, ref_dn = dn.cpu(), ref_dn.cpu()
        assert bool(torch.isnan(dn[0][rows10]).all()) and bool(torch.isnan(ds).all())
        assert torch.equal(dn[0][~rows10], ref_dn[0][~rows10]) and torch.equal(dn[1], ref_dn[1])


@pytest.mark.gpu
def test_seed_solve_is_the_forward_bit_for_bit_and_its_backward_the_kernel():
    from pointdsc_amd import seed_solve
    c = case(0.8, 40)
    inp = c["inp"]
    nd, sg = g(inp["normed"]).requires_grad_(True), g(inp["sigma"]).requires_grad_(True)
    trans = seed_solve(nd, g(inp["src"]), g(inp["tgt"]), c["knn"], sg, g(inp["sigma_spat"]), SO.NUM_ITER)
    assert trans.requires_grad and torch.equal(trans.detach(), c["trans"])
    dn, ds = torch.autograd.grad(trans, (nd, sg), g(inp["dtrans"]))
    ref_dn, ref_ds = device_backward(inp, c["knn"], c["mask"], SO.NUM_ITER)
    assert torch.equal(dn, ref_dn) and torch.equal(ds, ref_ds.to(torch.float32)) and ds.shape == sg.shape
    with torch.no_grad():
        assert not seed_solve(nd, g(inp["src"]), g(inp["tgt"]), c["knn"], sg, g(inp["sigma_spat"]), SO.NUM_ITER).requires_grad
    with pytest.raises(TypeError):
        seed_solve(nd, g(inp["src"]), g(inp["tgt"]), c["knn"].long(), sg, g(inp["sigma_spat"]), SO.NUM_ITER)
    with pytest.raises(ValueError, match="k = 65"):
        seed_solve(nd, g(inp["src"]), g(inp["tgt"]), torch.zeros(SO.BS, SO.S, 65, dtype=torch.int32, device="cuda:0"), sg,
                   g(inp["sigma_spat"]), SO.NUM_ITER)
