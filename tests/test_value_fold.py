"""fc_message's first conv folded into the value projection (enum pdsc_value_fold): config rules, the split-weight buffer's
layout with the fold off (unchanged) and on, the algebra the fold rests on, and on the GPU the folded forward against the
128-channel one and the folded weights against an fp64 recomputation."""
import ctypes as C

import numpy as np
import pytest
import torch

from pointdsc_amd import _lib, synthetic, workloads
from pointdsc_amd.model import PointDSC

CH, HALF = 128, 64
FOLD_TAIL, FOLD_HEAD, FOLD_W = 104, 105, 106


def _cfg(prec=0, fmt=1, gemm=1, leaves=1, fold=1):
    return _lib.PdscConfig(6, 12, CH, 10, 40, 20, 0.1, 0.1, 0.1, prec, fmt, gemm, leaves, fold)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_config_accepts_the_fold_only_with_split_attention_and_h3_gemms(lib):
    assert lib.pdsc_wpack_floats(C.byref(_cfg())) > 0
    assert lib.pdsc_wpack_floats(C.byref(_cfg(fold=0))) > 0
    assert lib.pdsc_wpack_floats(C.byref(_cfg(prec=1, fold=0))) > 0
    for bad in (_cfg(prec=1), _cfg(gemm=0), _cfg(fold=2), _cfg(fold=-1)):
        assert lib.pdsc_wpack_floats(C.byref(bad)) == -1
        assert b"value_fold" in lib.pdsc_last_error()


def test_wsplit_layout_with_the_fold_off_is_unchanged_and_grows_by_the_fold_sections(lib):
    per_layer = 2 * 2 * (128 * 128 + 384 * 128 + 64 * 128 + 64 * 64 + 128 * 64)
    frag = lib.pdsc_wfrag_tail_bytes() + lib.pdsc_wfrag_head_bytes()
    off, on = _cfg(fold=0), _cfg(fold=1)
    assert lib.pdsc_wsplit_bytes(C.byref(off)) == 12 * (per_layer + 2 * frag)
    for sec in (FOLD_TAIL, FOLD_HEAD, FOLD_W):
        assert lib.pdsc_wsplit_offset(C.byref(off), sec, 0) == -1
    assert lib.pdsc_wsplit_offset(C.byref(off), 107, 0) == -1 and lib.pdsc_wsplit_offset(C.byref(on), 107, 0) == -1
    # fc2 + fc3 chunks, their 6 bias tiles, b'; pcn + q, k, v' chunks, 14 bias tiles
    assert lib.pdsc_wfrag_fold_tail_bytes() == 6 * 8192 + 6 * 256 + 256
    assert lib.pdsc_wfrag_fold_head_bytes() == 28 * 8192 + 14 * 256
    fold = lib.pdsc_wfrag_fold_tail_bytes() + lib.pdsc_wfrag_fold_head_bytes() + HALF * (CH + 1) * 4
    assert lib.pdsc_wsplit_bytes(C.byref(on)) == 12 * (per_layer + 2 * frag + fold)
    base = 12 * (per_layer + 2 * frag)
    for layer in (0, 5, 11):
        t = lib.pdsc_wsplit_offset(C.byref(on), FOLD_TAIL, layer) * 2
        assert t == base + layer * fold and t % 16 == 0
        assert lib.pdsc_wsplit_offset(C.byref(on), FOLD_HEAD, layer) * 2 == t + lib.pdsc_wfrag_fold_tail_bytes()
        assert lib.pdsc_wsplit_offset(C.byref(on), FOLD_W, layer) * 2 == t + lib.pdsc_wfrag_fold_tail_bytes() + lib.pdsc_wfrag_fold_head_bytes()
    # the sections the 128-channel path uses sit where they always did
    for sec, layer in ((100, 0), (101, 1), (102, 1), (103, 11)):
        assert lib.pdsc_wsplit_offset(C.byref(on), sec, layer) == lib.pdsc_wsplit_offset(C.byref(off), sec, layer)


def _bn_fold(w, b, gamma, beta, mean, var, eps=1e-5):
    s = gamma / np.sqrt(var + eps)
    return w * s[:, None], (b - mean) * s + beta


def test_folded_value_projection_equals_the_nonlocal_block_formula():
    """models/PointDSC.py:12-20,36-44 in fp64 -- softmax(M * QK^T / sqrt(C)) V, then conv 128 -> 64 + BN -- against the fold
    (P (W1f Wv) f + W1f bv + b1f); and the fp32 evaluation of the fold within fp32 round-off of the fp64 result."""
    rs = np.random.RandomState(3)
    n = 300
    f = rs.standard_normal((n, CH))
    wq, wk, wv = (rs.standard_normal((CH, CH)) / np.sqrt(CH) for _ in range(3))
    bq, bk, bv = (0.1 * rs.standard_normal(CH) for _ in range(3))
    w1, b1 = rs.standard_normal((HALF, CH)) / np.sqrt(CH), 0.1 * rs.standard_normal(HALF)
    gamma, beta = 1 + 0.1 * rs.standard_normal(HALF), 0.1 * rs.standard_normal(HALF)
    mean, var = 0.1 * rs.standard_normal(HALF), 0.5 + rs.random_sample(HALF)
    m = rs.random_sample((n, n))
    q, k, v = f @ wq.T + bq, f @ wk.T + bk, f @ wv.T + bv
    logits = m * (q @ k.T) / np.sqrt(CH)
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    msg = p @ v
    ref = ((msg @ w1.T + b1) - mean) * (gamma / np.sqrt(var + 1e-5)) + beta
    w1f, b1f = _bn_fold(w1, b1, gamma, beta, mean, var)
    wfold, bprime = w1f @ wv, w1f @ bv + b1f
    folded = p @ (f @ wfold.T) + bprime
    assert np.abs(folded - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    f32 = lambda x: x.astype(np.float32)
    got = f32(p) @ (f32(f) @ f32(wfold).T) + f32(bprime)
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


def test_module_carries_the_fold_only_where_it_applies():
    model = PointDSC()
    assert model.value_fold == 1 and model._config().value_fold == 1
    model.attention_precision = "fp32"
    assert model._config().value_fold == 0
    model.attention_precision, model.layer_gemm = "fp16x3", "f32"
    assert model._config().value_fold == 0
    model.layer_gemm, model.value_fold = "h3", 0
    assert model._config().value_fold == 0
    model.value_fold = 2
    with pytest.raises(ValueError):
        model._config()


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _bench(name):
    w = workloads.WORKLOADS[name]
    model = PointDSC(**w["model"])
    model.load_state_dict(workloads.state_dict(name, model.state_dict()))
    return model.eval().to("cuda")


def _run(model, batch):
    data = {k: batch[k].to("cuda").contiguous() for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["testing"] = True
    with torch.no_grad():
        res = model(data)
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
def test_folded_weights_match_an_fp64_recomputation():
    lib = _lib.load()
    model = _bench("n5000_b32")
    pack = model.packed_weights().cpu().double().numpy()
    wsplit = model.split_weights()
    cfg = model._config()
    assert cfg.value_fold == 1
    for layer in (0, 7, 11):
        o = lambda sec: int(lib.pdsc_wpack_offset(C.byref(cfg), _lib.W[sec], layer))
        w1 = pack[o("FC1_W"):o("FC1_W") + HALF * CH].reshape(HALF, CH)
        b1 = pack[o("FC1_B"):o("FC1_B") + HALF]
        wqkv = pack[o("QKV_W"):o("QKV_W") + 3 * CH * CH].reshape(3 * CH, CH)
        bqkv = pack[o("QKV_B"):o("QKV_B") + 3 * CH]
        start = int(lib.pdsc_wsplit_offset(C.byref(cfg), FOLD_W, layer)) * 2
        got = wsplit[start:start + HALF * (CH + 1) * 4].cpu().view(torch.float32).double().numpy()
        want_w = w1 @ wqkv[2 * CH:]
        want_b = w1 @ bqkv[2 * CH:] + b1
        assert np.abs(got[:HALF * CH].reshape(HALF, CH) - want_w).max() <= 6e-8 * max(1.0, np.abs(want_w).max())
        assert np.abs(got[HALF * CH:] - want_b).max() <= 6e-8 * max(1.0, np.abs(want_b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name,bs,leaves", [("n1000_b1", 1, "canonical"), ("n5000_b32", 4, "canonical"), ("n5000_b32", 32, "canonical"),
                                            ("n5000_b32", 8, "per_launch"), ("kitti_n5000_b16", 4, "canonical"),
                                            ("lomatch_n10000_b8", 2, "canonical")])
def test_folded_forward_agrees_with_the_128_channel_forward(name, bs, leaves):
    """value_fold 1 vs 0 on the bench workloads' pairs: same labels, R/t within 1e-4, and within 1e-5 on all but a few pairs (the
    refinement amplifies the changed association order on pairs whose solve is ill-conditioned: 3 of 32 at 9.9e-5 measured)."""
    model = _bench(name)
    batch = workloads.batch(name, 0, bs)
    out = {}
    try:
        model.att_leaves = leaves
        for fold in (0, 1):
            model.value_fold = fold
            out[fold] = _run(model, batch)
    finally:
        model.value_fold, model.att_leaves = 1, "canonical"
    dT = (out[0]["final_trans"] - out[1]["final_trans"]).abs().amax(dim=(1, 2))
    flips = (out[0]["final_labels"] != out[1]["final_labels"]).sum(dim=1)
    print(name, bs, leaves, "max dT", float(dT.max()), "label flips", flips.tolist())
    assert torch.isfinite(out[1]["final_trans"]).all()
    assert int(flips.sum()) == 0, flips.tolist()
    assert int((dT >= 1e-5).sum()) <= max(1, bs // 8), dT.tolist()
    assert float(dT.max()) < 1e-4


@pytest.mark.gpu
def test_folded_forward_is_batch_invariant_and_repeatable():
    """The canonical leaf form with the fold: a pair's bits do not depend on the batch (the four-wavefront and the one-wavefront
    folded layer kernels agree bit for bit), and repeated calls agree."""
    model = _bench("n5000_b32")
    batch = workloads.batch("n5000_b32", 0, 32)
    big = _run(model, batch)
    for bs in (1, 4):
        small = _run(model, {k: v[:bs] for k, v in batch.items()})
        assert torch.equal(small["final_trans"].view(torch.int32), big["final_trans"][:bs].view(torch.int32)), bs
        assert torch.equal(small["final_labels"], big["final_labels"][:bs]), bs
    again = _run(model, batch)
    assert torch.equal(again["final_trans"].view(torch.int32), big["final_trans"].view(torch.int32))


@pytest.mark.gpu
def test_folded_key_split_forward_over_the_fp32_matrix_treats_a_pair_alone_as_in_a_batch(lib):
    """The per-launch key split with the fold over the fp32 spatial-consistency matrix below 48 query blocks of 256: the 4-wave,
    fp32-compat, 64-wide key-split instantiation of the attention kernel, which no other test launches.  N = 255 is the smallest
    class with a key split above one (8 key tiles, the last one ragged); one pair and two pairs get the same split there, so a
    pair's arithmetic does not depend on the batch: bit equality with the pairs run one at a time."""
    n, bs = 255, 2
    assert lib.pdsc_attention_split_default_split(1, n) == lib.pdsc_attention_split_default_split(bs, n) == 2
    model = _bench("n1000_b1")
    model.att_leaves, model.compat_format, model.value_fold = "per_launch", "f32", 1
    batch = synthetic.make_batch(bs, n, seed=255, inlier_ratio=0.3)
    both = _run(model, batch)
    assert torch.isfinite(both["final_trans"]).all()
    for i in range(bs):
        one = _run(model, {k: v[i:i + 1] for k, v in batch.items()})
        assert torch.equal(one["final_trans"].view(torch.int32), both["final_trans"][i:i + 1].view(torch.int32)), i
        assert torch.equal(one["final_labels"], both["final_labels"][i:i + 1]), i


@pytest.mark.gpu
def test_fold_leaves_calls_beyond_its_size_bound_on_the_128_channel_path():
    """N = 20000 > PDSC_VALUE_FOLD_MAX_N: value_fold 1 and 0 give the same bits."""
    model = _bench("multiway_n20000_b1")
    batch = workloads.batch("multiway_n20000_b1", 0, 1)
    out = {}
    try:
        for fold in (0, 1):
            model.value_fold = fold
            out[fold] = _run(model, batch)
    finally:
        model.value_fold = 1
    assert torch.equal(out[0]["final_trans"].view(torch.int32), out[1]["final_trans"].view(torch.int32))
    assert torch.equal(out[0]["final_labels"], out[1]["final_labels"])
