"""The attention's leaf form with the merge inside the workgroup.

A workgroup that owns every leaf of its query block (key split 1) runs the layer kernel's flat merge itself -- the row weights and
the fmaf chain of merge_partials.h over the leaf partials it stored, in leaf order -- and leaves ONE partial (the un-normalised
chain sum with m = 0, l = the merge's denominator) in the pair's leaf-0 slot; the layer launch merges that one partial, which
reproduces the many-way merge bit for bit.  With any other key split the layer kernel merges the leaves, as it always has.  So the
key split (pdsc_attention_leaf_split_override: every divisor of the leaf count) must not move a single bit of the forward.
"""
import ctypes as C

import pytest
import torch

from pointdsc_amd import PointDSC, _lib, synthetic

DEV = "cuda:0"
KW = dict(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
          sigma_d=0.10, k=40, nms_radius=0.10)
# N -> canonical leaves: 257 (9 tiles) 2; 700 (22 tiles: leaves of 6, 6, 5, 5, ragged last tile, last query block 188 rows) 4;
# 1000 (32 tiles) 8; 2053 (65 tiles: 17, 16, 16, 16) 4
LEAVES = {257: 2, 700: 4, 1000: 8, 2053: 4}
_MODEL = {}


def _model():
    if not _MODEL:
        model = PointDSC(**KW)
        model.load_state_dict(synthetic.make_state_dict(model.state_dict(), seed=6))
        _MODEL["m"] = model.eval().to(DEV)
    return _MODEL["m"]


def _divisors(c):
    return [d for d in range(1, c + 1) if c % d == 0]


def _data(batch, bs, testing):
    data = {k: batch[k][:bs].to(DEV).contiguous() for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    if testing:
        data["testing"] = True
    return data


def _outputs(model, data):
    """(final_trans, final_labels) of the testing forward, (M, final_labels) of the validation forward, as int32 bit patterns"""
    with torch.no_grad():
        res = model(data)
    torch.cuda.synchronize()
    first = res["final_trans"] if "testing" in data else res["M"]
    labels = res["final_labels"]
    labels = torch.cat([x.reshape(-1) for x in labels]) if isinstance(labels, list) else labels
    return first.clone().view(torch.int32), labels.clone().view(torch.int32)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture
def hook():
    lib = _lib.load()
    model = _model()
    saved = (model.value_fold, model.compat_format, model.att_leaves)
    try:
        yield lib
    finally:
        lib.pdsc_attention_leaf_split_override(0)
        model.value_fold, model.compat_format, model.att_leaves = saved


def _set(lib, d):
    _lib.check(lib.pdsc_attention_leaf_split_override(d), "pdsc_attention_leaf_split_override")


def test_leaf_split_override_is_honoured_by_the_plan():
    """Host side (no GPU): 0 = the planner's own rule, a divisor of the leaf count is taken as the key split, anything else is an
    error of the call that plans -- where the leaf count is known -- and the leaf count itself never moves."""
    from pointdsc_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    ns, nl = C.c_int(), C.c_int()
    try:
        for n, leaves in LEAVES.items():
            for d in _divisors(leaves):
                assert lib.pdsc_attention_leaf_split_override(d) == 0
                for bs in (1, 3, 16, 32):
                    assert lib.pdsc_attention_leaf_plan(bs, n, 1, C.byref(ns), C.byref(nl)) == 0
                    assert (ns.value, nl.value) == (d, leaves), (n, bs, d)
        assert lib.pdsc_attention_leaf_split_override(3) == 0
        assert lib.pdsc_attention_leaf_plan(1, 700, 1, C.byref(ns), C.byref(nl)) != 0 and b"divide" in lib.pdsc_last_error()
        assert lib.pdsc_attention_leaf_split_override(-1) != 0 and lib.pdsc_attention_leaf_split_override(9) != 0
        assert lib.pdsc_attention_leaf_split_override(0) == 0
        for bs in (1, 4, 8, 16, 32):
            assert lib.pdsc_attention_leaf_plan(bs, 5000, 1, C.byref(ns), C.byref(nl)) == 0
            assert nl.value == 4 and 4 % ns.value == 0
    finally:
        lib.pdsc_attention_leaf_split_override(0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bs", [(257, 1), (257, 3), (700, 1), (700, 3), (700, 16), (1000, 1), (1000, 3), (1000, 13), (2053, 1), (2053, 3)])
def test_every_key_split_of_the_leaf_form_returns_the_same_bits(n, bs, hook):
    """Testing forward (final_trans, final_labels) and validation forward (M = a function of every feature channel of every
    correspondence, and the logits) under every divisor of the leaf count, both value widths, both compat formats.  d = 1 is the
    in-workgroup merge followed by the layer kernels' one-partial instantiation; every other d is the layer kernels' own merge."""
    model = _model()
    batch = synthetic.make_batch(bs, n, seed=900 + n, inlier_ratio=0.3)
    for fold in (1, 0):
        for fmt in ("u16", "f32"):
            model.value_fold, model.compat_format = fold, fmt
            for testing in (True, False):
                data = _data(batch, bs, testing)
                outs = {}
                for d in _divisors(LEAVES[n]):
                    _set(hook, d)
                    outs[d] = _outputs(model, data)
                ref = outs[LEAVES[n]]
                for d, got in outs.items():
                    assert _same(got, ref), (n, bs, fold, fmt, testing, d)


@pytest.mark.gpu
def test_ragged_batch_under_every_key_split(hook):
    """Pairs of 700 and 650 correspondences in one launch (both 4 leaves): every pair cuts ITS OWN tiles into leaves, and the
    workgroups past a pair's rows leave nothing for the layer kernel to read."""
    model = _model()
    big, small = synthetic.make_pair(700, inlier_ratio=0.3, seed=31), synthetic.make_pair(650, inlier_ratio=0.3, seed=32)
    keys = ("corr_pos", "src_keypts", "tgt_keypts")
    data = {k: [big[k].reshape(700, -1).to(DEV), small[k].reshape(650, -1).to(DEV), big[k].reshape(700, -1).to(DEV)] for k in keys}
    data["testing"] = True
    outs = {}
    for d in (1, 2, 4):
        _set(hook, d)
        outs[d] = _outputs(model, data)
    assert _same(outs[1], outs[4]) and _same(outs[2], outs[4])


@pytest.mark.gpu
def test_ten_merged_forwards_return_one_result(hook):
    model = _model()
    batch = synthetic.make_batch(3, 700, seed=77, inlier_ratio=0.3)
    _set(hook, 1)
    for testing in (True, False):
        data = _data(batch, 3, testing)
        first = _outputs(model, data)
        for _ in range(9):
            assert _same(_outputs(model, data), first), testing


@pytest.mark.gpu
@pytest.mark.parametrize("n,bs", [(700, 3), (1000, 1)])
def test_merged_path_reads_only_what_it_wrote(n, bs, hook):
    """att_scratch filled with NaN before the forward: the merging workgroup reads back its own leaf partials and nothing else, and
    the layer launch reads the merged slot of the tiles that hold rows and nothing else -- any other read would poison the result."""
    lib = hook
    model = _model()
    batch = synthetic.make_batch(bs, n, seed=55 + n, inlier_ratio=0.3)
    data = _data(batch, bs, True)
    for d in _divisors(LEAVES[n]):
        _set(lib, d)
        want = _outputs(model, data)
        cfg = model._config()
        off = {name: int(lib.pdsc_workspace_offset(C.byref(cfg), bs, n, int(n * model.ratio), name)) for name in (b"att_scratch", b"q_split")}
        assert 0 <= off[b"att_scratch"] < off[b"q_split"]
        scratch = model._workspace[off[b"att_scratch"]:off[b"q_split"]]
        scratch[: scratch.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
        got = _outputs(model, data)
        assert not torch.isnan(got[0].view(torch.float32)).any()
        assert _same(got, want), (n, bs, d)
