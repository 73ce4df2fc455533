"""The fp16 range sentinel on every route of the forward, one conversion site at a time.

Contract (include/pointdsc_hip.h, INTEGRATION.md, pdsc_common.h): every forward of the split-precision arithmetic carries a
device-side sentinel; a pair one of whose activations reaches 65504 on its way into an fp16 hi / lo pair gets a non-zero word in the
workspace entry "range_flag" and a NaN pose, never a plausible wrong one; the other pairs of the batch are untouched.

Reference: tests/range_oracle.py -- the encoder of one pair in float64 on the CPU, the largest |value| of every operand kind, and
which kinds the kernels of a route convert.  The recipes (same file) push ONE kind out of range, so a route test fails when the
note of that kind's conversion site is missing from the kernel that ran; each test asserts through the library's own planners that
its shape reaches the kernel it names.  The library is taken alone (range_guard = "off", weights packed and the first-input probe
marked done: the probe would catch the recipes, which is its job); the module's guard has its own tests at the end.
"""
import ctypes as C
import warnings

import pytest
import torch

import range_oracle as R
from pointdsc_amd import synthetic
from pointdsc_amd.model import PointDSC

DEV = "cuda:0"
INPUTS = ("corr_pos", "src_keypts", "tgt_keypts")
HOT_SEED = 3
ALL = tuple(R.RECIPES)

# route -> module attributes, shape, the oracle's operand list, recipes, positions of the hot pairs
ROUTES = {
    "coop_folded": dict(attrs={}, bs=2, n=400, kinds="folded", recipes=ALL, hot=(0,)),
    "coop_unfolded": dict(attrs=dict(value_fold=0), bs=2, n=400, kinds="unfolded", recipes=ALL, hot=(1,)),
    "pipelined": dict(attrs={}, bs=81, n=1024, kinds="folded", recipes=ALL, hot=(0, 40, 80)),
    "pipelined_unfolded": dict(attrs=dict(value_fold=0), bs=81, n=1024, kinds="unfolded", recipes=ALL, hot=(1, 41, 79)),
    "per_launch_split_1": dict(attrs=dict(att_leaves="per_launch"), bs=2, n=200, kinds="unfolded", recipes=("benign", "k", "hidden 2"), hot=(1,)),
    "per_launch_split_9": dict(attrs=dict(att_leaves="per_launch"), bs=1, n=2053, kinds="unfolded", recipes=("benign", "k", "hidden 2"), hot=(0,)),
    "f32_block": dict(attrs=dict(layer_gemm="f32"), bs=2, n=400, kinds="f32", recipes=("benign", "PointCN", "q", "k", "v"), hot=(0,)),
    "f32_wave": dict(attrs=dict(layer_gemm="f32"), bs=10, n=1000, kinds="f32", recipes=("benign", "PointCN", "q", "k", "v"), hot=(0, 9)),
}
ROUTE_CASES = [(route, recipe, ch) for route, spec in ROUTES.items() for recipe in spec["recipes"] for ch in R.channels(recipe)]
RECIPE_CASES = [(recipe, ch) for recipe in ALL for ch in R.channels(recipe)]


# ------------------------------------------------------------------------------------------------------------------------
# shared, computed once: weights, pairs, the oracle's verdicts
# ------------------------------------------------------------------------------------------------------------------------
_BASE, _PAIRS, _KINDS, _MODELS = [], {}, {}, {}


def base_state_dict():
    if not _BASE:
        _BASE.append(synthetic.make_state_dict(PointDSC(num_layers=R.LAYERS, **R.KW).state_dict(), seed=R.WSEED))
    return _BASE[0]


def pair(n, seed):
    if (n, seed) not in _PAIRS:
        _PAIRS[(n, seed)] = synthetic.make_pair(n, inlier_ratio=0.4, seed=seed)
    return _PAIRS[(n, seed)]


def kinds_of(recipe, ch, n, seed, hot):
    key = (recipe, ch, n, seed, hot)
    if key not in _KINDS:
        p = R.recipe_input(pair(n, seed), recipe, hot)
        _KINDS[key] = R.encoder_kinds(R.recipe_state_dict(base_state_dict(), recipe, ch), p["corr_pos"][0], p["src_keypts"][0], p["tgt_keypts"][0])
    return _KINDS[key]


def decisive(kinds, route_kinds):
    """The oracle's verdict on a pair, asserted to be far from the bound: every kind of the route <= 3e4, or one >= 7e4."""
    vals = {k: kinds[k] for k in R.ROUTE_KINDS[route_kinds]}
    assert all(v <= R.OTHERS_MAX or v >= R.TARGET_MIN for v in vals.values()), vals
    return R.expected_flag(kinds, route_kinds)


def batch_of(recipe, bs, n, hot):
    """bs pairs: seed 3 with the recipe's hot input at the positions `hot`, seeds 4 / 5 with its cold input elsewhere.
    Returns (batch, [(seed, is_hot)])."""
    who = [(HOT_SEED, True) if i in hot else (4 + i % 2, False) for i in range(bs)]
    pairs = [R.recipe_input(pair(n, seed), recipe, is_hot) for seed, is_hot in who]
    return {k: torch.cat([p[k] for p in pairs]).contiguous() for k in INPUTS}, who


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the recipes isolate what they claim
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,ch", RECIPE_CASES)
def test_recipes_isolate_one_kind(recipe, ch):
    """fp64, N = 400, seed 3, both channel variants: on the folded and on the unfolded operand list the target kind is >= 7e4 and every other kind <= 3e4
    (kinds the target implies excepted: range_oracle.py says which and why); a list that does not hold the target stays in range;
    every folded weight is below the packing check's 3e4.  The cold input is in range where the recipe says so, and hot where the
    overflow comes from a bias (such a recipe flags every pair of a batch)."""
    spec = R.RECIPES[recipe]
    hot, cold = kinds_of(recipe, ch, 400, HOT_SEED, True), kinds_of(recipe, ch, 400, HOT_SEED, False)
    print(recipe, ch, {k: f"{v:.3g}" for k, v in hot.items()})
    assert abs(hot["hidden 1"] - hot["hidden 1 folded"]) <= 1e-9 * max(1.0, hot["hidden 1"])
    assert R.folded_weight_max(R.recipe_state_dict(base_state_dict(), recipe, ch)) < R.WEIGHT_MAX
    targets = (spec["target"], f"{spec['target']} folded")
    for route in ("folded", "unfolded"):
        for kind in R.ROUTE_KINDS[route]:
            if kind in targets:
                assert hot[kind] >= R.TARGET_MIN, (route, kind, hot[kind])
            elif kind not in spec["implies"]:
                assert hot[kind] <= R.OTHERS_MAX, (route, kind, hot[kind])
        assert decisive(hot, route) == any(k in targets for k in R.ROUTE_KINDS[route])
        assert decisive(cold, route) == (decisive(hot, route) and spec.get("every_pair", False)), (route, cold)
    assert R.expected_flag(hot, "f32") == (recipe in ("PointCN", "q", "k", "v"))


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pointdsc_amd import build
    build.build(verbose=False)
    from pointdsc_amd import _lib
    return _lib.load()


def library_model(recipe, ch, attrs):
    """The 2-layer model of a recipe's channel variant (or of "boundary") with `attrs` set, weights packed, the first-input probe
    marked done, the guard off; cached."""
    key = (recipe, ch, tuple(sorted(attrs.items())))
    if key not in _MODELS:
        model = PointDSC(num_layers=R.LAYERS, **R.KW)
        model.load_state_dict(boundary_state_dict() if recipe == "boundary" else R.recipe_state_dict(base_state_dict(), recipe, ch))
        model = model.eval().to(DEV)
        for a, v in attrs.items():
            setattr(model, a, v)
        model.range_guard = "off"
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # the weight check at packing must not fall back
            model.packed_weights(torch.device(DEV))
        model._h3_range_checked = True
        _MODELS[key] = model
    return _MODELS[key]


def run(model, batch, testing=True, counts=None):
    """One forward of the library alone; (final_trans, final_labels, range words) on the host."""
    want = (model.attention_precision, model.layer_gemm)
    data = {k: batch[k].to(DEV).contiguous() for k in INPUTS}
    if testing:
        data["testing"] = True
    if counts is not None:
        data["num_corr"] = counts
    with torch.no_grad():
        res = model(data)
    torch.cuda.synchronize()
    assert (model.attention_precision, model.layer_gemm) == want == ("fp16x3", want[1]) and model._h3_range_checked
    bs, n = batch["corr_pos"].shape[:2]
    flags = model.workspace_view("range_flag", bs, n, torch.int32)[:bs].cpu().tolist()
    return res["final_trans"].cpu(), res["final_labels"].cpu(), flags


def assert_route(lib, route):
    """The shape of `route` reaches the kernel its name says, by the library's own planners."""
    spec = ROUTES[route]
    bs, n = spec["bs"], spec["n"]
    ns, nl = C.c_int(), C.c_int()
    split = lib.pdsc_attention_split_default_split(bs, n)
    if route.startswith("f32"):
        assert lib.pdsc_layer_prefers_block(bs, n) == (1 if route == "f32_block" else 0), (bs, n)
        return
    assert lib.pdsc_layer_h3_uses_coop(bs, n) == (0 if route.startswith("pipelined") else 1), (bs, n)
    if route.startswith("pipelined"):
        assert bs * -(-n // 32) == 2592 > 2560
    if route == "per_launch_split_1":
        assert split == 1, split                   # no partials to merge: the layer kernel reads msg rows
    elif route == "per_launch_split_9":
        assert split > 8, split                    # more than the H3 kernels merge (MERGE_MAX_SPLIT_H3): combine launch + msg rows
    else:
        assert lib.pdsc_attention_leaf_plan(bs, n, 1, C.byref(ns), C.byref(nl)) == 0 and nl.value == lib.pdsc_attention_leaf_count(n)


def test_route_shapes_reach_their_kernels(lib):
    for route in ROUTES:
        assert_route(lib, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route,recipe,ch", ROUTE_CASES)
def test_flags_follow_the_oracle_on_every_route(lib, route, recipe, ch):
    """Per pair: the range word equals the fp64 oracle's verdict on the operands of the route that ran; flagged pairs have an
    all-NaN pose; unflagged pairs equal, bit for bit, the same pairs in a batch whose hot pairs got their cold input."""
    assert_route(lib, route)
    spec = ROUTES[route]
    bs, n = spec["bs"], spec["n"]
    model = library_model(recipe, ch, spec["attrs"])
    batch, who = batch_of(recipe, bs, n, spec["hot"])
    want = [int(decisive(kinds_of(recipe, ch, n, seed, hot), spec["kinds"])) for seed, hot in who]
    trans, labels, flags = run(model, batch)
    print(route, recipe, ch, "flags", flags)
    assert [int(f != 0) for f in flags] == want, (flags, want)
    if recipe == "benign":
        assert not any(want)
    elif R.RECIPES[recipe]["target"] in R.ROUTE_KINDS[spec["kinds"]] or f"{R.RECIPES[recipe]['target']} folded" in R.ROUTE_KINDS[spec["kinds"]]:
        assert all(want[i] for i in spec["hot"])
    calm, calm_who = batch_of(recipe, bs, n, ())
    calm_want = [int(decisive(kinds_of(recipe, ch, n, seed, hot), spec["kinds"])) for seed, hot in calm_who]
    ctrans, clabels, cflags = run(model, calm)
    assert [int(f != 0) for f in cflags] == calm_want, (cflags, calm_want)
    for i in range(bs):
        if want[i]:
            assert bool(torch.isnan(trans[i]).all()), (i, trans[i])
        else:
            assert bool(torch.isfinite(trans[i]).all()), (i, trans[i])
            if i not in spec["hot"]:
                assert not calm_want[i]
                assert torch.equal(trans[i], ctrans[i]) and torch.equal(labels[i], clabels[i]), i


@pytest.mark.gpu
def test_validation_forward_returns_nan_for_a_flagged_pair(lib):
    """The validation forward (eval mode, no 'testing' key) has no refinement launch: the flagged pair's pose must be NaN all the
    same; the other pair is the pair of its call alone, bit for bit."""
    model = library_model("k", R.CHANNELS[0], {})
    batch, who = batch_of("k", 2, 400, (0,))
    want = [int(decisive(kinds_of("k", R.CHANNELS[0], 400, seed, hot), "folded")) for seed, hot in who]
    assert want == [1, 0]
    trans, labels, flags = run(model, batch, testing=False)
    assert [int(f != 0) for f in flags] == want, flags
    assert bool(torch.isnan(trans[0]).all()) and bool(torch.isfinite(trans[1]).all()), trans
    alone = {k: batch[k][1:2] for k in INPUTS}
    atrans, alabels, aflags = run(model, alone, testing=False)
    assert aflags == [0]
    assert torch.equal(trans[1], atrans[0]) and torch.equal(labels[1], alabels[0])


def boundary_state_dict(channel=5, coord=2):
    """Channel `channel` of layer0 := corr_pos[:, coord] exactly (unit row, bias 0), no other channel of layer0 reads that
    coordinate, and PointCN_layer_0 does not read that channel: only the head-only launch's conversion of feat_in sees the value."""
    sd = {k: v.clone() for k, v in base_state_dict().items()}
    sd["encoder.layer0.weight"][:, coord] = 0.0
    sd["encoder.layer0.weight"][channel] = 0.0
    sd["encoder.layer0.weight"][channel, coord, 0] = 1.0
    sd["encoder.layer0.bias"][channel] = 0.0
    sd["encoder.blocks.PointCN_layer_0.0.weight"][:, channel] = 0.0
    return sd


@pytest.mark.gpu
@pytest.mark.parametrize("route,b,row", [("coop_folded", 1, 399), ("pipelined", 40, 1023)])
def test_the_bound_is_exact(lib, route, b, row):
    """One coordinate equal to 65504.0 flags its pair; the next float below does not, and the pose is then bit-identical to the
    pose with that coordinate at 0 (the value meets a zero weight column and nothing else)."""
    assert_route(lib, route)
    spec = ROUTES[route]
    bs, n = spec["bs"], spec["n"]
    model = library_model("boundary", None, {})
    batch, _ = batch_of("benign", bs, n, ())
    below = float(torch.nextafter(torch.tensor(65504.0, dtype=torch.float32), torch.tensor(0.0, dtype=torch.float32)))
    assert below == 65504.0 - 2.0 ** -8                # the fp32 neighbour, not the fp64 one
    out = {}
    for name, value in (("at", 65504.0), ("below", below), ("zero", 0.0)):
        x = {k: v.clone() for k, v in batch.items()}
        x["corr_pos"][b, row, 2] = value
        out[name] = run(model, x)
    want = [int(i == b) for i in range(bs)]
    assert [int(f != 0) for f in out["at"][2]] == want, out["at"][2]
    assert bool(torch.isnan(out["at"][0][b]).all())
    assert not any(out["below"][2]) and not any(out["zero"][2]), (out["below"][2], out["zero"][2])
    assert bool(torch.isfinite(out["below"][0]).all())
    assert torch.equal(out["below"][0], out["zero"][0]) and torch.equal(out["below"][1], out["zero"][1])
    others = [i for i in range(bs) if i != b]
    assert torch.equal(out["at"][0][others], out["zero"][0][others])


PADDING = {
    "coop_folded": [480, 300, 225],
    "f32_block": [480, 300, 225],
    "f32_wave": [1000, 997, 1000, 993, 1000, 1000, 999, 1000, 1000, 1000],
}


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(PADDING))
def test_padding_rows_cannot_raise_a_flag(lib, route):
    """Ragged batch as padded tensors + num_corr: the padding rows may hold any values.  1e30 there, in corr_pos and in the
    keypoints, raises no flag and changes no bit against the same batch padded with NaN (which v_max3 ignores anyway)."""
    counts = PADDING[route]
    bs, n = len(counts), max(counts)
    if route == "coop_folded":
        assert lib.pdsc_layer_h3_uses_coop(bs, n) == 1
    else:
        assert lib.pdsc_layer_prefers_block(bs, n) == (1 if route == "f32_block" else 0)
    model = library_model("benign", None, ROUTES[route]["attrs"])
    groups = model._ragged_groups(list(counts))
    assert len(groups) == 1 and sorted(groups[0]) == list(range(bs)), groups      # one launch: the words read below are the whole batch's
    out = {}
    for fill in (float("nan"), 1.0e30):
        pad = {k: torch.full((bs, n, pair(n, 4)[k].shape[-1]), fill) for k in INPUTS}
        for i, c in enumerate(counts):
            for k in INPUTS:
                pad[k][i, :c] = pair(c, 10 + i)[k][0]
        out[fill != fill] = run(model, pad, counts=list(counts))
    assert not any(out[True][2]) and not any(out[False][2]), (out[True][2], out[False][2])
    assert bool(torch.isfinite(out[False][0]).all())
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["coop_folded", "f32_block"])
def test_nan_in_a_valid_row_is_not_an_overflow(lib, route):
    """pdsc_common.h: a NaN input is not an overflow and propagates on its own -- no flag, and the other pair does not move."""
    spec = ROUTES[route]
    model = library_model("benign", None, spec["attrs"])
    batch, _ = batch_of("benign", 2, 400, ())
    clean = run(model, batch)
    x = {k: v.clone() for k, v in batch.items()}
    x["corr_pos"][0, 5, 2] = float("nan")
    trans, labels, flags = run(model, x)
    assert flags == [0, 0] and clean[2] == [0, 0], (flags, clean[2])
    assert torch.equal(trans[1], clean[0][1]) and torch.equal(labels[1], clean[1][1])


def _module(attrs):
    model = PointDSC(num_layers=R.LAYERS, **R.KW)
    model.load_state_dict(base_state_dict())
    model = model.eval().to(DEV)
    for a, v in attrs.items():
        setattr(model, a, v)
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["f32_block", "per_launch_split_1"])
def test_module_guard_falls_back_on_these_routes_too(lib, route):
    """The "sync" and the "lazy" part of test_range_guard_catches_a_later_input_that_leaves_the_fp16_range (test_gpu_parity.py) on
    a route whose launches carried no sentinel: a benign first batch, then one scaled by 1e5 -- the call warns, the module switches
    to exact fp32 and "sync" returns, bit for bit, what a module set to fp32 from the start returns."""
    assert_route(lib, route)
    spec = ROUTES[route]
    attrs = spec["attrs"]
    small = batch_of("benign", spec["bs"], spec["n"], ())[0]
    big = {k: v * 1.0e5 for k, v in batch_of("benign", spec["bs"], spec["n"], (0,))[0].items()}

    def forward(model, batch):
        with torch.no_grad():
            res = model(dict({k: batch[k].to(DEV).contiguous() for k in INPUTS}, testing=True))
        torch.cuda.synchronize()
        return res

    model = _module(attrs)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # the benign batch must not warn
        first = forward(model, small)
    assert model.attention_precision == "fp16x3" and model.layer_gemm == attrs.get("layer_gemm", "h3") and model.range_fallbacks == 0
    assert bool(torch.isfinite(first["final_trans"]).all())
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        got = forward(model, big)
    assert model.attention_precision == "fp32" and model.layer_gemm == "f32" and model.range_fallbacks == 1
    ref = _module(attrs)
    ref.attention_precision, ref.layer_gemm = "fp32", "f32"
    want = forward(ref, big)
    assert bool(torch.isfinite(got["final_trans"]).all())
    assert torch.equal(got["final_trans"], want["final_trans"]) and torch.equal(got["final_labels"], want["final_labels"])
    # -- lazy, inside a pipeline
    from pointdsc_amd.pipeline import InFlight
    model = _module(attrs)
    pipe = InFlight(model, depth=2)
    d_small = dict({k: small[k].to(DEV).contiguous() for k in INPUTS}, testing=True)
    d_big = dict({k: big[k].to(DEV).contiguous() for k in INPUTS}, testing=True)
    r0 = pipe(d_small)
    r1 = pipe(d_big)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        pipe.synchronize()
        model.check_range()
    assert bool(torch.isfinite(r0["final_trans"]).all()) and bool(torch.isnan(r1["final_trans"]).all())
    assert model.attention_precision == "fp32" and model.range_fallbacks == 1
    r2 = pipe(d_big)
    pipe.synchronize()
    assert torch.equal(r2["final_trans"], want["final_trans"])
    pipe.close()
