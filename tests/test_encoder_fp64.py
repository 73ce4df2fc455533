"""The shipped encoder path -- split-precision attention in leaf form, H3 layer GEMMs, point-fragment hand-offs, the 64-channel
value fold over a unorm16 compat matrix -- against the same encoder evaluated in fp64, layer by layer.

None of those kernels has a C entry point of its own (plan_encoder is the only way in), so the fp64 stage tests of
test_gpu_parity.py never reach them, and the whole-path tests compare our kernels with each other or with the fp32 oracle at
3e-5 after 12 layers.  With the seeded Xavier weights the attention is almost uniform (largest |logit| 0.46, largest softmax weight
1.5 / N): the running maximum, the online rescale and the leaf merge weights are all ~1 there, and a defect in the key dimension
hides.  test_reference_discriminates_deliberate_defects records it: in that regime two swapped compat columns move the 12-layer
features by less than 3e-5 of scale -- inside the old tolerance.  That is the reason this file exists.

Reference: oracle.encoder with every floating tensor cast to float64 (`collect` = the features after every layer).  The fp32
call of the same function on the same inputs is the YARDSTICK, never the reference.  Metric: e(x) = max|x - ref64| / max(1,
max|ref64|) over the valid rows.  Bound of a case: K * e(fp32 oracle) of that case and layer, K_SPLIT for the split-precision
modes and K_EXACT for exact fp32 ("Encoder against fp64": where the two come from, and the ratio table;
every GPU check prints its ratio e_gpu / e_fp32oracle before it asserts).

Weights: synthetic.make_state_dict(seed 6) with every projection_q / projection_k weight times `gain`; gain 1 is the regime of
every other test, gain 8 the sharp one (logits to +-28, one key taking 99.85 % of a row; activations stay below 3e4, so the range
probe keeps fp16x3 / h3 -- asserted after each forward).  The model is built with num_layers = L and loads the first L layers:
L = 1 isolates head(0) -> leaf attention -> folded tail, L = 2 adds the fused tail + head launch, L = 12 is the shipped depth.
With compat_format "u16" the reference is fed the decoded unorm16 matrix, so the matrix's own quantisation (bounded by its own
test) is not charged to the attention; the fp64 arithmetic on it stays independent.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pointdsc_oracle as O
from pointdsc_amd import synthetic
from pointdsc_amd.model import PointDSC

KW = dict(in_dim=6, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10)
WSEED, DEV = 6, "cuda:0"
DEPTHS = (1, 2, 12)
# bs = 1 sizes: a second tile of 9 keys, exact multiples of 32, every leaf-count boundary from both sides, Npad = 256 boundaries
SIZES = (41, 64, 224, 225, 257, 480, 481, 992, 993, 1504, 1505)
LEAVES = (1, 1, 1, 2, 2, 2, 4, 4, 8, 8, 4)
RAGGED = ((480, 300, 225), (1504, 1200, 993))
BATCHES = ((12, 1000, 12), (81, 1024, 2))          # (bs, N, L): 8-wave attention workgroups / 2592 tiles = layer_h3_kernel
EXACT = dict(attention_precision="fp32", compat_format="f32", layer_gemm="f32")
# bound = K * e(fp32 oracle); DESIGN.md section 5 "Encoder against fp64" holds the table these come from
K_SPLIT = 8          # split precision: 2^-21 per product against fp32's 2^-24
K_EXACT = 4          # exact fp32: the yardstick's format in another summation order, hardware exp2 / rcp

_RATIOS = []


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
_SD = {}


def state_dict(gain):
    if gain not in _SD:
        sd = synthetic.make_state_dict(PointDSC(num_layers=12, **KW).state_dict(), seed=WSEED)
        for name in sd:
            if name.endswith(("projection_q.weight", "projection_k.weight")):
                sd[name] = sd[name] * float(gain)
        _SD[gain] = sd
    return _SD[gain]


def to64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def err(x, ref):
    return float((x.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def pair(n, seed=21):
    return synthetic.make_pair(n, inlier_ratio=0.3, seed=seed)


def cpu_compat(p):
    return O.spatial_compat(p["src_keypts"][0], p["tgt_keypts"][0], torch.tensor([KW["sigma_d"]]))[1]


_REF = {}


def reference(key, gain, corr, compat, layers=12):
    """fp64 encoder on (corr [N,6], compat [N,N] fp32) and the fp32 oracle's error against it, per layer; computed once per key.
    Returns dict(feat=[L x [N,128] fp64], normed, conf (of the last layer), e32=[L], e32_normed, e32_conf)."""
    key = (key, gain, layers)
    if key not in _REF:
        sd = state_dict(gain)
        sd64 = to64(sd)
        f64, f32 = [], []
        O.encoder(sd64, corr.double(), compat.double(), layers, 128, f64)
        O.encoder(sd, corr, compat, layers, 128, f32)
        normed, conf = O.l2_normalize(f64[-1]), O.classify(sd64, f64[-1])
        _REF[key] = dict(feat=f64, normed=normed, conf=conf, e32=[err(a, b) for a, b in zip(f32, f64)],
                         e32_normed=err(O.l2_normalize(f32[-1]), normed), e32_conf=err(O.classify(sd, f32[-1]), conf))
    return _REF[key]


@pytest.fixture(scope="module")
def built_lib():
    from pointdsc_amd import build
    build.build(verbose=False)
    from pointdsc_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the reference's precision, its power to discriminate, and what the shapes reach
# ------------------------------------------------------------------------------------------------------------------------
CPU_CASES = [(n, 8) for n in sorted(set(SIZES + (33, 1000, 1024) + sum(RAGGED, ())))] + [(257, 1), (1000, 1)]


@pytest.mark.parametrize("n,gain", CPU_CASES)
def test_fp32_oracle_lies_within_5e6_of_the_fp64_encoder(n, gain):
    """The yardstick is fp32 round-off and nothing else: at most 1.6e-6 at gain 8 and 1e-6 at gain 1 measured, at every depth."""
    p = pair(n)
    r = reference(("cpu", n), gain, p["corr_pos"][0], cpu_compat(p))
    print(f"N={n} gain={gain}: e(fp32 oracle) L=1 {r['e32'][0]:.2e}  L=2 {r['e32'][1]:.2e}  L=12 {r['e32'][11]:.2e}")
    assert len(r["e32"]) == 12 and all(0.0 < e < 5e-6 for e in r["e32"]), r["e32"]
    assert r["e32_normed"] < 5e-6 and r["e32_conf"] < 5e-6


def _leaves_without_maxima(leaves):
    """Softmax over the keys cut into `leaves` runs of whole 32-key tiles, every run normalised to ITS OWN maximum and the runs
    then summed as if they shared one: a leaf merge that drops the weights exp(m_leaf - max m)."""
    def weights(s):
        tiles = (s.shape[1] + 31) // 32
        cuts = [32 * ((tiles * i) // leaves) for i in range(leaves)] + [s.shape[1]]
        p = torch.cat([torch.exp(s[:, a:b] - s[:, a:b].max(dim=-1, keepdim=True).values) for a, b in zip(cuts, cuts[1:])], dim=-1)
        return p / p.sum(dim=-1, keepdim=True)
    return weights


def _encoder_with(sd, corr, compat, num_layers, weights):
    """oracle.encoder with the softmax replaced by `weights(logits)`."""
    feat = O._conv(sd, "encoder.layer0", corr.t())
    for i in range(num_layers):
        p, nl = f"encoder.blocks.PointCN_layer_{i}", f"encoder.blocks.NonLocal_layer_{i}"
        feat = torch.relu(O._bn(sd, p + ".1", O._conv(sd, p + ".0", feat)))
        q, k, v = (O._conv(sd, f"{nl}.projection_{x}", feat) for x in "qkv")
        m = (weights(compat * ((q.t() @ k) / 128 ** 0.5)) @ v.t()).t().contiguous()
        m = torch.relu(O._bn(sd, nl + ".fc_message.1", O._conv(sd, nl + ".fc_message.0", m)))
        m = torch.relu(O._bn(sd, nl + ".fc_message.4", O._conv(sd, nl + ".fc_message.3", m)))
        feat = feat + O._conv(sd, nl + ".fc_message.6", m)
    return feat.t().contiguous()


def _defective(defect, sd64, corr, compat, layers):
    n = corr.shape[0]
    if defect == "padding key":            # one extra key that is a copy of the last row (a leaked point-fragment padding row)
        corr = torch.cat([corr, corr[-1:]])
        compat = torch.cat([torch.cat([compat, compat[:, -1:]], dim=1), torch.cat([compat[-1:], compat[-1:, -1:]], dim=1)])
    elif defect == "column swap":          # two columns of one 32-group of the unorm16 tile order mistaken for each other
        compat = compat.clone()
        compat[:, [8, 9]] = compat[:, [9, 8]]
    elif defect == "missing bias term":    # b' = W1f bv + b1f without W1f bv: softmax rows sum to 1, so this is bv = 0
        sd64 = {k: torch.zeros_like(v) if k.endswith("projection_v.bias") else v for k, v in sd64.items()}
    elif defect == "merge without maxima":
        return _encoder_with(sd64, corr, compat, layers, _leaves_without_maxima(4))[:n]
    return O.encoder(sd64, corr, compat, layers, 128)[:n]


DEFECTS = [("padding key", 1000), ("padding key", 33), ("padding key", 1505), ("column swap", 1000), ("column swap", 33),
           ("merge without maxima", 1000), ("missing bias term", 1000)]


@pytest.mark.parametrize("defect,n", DEFECTS)
def test_reference_discriminates_deliberate_defects(defect, n):
    """Four defects of the kind the shared code (merge_partials.h, the fragment-stream builder, the fold builder, the unorm16 tile
    order) could carry, applied to the fp64 encoder at gain 8 and L = 1: each moves e by at least 10 times the bound a GPU case of
    that shape gets.  Measured e at L = 1 (N = 1000 / 33 / 1505): padding key 2.0e-3 / 2.0e-2 / 5.2e-4, column swap 7.9e-3 / 2.9e-2,
    merge without maxima 1.6e-1, missing bias term 4.6e-2.
    At gain 1 and L = 12 -- the regime of every other whole-path feature test -- the column swap moves e by less than 3e-5 (6.0e-6
    measured at N = 1000): below the 3e-5 tolerance of test_encoder_and_head_match_oracle.  That is the reason this file exists."""
    p = pair(n)
    corr, compat = p["corr_pos"][0], cpu_compat(p)
    r = reference(("cpu", n), 8, corr, compat)
    sd64 = to64(state_dict(8))
    if defect == "merge without maxima":   # the restated layer loop is the oracle's
        assert torch.equal(_encoder_with(sd64, corr.double(), compat.double(), 1, lambda s: torch.softmax(s, dim=-1)), r["feat"][0])
    moved = err(_defective(defect, sd64, corr.double(), compat.double(), 1), r["feat"][0])
    bound = max(K_SPLIT, K_EXACT) * r["e32"][0]
    print(f"{defect}, N={n}, gain 8, L=1: e = {moved:.2e}, bound of the case = {bound:.2e}")
    assert moved >= 10 * bound, (moved, bound)
    if defect == "column swap" and n == 1000:
        r1 = reference(("cpu", n), 1, corr, compat)
        quiet = err(_defective(defect, to64(state_dict(1)), corr.double(), compat.double(), 12), r1["feat"][11])
        print(f"{defect}, N={n}, gain 1, L=12: e = {quiet:.2e}")
        assert quiet < 3e-5, quiet


def test_shapes_reach_the_leaf_classes_and_both_layer_kernels(built_lib):
    ns, nl = C.c_int(), C.c_int()
    assert tuple(built_lib.pdsc_attention_leaf_count(n) for n in SIZES) == LEAVES
    splits = {}
    for bs, n in [(1, n) for n in SIZES + (1000,)] + [(b, n) for b, n, _ in BATCHES] + [(3, max(c)) for c in RAGGED]:
        assert built_lib.pdsc_attention_leaf_plan(bs, n, 1, C.byref(ns), C.byref(nl)) == 0
        assert nl.value == built_lib.pdsc_attention_leaf_count(n) and nl.value % ns.value == 0
        splits[(bs, n)] = ns.value
        assert built_lib.pdsc_layer_h3_uses_coop(bs, n) == (0 if (bs, n) == (81, 1024) else 1), (bs, n)
    assert max(splits.values()) > 1 and min(splits.values()) == 1, splits      # workgroups that own one leaf and several leaves
    assert 81 * 1024 // 32 == 2592 > 2560                                       # layer_h3_coop_kernel takes at most 2560 tiles
    assert 12 * -(-1000 // 256) >= 48 > 1 * -(-1505 // 256)                     # 8-wave attention workgroups from 48 query blocks on
    for counts in RAGGED:
        assert len({built_lib.pdsc_attention_leaf_count(c) for c in counts}) == 1
        assert PointDSC(num_layers=1, **KW)._ragged_groups(list(counts)) == [[0, 1, 2]]


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_for(layers, gain):
    if (layers, gain) not in _MODELS:
        model = PointDSC(num_layers=layers, **KW)
        model.load_state_dict({k: state_dict(gain)[k] for k in model.state_dict()})
        _MODELS[(layers, gain)] = model.eval().to(DEV)
    return _MODELS[(layers, gain)]


def gpu_compat(fmt, src, tgt):
    """The matrix the attention of one pair streams, as fp32 [N,N] on the host: src / tgt [N,3]."""
    if fmt == "f32":
        return O.spatial_compat(src, tgt, torch.tensor([KW["sigma_d"]]))[1]
    from pointdsc_amd import ops
    s, t = src[None].to(DEV).contiguous(), tgt[None].to(DEV).contiguous()
    return ops.decode_compat_u16(ops.spatial_compat_u16(s, t, torch.tensor([KW["sigma_d"]], device=DEV)), src.shape[0])[0].cpu()


def forward(layers, gain, data, bs, n, **attrs):
    """One testing forward of the L-layer model with `attrs` set for its duration; returns (featA, normed, conf) as
    [bs,n,128] / [bs,n,128] / [bs,n] host tensors."""
    model = model_for(layers, gain)
    keep = {a: getattr(model, a) for a in attrs}
    try:
        for a, v in attrs.items():
            setattr(model, a, v)
        want = (model.attention_precision, model.layer_gemm)
        with torch.no_grad():
            model(dict({k: v.to(DEV).contiguous() if torch.is_tensor(v) else v for k, v in data.items()}, testing=True))
        torch.cuda.synchronize()
        # neither the range probe nor the range guard left the arithmetic under test
        assert (model.attention_precision, model.layer_gemm) == want and model.range_fallbacks == 0
        if want[0] != "fp32":
            assert max(model.last_range_probe.values()) < 3.0e4, model.last_range_probe
        view = lambda name, width: model.workspace_view(name, bs, n)[: bs * n * width].reshape(bs, n, width).cpu().clone()
        return view("featA", 128), view("normed", 128), view("conf", 1)[..., 0]
    finally:
        for a, v in keep.items():
            setattr(model, a, v)


def check(what, got, ref, yardstick, k):
    """e(got) against K times the fp32 oracle's own error of the same case and layer; the ratio is printed before it is judged."""
    e = err(got, ref)
    _RATIOS.append((what, e, yardstick, e / yardstick))
    print(f"RATIO {what}: e_gpu = {e:.2e}  e_fp32oracle = {yardstick:.2e}  ratio = {e / yardstick:.2f}  (k = {k})")
    assert e <= k * yardstick, (what, e, yardstick, e / yardstick)


def single(n, gain, fmt):
    p = pair(n)
    return p, reference((fmt, n), gain, p["corr_pos"][0], gpu_compat(fmt, p["src_keypts"][0], p["tgt_keypts"][0]))


INPUTS = ("corr_pos", "src_keypts", "tgt_keypts")


@pytest.mark.gpu
@pytest.mark.parametrize("layers", DEPTHS)
@pytest.mark.parametrize("n", SIZES)
def test_size_edges_match_fp64(n, layers):
    """bs = 1, gain 8, the default model (fp16x3, u16, h3, canonical leaves, fold 1) at every size edge of the leaf form."""
    p, r = single(n, 8, "u16")
    feat, _, _ = forward(layers, 8, {k: p[k] for k in INPUTS}, 1, n)
    check(f"default N={n} L={layers}", feat[0], r["feat"][layers - 1], r["e32"][layers - 1], K_SPLIT)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_size_edges_match_fp64_in_exact_mode(n):
    p, r = single(n, 8, "f32")
    feat, _, _ = forward(12, 8, {k: p[k] for k in INPUTS}, 1, n, **EXACT)
    check(f"exact N={n} L=12", feat[0], r["feat"][11], r["e32"][11], K_EXACT)


@pytest.mark.gpu
@pytest.mark.parametrize("layers", (1, 12))
@pytest.mark.parametrize("fmt", ("u16", "f32"))
@pytest.mark.parametrize("gain", (1, 8))
@pytest.mark.parametrize("n", (257, 1000))
def test_both_regimes_and_both_matrices_match_fp64(n, gain, fmt, layers):
    """Near-uniform and sharp attention over the unorm16 and the fp32 matrix; at the shipped depth the normalised features and the
    confidence logits too, each against K times the fp32 oracle's error of the same quantity."""
    p, r = single(n, gain, fmt)
    feat, normed, conf = forward(layers, gain, {k: p[k] for k in INPUTS}, 1, n, compat_format=fmt)
    what = f"N={n} gain={gain} {fmt} L={layers}"
    check("feat " + what, feat[0], r["feat"][layers - 1], r["e32"][layers - 1], K_SPLIT)
    if layers == 12:
        check("normed " + what, normed[0], r["normed"], r["e32_normed"], K_SPLIT)
        check("conf " + what, conf[0], r["conf"], r["e32_conf"], K_SPLIT)


@pytest.mark.gpu
@pytest.mark.parametrize("layers", (1, 12))
@pytest.mark.parametrize("n", (224, 257, 992, 1000, 1505))
def test_fold_and_leaf_form_really_ran(n, layers, built_lib):
    """One size per leaf class (1, 2, 4, 8 and the 4 of N >= 1505): the 128-channel value path gives other bits than the folded
    one, and so does the per-launch key split wherever its plan differs from the canonical leaves -- so the default forward above
    went through the fold and the leaf form -- and both variants meet the same fp64 bound."""
    p, r = single(n, 8, "u16")
    data = {k: p[k] for k in INPUTS}
    ref, yard = r["feat"][layers - 1], r["e32"][layers - 1]
    default = forward(layers, 8, data, 1, n)[0]
    unfolded = forward(layers, 8, data, 1, n, value_fold=0)[0]
    per_launch = forward(layers, 8, data, 1, n, att_leaves="per_launch")[0]
    check(f"fold 0 N={n} L={layers}", unfolded[0], ref, yard, K_SPLIT)
    check(f"per_launch N={n} L={layers}", per_launch[0], ref, yard, K_SPLIT)
    assert not torch.equal(default, unfolded), "value_fold = 1 ran the 128-channel path"
    ns, nl = C.c_int(), C.c_int()
    assert built_lib.pdsc_attention_leaf_plan(1, n, 1, C.byref(ns), C.byref(nl)) == 0
    if int(built_lib.pdsc_attention_split_default_split(1, n)) != nl.value:
        assert not torch.equal(default, per_launch), "att_leaves = 'canonical' summed like the per-launch key split"


@pytest.mark.gpu
@pytest.mark.parametrize("bs,n,layers", BATCHES)
def test_batch_routes_match_fp64(bs, n, layers, built_lib):
    """The launches a one-pair call never takes: 8-wave attention workgroups (bs * ceil(N / 256) >= 48) and layer_h3_kernel (more
    than 2560 tiles); pairs 0, bs // 2 and bs - 1 against the fp64 encoder of each alone."""
    assert bs * -(-n // 256) >= 48
    assert built_lib.pdsc_layer_h3_uses_coop(bs, n) == (0 if bs * n // 32 > 2560 else 1)
    assert built_lib.pdsc_layer_h3_uses_coop(bs, n) == (0 if layers == 2 else 1)
    batch = synthetic.make_batch(bs, n, seed=300, inlier_ratio=0.3)
    feat, _, _ = forward(layers, 8, {k: batch[k] for k in INPUTS}, bs, n)
    for i in (0, bs // 2, bs - 1):
        r = reference(("u16 batch", n, i), 8, batch["corr_pos"][i], gpu_compat("u16", batch["src_keypts"][i], batch["tgt_keypts"][i]), layers)
        check(f"batch bs={bs} N={n} L={layers} pair {i}", feat[i], r["feat"][layers - 1], r["e32"][layers - 1], K_SPLIT)


def _ragged_case(counts):
    """Padded tensors + num_corr; the padding rows of all three inputs hold finite non-zero values of the data's magnitude."""
    pairs = [pair(c, seed=40 + i) for i, c in enumerate(counts)]
    rs = np.random.RandomState(sum(counts))
    data = {"num_corr": list(counts)}
    for k in INPUTS:
        t = torch.from_numpy(rs.uniform(0.5, 3.0, (len(counts), max(counts), pairs[0][k].shape[-1])).astype(np.float32))
        for i, p in enumerate(pairs):
            t[i, : counts[i]] = p[k][0]
        data[k] = t
    return pairs, data


def _check_ragged(counts, layers, fmt, k, **attrs):
    pairs, data = _ragged_case(counts)
    model = model_for(layers, 8)
    keep = {a: getattr(model, a) for a in attrs}
    try:
        for a, v in attrs.items():
            setattr(model, a, v)
        assert len(model._ragged_groups(list(counts))) == 1             # one launch
    finally:
        for a, v in keep.items():
            setattr(model, a, v)
    feat, _, _ = forward(layers, 8, data, len(counts), max(counts), **attrs)
    for i, (c, p) in enumerate(zip(counts, pairs)):
        r = reference((fmt + " ragged", c, i), 8, p["corr_pos"][0], gpu_compat(fmt, p["src_keypts"][0], p["tgt_keypts"][0]))
        check(f"ragged {counts} {'exact ' if attrs else ''}L={layers} pair {i} (N={c})", feat[i, :c], r["feat"][layers - 1],
              r["e32"][layers - 1], k)


@pytest.mark.gpu
@pytest.mark.parametrize("layers", (1, 12))
@pytest.mark.parametrize("counts", RAGGED)
def test_ragged_batch_matches_fp64_of_each_pair_alone(counts, layers):
    """One launch over pairs of unequal length: rows past a pair's count -- in the inputs, and the copies of its last row that pad
    the point-fragment buffers -- must never act as keys."""
    _check_ragged(counts, layers, "u16", K_SPLIT)


@pytest.mark.gpu
@pytest.mark.parametrize("counts", RAGGED)
def test_ragged_batch_matches_fp64_in_exact_mode(counts):
    _check_ragged(counts, 12, "f32", K_EXACT, **EXACT)
