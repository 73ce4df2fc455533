"""fp64 oracle of the fp16 range sentinel (pdsc_common.h: range_note / range_report) and the recipes its tests run.

The split-precision arithmetic carries activations as fp16 hi / lo pairs, so every value a kernel converts must stay below 65504;
a pair one of whose converted values reaches the bound gets a non-zero word in the workspace entry "range_flag" and a NaN pose.
`encoder_kinds` runs the L-layer encoder of ONE pair in float64 on the CPU (oracle/pointdsc_oracle.py: _conv, _bn, spatial_compat,
the way tests/test_encoder_fp64.py restates the layer loop) and returns the largest |value| of every operand KIND some kernel
converts; `ROUTE_KINDS` says which kinds the kernels of a route convert, `expected_flag` is "some kind of the route that ran
reaches 65504".

Kinds (the maxima are over all layers unless said otherwise; hidden activations and the PointCN output after their ReLU, which is
what the kernels convert):
    layer0            encoder.layer0 output: the head-only launch converts feat_in (H3 routes)
    PointCN           relu(BN(conv)): operand of the q|k|v projection (every route) and the residual
    q, k, v           the attention's streams; q with the pre-scale log2(e) / sqrt(C) of the packed weights (model.packed_weights)
    message           softmax(compat * q^T k) v: operand of fc_message's first conv (unfolded H3 routes)
    hidden 1 / 2      fc_message's hidden activations (H3 routes)
    feature           PointCN output + fc_message output of layers 0 .. L-2: what feeds the NEXT layer's PointCN (H3 routes; the
                      last layer's feature leaves as fp32 rows and is never converted)
  and on the folded route (value_fold = 1, default arithmetic, N <= 16384) two operands differ:
    V'                W1f Wv featB, no bias (W1f = fc_message's first conv with its BatchNorm folded): replaces v and message
    hidden 1 folded   relu(P V' + b'), b' = W1f bv + b1f: the same number as hidden 1 in exact arithmetic, computed the folded way

Recipes: weight scalings of synthetic.make_state_dict(..., seed=2) on a 2-layer model plus a scaling of corr_pos alone (corr_pos
is not an input of the spatial-compatibility matrix, so nothing else moves with it).  Each pushes ONE kind -- one channel of it:
CHANNELS -- past 7e4 on the "hot"
input and keeps every other kind of both operand lists below 3e4 (the range probe's own margin, model.py); on the "cold" input of the
same pair (corr_pos scaled down) every kind stays below 3e4, which gives a batch its unflagged pairs under the same weights
(one exception, "hidden 1": see every_pair below).  The gain of a recipe is spread over two convs and the input so that no folded
weight comes near the packing check's 3e4.
tests/test_range_sentinel.py::test_recipes_isolate_one_kind asserts all of it in fp64.  Two kinds cannot be isolated:
    PointCN   its output is the residual, so the feature that follows overflows with it      -> recipe "PointCN" (implies feature)
    message   |message| <= max |v| (a convex combination of v's rows)                          -> recipe "v" (implies message; the
              recipe brings fc_message's first conv down with it, so hidden 1 stays in range and V' = W1f Wv featB too)
"""
import math

import torch

from oracle import pointdsc_oracle as O

F16_RANGE = 65504.0
TARGET_MIN, OTHERS_MAX, WEIGHT_MAX = 7.0e4, 3.0e4, 3.0e4
KW = dict(in_dim=6, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10)
LAYERS, WSEED = 2, 2

ROUTE_KINDS = {
    "unfolded": ("layer0", "PointCN", "q", "k", "v", "message", "hidden 1", "hidden 2", "feature"),
    "folded": ("layer0", "PointCN", "q", "k", "V'", "hidden 1 folded", "hidden 2", "feature"),
    "f32": ("PointCN", "q", "k", "v"),           # layer_gemm = "f32": only the attention's operands are fp16 pairs
}

NL0, NL1 = "encoder.blocks.NonLocal_layer_0.", "encoder.blocks.NonLocal_layer_1."
PCN0, PCN1 = "encoder.blocks.PointCN_layer_0.0.", "encoder.blocks.PointCN_layer_1.0."

# name -> dict(scales = {state_dict key: factor} applied to the whole tensor, rows = {key: factor} applied to ONE output row (the
#              channel of the recipe's variant: only that channel of the target kind leaves the range, so a sentinel that misses
#              part of an operand's channels -- one of two k-steps, one lane half -- is caught), corr = factor of corr_pos on the hot
#              input, cold = factor on the cold input, target = the kind pushed out of range, implies = kinds that cannot help
#              following it, every_pair = the overflow comes from a scaled bias (on the folded route hidden 1 = P V' + b' can leave
#              the range with V' in range only through b'), so the cold input overflows too: such a recipe flags EVERY pair)
RECIPES = {
    "benign": dict(scales={}, rows={}, corr=1.0, cold=1.0, target=None, implies=()),
    "layer0": dict(scales={PCN0 + "weight": 1.0e-5}, rows={"encoder.layer0.weight": 1.0e3}, corr=3.0e2, cold=1.0, target="layer0", implies=()),
    "PointCN": dict(scales={NL0 + "projection_q.weight": 1.0e-5, NL0 + "projection_k.weight": 1.0e-5, NL0 + "projection_v.weight": 1.0e-5,
                            PCN1 + "weight": 1.0e-5},
                    rows={PCN0 + "weight": 3.0e2}, corr=1.0e3, cold=1.0e-2, target="PointCN", implies=("feature",)),
    "k": dict(scales={}, rows={NL0 + "projection_k.weight": 6.0e4, NL0 + "projection_k.bias": 6.0e4}, corr=3.0, cold=1.0e-3, target="k", implies=()),
    "q": dict(scales={}, rows={NL0 + "projection_q.weight": 2.0e5, NL0 + "projection_q.bias": 2.0e5}, corr=8.0, cold=1.0e-3, target="q", implies=()),
    "v": dict(scales={NL0 + "fc_message.0.weight": 1.0e-5}, rows={NL0 + "projection_v.weight": 6.0e4, NL0 + "projection_v.bias": 6.0e4},
              corr=1.8, cold=1.0e-3, target="v", implies=("message",)),
    "hidden 1": dict(scales={NL0 + "projection_v.bias": 1.0e4, NL0 + "fc_message.3.weight": 1.0e-6}, rows={NL0 + "fc_message.0.weight": 3.0e2},
                     corr=1.0, cold=1.0e-3, target="hidden 1", implies=(), every_pair=True),
    "hidden 2": dict(scales={NL0 + "fc_message.0.weight": 30.0, NL0 + "fc_message.6.weight": 1.0e-6}, rows={NL0 + "fc_message.3.weight": 1.0e3},
                     corr=30.0, cold=1.0, target="hidden 2", implies=()),
    "feature": dict(scales={NL0 + "fc_message.3.weight": 30.0, PCN1 + "weight": 1.0e-6}, rows={NL0 + "fc_message.6.weight": 1.0e3},
                    corr=30.0, cold=1.0, target="feature", implies=()),
}
# the variants of every recipe: a channel of the first and one of the second 16-channel k-step of a 32-channel tile (the fused
# layer kernels convert the two in statements of their own), both below 64 (the hidden activations have 64 channels), and for the
# 128-channel kinds a channel of the upper half (in the few-tile H3 kernel wavefronts 2 and 3 own it, with a report of their own)
CHANNELS = (37, 21)
UPPER_CHANNEL = 68


def channels(name):
    if name == "benign":
        return CHANNELS[:1]
    return CHANNELS if RECIPES[name]["target"].startswith("hidden") else CHANNELS + (UPPER_CHANNEL,)


def recipe_state_dict(base, name, channel):
    """`base` (a state_dict) with the recipe's scalings, the row scalings on output row `channel`; `base` is left alone."""
    sd = {k: v.clone() for k, v in base.items()}
    for key, scale in RECIPES[name]["scales"].items():
        sd[key] = sd[key] * scale
    for key, scale in RECIPES[name]["rows"].items():
        sd[key][channel] = sd[key][channel] * scale
    return sd


def recipe_input(pair, name, hot):
    """The pair with corr_pos scaled by the recipe's hot / cold factor (keypoints untouched: the compat matrix does not move)."""
    f = RECIPES[name]["corr" if hot else "cold"]
    return {k: (v * f if k == "corr_pos" else v) for k, v in pair.items()}


def _fold(sd, conv, bn=None):
    w, b = sd[conv + ".weight"][:, :, 0], sd[conv + ".bias"]
    if bn is not None:
        s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + O.BN_EPS)
        w, b = w * s[:, None], (b - sd[bn + ".running_mean"]) * s + sd[bn + ".bias"]
    return w, b


def folded_weight_max(sd, layers=LAYERS, channels=128):
    """Largest |entry| of what the module packs (BatchNorm folded in fp64, q pre-scaled) and of the folded layer's W1f Wv."""
    sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    qs = math.log2(math.e) / math.sqrt(channels)
    parts = list(_fold(sd, "encoder.layer0"))
    for i in range(layers):
        p, nl = f"encoder.blocks.PointCN_layer_{i}", f"encoder.blocks.NonLocal_layer_{i}"
        parts += _fold(sd, p + ".0", p + ".1")
        wq, bq = _fold(sd, nl + ".projection_q")
        wv, bv = _fold(sd, nl + ".projection_v")
        w1, b1 = _fold(sd, nl + ".fc_message.0", nl + ".fc_message.1")
        parts += [wq * qs, bq * qs, wv, bv, w1, b1, w1 @ wv]      # (b' = W1f bv + b1f stays fp32 in the folded stream: not a converted weight)
        parts += _fold(sd, nl + ".projection_k")
        parts += _fold(sd, nl + ".fc_message.3", nl + ".fc_message.4")
        parts += _fold(sd, nl + ".fc_message.6")
    for j in (0, 2, 4):
        parts += _fold(sd, f"classification.{j}")
    return max(float(t.abs().max()) for t in parts)


def encoder_kinds(sd, corr_pos, src, tgt, layers=LAYERS, channels=128):
    """{kind: largest |value|} of one pair in float64: corr_pos [N,in_dim], src / tgt [N,3] (any float dtype)."""
    sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    compat = O.spatial_compat(src.float(), tgt.float(), sd["sigma_spat"].float())[1].double()      # the fp32 matrix the kernels stream
    top = {}

    def note(kind, x):
        top[kind] = max(top.get(kind, 0.0), float(x.abs().max()))

    feat = O._conv(sd, "encoder.layer0", corr_pos.double().t())
    note("layer0", feat)
    for i in range(layers):
        p, nl = f"encoder.blocks.PointCN_layer_{i}", f"encoder.blocks.NonLocal_layer_{i}"
        feat = torch.relu(O._bn(sd, p + ".1", O._conv(sd, p + ".0", feat)))
        note("PointCN", feat)
        q, k, v = (O._conv(sd, f"{nl}.projection_{x}", feat) for x in "qkv")
        note("q", q * (math.log2(math.e) / math.sqrt(channels)))
        note("k", k)
        note("v", v)
        P = torch.softmax(compat * ((q.t() @ k) / channels ** 0.5), dim=-1)
        message = (P @ v.t()).t()
        note("message", message)
        h1 = torch.relu(O._bn(sd, nl + ".fc_message.1", O._conv(sd, nl + ".fc_message.0", message)))
        note("hidden 1", h1)
        w1f, b1f = _fold(sd, nl + ".fc_message.0", nl + ".fc_message.1")
        wv, bv = _fold(sd, nl + ".projection_v")
        vprime = (w1f @ wv) @ feat
        note("V'", vprime)
        note("hidden 1 folded", torch.relu((P @ vprime.t()).t() + (w1f @ bv + b1f)[:, None]))
        h2 = torch.relu(O._bn(sd, nl + ".fc_message.4", O._conv(sd, nl + ".fc_message.3", h1)))
        note("hidden 2", h2)
        feat = feat + O._conv(sd, nl + ".fc_message.6", h2)
        if i + 1 < layers:
            note("feature", feat)
    top.setdefault("feature", 0.0)
    return top


def expected_flag(kinds, route):
    return any(not kinds[k] < F16_RANGE for k in ROUTE_KINDS[route])
