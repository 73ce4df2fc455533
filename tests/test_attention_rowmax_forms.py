"""The split attention kernel's row maximum (row_max4, attention_common.h) on every path that forms one.

Every body of the tile loop -- the first tile, the ordinary iteration in its three compat modes, a leaf BOUNDARY, the ragged last
tile -- computes the maximum of a tile's 16 logits per lane half with the same chain of three-operand maxima.  max is exact, so the
partials (O, m, l) must agree bit for bit between paths that differ only in where a maximum is formed:

  * unorm16 against fp32 compat, on a matrix whose entries are all 0 or 1 (both formats hold them exactly), in the key-split form
    (pdsc_sc_attention_split_partials): N = 33 (two key tiles, ragged last tile; key split 2: first-tile code and LAST only),
    N = 97 (key split 2: one ordinary iteration per workgroup, the second one towards the ragged tile; key split 4: first tile and
    LAST), N = 1505 (key split 4: twelve tiles per workgroup);
  * the leaf form (reached through the forward, pdsc_forward; its partials are read from the workspace's att_scratch) at N = 1505
    = 4 canonical leaves of 12 tiles: key split 4 (every leaf starts with the first-tile code and ends with LAST) against key
    split 2 (leaves 1 and 3 start at a BOUNDARY / RESTART pair) and key split 1 (leaves 1 and 2 do, and survive the in-workgroup
    merge in their slots; leaves 0 and 3 are merged into slot 0, whose bits the forward's outputs check in
    test_leaf_merge_in_workgroup.py).

and one value-level check: with one-hot keys the kernel's own s = K Q^T is the query row itself (fp16-exact entries: the low
parts of the operand split are zero and every MFMA sum has one non-zero term), so the host knows the kernel's logits exactly and
m must EQUAL max_j(compat * s) - ATT_P_BIAS (= 7) computed in fp32: for rows whose maximum sits in each of the 32 positions of a
tile (16 registers x 2 lane halves), in the first tile of a workgroup's range or a later one (then it exceeds the reference by more
than the rescale threshold 8 + 7 and moves it), rows with all logits equal, and rows of negative logits in front of masked tail
keys whose unmasked value (0 * 1) would win.  Everything is on a grid of 1/4, so every fp32 operation of the reference is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pointdsc_amd import PointDSC, _lib, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIAS, THR = 7.0, 8.0            # ATT_P_BIAS, ATT_RESCALE_THR (attention_split_kernel.h)
PEAK = 40.0                     # more than THR + BIAS above every other logit


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _encode_u16(c01: torch.Tensor, ld: int, pad: int) -> torch.Tensor:
    """0/1 matrix [n, n] -> unorm16 [1, n, ld] in the kernel's tile order (inverse of ops.decode_compat_u16); padding columns = pad"""
    n = c01.shape[0]
    nat = torch.full((n, ld), pad, dtype=torch.int32)
    nat[:, :n] = c01.to(torch.int32)
    j = torch.arange(ld)
    r = j & 31
    pos = (j & ~31) + 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)
    stored = torch.empty_like(nat)
    stored[:, pos] = nat                          # natural key j lives at position pos[j]
    u = (stored.numpy() * 65535).astype(np.uint16)
    return torch.from_numpy(u.view(np.int16)).reshape(1, n, ld).to(DEV)


def _encode_f32(c01: torch.Tensor, ld: int, pad: int) -> torch.Tensor:
    n = c01.shape[0]
    nat = torch.full((n, ld), float(pad), dtype=torch.float32)
    nat[:, :n] = c01.float()
    return nat.reshape(1, n, ld).to(DEV)


def _partials(qkv, compat, n, nsplit):
    """(O bits, ml [nsplit, Npad, 2]) of pdsc_sc_attention_split_partials in point-fragment order, scratch zeroed first"""
    lib = _lib.load()
    qs, kv = ops.pack_qkv_split(qkv, 1, n)
    nb = int(lib.pdsc_attention_split_scratch_bytes(1, n, nsplit))
    scratch = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    c16 = compat.dtype == torch.int16
    _lib.check(lib.pdsc_sc_attention_split_partials(_ptr(qs), _ptr(kv), _ptr(compat), 1 if c16 else 0, compat.shape[-1], _ptr(scratch), nb,
                                                    1, n, nsplit, 1, torch.cuda.current_stream().cuda_stream), "pdsc_sc_attention_split_partials")
    torch.cuda.synchronize()
    npad = (n + 255) // 256 * 256
    words = scratch.view(torch.int32).cpu()
    assert words.numel() == nsplit * npad * 130
    o = words[: nsplit * npad * 128]
    ml = words[nsplit * npad * 128:].view(torch.float32).reshape(nsplit, npad, 2)
    return o, ml


def _tile_ranges(n, nsplit):
    tiles = (n + 31) // 32
    per, rem = divmod(tiles, nsplit)
    return [(sp * per + min(sp, rem), sp * per + min(sp, rem) + per + (1 if sp < rem else 0)) for sp in range(nsplit)]


def _exact_problem(n, shift, seed):
    """(qkv [n, 384], c01 [n, n], logits [n, n], designed rows): one-hot keys, so s[i][j] = q[i][j] exactly"""
    assert n <= 128
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-16, 17, (n, n), generator=g).float() / 4            # base logits in [-4, 4]
    c01 = (torch.rand(n, n, generator=g) < 0.6).float()
    peak = (torch.arange(n) + shift) % n                                     # the row maximum walks through every tile position
    s[torch.arange(n), peak] = PEAK
    c01[torch.arange(n), peak] = 1.0
    equal_rows = [r for r in (5, 70) if r < n]                               # all logits equal
    for r in equal_rows:
        s[r], c01[r] = -2.5, 1.0
    neg_rows = [r for r in (6, 71) if r < n]                                 # all logits negative, falling: the maximum of every key
    for r in neg_rows:                                                       # range is its first key; a masked key's 0 would win
        s[r], c01[r] = -1.0 - torch.arange(n).float() / 4, 1.0
    qkv = torch.zeros(n, 384)
    qkv[:, :n] = s
    qkv[torch.arange(n), 128 + torch.arange(n)] = 1.0                        # k_j = e_j
    qkv[:, 256:] = torch.randn(n, 128, generator=g)
    return qkv.to(DEV), c01, c01 * s, peak, equal_rows + neg_rows


def _m_rule(row, t0, t1, n):
    """the kernel's reference exponent for keys of tiles [t0, t1): first tile's maximum - 7, moved to a later tile's maximum - 7 when
    that exceeds it by more than 8 + 7 (fp32; exact on this grid).  Returns (m, maximum over the range)."""
    f = np.float32
    keys = lambda t: row[t * 32: min((t + 1) * 32, n)]
    m = f(keys(t0).max()) - f(BIAS)
    for t in range(t0 + 1, t1):
        mloc = f((keys(t).astype(np.float32) - m).max())
        if mloc > f(THR + BIAS):
            m = f(m + f(mloc - f(BIAS)))
    return f(m), f(row[t0 * 32: min(t1 * 32, n)].max())


@pytest.mark.parametrize("n,nsplit,shift", [(33, 2, 0), (97, 2, 0), (97, 2, 13), (97, 4, 0)])
def test_m_is_the_row_maximum_minus_the_bias(n, nsplit, shift):
    qkv, c01, logits, peak, special = _exact_problem(n, shift, seed=100 + n + shift)
    ld = ops.compat_ld(n)
    got = {fmt: _partials(qkv, enc(c01, ld, 1), n, nsplit) for fmt, enc in (("u16", _encode_u16), ("f32", _encode_f32))}
    assert torch.equal(got["u16"][0], got["f32"][0]), "O differs between the compat formats"
    assert torch.equal(got["u16"][1].view(torch.int32), got["f32"][1].view(torch.int32)), "(m, l) differs between the compat formats"
    ml = got["u16"][1].numpy()
    lg = logits.numpy()
    checked_designed = 0
    for sp, (t0, t1) in enumerate(_tile_ranges(n, nsplit)):
        for i in range(n):
            want, mx = _m_rule(lg[i], t0, t1, n)
            assert ml[sp, i, 0] == want, (sp, i, ml[sp, i, 0], want)
            designed = i in special or t0 * 32 <= int(peak[i]) < t1 * 32
            if designed:                                   # here the rule's reference IS the maximum of the whole range
                assert ml[sp, i, 0] == np.float32(mx) - np.float32(BIAS), (sp, i, ml[sp, i, 0], mx)
                checked_designed += 1
            assert ml[sp, i, 1] > 0 and np.isfinite(ml[sp, i, 1])
    assert checked_designed >= n                            # every row has its peak in exactly one range


def test_peak_positions_cover_a_tile():
    """(host) the diagonal of the N = 97 problem puts a row maximum in each of the 16 registers of both lane halves, in a first tile
    and in a later tile of a key split's range"""
    seen = set()
    for i in range(97):
        t, p = divmod(i, 32)
        seen.add((t & 1, (p >> 2) & 1, (p & 3) + 4 * (p >> 3)))         # (later tile of split-2 range?, lane half, register)
    assert {(0, h, r) for h in range(2) for r in range(16)} <= seen and {(1, h, r) for h in range(2) for r in range(16)} <= seen


@pytest.mark.parametrize("n,nsplit", [(33, 2), (97, 2), (1505, 4)])
def test_unorm16_and_fp32_compat_give_the_same_partials(n, nsplit):
    """random operands, 0/1 matrix: the two compat modes differ in the decode and in where the maximum's operands come from, not in a bit"""
    g = torch.Generator().manual_seed(7 + n)
    qkv = (torch.randn(n, 384, generator=g) * 0.3).to(DEV)
    c01 = (torch.rand(n, n, generator=g) < 0.5).float()
    ld = ops.compat_ld(n)
    o16, ml16 = _partials(qkv, _encode_u16(c01, ld, 0), n, nsplit)
    o32, ml32 = _partials(qkv, _encode_f32(c01, ld, 0), n, nsplit)
    assert torch.equal(o16, o32)
    assert torch.equal(ml16.view(torch.int32), ml32.view(torch.int32))
    assert torch.isfinite(ml16[:, :n]).all() and (ml16[:, :n, 1] > 0).all()


KW = dict(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
          sigma_d=0.10, k=40, nms_radius=0.10)


def test_leaf_partials_do_not_depend_on_the_key_split():
    """N = 1505: 4 leaves x 12 tiles.  The last layer's leaf partials, as the attention launch left them in att_scratch."""
    n, leaves = 1505, 4
    lib = _lib.load()
    assert lib.pdsc_attention_leaf_count(n) == leaves
    model = PointDSC(**KW)
    model.load_state_dict(synthetic.make_state_dict(model.state_dict(), seed=6))
    model = model.eval().to(DEV)
    pair = synthetic.make_pair(n, inlier_ratio=0.3, seed=41)
    data = {k: pair[k].to(DEV).contiguous() for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["testing"] = True
    npad = (n + 255) // 256 * 256

    def run(d, vw):
        _lib.check(lib.pdsc_attention_leaf_split_override(d), "pdsc_attention_leaf_split_override")
        with torch.no_grad():
            model(data)                                   # (sizes the workspace)
        torch.cuda.synchronize()
        cfg = model._config()
        off = {name: int(lib.pdsc_workspace_offset(C.byref(cfg), 1, n, int(n * model.ratio), name)) for name in (b"att_scratch", b"q_split")}
        scratch = model._workspace[off[b"att_scratch"]:off[b"q_split"]]
        words = scratch[: scratch.numel() // 4 * 4].view(torch.int32)
        assert words.numel() >= leaves * npad * (vw + 2)
        words.fill_(0x7FC00000)                           # NaN: a slot nobody writes stays recognisable
        with torch.no_grad():
            model(data)
        torch.cuda.synchronize()
        w = words[: leaves * npad * (vw + 2)].cpu()
        return w[: leaves * npad * vw].reshape(leaves, npad * vw), w[leaves * npad * vw:].reshape(leaves, npad, 2)

    saved = (model.value_fold, model.compat_format)
    try:
        for fold, vw in ((1, 64), (0, 128)):
            for fmt in ("u16", "f32"):
                model.value_fold, model.compat_format = fold, fmt
                o4, ml4 = run(4, vw)
                assert not torch.isnan(ml4.view(torch.float32)[:, :n]).any()
                o2, ml2 = run(2, vw)
                assert torch.equal(o2, o4) and torch.equal(ml2, ml4), (fold, fmt, "key split 2")
                o1, ml1 = run(1, vw)
                assert torch.equal(o1[1:3], o4[1:3]) and torch.equal(ml1[1:3], ml4[1:3]), (fold, fmt, "key split 1, leaves 1 and 2")
                merged = ml1[0].view(torch.float32)[:n]
                assert (merged[:, 0] == 0).all() and (merged[:, 1] > 0).all()      # slot 0: the merged partial, (m, l) = (0, den)
    finally:
        lib.pdsc_attention_leaf_split_override(0)
        model.value_fold, model.compat_format = saved
