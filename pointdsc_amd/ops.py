"""Stage-level tensor wrappers over the C-ABI (one per entry point of include/pointdsc_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic happens in
libpointdsc_hip.so.  Every wrapper validates device/dtype/contiguity, allocates outputs with torch and
enqueues on ``torch.cuda.current_stream()``.  Names and argument meaning follow the reference functions
they stand in for (``rigid_transform_3d``, ``knn`` ... in /root/reference/models/common.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _on_device(fn):
    """Run the wrapper with the first CUDA tensor argument's device current (the library launches on the calling
    thread's current device and on that device's current stream), like PointDSC.forward does."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if torch.is_tensor(a) and a.is_cuda:
                with torch.cuda.device(a.device):
                    return fn(*args, **kwargs)
            if isinstance(a, (tuple, list)) and a and torch.is_tensor(a[0]) and a[0].is_cuda:
                with torch.cuda.device(a[0].device):
                    return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return wrapped


def _chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def compat_ld(n: int) -> int:
    return int(_lib.load().pdsc_compat_ld(n))


@_on_device
def spatial_compat(src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, sigma_spat: torch.Tensor,
                   want_dist: bool = False):
    """[bs,N,3] x2 -> compat [bs,N,ld] (view [..., :N] is the reference matrix), optional src_dist."""
    lib = _lib.load()
    src, tgt = _chk(src_keypts, "src_keypts"), _chk(tgt_keypts, "tgt_keypts")
    sig = _chk(sigma_spat.reshape(-1), "sigma_spat")
    bs, n = src.shape[0], src.shape[1]
    ld = compat_ld(n)
    compat = torch.empty(bs, n, ld, device=src.device, dtype=torch.float32)
    dist = torch.empty_like(compat) if want_dist else None
    _lib.check(lib.pdsc_spatial_compat(_p(src), _p(tgt), _p(sig), _p(compat), _p(dist), ld, bs, n, _stream()),
               "pdsc_spatial_compat")
    return (compat, dist) if want_dist else compat


@_on_device
def spatial_compat_u16(src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, sigma_spat: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[bs,N,3] x2 -> unorm16 compat [bs,N,ld] (int16 storage of uint16 bits) in the attention kernel's tile order
    (pdsc_spatial_compat_u16); decode with `decode_compat_u16`."""
    lib = _lib.load()
    src, tgt = _chk(src_keypts, "src_keypts"), _chk(tgt_keypts, "tgt_keypts")
    sig = _chk(sigma_spat.reshape(-1), "sigma_spat")
    bs, n = src.shape[0], src.shape[1]
    ld = compat_ld(n)
    if out is None:
        out = torch.empty(bs, n, ld, device=src.device, dtype=torch.int16)
    _lib.check(lib.pdsc_spatial_compat_u16(_p(src), _p(tgt), _p(sig), _p(out), ld, bs, n, _stream()), "pdsc_spatial_compat_u16")
    return out


def decode_compat_u16(c16: torch.Tensor, n: int) -> torch.Tensor:
    """unorm16 tile-order matrix -> fp32 [bs,N,N] in natural column order (tests)."""
    bs, rows, ld = c16.shape
    u = (c16.to(torch.int32) & 0xFFFF).to(torch.float32) / 65535.0
    j = torch.arange(ld, device=c16.device)
    r = j & 31
    pos = (j & ~31) + 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)
    return u[:, :, pos][:, :, :n]


@_on_device
def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
           residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M,K] @ weight[Nout,K]^T (+bias)(relu)(+residual) -> [M,Nout]."""
    lib = _lib.load()
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    m, k = x.shape
    nout = weight.shape[0]
    y = torch.empty(m, nout, device=x.device, dtype=torch.float32)
    b = _chk(bias, "bias") if bias is not None else None
    r = _chk(residual, "residual") if residual is not None else None
    _lib.check(lib.pdsc_linear(_p(x), k, _p(weight), _p(b), _p(r), nout, _p(y), nout, m, k, nout, int(relu), _stream()),
               "pdsc_linear")
    return y


@_on_device
def classifier_hidden(feat: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """feat [M,128] -> h2 [M,32] = relu(w2 relu(w1 feat + b1) + b2) in one launch (pdsc_classifier_hidden): bit-identical to
    linear(linear(feat, w1, b1, relu=True), w2, b2, relu=True)."""
    lib = _lib.load()
    x = _chk(feat, "feat")
    w1, b1, w2, b2 = _chk(w1, "w1"), _chk(b1, "b1"), _chk(w2, "w2"), _chk(b2, "b2")
    assert x.shape[1] == 128 and w1.shape == (32, 128) and w2.shape == (32, 32) and b1.shape == (32,) and b2.shape == (32,)
    h2 = torch.empty(x.shape[0], 32, device=x.device, dtype=torch.float32)
    _lib.check(lib.pdsc_classifier_hidden(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(h2), x.shape[0], _stream()), "pdsc_classifier_hidden")
    return h2


@_on_device
def layer0(corr_pos: torch.Tensor, w0_padded: torch.Tensor, b0: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x = _chk(corr_pos, "corr_pos").reshape(-1, corr_pos.shape[-1])
    w, b = _chk(w0_padded, "w0"), _chk(b0, "b0")
    y = torch.empty(x.shape[0], 128, device=x.device, dtype=torch.float32)
    _lib.check(lib.pdsc_layer0(_p(x), x.shape[1], _p(w), _p(b), _p(y), x.shape[0], _stream()), "pdsc_layer0")
    return y


LAYER_GEMMS = {"f32": 0, "h3": 1}      # enum pdsc_layer_gemm
LAYER_KERNELS = {"auto": 0, "block": 1, "wave": 2, "h3": 3, "x3": 4}      # enum pdsc_layer_kernel
PF_PARTIALS, PF_RES, PF_FEATB = 1, 2, 4      # enum pdsc_layer_io
_TAIL_W, _HEAD_W = ("w1", "b1", "w2", "b2", "w3", "b3"), ("wp", "bp", "wq", "bq")


def pf_rows(n: int) -> int:
    """rows per pair of a point-fragment buffer: whole tiles of 32."""
    return (n + 31) // 32 * 32


def _natural_weights(tail_w, head_w) -> dict:
    """(w1,b1,w2,b2,w3,b3) / (wp,bp,wq,bq), either may be None -> the natural-layout weight fields of pdsc_layer_call."""
    w = {k: _chk(t, "tail_w") for k, t in zip(_TAIL_W, tail_w or ())}
    w.update({k: _chk(t, "head_w") for k, t in zip(_HEAD_W, head_w or ())})
    return w


def _layer_run(bs: int, n: int, weights: dict, msg=None, partials=None, res=None, feat_in=None, want_feat=False, want_qkv=False,
               want_streams=True, gemm: str = "f32", io_flags: int = 0, kernel: str = "auto"):
    """Every fused-layer wrapper below: allocate the outputs, fill one pdsc_layer_call, pdsc_layer_run.
    weights: pdsc_layer_call field name -> tensor; the tail runs when it holds w1 or wfrag_tail, the head when it holds wp or
    wfrag_head.  partials = (scratch, nsplit) of sc_attention_split(..., merge=False) replaces msg.
    Returns (feat or None, featB or None, qkv or None, q_split or None, kv_tiles or None); feat comes back when asked for or when
    there is no head, featB holds whole tiles per pair when it is written in point-fragment order."""
    lib = _lib.load()
    has_tail, has_head = "w1" in weights or "wfrag_tail" in weights, "wp" in weights or "wfrag_head" in weights
    dev = next(t for t in (res, feat_in, msg) if t is not None).device
    m = bs * n

    def new(rows, cols):
        return torch.empty(rows, cols, device=dev, dtype=torch.float32)

    feat = new(m, 128) if has_tail and (want_feat or not has_head) else None
    featB = new(bs * pf_rows(n) if io_flags & PF_FEATB else m, 128) if has_head else None
    qkv = new(m, 384) if has_head and want_qkv else None
    streams = has_head and want_streams
    qs = torch.empty(int(lib.pdsc_split_q_bytes(bs, n)), device=dev, dtype=torch.uint8) if streams else None
    kv = torch.zeros(int(lib.pdsc_split_kv_bytes(bs, n)), device=dev, dtype=torch.uint8) if streams else None
    call = _lib.PdscLayerCall(bs=bs, N=n, gemm_format=LAYER_GEMMS[gemm], io_flags=io_flags, kernel=LAYER_KERNELS[kernel])
    if partials is not None:
        scratch, call.nsplit = partials
        call.Npad = (n + 255) // 256 * 256
        call.part_o = scratch.data_ptr()
        call.part_ml = scratch.data_ptr() + bs * call.nsplit * call.Npad * 128 * 4
    inputs = {k: _chk(t, k) for k, t in (("msg", msg), ("res", res), ("feat_in", feat_in)) if t is not None}
    outputs = dict(feat_out=feat, featB_out=featB, qkv_out=qkv, q_split=qs, kv_tiles=kv)
    for k, t in {**inputs, **outputs, **weights}.items():
        if t is not None:
            setattr(call, k, t.data_ptr())
    _lib.check(lib.pdsc_layer_run(C.byref(call), _stream()), "pdsc_layer_run")
    return feat, featB, qkv, qs, kv


@_on_device
def layer_fused(msg, res, feat_in, tail_w=None, head_w=None, want_feat=False):
    """Fused point-wise chain over one run of independent rows (pdsc_layer_run with bs = 1, N = rows).  tail_w =
    (w1,b1,w2,b2,w3,b3) folded fc_message of layer i, head_w = (wp,bp,wq,bq) folded PointCN / stacked qkv of layer i+1.
    Returns (feat or None, featB or None, qkv or None)."""
    src = msg if msg is not None else feat_in
    return _layer_run(1, src.shape[0], _natural_weights(tail_w, head_w), msg=msg, res=res, feat_in=feat_in, want_feat=want_feat,
                      want_qkv=True, want_streams=False)[:3]


@_on_device
def sc_attention(qkv: torch.Tensor, compat: torch.Tensor, bs: int, n: int, nsplit: int = 0) -> torch.Tensor:
    """qkv [bs*N,384] (q pre-scaled by log2(e)/sqrt(128)), compat [bs,N,ld] -> msg [bs*N,128]."""
    lib = _lib.load()
    qkv, compat = _chk(qkv, "qkv"), _chk(compat, "compat")
    ld = compat.shape[-1]
    msg = torch.empty(bs * n, 128, device=qkv.device, dtype=torch.float32)
    nb = int(lib.pdsc_attention_scratch_bytes(bs, n, nsplit))
    scratch = torch.empty(max(nb, 16), device=qkv.device, dtype=torch.uint8)
    _lib.check(lib.pdsc_sc_attention(_p(qkv), _p(compat), ld, _p(msg), _p(scratch), nb, bs, n, nsplit, _stream()),
               "pdsc_sc_attention")
    return msg


@_on_device
def sc_attention_lse(qkv: torch.Tensor, compat: torch.Tensor, bs: int, n: int, nsplit: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """sc_attention that also leaves the softmax's row statistic: -> (msg [bs*N,128], lse [bs*N]), lse = m + log2(l) in the
    log2 domain of the pre-scaled q.  msg is bit for bit sc_attention's at the same nsplit."""
    lib = _lib.load()
    qkv, compat = _chk(qkv, "qkv"), _chk(compat, "compat")
    ld = compat.shape[-1]
    msg = torch.empty(bs * n, 128, device=qkv.device, dtype=torch.float32)
    lse = torch.empty(bs * n, device=qkv.device, dtype=torch.float32)
    nb = int(lib.pdsc_attention_scratch_bytes(bs, n, nsplit))
    scratch = torch.empty(max(nb, 16), device=qkv.device, dtype=torch.uint8)
    _lib.check(lib.pdsc_sc_attention_lse(_p(qkv), _p(compat), ld, _p(msg), _p(lse), _p(scratch), nb, bs, n, nsplit, _stream()),
               "pdsc_sc_attention_lse")
    return msg, lse


@_on_device
def sc_attention_backward(qkv: torch.Tensor, compat: torch.Tensor, msg: torch.Tensor, lse: torch.Tensor, dmsg: torch.Tensor,
                          bs: int, n: int, nsplit: int = 0) -> torch.Tensor:
    """Backward of sc_attention: (qkv, compat, msg, lse) of sc_attention_lse and dmsg [bs*N,128] -> dqkv [bs*N,384], the gradient
    with respect to the (q | k | v) rows as passed (q pre-scaled).  compat gets no gradient.  nsplit forces the number of ranges
    the tile walk of both kernels is split into (0: the library's choice for the shape)."""
    lib = _lib.load()
    qkv, compat, msg, lse, dmsg = (_chk(t, name) for t, name in ((qkv, "qkv"), (compat, "compat"), (msg, "msg"), (lse, "lse"),
                                                                 (dmsg, "dmsg")))
    dqkv = torch.empty(bs * n, 384, device=qkv.device, dtype=torch.float32)
    nb = int(lib.pdsc_attention_backward_split_workspace_bytes(bs, n, nsplit))
    ws = torch.empty(max(nb, 16), device=qkv.device, dtype=torch.uint8)
    _lib.check(lib.pdsc_sc_attention_backward_split(_p(qkv), _p(compat), compat.shape[-1], _p(msg), _p(lse), _p(dmsg), _p(dqkv), _p(ws),
                                                    nb, bs, n, nsplit, _stream()), "pdsc_sc_attention_backward")
    return dqkv


@_on_device
def pack_qkv_split(qkv: torch.Tensor, bs: int, n: int):
    """fp32 (q|k|v) rows [bs*N,384] -> (q_split, kv_tiles) byte tensors in the layout of csrc/split_layout.h."""
    lib = _lib.load()
    qkv = _chk(qkv, "qkv")
    qs = torch.empty(int(lib.pdsc_split_q_bytes(bs, n)), device=qkv.device, dtype=torch.uint8)
    kv = torch.zeros(int(lib.pdsc_split_kv_bytes(bs, n)), device=qkv.device, dtype=torch.uint8)
    _lib.check(lib.pdsc_pack_qkv_split(_p(qkv), _p(qs), _p(kv), bs, n, _stream()), "pdsc_pack_qkv_split")
    return qs, kv


@_on_device
def sc_attention_split(q_split: torch.Tensor, kv_tiles: torch.Tensor, compat: torch.Tensor, bs: int, n: int,
                       nsplit: int = 0, merge: bool = True, layout: str = "rows"):
    """Split-precision (fp16 hi/lo, three MFMAs per operand pair) attention on the packed streams -> msg [bs*N,128].
    merge=False (needs a key split > 1): returns (scratch, nsplit) with the un-merged partials for the fused layer wrappers;
    layout="pf": those partials in point-fragment order (csrc/split_layout.h) for layer_fused_io."""
    lib = _lib.load()
    c16 = compat.dtype == torch.int16                  # unorm16 matrix of spatial_compat_u16
    compat = _chk(compat, "compat", torch.int16 if c16 else torch.float32)
    qs, kv = _chk(q_split, "q_split", torch.uint8), _chk(kv_tiles, "kv_tiles", torch.uint8)
    if nsplit <= 0:
        nsplit = int(lib.pdsc_attention_split_default_split(bs, n))
    msg = torch.empty(bs * n, 128, device=compat.device, dtype=torch.float32) if merge else None
    nb = int(lib.pdsc_attention_split_scratch_bytes(bs, n, nsplit))
    scratch = torch.empty(max(nb, 16), device=compat.device, dtype=torch.uint8)
    if layout == "pf":       # un-merged partials in point-fragment order (enum pdsc_partial_layout)
        assert not merge, "point-fragment partials are merged by the fused layer kernel"
        _lib.check(lib.pdsc_sc_attention_split_partials(_p(qs), _p(kv), _p(compat), 1 if c16 else 0, compat.shape[-1], _p(scratch), nb,
                                                        bs, n, nsplit, 1, _stream()), "pdsc_sc_attention_split_partials")
        return scratch, nsplit
    fn = lib.pdsc_sc_attention_split_u16 if c16 else lib.pdsc_sc_attention_split
    _lib.check(fn(_p(qs), _p(kv), _p(compat), compat.shape[-1], _p(msg), _p(scratch), nb, bs, n, nsplit, _stream()),
               "pdsc_sc_attention_split")
    return msg if merge else (scratch, nsplit)


@_on_device
def frag_weights_tail(tail_w, gemm: str = "f32") -> torch.Tensor:
    """(fc1 w, b, fc2 w, b, fc3 w, b) fp32 [out][in] -> the fragment-ordered tail stream (pdsc_layer_call.wfrag_tail);
    gemm = "h3": the chunks as fp16 hi / scaled-lo pairs (enum pdsc_layer_gemm)."""
    lib = _lib.load()
    out = torch.empty(int(lib.pdsc_wfrag_tail_bytes()), dtype=torch.uint8, device=tail_w[0].device)
    _lib.check(lib.pdsc_wfrag_build_tail(*[_p(_chk(w, "tail_w")) for w in tail_w], _p(out), LAYER_GEMMS[gemm], _stream()),
               "pdsc_wfrag_build_tail")
    return out


@_on_device
def frag_weights_head(head_w, gemm: str = "f32") -> torch.Tensor:
    """(pcn w, b, qkv w, b): pcn kept fp32 (gemm "f32") or fp16 hi / scaled lo ("h3"), q|k|v -> fp16 hi / lo, biases as
    one more k-step -> the head stream."""
    lib = _lib.load()
    out = torch.empty(int(lib.pdsc_wfrag_head_bytes()), dtype=torch.uint8, device=head_w[0].device)
    _lib.check(lib.pdsc_wfrag_build_head(*[_p(_chk(w, "head_w")) for w in head_w], _p(out), LAYER_GEMMS[gemm], _stream()),
               "pdsc_wfrag_build_head")
    return out


def _frag_weights(tail_w, head_w, gemm: str) -> dict:
    """... or the fragment-stream fields, built in `gemm` format from the same tuples."""
    w = {"wfrag_tail": frag_weights_tail(tail_w, gemm)} if tail_w is not None else {}
    if head_w is not None:
        w["wfrag_head"] = frag_weights_head(head_w, gemm)
    return w


@_on_device
def layer_fused_split(msg, res, feat_in, tail_w, head_w, bs: int, n: int, want_qkv: bool = False, partials=None,
                      qkv_split: bool = False, frag: bool = False, gemm: str = "f32", want_feat: bool = True):
    """Like layer_fused, rows = bs pairs of n points, head emits the split streams (pdsc_layer_run, kernel chosen by the library).
    partials = (scratch, nsplit) from sc_attention_split(..., merge=False) replaces msg.
    qkv_split: run the q|k|v projection in split precision (fp16 hi/lo weights).
    frag: weights as fragment-ordered streams (implies qkv_split) -- what the forward uses; gemm = "h3" (frag only):
    fc1..fc3 / PointCN in the fp16 hi / scaled-lo arithmetic.
    want_feat = False: no feat output (what the forward asks of every layer but the last); head_w = None (frag only):
    tail only (the forward's last layer).
    Returns (feat or None, featB or None, qkv or None, q_split or None, kv_tiles or None)."""
    assert (res if res is not None else feat_in).shape[0] == bs * n
    assert head_w is not None or frag, "tail-only launches exist on fragment streams only"
    if frag:
        weights = _frag_weights(tail_w, head_w, gemm)
    else:
        assert gemm == "f32", "the H3 arithmetic exists on fragment streams only"
        weights = _natural_weights(tail_w, head_w)
        if qkv_split:
            weights["wq_split"] = split_weight(weights["wq"])
    return _layer_run(bs, n, weights, msg=msg, partials=partials, res=res, feat_in=feat_in, want_feat=want_feat, want_qkv=want_qkv,
                      gemm=gemm)


def rows_to_pf(x: torch.Tensor, bs: int, n: int) -> torch.Tensor:
    """[bs*n,128] rows -> point-fragment order [bs * pf_rows(n) * 128] (padding rows = copies of the pair's last row)."""
    t = pf_rows(n) // 32
    x = x.reshape(bs, n, 128)
    x = torch.cat([x, x[:, -1:].expand(bs, t * 32 - n, 128)], dim=1)            # [bs, t*32, 128]
    x = x.reshape(bs, t, 32, 16, 2, 4)                                          # [b, tile, l31, q, h, e]
    return x.permute(0, 1, 3, 4, 2, 5).contiguous().reshape(-1)                 # [b, tile, q, h, l31, e]: lane = 32 h + l31


def pf_to_rows(x: torch.Tensor, bs: int, rows_per_pair: int) -> torch.Tensor:
    """point-fragment buffer with rows_per_pair (multiple of 32) rows per pair -> [bs, rows_per_pair, 128]."""
    t = rows_per_pair // 32
    x = x.reshape(bs, t, 16, 2, 32, 4)
    return x.permute(0, 1, 4, 2, 3, 5).contiguous().reshape(bs, rows_per_pair, 128)


@_on_device
def layer_fused_io(res, feat_in, tail_w, head_w, bs: int, n: int, io_flags: int, partials=None):
    """H3 fragment streams, the forward's output set, hand-offs in point-fragment order per io_flags (pdsc_layer_call.io_flags):
    partials = (scratch, nsplit) of sc_attention_split(merge=False, layout "pf" if io_flags & PF_PARTIALS);
    res in PF order if io_flags & PF_RES; featB comes back in PF order if io_flags & PF_FEATB.
    tail_w None = head only (feat_in rows), head_w None = tail only.  Returns (feat or None, featB or None, q_split, kv_tiles)."""
    feat, featB, _, qs, kv = _layer_run(bs, n, _frag_weights(tail_w, head_w, "h3"), partials=partials, res=res, feat_in=feat_in,
                                        gemm="h3", io_flags=io_flags)
    return feat, None if featB is None else featB.reshape(-1), qs, kv


def split_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 matrix [out,in] -> uint8 tensor holding fp16 hi [out,in] then fp16 lo [out,in] (layout of pdsc_wsplit_build)."""
    w = _chk(w, "weight")
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.cat([hi.reshape(-1), lo.reshape(-1)]).view(torch.uint8)


@_on_device
def layer_fused_x3(msg, res, feat_in, tail_w, head_w, bs: int, n: int, partials=None, want_qkv: bool = False,
                   want_feat: bool = False):
    """The all-split layer kernel (pdsc_layer_run with PDSC_LAYER_KERNEL_X3; experiments builds).  tail_w/head_w as in
    layer_fused (fp32 matrices; split here).
    partials = (scratch uint8 tensor, nsplit) left by sc_attention_split(..., merge=False) replaces msg.
    Returns (feat or None, featB or None, qkv or None, q_split or None, kv_tiles or None)."""
    assert (res if res is not None else feat_in).shape[0] == bs * n
    weights = {k: split_weight(t) if k[0] == "w" else t for k, t in _natural_weights(tail_w, head_w).items()}
    return _layer_run(bs, n, weights, msg=msg, partials=partials, res=res, feat_in=feat_in, want_feat=want_feat, want_qkv=want_qkv,
                      kernel="x3")


STATS_COLUMNS = ("success", "RE_deg", "TE_cm", "num_gt_inliers", "gt_inlier_ratio", "num_true_positives", "precision", "recall", "f1")


@_on_device
def eval_stats(trans, gt_trans, pred_labels, gt_labels, re_thre: float = 15.0, te_thre: float = 30.0) -> torch.Tensor:
    """[bs,9] evaluation rows on the device (columns: STATS_COLUMNS) -- libs/loss.py:44-51,96-100 and the stats row of
    evaluation/test_3DMatch.py:90-98 without the per-pair device->host copies."""
    lib = _lib.load()
    T, G = _chk(trans, "trans"), _chk(gt_trans, "gt_trans")
    p, g = _chk(pred_labels, "pred_labels"), _chk(gt_labels.to(torch.float32), "gt_labels")
    bs, n = p.shape
    stats = torch.empty(bs, 9, device=p.device, dtype=torch.float32)
    _lib.check(lib.pdsc_eval_stats(_p(T), _p(G), _p(p), _p(g), float(re_thre), float(te_thre), _p(stats), bs, n, _stream()),
               "pdsc_eval_stats")
    return stats


@_on_device
def feature_compat(normed: torch.Tensor, sigma: torch.Tensor, bs: int, n: int) -> torch.Tensor:
    """normed [bs*N,128] -> M [bs,N,N] = clamp(1 - (1 - F F^T)/sigma^2, 0, 1), zero diagonal (models/PointDSC.py:158-163)."""
    lib = _lib.load()
    normed, sig = _chk(normed, "normed"), _chk(sigma.reshape(-1), "sigma")
    m = torch.empty(bs, n, n, device=normed.device, dtype=torch.float32)
    _lib.check(lib.pdsc_feature_compat(_p(normed), _p(sig), _p(m), n, bs, n, _stream()), "pdsc_feature_compat")
    return m


@_on_device
def feature_compat_backward(normed: torch.Tensor, sigma: torch.Tensor, dM: torch.Tensor, bs: int, n: int, want_dnormed: bool = True,
                            want_dsigma: bool = True):
    """Backward of feature_compat: normed [bs*N,128], sigma [1], dM [bs,N,ld >= N] (any values, not assumed symmetric; the pad
    columns are never read) -> (dnormed fp32 [bs*N,128] or None, dsigma fp64 [1] or None).  pdsc_feature_compat_backward."""
    if not (want_dnormed or want_dsigma):
        raise ValueError("feature_compat_backward: ask for at least one of dnormed and dsigma")
    lib = _lib.load()
    normed, sig, dM = _chk(normed, "normed"), _chk(sigma.reshape(-1), "sigma"), _chk(dM, "dM")
    if normed.numel() != bs * n * 128 or normed.shape[-1] != 128 or sig.numel() != 1:
        raise ValueError("normed must hold bs * N rows of 128 channels and sigma one value")
    if dM.dim() != 3 or dM.shape[0] != bs or dM.shape[1] != n or dM.shape[2] < n:
        raise ValueError(f"dM must be [bs,N,N] or [bs,N,ld >= N], got {tuple(dM.shape)}")
    nb = int(lib.pdsc_feature_compat_backward_workspace_bytes(bs, n))
    ws = torch.empty(max(nb // 8, 1), device=normed.device, dtype=torch.float64)
    dnormed = torch.empty(bs * n, 128, device=normed.device, dtype=torch.float32) if want_dnormed else None
    dsigma = torch.empty(1, device=normed.device, dtype=torch.float64) if want_dsigma else None
    _lib.check(lib.pdsc_feature_compat_backward(_p(normed), _p(sig), _p(dM), dM.shape[2], _p(dnormed), _p(dsigma), _p(ws), ws.numel() * 8,
                                                bs, n, _stream()), "pdsc_feature_compat_backward")
    return dnormed, dsigma


@_on_device
def normalize_confidence(feat, h2, w3, b3) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    feat, h2, w3, b3 = _chk(feat, "feat"), _chk(h2, "h2"), _chk(w3.reshape(-1), "w3"), _chk(b3.reshape(-1), "b3")
    m = feat.shape[0]
    normed = torch.empty_like(feat)
    conf = torch.empty(m, device=feat.device, dtype=torch.float32)
    _lib.check(lib.pdsc_normalize_confidence(_p(feat), _p(h2), _p(w3), _p(b3), _p(normed), _p(conf), m, _stream()),
               "pdsc_normalize_confidence")
    return normed, conf


@_on_device
def normalize_confidence_pf(feat, h2, w3, b3):
    """feat [bs,N,128], h2 [bs,N,32] -> (normed [bs,N,128], normed_pf [bs,ceil(N/32)*32,128] point-fragment order, conf [bs,N])."""
    lib = _lib.load()
    feat, h2, w3, b3 = _chk(feat, "feat"), _chk(h2, "h2"), _chk(w3.reshape(-1), "w3"), _chk(b3.reshape(-1), "b3")
    bs, n = feat.shape[0], feat.shape[1]
    normed = torch.empty_like(feat)
    normed_pf = torch.empty(bs, (n + 31) // 32 * 32, 128, device=feat.device, dtype=torch.float32)
    conf = torch.empty(bs, n, device=feat.device, dtype=torch.float32)
    _lib.check(lib.pdsc_normalize_confidence_pf(_p(feat), _p(h2), _p(w3), _p(b3), _p(normed), _p(normed_pf), _p(conf), bs, n, _stream()),
               "pdsc_normalize_confidence_pf")
    return normed, normed_pf, conf


@_on_device
def nms_keys(src_keypts, conf, radius: float) -> torch.Tensor:
    lib = _lib.load()
    src, conf = _chk(src_keypts, "src_keypts"), _chk(conf, "conf")
    bs, n = src.shape[0], src.shape[1]
    keys = torch.empty(bs, n, device=src.device, dtype=torch.float32)
    _lib.check(lib.pdsc_nms_keys(_p(src), _p(conf), float(radius), _p(keys), bs, n, _stream()), "pdsc_nms_keys")
    return keys


@_on_device
def nms_keys_grid(src_keypts, conf, radius: float) -> torch.Tensor:
    """pdsc_nms_keys_grid: the same keys from the 3 x 3 neighbouring cells of a 2-D grid (what the forward calls)."""
    lib = _lib.load()
    src, conf = _chk(src_keypts, "src_keypts"), _chk(conf, "conf")
    bs, n = src.shape[0], src.shape[1]
    keys = torch.empty(bs, n, device=src.device, dtype=torch.float32)
    nb = int(lib.pdsc_nms_workspace_bytes(bs, n))
    ws = torch.empty(nb, device=src.device, dtype=torch.uint8)
    _lib.check(lib.pdsc_nms_keys_grid(_p(src), _p(conf), float(radius), _p(keys), _p(ws), nb, bs, n, _stream()), "pdsc_nms_keys_grid")
    return keys


@_on_device
def rank_select(keys, num_seeds: int) -> torch.Tensor:
    lib = _lib.load()
    keys = _chk(keys, "keys")
    bs, n = keys.shape
    seeds = torch.empty(bs, num_seeds, device=keys.device, dtype=torch.int32)
    _lib.check(lib.pdsc_rank_select(_p(keys), _p(seeds), bs, n, num_seeds, _stream()), "pdsc_rank_select")
    return seeds


@_on_device
def pick_seeds(src_keypts, scores, R: float, max_num: int) -> torch.Tensor:
    """reference PointDSC.pick_seeds (dists replaced by the keypoints they were computed from)."""
    return rank_select(nms_keys(src_keypts, scores, R), max_num).long()


@_on_device
def knn_seeds(normed, seeds, k: int, return_dist: bool = False, form: str = "auto", normed_pf=None):
    """normed [bs,N,128], seeds [bs,S] int32 -> knn_idx [bs,S,k] int32.  form: "auto" (the library's choice), "matrix" (Gram rows
    written to HBM, then a selection launch) or "fused" (one launch, no S x N matrix; the returned distances are then undefined).
    normed_pf: the rows in point-fragment order (ops.normalize_confidence_pf), the fused form's fast column operand."""
    forms = {"auto": 0, "matrix": 1, "fused": 2}
    if return_dist:
        #  only the matrix form writes the S x N distances: "auto" may pick the fused form for large batches
        if form == "fused":
            raise ValueError('knn_seeds(return_dist=True) needs form="matrix" (the fused form never writes the S x N distance matrix)')
        form = "matrix"
    lib = _lib.load()
    normed, seeds = _chk(normed, "normed"), _chk(seeds, "seeds", torch.int32)
    bs, n = normed.shape[0], normed.shape[1]
    s = seeds.shape[1]
    ld = compat_ld(n)
    dist = torch.empty(bs, s, ld, device=normed.device, dtype=torch.float32)
    idx = torch.empty(bs, s, k, device=normed.device, dtype=torch.int32)
    _lib.check(lib.pdsc_knn_seeds_form(_p(normed), _p(normed_pf) if normed_pf is not None else None, _p(seeds), _p(dist), _p(idx), bs, n, s, k,
                                       forms[form], _stream()), "pdsc_knn_seeds")
    return (idx, dist[..., :n]) if return_dist else idx


@_on_device
def seed_power_iteration(normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations: int, want_M: bool = False):
    lib = _lib.load()
    normed, src, tgt = _chk(normed, "normed"), _chk(src, "src"), _chk(tgt, "tgt")
    knn_idx = _chk(knn_idx, "knn_idx", torch.int32)
    sigma, sigma_spat = _chk(sigma.reshape(-1), "sigma"), _chk(sigma_spat.reshape(-1), "sigma_spat")
    bs, n = src.shape[0], src.shape[1]
    s, k = knn_idx.shape[1], knn_idx.shape[2]
    iters = torch.zeros(bs, s, max(num_iterations, 1), 64, device=src.device, dtype=torch.float32)
    mask = torch.empty(bs, device=src.device, dtype=torch.int32)
    M = torch.empty(bs, s, k, k, device=src.device, dtype=torch.float32) if want_M else None
    _lib.check(lib.pdsc_seed_power_iteration(_p(normed), _p(src), _p(tgt), _p(knn_idx), _p(sigma), _p(sigma_spat),
                                             _p(iters), _p(mask), _p(M), bs, n, s, k, num_iterations, _stream()),
               "pdsc_seed_power_iteration")
    return iters, mask, M


@_on_device
def seed_transforms(src, tgt, knn_idx, iters, mask, num_iterations: int):
    lib = _lib.load()
    src, tgt = _chk(src, "src"), _chk(tgt, "tgt")
    knn_idx = _chk(knn_idx, "knn_idx", torch.int32)
    bs, n = src.shape[0], src.shape[1]
    s, k = knn_idx.shape[1], knn_idx.shape[2]
    trans = torch.empty(bs, s, 4, 4, device=src.device, dtype=torch.float32)
    w = torch.empty(bs, s, k, device=src.device, dtype=torch.float32)
    _lib.check(lib.pdsc_seed_transforms(_p(src), _p(tgt), _p(knn_idx), _p(iters), _p(mask), _p(trans), _p(w),
                                        bs, n, s, k, num_iterations, _stream()), "pdsc_seed_transforms")
    return trans, w


@_on_device
def seed_solve(normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations: int, want_M: bool = False):
    """The per-seed solver as the testing forward launches it (pdsc_seed_solve with seed_trans: the fused solver, then the early-exit
    fix-up with the 3x3 decompositions) -> (iters [bs,S,max(num_iterations,1),64], mask [bs] int32, trans [bs,S,4,4],
    weights [bs,S,k], M [bs,S,k,k] or None)."""
    lib = _lib.load()
    normed, src, tgt = _chk(normed, "normed"), _chk(src, "src"), _chk(tgt, "tgt")
    knn_idx = _chk(knn_idx, "knn_idx", torch.int32)
    sigma, sigma_spat = _chk(sigma.reshape(-1), "sigma"), _chk(sigma_spat.reshape(-1), "sigma_spat")
    bs, n = src.shape[0], src.shape[1]
    s, k = knn_idx.shape[1], knn_idx.shape[2]
    iters = torch.zeros(bs, s, max(num_iterations, 1), 64, device=src.device, dtype=torch.float32)
    mask = torch.empty(bs, device=src.device, dtype=torch.int32)
    M = torch.empty(bs, s, k, k, device=src.device, dtype=torch.float32) if want_M else None
    trans = torch.empty(bs, s, 4, 4, device=src.device, dtype=torch.float32)
    w = torch.empty(bs, s, k, device=src.device, dtype=torch.float32)
    _lib.check(lib.pdsc_seed_solve(_p(normed), _p(src), _p(tgt), _p(knn_idx), _p(sigma), _p(sigma_spat), _p(iters), _p(mask), _p(M),
                                   _p(trans), _p(w), bs, n, s, k, num_iterations, _stream()), "pdsc_seed_solve")
    return iters, mask, trans, w, M


@_on_device
def seed_solve_backward(normed, src, tgt, knn_idx, sigma, sigma_spat, mask, num_iterations: int, d_seed_trans,
                        want_dnormed: bool = True, want_dsigma: bool = True):
    """Backward of seed_power_iteration + seed_transforms (pdsc_seed_solve_backward): normed [bs,N,128], src, tgt [bs,N,3],
    knn_idx [bs,S,k] int32, sigma, sigma_spat one value each, mask [bs] int32 as seed_transforms took it, d_seed_trans [bs,S,4,4]
    (row 3 ignored) -> (dnormed fp32 [bs,N,128] or None, dsigma fp64 [1] or None)."""
    if not (want_dnormed or want_dsigma):
        raise ValueError("seed_solve_backward: ask for at least one of dnormed and dsigma")
    lib = _lib.load()
    normed, src, tgt = _chk(normed, "normed"), _chk(src, "src"), _chk(tgt, "tgt")
    knn_idx, mask = _chk(knn_idx, "knn_idx", torch.int32), _chk(mask, "mask", torch.int32)
    sigma, sigma_spat = _chk(sigma.reshape(-1), "sigma"), _chk(sigma_spat.reshape(-1), "sigma_spat")
    d_seed_trans = _chk(d_seed_trans, "d_seed_trans")
    if src.dim() != 3 or src.shape[2] != 3 or tgt.shape != src.shape:
        raise ValueError(f"src and tgt must be [bs,N,3] alike, got {tuple(src.shape)} {tuple(tgt.shape)}")
    bs, n = src.shape[0], src.shape[1]
    if normed.shape != (bs, n, 128) or knn_idx.dim() != 3 or knn_idx.shape[0] != bs:
        raise ValueError(f"normed must be [bs,N,128] and knn_idx [bs,S,k], got {tuple(normed.shape)} {tuple(knn_idx.shape)}")
    s, k = knn_idx.shape[1], knn_idx.shape[2]
    if d_seed_trans.shape != (bs, s, 4, 4) or mask.numel() != bs or sigma.numel() != 1 or sigma_spat.numel() != 1:
        raise ValueError("d_seed_trans must be [bs,S,4,4], mask [bs], sigma and sigma_spat one value each")
    if not 1 <= k <= 64:
        raise ValueError(f"seed_solve_backward: k = {k} (1 .. 64)")
    nb = int(lib.pdsc_seed_solve_backward_workspace_bytes(bs, n, s, k))
    ws = torch.empty(max((nb + 7) // 8, 1), device=src.device, dtype=torch.float64)
    dnormed = torch.empty(bs, n, 128, device=src.device, dtype=torch.float32) if want_dnormed else None
    dsigma = torch.empty(1, device=src.device, dtype=torch.float64) if want_dsigma else None
    _lib.check(lib.pdsc_seed_solve_backward(_p(normed), _p(src), _p(tgt), _p(knn_idx), _p(sigma), _p(sigma_spat), _p(mask),
                                            _p(d_seed_trans), _p(dnormed), _p(dsigma), _p(ws), ws.numel() * 8, bs, n, s, k,
                                            int(num_iterations), _stream()), "pdsc_seed_solve_backward")
    return dnormed, dsigma


@_on_device
def rigid_transform_3d(A: torch.Tensor, B: torch.Tensor, weights: Optional[torch.Tensor] = None,
                       weight_threshold: float = 0) -> torch.Tensor:
    """Drop-in for reference models/common.py:rigid_transform_3d: A,B [bs,n,3] -> [bs,4,4]."""
    lib = _lib.load()
    A, B = _chk(A, "A"), _chk(B, "B")
    bs, n = A.shape[0], A.shape[1]
    w = _chk(weights, "weights") if weights is not None else None
    T = torch.empty(bs, 4, 4, device=A.device, dtype=torch.float32)
    _lib.check(lib.pdsc_rigid_transform_3d(_p(A), _p(B), _p(w), float(weight_threshold), _p(T), bs, n, _stream()),
               "pdsc_rigid_transform_3d")
    return T


@_on_device
def score_hypotheses(seed_trans, src, tgt, inlier_threshold: float):
    lib = _lib.load()
    seed_trans, src, tgt = _chk(seed_trans, "seed_trans"), _chk(src, "src"), _chk(tgt, "tgt")
    bs, n = src.shape[0], src.shape[1]
    s = seed_trans.shape[1]
    counts = torch.empty(bs, s, device=src.device, dtype=torch.int32)
    _lib.check(lib.pdsc_score_hypotheses(_p(seed_trans), _p(src), _p(tgt), float(inlier_threshold), _p(counts),
                                         bs, n, s, _stream()), "pdsc_score_hypotheses")
    best = torch.empty(bs, device=src.device, dtype=torch.int32)
    initial = torch.empty(bs, 4, 4, device=src.device, dtype=torch.float32)
    labels = torch.empty(bs, n, device=src.device, dtype=torch.float32)
    _lib.check(lib.pdsc_select_best(_p(counts), _p(seed_trans), _p(src), _p(tgt), float(inlier_threshold), _p(best),
                                    _p(initial), _p(labels), bs, n, s, _stream()), "pdsc_select_best")
    return counts, best, initial, labels


@_on_device
def post_refinement(initial_trans, src, tgt, threshold: float, max_iters: int = 20):
    lib = _lib.load()
    initial_trans, src, tgt = _chk(initial_trans, "initial_trans"), _chk(src, "src"), _chk(tgt, "tgt")
    bs, n = src.shape[0], src.shape[1]
    final = torch.empty(bs, 4, 4, device=src.device, dtype=torch.float32)
    solves = torch.empty(bs, device=src.device, dtype=torch.int32)
    _lib.check(lib.pdsc_post_refinement(_p(initial_trans), _p(src), _p(tgt), float(threshold), max_iters, _p(final),
                                        _p(solves), bs, n, _stream()), "pdsc_post_refinement")
    return final, solves


POINTWISE_TRAIN_SHAPES = ((128, 128), (128, 64), (64, 64))      # (Cin, Cout) of pdsc_pointwise_train_*


def _train_dims(x: torch.Tensor, weight: torch.Tensor, what: str) -> Tuple[int, int, int]:
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: x must be [M,Cin] and weight [Cout,Cin], got {tuple(x.shape)} {tuple(weight.shape)}")
    return x.shape[0], x.shape[1], weight.shape[0]


def _train_workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max((int(nbytes) + 7) // 8, 1), device=device, dtype=torch.float64)


def _out(want: bool, device, *shape):
    return torch.empty(*shape, device=device, dtype=torch.float32) if want else None


def _pointwise_train_dims(x: torch.Tensor, weight: torch.Tensor, what: str) -> Tuple[int, int, int]:
    m, cin, cout = _train_dims(x, weight, what)
    if (cin, cout) not in POINTWISE_TRAIN_SHAPES:
        raise ValueError(f"{what}: (Cin, Cout) = ({cin}, {cout}); supported: {POINTWISE_TRAIN_SHAPES}")
    if m < 2:
        raise ValueError(f"{what}: M = {m} rows (batch statistics need at least 2 values per channel)")
    return m, cin, cout


@_on_device
def pointwise_train_forward(x, weight, bias, gamma, beta, running_mean, running_var, momentum: float = 0.1, eps: float = 1e-5):
    """Conv1d(k=1) -> BatchNorm1d with batch statistics -> ReLU on rows (pdsc_pointwise_train_forward): x [M,Cin], weight [Cout,Cin],
    bias, gamma, beta, running_mean, running_var [Cout] fp32 -> (z [M,Cout], y [M,Cout], mean [Cout] fp64, invstd [Cout] fp64).
    running_mean and running_var are updated IN PLACE (they must be contiguous: the kernel writes through their pointers)."""
    lib = _lib.load()
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    m, cin, cout = _pointwise_train_dims(x, weight, "pointwise_train_forward")
    bias, gamma, beta = _chk(bias, "bias"), _chk(gamma, "gamma"), _chk(beta, "beta")
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if not _chk(t, name).data_ptr() == t.data_ptr():
            raise ValueError(f"{name} must be contiguous: it is updated in place")
    for t, name in ((bias, "bias"), (gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t.shape != (cout,):
            raise ValueError(f"pointwise_train_forward: {name} must be [{cout}], got {tuple(t.shape)}")
    y = torch.empty(m, cout, device=x.device, dtype=torch.float32)
    z = torch.empty_like(y)
    mean = torch.empty(cout, device=x.device, dtype=torch.float64)
    invstd = torch.empty_like(mean)
    ws = _train_workspace(lib.pdsc_pointwise_train_workspace_bytes(m, cin, cout), x.device)
    _lib.check(lib.pdsc_pointwise_train_forward(_p(x), _p(weight), _p(bias), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                                float(momentum), float(eps), _p(y), _p(z), _p(mean), _p(invstd), _p(ws),
                                                ws.numel() * 8, m, cin, cout, _stream()), "pdsc_pointwise_train_forward")
    return z, y, mean, invstd


@_on_device
def pointwise_train_backward(x, weight, gamma, beta, y, mean, invstd, dz, want_dx: bool = True, want_dw: bool = True,
                             want_db: bool = True, want_dgamma: bool = True, want_dbeta: bool = True):
    """Backward of pointwise_train_forward (pdsc_pointwise_train_backward): x, weight, gamma, beta as the forward took them, y, mean,
    invstd as it returned them, dz [M,Cout] -> (dx [M,Cin], dw [Cout,Cin], db, dgamma, dbeta [Cout]); None where not wanted."""
    if not (want_dx or want_dw or want_db or want_dgamma or want_dbeta):
        raise ValueError("pointwise_train_backward: ask for at least one gradient")
    lib = _lib.load()
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    m, cin, cout = _pointwise_train_dims(x, weight, "pointwise_train_backward")
    gamma, beta = _chk(gamma, "gamma"), _chk(beta, "beta")
    mean, invstd = _chk(mean, "mean", torch.float64), _chk(invstd, "invstd", torch.float64)
    y, dz = _chk(y, "y"), _chk(dz, "dz")
    if y.shape != (m, cout) or dz.shape != (m, cout):
        raise ValueError(f"pointwise_train_backward: y and dz must be [{m},{cout}], got {tuple(y.shape)} {tuple(dz.shape)}")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd")):
        if t.shape != (cout,):
            raise ValueError(f"pointwise_train_backward: {name} must be [{cout}], got {tuple(t.shape)}")
    dx, dw = _out(want_dx, x.device, m, cin), _out(want_dw, x.device, cout, cin)
    db, dgamma, dbeta = _out(want_db, x.device, cout), _out(want_dgamma, x.device, cout), _out(want_dbeta, x.device, cout)
    ws = _train_workspace(lib.pdsc_pointwise_train_workspace_bytes(m, cin, cout), x.device)
    _lib.check(lib.pdsc_pointwise_train_backward(_p(x), _p(weight), _p(gamma), _p(beta), _p(y), _p(mean), _p(invstd), _p(dz), _p(dx),
                                                 _p(dw), _p(db), _p(dgamma), _p(dbeta), _p(ws), ws.numel() * 8, m, cin, cout,
                                                 _stream()), "pdsc_pointwise_train_backward")
    return dx, dw, db, dgamma, dbeta


LINEAR_TRAIN_COUT = 128
HEAD_HIDDEN = 32


def linear_train_shape_ok(cin: int, cout: int) -> bool:
    """(Cin, Cout) of pdsc_linear_train_*: (1 .. 16, 128) layer0, (64, 128) fc_message.6."""
    return cout == LINEAR_TRAIN_COUT and (1 <= cin <= 16 or cin == 64)


def _linear_train_dims(x: torch.Tensor, weight: torch.Tensor, what: str) -> Tuple[int, int, int]:
    m, cin, cout = _train_dims(x, weight, what)
    if not linear_train_shape_ok(cin, cout):
        raise ValueError(f"{what}: (Cin, Cout) = ({cin}, {cout}); supported: (1..16, 128), (64, 128)")
    if m < 1:
        raise ValueError(f"{what}: M = {m} rows")
    return m, cin, cout


@_on_device
def linear_train_forward(x, weight, bias, residual=None):
    """y = x weight^T + bias (+ residual) on rows (pdsc_linear_train_forward): x [M,Cin], weight [128,Cin], bias [128],
    residual [M,128] or None -> y [M,128]."""
    lib = _lib.load()
    x, weight, bias = _chk(x, "x"), _chk(weight, "weight"), _chk(bias, "bias")
    m, cin, cout = _linear_train_dims(x, weight, "linear_train_forward")
    if bias.shape != (cout,):
        raise ValueError(f"linear_train_forward: bias must be [{cout}], got {tuple(bias.shape)}")
    if residual is not None:
        residual = _chk(residual, "residual")
        if residual.shape != (m, cout):
            raise ValueError(f"linear_train_forward: residual must be [{m},{cout}], got {tuple(residual.shape)}")
    y = torch.empty(m, cout, device=x.device, dtype=torch.float32)
    _lib.check(lib.pdsc_linear_train_forward(_p(x), _p(weight), _p(bias), _p(residual), _p(y), m, cin, cout, _stream()),
               "pdsc_linear_train_forward")
    return y


@_on_device
def linear_train_backward(x, weight, dy, want_dx: bool = True, want_dw: bool = True, want_db: bool = True):
    """Backward of linear_train_forward (pdsc_linear_train_backward): dy [M,128] -> (dx [M,Cin], dw [128,Cin], db [128]); None where
    not wanted.  The residual's gradient is dy itself."""
    if not (want_dx or want_dw or want_db):
        raise ValueError("linear_train_backward: ask for at least one gradient")
    lib = _lib.load()
    x, weight, dy = _chk(x, "x"), _chk(weight, "weight"), _chk(dy, "dy")
    m, cin, cout = _linear_train_dims(x, weight, "linear_train_backward")
    if dy.shape != (m, cout):
        raise ValueError(f"linear_train_backward: dy must be [{m},{cout}], got {tuple(dy.shape)}")
    dx, dw, db = _out(want_dx, x.device, m, cin), _out(want_dw, x.device, cout, cin), _out(want_db, x.device, cout)
    ws = _train_workspace(lib.pdsc_linear_train_workspace_bytes(m, cin, cout), x.device)
    _lib.check(lib.pdsc_linear_train_backward(_p(x), _p(weight), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), ws.numel() * 8, m, cin, cout,
                                              _stream()), "pdsc_linear_train_backward")
    return dx, dw, db


def _qkv_train_dims(x, weights, what: str) -> int:
    c = LINEAR_TRAIN_COUT
    if x.dim() != 2 or x.shape[1] != c or x.shape[0] < 1:
        raise ValueError(f"{what}: x must be [M,{c}] with M >= 1, got {tuple(x.shape)}")
    for w in weights:
        if w.shape != (c, c):
            raise ValueError(f"{what}: the three weights must be [{c},{c}], got {tuple(w.shape)}")
    return x.shape[0]


@_on_device
def qkv_train_forward(x, wq, bq, wk, bk, wv, bv, q_scale: float):
    """qkv [M,384] = (q_scale (x wq^T + bq) | x wk^T + bk | x wv^T + bv) in one launch (pdsc_qkv_train_forward): the rows
    sc_attention_lse takes; x [M,128], weights [128,128], biases [128]."""
    lib = _lib.load()
    x = _chk(x, "x")
    wq, wk, wv = _chk(wq, "wq"), _chk(wk, "wk"), _chk(wv, "wv")
    bq, bk, bv = _chk(bq, "bq"), _chk(bk, "bk"), _chk(bv, "bv")
    m = _qkv_train_dims(x, (wq, wk, wv), "qkv_train_forward")
    for b in (bq, bk, bv):
        if b.shape != (LINEAR_TRAIN_COUT,):
            raise ValueError(f"qkv_train_forward: the three biases must be [{LINEAR_TRAIN_COUT}], got {tuple(b.shape)}")
    qkv = torch.empty(m, 3 * LINEAR_TRAIN_COUT, device=x.device, dtype=torch.float32)
    _lib.check(lib.pdsc_qkv_train_forward(_p(x), _p(wq), _p(bq), _p(wk), _p(bk), _p(wv), _p(bv), float(q_scale), _p(qkv), m, _stream()),
               "pdsc_qkv_train_forward")
    return qkv


@_on_device
def qkv_train_backward(x, wq, wk, wv, q_scale: float, dqkv, want=(True,) * 7):
    """Backward of qkv_train_forward (pdsc_qkv_train_backward): dqkv [M,384] -> (dx [M,128], dwq, dbq, dwk, dbk, dwv, dbv) of the
    UN-scaled parameters; `want`: seven flags in that order, None where not wanted."""
    want = tuple(bool(w) for w in want)
    if len(want) != 7 or not any(want):
        raise ValueError("qkv_train_backward: `want` takes seven flags, at least one of them set")
    lib = _lib.load()
    x, dqkv = _chk(x, "x"), _chk(dqkv, "dqkv")
    wq, wk, wv = _chk(wq, "wq"), _chk(wk, "wk"), _chk(wv, "wv")
    m = _qkv_train_dims(x, (wq, wk, wv), "qkv_train_backward")
    c = LINEAR_TRAIN_COUT
    if dqkv.shape != (m, 3 * c):
        raise ValueError(f"qkv_train_backward: dqkv must be [{m},{3 * c}], got {tuple(dqkv.shape)}")
    shapes = ((m, c), (c, c), (c,), (c, c), (c,), (c, c), (c,))
    outs = [_out(w, x.device, *s) for w, s in zip(want, shapes)]
    ws = _train_workspace(lib.pdsc_qkv_train_workspace_bytes(m), x.device)
    _lib.check(lib.pdsc_qkv_train_backward(_p(x), _p(wq), _p(wk), _p(wv), float(q_scale), _p(dqkv), *(_p(o) for o in outs), _p(ws),
                                           ws.numel() * 8, m, _stream()), "pdsc_qkv_train_backward")
    return tuple(outs)


def _head_train_dims(x, w0, b0, w1, b1, w2, what: str) -> int:
    c, hd = LINEAR_TRAIN_COUT, HEAD_HIDDEN
    if x.dim() != 2 or x.shape[1] != c or x.shape[0] < 1:
        raise ValueError(f"{what}: feat must be [M,{c}] with M >= 1, got {tuple(x.shape)}")
    for t, shape, name in ((w0, (hd, c), "w0"), (b0, (hd,), "b0"), (w1, (hd, hd), "w1"), (b1, (hd,), "b1"), (w2, (1, hd), "w2")):
        if t.shape != shape:
            raise ValueError(f"{what}: {name} must be {list(shape)}, got {tuple(t.shape)}")
    return x.shape[0]


@_on_device
def head_train_forward(x, w0, b0, w1, b1, w2, b2, want_pre: bool = False):
    """logits [M] = relu(relu(x w0^T + b0) w1^T + b1) . w2 + b2 in one launch (pdsc_head_train_forward): x [M,128], w0 [32,128],
    w1 [32,32], w2 [1,32], b0, b1 [32], b2 [1].  want_pre: -> (logits, pre [M,64]), the kernel's two pre-activations side by side
    (what its ReLU masks, and the backward's, are taken from); the training path does not ask for them."""
    lib = _lib.load()
    x, w0, b0, w1, b1, w2, b2 = (_chk(t, n) for t, n in ((x, "feat"), (w0, "w0"), (b0, "b0"), (w1, "w1"), (b1, "b1"), (w2, "w2"),
                                                         (b2, "b2")))
    m = _head_train_dims(x, w0, b0, w1, b1, w2, "head_train_forward")
    if b2.shape != (1,):
        raise ValueError(f"head_train_forward: b2 must be [1], got {tuple(b2.shape)}")
    logits = torch.empty(m, device=x.device, dtype=torch.float32)
    pre = _out(want_pre, x.device, m, 2 * HEAD_HIDDEN)
    _lib.check(lib.pdsc_head_train_forward(_p(x), _p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), _p(logits), _p(pre), m, _stream()),
               "pdsc_head_train_forward")
    return (logits, pre) if want_pre else logits


@_on_device
def head_train_backward(x, w0, b0, w1, b1, w2, dlogits, want=(True,) * 7):
    """Backward of head_train_forward (pdsc_head_train_backward): dlogits [M] -> (dfeat [M,128], dw0, db0, dw1, db1, dw2, db2);
    `want`: seven flags in that order, None where not wanted.  The hidden layers are recomputed, nothing of the forward is kept."""
    want = tuple(bool(w) for w in want)
    if len(want) != 7 or not any(want):
        raise ValueError("head_train_backward: `want` takes seven flags, at least one of them set")
    lib = _lib.load()
    x, w0, b0, w1, b1, w2, dlogits = (_chk(t, n) for t, n in ((x, "feat"), (w0, "w0"), (b0, "b0"), (w1, "w1"), (b1, "b1"), (w2, "w2"),
                                                              (dlogits, "dlogits")))
    m = _head_train_dims(x, w0, b0, w1, b1, w2, "head_train_backward")
    if dlogits.shape != (m,):
        raise ValueError(f"head_train_backward: dlogits must be [{m}], got {tuple(dlogits.shape)}")
    c, hd = LINEAR_TRAIN_COUT, HEAD_HIDDEN
    shapes = ((m, c), (hd, c), (hd,), (hd, hd), (hd,), (1, hd), (1,))
    outs = [_out(w, x.device, *s) for w, s in zip(want, shapes)]
    ws = _train_workspace(lib.pdsc_head_train_workspace_bytes(m), x.device)
    _lib.check(lib.pdsc_head_train_backward(_p(x), _p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(dlogits), *(_p(o) for o in outs), _p(ws),
                                            ws.numel() * 8, m, _stream()), "pdsc_head_train_backward")
    return tuple(outs)


# ---- the trainer's update (pdsc_optim_*; pointdsc_amd.optim builds the call structs) -----------------------------------------------
def optim_tensors_per_launch() -> int:
    """Rows of a step's table that one launch carries in its kernel arguments (pdsc_optim_tensors_per_launch)."""
    return int(_lib.load().pdsc_optim_tensors_per_launch())


def optim_state_bytes(kind: int, numels) -> int:
    """Bytes of the opaque state buffer of one parameter group (pdsc_optim_state_bytes); zero-filled = fresh."""
    arr = (C.c_longlong * len(numels))(*numels)
    n = int(_lib.load().pdsc_optim_state_bytes(kind, C.cast(arr, C.c_void_p), len(numels)))
    if n == 0:
        raise ValueError(f"optim_state_bytes: kind {kind}, {len(numels)} tensors: unsupported")
    return n


def optim_check(call) -> None:
    """Scan the present gradients of one group for NaN / Inf into the guard flag (pdsc_optim_check); enqueue only."""
    _lib.check(_lib.load().pdsc_optim_check(C.byref(call), _stream()), "pdsc_optim_check")


def optim_update(call) -> None:
    """Apply the rule to one group unless the guard flag is set (pdsc_optim_update); enqueue only."""
    _lib.check(_lib.load().pdsc_optim_update(C.byref(call), _stream()), "pdsc_optim_update")


def optim_finish(call, last: bool) -> None:
    """Commit one group's per-tensor step state; `last`: settle the guard block (pdsc_optim_finish); enqueue only."""
    _lib.check(_lib.load().pdsc_optim_finish(C.byref(call), int(bool(last)), _stream()), "pdsc_optim_finish")
