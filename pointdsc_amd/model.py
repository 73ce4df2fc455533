"""``PointDSC`` -- the reference's module boundary over the HIP hot path.

Mirrors reference ``models/PointDSC.py``:
  * constructor signature and defaults                               (:81-91)
  * parameter / buffer tree, hence the 358-entry ``state_dict`` of the released snapshots
    (``load_state_dict(torch.load(...), strict=False)`` works unchanged, evaluation/test_3DMatch.py:225)
  * ``forward(data: dict) -> {'final_trans', 'final_labels', 'M'}``   (:128-197) in testing mode and, without the
    'testing' key on an eval() module, the validation forward (M matrix + logits; forward only)
so the reference's callers (evaluation/test_3DMatch.py:53, demo_registration.py:117) only swap the import.

The sub-modules below are weight containers only; the arithmetic runs in libpointdsc_hip.so through
``pdsc_forward`` (include/pointdsc_hip.h).  There is no CPU or eager-PyTorch fallback: inputs
must be CUDA(ROCm) tensors and the library must be built, otherwise forward raises.

Extension over the reference: testing mode accepts bs >= 1 (the reference asserts bs == 1,
:210/:414); a batch is processed as bs independent pairs in the same kernels.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib

_NUM_CHANNELS = 128
# enum pdsc_attention_precision (include/pointdsc_hip.h)
ATTENTION_PRECISIONS = {"fp16x3": 0, "fp32": 1, "fp16x3_all": 2}
# r06: "bf16x3", the rounds 1-4 name, is no longer an alias -- the operand pairs are fp16 since r05 and do NOT have bf16's
# (= fp32's) range, so a caller who asks for the old mode by name gets an error that says so instead of silently different arithmetic
_RETIRED_PRECISIONS = {"bf16x3": "fp16x3", "bf16x3_all": "fp16x3_all"}
# enum pdsc_compat_format
COMPAT_FORMATS = {"f32": 0, "u16": 1}
# enum pdsc_layer_gemm
LAYER_GEMMS = {"f32": 0, "h3": 1}
# enum pdsc_att_leaves (an int >= 2 = that many leaves)
ATT_LEAVES = {"per_launch": 0, "canonical": 1}


def _conv(cin: int, cout: int) -> nn.Conv1d:
    return nn.Conv1d(cin, cout, kernel_size=1, bias=True)


class _NonLocalParams(nn.Module):
    """Weights of one SCNonlocal block (reference NonLocalBlock, models/PointDSC.py:9-25)."""

    def __init__(self, c: int):
        super().__init__()
        h = c // 2
        self.fc_message = nn.Sequential(_conv(c, h), nn.BatchNorm1d(h), nn.ReLU(inplace=True),
                                        _conv(h, h), nn.BatchNorm1d(h), nn.ReLU(inplace=True), _conv(h, c))
        self.projection_q = _conv(c, c)
        self.projection_k = _conv(c, c)
        self.projection_v = _conv(c, c)


class _EncoderParams(nn.Module):
    """Weights of the 12-layer encoder (reference NonLocalNet, models/PointDSC.py:48-63)."""

    def __init__(self, in_dim: int, num_layers: int, c: int):
        super().__init__()
        self.num_layers = num_layers
        self.blocks = nn.ModuleDict()
        self.layer0 = _conv(in_dim, c)
        for i in range(num_layers):
            self.blocks[f"PointCN_layer_{i}"] = nn.Sequential(_conv(c, c), nn.BatchNorm1d(c), nn.ReLU(inplace=True))
            self.blocks[f"NonLocal_layer_{i}"] = _NonLocalParams(c)


def _fold_bn(conv: nn.Conv1d, bn: Optional[nn.BatchNorm1d]):
    """Conv1d(k=1) followed by eval-mode BatchNorm1d as one affine map, folded in fp64."""
    w = conv.weight.detach()[:, :, 0].double()
    b = conv.bias.detach().double()
    if bn is not None:
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w = w * scale[:, None]
        b = (b - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
    return w, b


class PointDSC(nn.Module):
    def __init__(self, in_dim=6, num_layers=6, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10):
        super().__init__()
        if num_channels != _NUM_CHANNELS:
            raise ValueError(f"pointdsc_amd supports num_channels={_NUM_CHANNELS} (the released models); got {num_channels}")
        # limits of the HIP path (include/pointdsc_hip.h), checked here so that they do not surface at the first forward:
        # the first conv is packed with 16 input columns (the released models use in_dim = 6; the reference's data loaders
        # also build 9- and 12-column inputs, datasets/ThreeDMatch.py:299-312), one wavefront lane per neighbour, at most 32
        # power iterates kept
        if not 1 <= in_dim <= 16:
            raise ValueError(f"pointdsc_amd supports 1 <= in_dim <= 16 (released models: 6); got {in_dim}")
        if not 1 <= k <= 64:
            raise ValueError(f"pointdsc_amd supports 1 <= k <= 64 neighbours per seed (released models: 40); got {k}")
        if not 0 <= num_iterations <= 32:
            raise ValueError(f"pointdsc_amd supports 0 <= num_iterations <= 32 (released models: 10); got {num_iterations}")
        self.in_dim = in_dim
        self.num_layers = num_layers
        self.num_iterations = num_iterations
        self.ratio = ratio
        self.num_channels = num_channels
        self.inlier_threshold = inlier_threshold
        self.sigma = nn.Parameter(torch.tensor([1.0], dtype=torch.float32), requires_grad=True)
        self.sigma_spat = nn.Parameter(torch.tensor([sigma_d], dtype=torch.float32), requires_grad=False)
        self.k = k
        self.nms_radius = nms_radius
        self.encoder = _EncoderParams(in_dim, num_layers, num_channels)
        self.classification = nn.Sequential(_conv(num_channels, 32), nn.ReLU(inplace=True), _conv(32, 32),
                                            nn.ReLU(inplace=True), _conv(32, 1))
        for m in self.modules():  # same initialiser family as the reference (:116-121)
            if isinstance(m, nn.Conv1d):
                nn.init.xavier_normal_(m.weight, gain=1)
            elif isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        # Not a reference constructor argument (the signature stays the reference's): arithmetic of the two
        # attention contractions.  "fp16x3" = split-precision f16 MFMA, every operand as an fp16 hi + lo pair (default; ~2^-21
        # per product), "fp32" = exact fp32 MFMA.  ("bf16x3", the rounds 1-4 mode with fp32's range, is gone: asking for it raises.)  (Experiments builds of the
        # library also take "fp16x3_all": the point-wise GEMMs in split precision too -- an A/B record, rejected by the product
        # library.)
        # Module attributes only -- neither the module nor the library reads the environment.  Set before calling forward.
        self.attention_precision = "fp16x3"
        # storage of the N x N spatial-consistency matrix between its build and the attention launches (split-precision
        # modes): "u16" = unorm16 (|error| <= 7.6e-6; default): half the workspace and HBM stream, 4.6 % more pairs/s at
        # N=5000 (tools/ab_forward.py), features as close to the exact-fp32 path as with "f32" (2e-6), parity census
        # over every pair of the bench workloads equal to "f32"'s; "f32" = the reference's fp32
        # matrix, bit-exact
        self.compat_format = "u16"
        # arithmetic of the fc_message / PointCN GEMMs in the fused layer kernel (enum pdsc_layer_gemm): "h3" = fp16 hi /
        # scaled-lo split on the f16 matrix cores (default: ~2^-21 per product, measured closer to the fp64 chain than the
        # fp32 MFMA's own round-off; with it the attention -> layer -> layer hand-offs go in point-fragment order);
        # "f32" = v_mfma_f32_32x32x2_f32
        self.layer_gemm = "h3"
        # summation tree of the attention's key dimension (enum pdsc_att_leaves): "canonical" = a leaf count that depends on N alone,
        # so a pair's result is bit-identical whatever the batch it shares a launch with (1 GPU x 32 pairs == 8 GPUs x 4 pairs);
        # "per_launch" = one partial per key split of the launch plan (the r01-r04 bits: they move with the batch size, within the
        # contract; the fastest form); int 2..8: that many leaves (tuning)
        self.att_leaves = "canonical"
        # fc_message's first conv folded into the value projection (enum pdsc_value_fold): 1 = the attention contracts P V' over
        # 64 channels (V' = W1f Wv f, b' = W1f bv + b1f added after the merge) -- half the P V work, same three-MFMA split arithmetic;
        # 0 = the 128-channel value path.  Applies with the split-precision attention and layer_gemm = "h3" only: the config
        # carries 0 whenever the exact-fp32 attention (the range guard's fallback included) or the fp32 GEMMs run.  The library folds
        # calls of up to N = 16384 correspondences (PDSC_VALUE_FOLD_MAX_N, include/pointdsc_hip.h); larger calls keep 128 channels.
        self.value_fold = 1
        # fp16 range guard of the split-precision arithmetic (r06).  Every forward carries a device-side sentinel (workspace entry
        # "range_flag": one word per pair, set by any activation that reaches 65504 on its way into an fp16 hi / lo pair; the library
        # returns NaN poses for such pairs, never a plausible wrong motion).  What the MODULE does with it:
        #   "sync" (default for the plain call): wait for the forward, read the words, and if any is set warn, switch this module to the
        #           exact-fp32 arithmetic (kept) and re-run THIS call -- the caller gets the fp32 answer.  Costs one 4 x bs byte copy and
        #           makes the call synchronous, which the reference's evaluation loop is anyway (it reads every result back).
        #   "lazy": the words are copied to pinned memory behind the forward and looked at by a later call (or check_range()): the
        #           affected call has returned NaN poses by then; the module warns and switches to fp32 for the calls that follow.
        #           pipeline.InFlight always runs in this mode (its forwards must not synchronise).
        #   "off" : nothing is read back (the NaN poses of the library remain).
        self.range_guard = "sync"
        self._guard_override = None             # set by pipeline.InFlight for the duration of its calls
        self._range_pending = []                # lazy mode: (event, pinned words, call number)
        self._range_pool = []                   # pinned [bs] int32 buffers, recycled
        self._calls = 0
        self.range_fallbacks = 0                # how many calls the guard found out of range (diagnostics / tests)
        self._report_host = None                # pinned [bs] int32 the forward's last launch writes the range words into ("sync" guard)
        self._report_ok = True
        self._wpack: Optional[torch.Tensor] = None
        self._wsplit: Optional[torch.Tensor] = None
        self._wpack_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._h3_range_checked = False
        self.last_range_probe = None            # {activation kind: largest |value|} of the last range probe (PDSC_FORWARD_PROBE)
        self._tail: Dict[int, tuple] = {}       # workspace slot -> (high-priority tail stream, fork event, join event): pipeline.InFlight(tail_streams=True)
        self._workspaces: Dict[int, torch.Tensor] = {}      # one per in-flight slot (pointdsc_amd.pipeline.InFlight); slot 0 = the plain call
        self._ws_slot = 0

    # ------------------------------------------------------------------------------------------
    def _config(self) -> _lib.PdscConfig:
        # reference post_refinement picks its threshold by exact equality with 0.10 (:415-418)
        refine_thr = 0.10 if self.inlier_threshold == 0.10 else 1.2
        if self.attention_precision in _RETIRED_PRECISIONS:
            raise ValueError(f"attention_precision {self.attention_precision!r} was retired in library version 8: the split operands are fp16 "
                             f"pairs now ({_RETIRED_PRECISIONS[self.attention_precision]!r}: 22 mantissa bits, but fp16's range -- |activation| "
                             "< 65504, guarded per forward by model.range_guard); there is no mode with bf16's range any more, use "
                             f"{_RETIRED_PRECISIONS[self.attention_precision]!r} or 'fp32'")
        if self.attention_precision not in ATTENTION_PRECISIONS:
            raise ValueError(f"attention_precision must be one of ['fp16x3', 'fp32'], got {self.attention_precision!r}")
        if self.attention_precision == "fp16x3_all" and not _lib.load().pdsc_experiments_enabled():
            raise ValueError('attention_precision "fp16x3_all" (all-split layer GEMMs, an A/B record) exists in experiments builds of the '
                             "library only (python -m pointdsc_amd.build --experiments); the product accepts 'fp16x3' and 'fp32'")
        if self.compat_format not in COMPAT_FORMATS:
            raise ValueError(f"compat_format must be one of {sorted(COMPAT_FORMATS)}, got {self.compat_format!r}")
        if self.layer_gemm not in LAYER_GEMMS:
            raise ValueError(f"layer_gemm must be one of {sorted(LAYER_GEMMS)}, got {self.layer_gemm!r}")
        if isinstance(self.att_leaves, int) and not isinstance(self.att_leaves, bool) and 2 <= self.att_leaves <= 8:
            leaves = int(self.att_leaves)
        elif self.att_leaves in ATT_LEAVES:
            leaves = ATT_LEAVES[self.att_leaves]
        else:
            raise ValueError(f"att_leaves must be one of {sorted(ATT_LEAVES)} or an int in [2, 8], got {self.att_leaves!r}")
        if self.value_fold not in (0, 1) or isinstance(self.value_fold, float):
            raise ValueError(f"value_fold must be 0 or 1, got {self.value_fold!r}")
        fold = int(bool(self.value_fold) and self.attention_precision == "fp16x3" and self.layer_gemm == "h3")
        return _lib.PdscConfig(self.in_dim, self.num_layers, self.num_channels, self.num_iterations, self.k, 20,
                               float(self.inlier_threshold), float(self.nms_radius), float(refine_thr),
                               ATTENTION_PRECISIONS[self.attention_precision], COMPAT_FORMATS[self.compat_format],
                               LAYER_GEMMS[self.layer_gemm], leaves, fold)

    # The packed buffer is rebuilt after anything that can change weights through the nn.Module API
    # (load_state_dict, .to()/.cuda()/.float(), train()); after editing parameters in place call
    # invalidate_packed_weights() yourself.
    def invalidate_packed_weights(self) -> None:
        self._wpack = None
        self._wsplit = None
        self._wpack_key = None
        self._tensors = None
        self._frozen_fp = None

    def freeze_weights(self, frozen: bool = True) -> "PointDSC":
        """Promise that no parameter or buffer is edited IN PLACE until freeze_weights(False): the per-call fingerprint below (a walk
        over the 358 tensors' version counters, ~30 us of host time = 6 % of a one-pair N = 1000 call) is then taken once and reused.
        Everything that goes through the nn.Module API (load_state_dict, .to() / .cuda(), train()) still invalidates the packed
        weights; what a frozen module no longer notices is ``p.data.copy_(...)`` / an optimizer step on its tensors.  The reference's
        evaluation loops (evaluation/test_3DMatch.py:32-54) never touch the weights between calls: bench.py --latency freezes."""
        self._frozen = bool(frozen)
        self._frozen_fp = None
        return self

    def _weights_fingerprint(self) -> int:
        """Changes whenever a parameter or buffer is modified in place (optimizer step, ``p.data.copy_``, a sub-module's
        ``load_state_dict``): the sum of the tensors' version counters.  ~30 us per call (freeze_weights() caches it)."""
        if getattr(self, "_frozen", False):
            if getattr(self, "_frozen_fp", None) is None or getattr(self, "_tensors", None) is None:
                self._frozen = False
                try:
                    self._frozen_fp = self._weights_fingerprint()
                finally:
                    self._frozen = True
            return self._frozen_fp
        if getattr(self, "_tensors", None) is None:
            self._tensors = list(self.parameters()) + list(self.buffers())
        return sum([t._version for t in self._tensors]) + 31 * sum([t.data_ptr() & 0xFFFF for t in self._tensors[:4]])

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_packed_weights()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_packed_weights()
        return super().load_state_dict(*args, **kwargs)

    def train(self, mode: bool = True):
        self.invalidate_packed_weights()
        return super().train(mode)

    def packed_weights(self, device=None) -> torch.Tensor:
        """The flat fp32 buffer of include/pointdsc_hip.h (``enum pdsc_wsection``): BatchNorm folded,
        q pre-scaled, sigma / sigma_spat appended (read from the Parameters, so a checkpoint overrides
        the constructor's sigma_d exactly like in the reference)."""
        lib = _lib.load()
        device = device or self.sigma.device
        key = (str(device), self.sigma.data_ptr(), self._weights_fingerprint())
        if self._wpack is not None and self._wpack_key == key:
            return self._wpack
        cfg = self._config()
        total = int(lib.pdsc_wpack_floats(C.byref(cfg)))
        if total <= 0:
            raise RuntimeError("pdsc_wpack_floats: " + _lib.last_error())
        pack = torch.zeros(total, dtype=torch.float32, device=device)

        def put(section: str, layer: int, value: torch.Tensor):
            off = int(lib.pdsc_wpack_offset(C.byref(cfg), _lib.W[section], layer))
            if off < 0:
                raise RuntimeError(f"pdsc_wpack_offset({section},{layer}): " + _lib.last_error())
            flat = value.reshape(-1).to(device=device, dtype=torch.float32)
            pack[off:off + flat.numel()] = flat

        c = self.num_channels
        w0, b0 = _fold_bn(self.encoder.layer0, None)
        w0p = torch.zeros(c, 16, dtype=torch.float64, device=w0.device)
        w0p[:, :self.in_dim] = w0
        put("LAYER0_W", 0, w0p)
        put("LAYER0_B", 0, b0)
        qscale = math.log2(math.e) / math.sqrt(c)      # softmax runs in the log2 domain on pre-scaled q
        for i in range(self.num_layers):
            pcn = self.encoder.blocks[f"PointCN_layer_{i}"]
            nl = self.encoder.blocks[f"NonLocal_layer_{i}"]
            w, b = _fold_bn(pcn[0], pcn[1])
            put("PCN_W", i, w); put("PCN_B", i, b)
            wq, bq = _fold_bn(nl.projection_q, None)
            wk, bk = _fold_bn(nl.projection_k, None)
            wv, bv = _fold_bn(nl.projection_v, None)
            put("QKV_W", i, torch.cat([wq * qscale, wk, wv], 0)); put("QKV_B", i, torch.cat([bq * qscale, bk, bv], 0))
            w, b = _fold_bn(nl.fc_message[0], nl.fc_message[1])
            put("FC1_W", i, w); put("FC1_B", i, b)
            w, b = _fold_bn(nl.fc_message[3], nl.fc_message[4])
            put("FC2_W", i, w); put("FC2_B", i, b)
            w, b = _fold_bn(nl.fc_message[6], None)
            put("FC3_W", i, w); put("FC3_B", i, b)
        for sec, j in (("CLS1", 0), ("CLS2", 2), ("CLS3", 4)):
            w, b = _fold_bn(self.classification[j], None)
            put(sec + "_W", 0, w); put(sec + "_B", 0, b)
        put("SIGMA", 0, self.sigma.detach())
        put("SIGMA_SPAT", 0, self.sigma_spat.detach())
        self._wpack, self._wsplit, self._wpack_key = pack, None, key
        # H3 (layer_gemm = "h3") carries every operand of the fc_message / PointCN GEMMs as fp16 hi + lo: |x| must stay below
        # 65504.  Checked once per packing: the folded weights here, the activations after the first forward (_run).
        self._h3_range_checked = False
        if self.layer_gemm == "h3" or self.attention_precision != "fp32":
            # (r05: the split-precision attention and q|k|v projection carry their operands as fp16 hi + lo too)
            wmax = float(pack.abs().max())
            if not wmax < 3.0e4:
                warnings.warn(f"pointdsc_amd: folded weights reach |w| = {wmax:.3g}, outside the fp16 range of the split-precision "
                              "arithmetic; falling back to layer_gemm='f32' and attention_precision='fp32' for this module", RuntimeWarning)
                self.layer_gemm = "f32"
                self.attention_precision = "fp32"
        return pack

    def split_weights(self, device=None) -> torch.Tensor:
        """fp16 hi/lo split of the per-layer matrices for the split-precision GEMMs (pdsc_wsplit_build): built on the
        GPU from the packed buffer, once per packing."""
        pack = self.packed_weights(device)
        cfg = self._config()
        if self._wsplit is not None and cfg.value_fold and not getattr(self, "_wsplit_fold", 0):
            self._wsplit = None                 # built without the folded sections (enum pdsc_value_fold): rebuild with them
        if self._wsplit is None:
            lib = _lib.load()
            nb = int(lib.pdsc_wsplit_bytes(C.byref(cfg)))
            wsplit = torch.empty(max(nb, 16), dtype=torch.uint8, device=pack.device)
            with torch.cuda.device(pack.device):
                _lib.check(lib.pdsc_wsplit_build(C.byref(cfg), C.c_void_p(pack.data_ptr()), C.c_void_p(wsplit.data_ptr()) if wsplit is not None else None,
                                                 torch.cuda.current_stream().cuda_stream), "pdsc_wsplit_build")
            self._wsplit = wsplit
            self._wsplit_fold = int(cfg.value_fold)
        return self._wsplit

    def _get_workspace(self, nbytes: int, device) -> torch.Tensor:
        ws = self._workspaces.get(self._ws_slot)
        if ws is None or ws.device != device or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._workspaces[self._ws_slot] = ws
        self._workspace = ws                               # workspace_view(): intermediates of the LAST forward
        return ws

    # ------------------------------------------------------------------------------------------
    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, Optional[torch.Tensor]]:
        """data: corr_pos [bs,N,in_dim], src_keypts [bs,N,3], tgt_keypts [bs,N,3].
        With the key 'testing' (reference :145): final_trans [bs,4,4] (refined), final_labels [bs,N] (0/1 float), M None.
        Without it (validation forward, reference :158-163,:176,:190-191): final_trans = best seed hypothesis,
        final_labels = confidence logits, M [bs,N,N] feature similarity matrix.  Forward only, eval() mode.

        Ragged batches (testing mode; the reference's real evaluation has a different N per pair and therefore runs one pair
        per call, evaluation/test_3DMatch.py:126, models/PointDSC.py:210): either pass LISTS of per-pair tensors
        (corr_pos[i] [N_i,in_dim], src_keypts[i] / tgt_keypts[i] [N_i,3]) -- final_labels is then a list of [N_i] tensors --
        or padded tensors plus data['num_corr'] (sequence / 1-D tensor of the bs valid counts; rows past a pair's count are
        ignored, its final_labels are zero there).  Pair i's result is that of a call on its own N_i rows."""
        testing = "testing" in data.keys()
        if self.training:
            raise RuntimeError(
                "call .eval() first: BatchNorm is folded with its running statistics.  The train()-mode forward (batch "
                "statistics + autograd, reference libs/trainer.py:68-156) is pointdsc_amd.training.TrainablePointDSC (the same "
                "parameters and state_dict) or training.train_forward(model, data); the validation forward (eval() mode without "
                "the 'testing' key, libs/trainer.py:158-222) is supported here.")
        corr_pos, src_keypts, tgt_keypts = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
        if isinstance(corr_pos, (list, tuple)):
            return self._forward_list(list(corr_pos), list(src_keypts), list(tgt_keypts), testing)
        if not corr_pos.is_cuda:
            raise RuntimeError("pointdsc_amd has no CPU path: move the model and data to the GPU (model.cuda())")
        dev = corr_pos.device
        corr_pos = corr_pos.detach().to(torch.float32).contiguous()
        src_keypts = src_keypts.detach().to(device=dev, dtype=torch.float32).contiguous()
        tgt_keypts = tgt_keypts.detach().to(device=dev, dtype=torch.float32).contiguous()
        bs, n = corr_pos.shape[0], corr_pos.shape[1]
        if corr_pos.shape[2] != self.in_dim or src_keypts.shape != (bs, n, 3) or tgt_keypts.shape != (bs, n, 3):
            raise ValueError("bad input shapes for PointDSC.forward")
        counts = data.get("num_corr") if hasattr(data, "get") else None
        if counts is not None:
            counts = [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]
            if len(counts) != bs or min(counts) < 2 or max(counts) > n:
                raise ValueError(f"num_corr must hold {bs} counts in [2, {n}]")
            if all(c == n for c in counts):
                counts = None
        return self._run(corr_pos, src_keypts, tgt_keypts, testing, counts)

    def _forward_list(self, corr, src, tgt, testing):
        """Ragged batch given as lists of per-pair tensors: pad to the longest pair, run, cut the labels back."""
        if not (len(corr) == len(src) == len(tgt)) or not corr:
            raise ValueError("corr_pos, src_keypts and tgt_keypts must be lists of the same (non-zero) length")
        if not corr[0].is_cuda:
            raise RuntimeError("pointdsc_amd has no CPU path: move the model and data to the GPU (model.cuda())")
        dev = corr[0].device
        squeeze = [t.reshape(-1, t.shape[-1]) for t in corr]            # accept [N_i, d] and the reference's [1, N_i, d]
        counts = [int(t.shape[0]) for t in squeeze]
        n_max = max(counts)

        def pad(ts, width):
            out = torch.zeros(len(ts), n_max, width, device=dev, dtype=torch.float32)
            for i, t in enumerate(ts):
                t = t.detach().reshape(-1, width).to(device=dev, dtype=torch.float32)
                if t.shape[0] != counts[i]:
                    raise ValueError(f"pair {i}: corr_pos / src_keypts / tgt_keypts disagree on the number of correspondences")
                out[i, : counts[i]] = t
            return out

        res = self._run(pad(squeeze, self.in_dim), pad(src, 3), pad(tgt, 3), testing, None if min(counts) == n_max else counts)
        res["final_labels"] = [res["final_labels"][i, : counts[i]] for i in range(len(counts))]
        return res

    def _ragged_groups(self, counts):
        """Index groups that can share a launch.  Split-precision attention:
          * att_leaves = "canonical" (r06): a pair's bits must be those of the call on that pair alone, whose attention cuts
            its key tiles into pdsc_attention_leaf_count(N_i) leaves.  One launch has ONE leaf count (that of its longest pair), so only
            pairs of the same leaf-count class share a launch, and a pair with fewer than two tiles per leaf -- which a ragged launch
            would silently hand to the per-launch key split -- runs as its own (uniform) call;
          * otherwise the key split (planned from the group's size and its longest pair) must leave the group's shortest pair at
            least one 32-key tile per split.  Greedy over the pairs sorted by size.
        Exact fp32 attention: its kernel takes any mix of sizes (an empty key range of a short pair merges with weight 0)."""
        lib = _lib.load()
        # a pair with no more than k correspondences takes the reference's per-pair clamp k = min(k, num_corr - 1)
        # (models/PointDSC.py:250): one launch has one k, so such a pair runs as its own (uniform) call
        small = [[i] for i in range(len(counts)) if counts[i] <= self.k]
        rest = [i for i in range(len(counts)) if counts[i] > self.k]
        if not rest:
            return small
        if self.attention_precision == "fp32":
            return [sorted(rest, key=lambda i: -counts[i])] + small
        classes = {}
        if self.att_leaves == "canonical":
            for i in rest:
                c = int(lib.pdsc_attention_leaf_count(counts[i]))
                if (counts[i] + 31) // 32 < 2 * c:
                    small.append([i])
                else:
                    classes.setdefault(c, []).append(i)
        else:
            classes[0] = rest
        out = []
        for members in classes.values():
            order = sorted(members, key=lambda i: -counts[i])
            groups, cur = [], []
            for i in order:
                trial = cur + [i]
                ns = int(lib.pdsc_attention_split_default_split(len(trial), counts[trial[0]]))
                if cur and (counts[i] + 31) // 32 < ns:
                    groups.append(cur)
                    cur = [i]
                else:
                    cur = trial
            groups.append(cur)
            # a group whose plan (decided by its final size) still asks too much of its shortest pair sheds that pair
            for g in groups:
                while len(g) > 1 and (counts[g[-1]] + 31) // 32 < int(lib.pdsc_attention_split_default_split(len(g), counts[g[0]])):
                    out.append([g.pop()])
                out.append(g)
        return out + small

    @staticmethod
    def _forward_call(cfg, wpack, wsplit, inputs, bs, n, num_seeds, ws) -> _lib.PdscForwardCall:
        """struct pdsc_forward_call with what every mode needs; the caller sets the mode and its optional fields.  The struct holds
        addresses only: the tensors stay the caller's to keep alive."""
        corr_pos, src_keypts, tgt_keypts = inputs
        return _lib.PdscForwardCall(
            cfg=C.pointer(cfg), wpack=wpack.data_ptr(), wsplit=wsplit.data_ptr() if wsplit is not None else None,
            corr_pos=corr_pos.data_ptr(), src_keypts=src_keypts.data_ptr(), tgt_keypts=tgt_keypts.data_ptr(),
            bs=bs, N=n, num_seeds=num_seeds, workspace=ws.data_ptr(), workspace_bytes=ws.numel())

    def _run(self, corr_pos, src_keypts, tgt_keypts, testing, counts=None, _in_fallback=False):
        lib = _lib.load()
        dev = corr_pos.device
        bs, n = corr_pos.shape[0], corr_pos.shape[1]
        if counts is not None:
            if not testing:
                raise NotImplementedError("ragged batches are supported in testing mode only (the validation forward returns an N x N matrix per pair)")
            groups = self._ragged_groups(counts)
            if len(groups) > 1 or min(counts) <= self.k:      # too heterogeneous for one launch plan (or pairs of at most k rows): one call per group
                final_trans = torch.empty(bs, 4, 4, device=dev, dtype=torch.float32)
                final_labels = torch.zeros(bs, n, device=dev, dtype=torch.float32)
                for g in groups:
                    idx = torch.tensor(g, device=dev)
                    ng = max(counts[i] for i in g)
                    cg = [counts[i] for i in g]
                    r = self._run(corr_pos[idx, :ng].contiguous(), src_keypts[idx, :ng].contiguous(), tgt_keypts[idx, :ng].contiguous(),
                                  testing, None if min(cg) == ng else cg)
                    final_trans[idx] = r["final_trans"]
                    final_labels[idx, :ng] = r["final_labels"]
                return {"final_trans": final_trans, "final_labels": final_labels, "M": None}
        num_seeds = int(n * self.ratio)                       # python double arithmetic, as the reference (:174)
        if self.attention_precision != "fp32" and self.num_layers > 0:
            self.packed_weights(dev)                           # (re)packs if needed and resets the flag below
            if not self._h3_range_checked and self.attention_precision != "fp32":
                self._h3_range_checked = True
                self._h3_range_probe(corr_pos, src_keypts, tgt_keypts, counts)      # first forward after packing: may switch to "f32" / "fp32"
        cfg = self._config()
        with torch.cuda.device(dev):
            wpack = self.packed_weights(dev)
            wsplit = self.split_weights(dev) if self.attention_precision != "fp32" else None
            nbytes = int(lib.pdsc_workspace_bytes(C.byref(cfg), bs, n, num_seeds))
            if nbytes == 0:
                raise RuntimeError(f"unsupported problem size bs={bs} N={n} seeds={num_seeds}: " + _lib.last_error())
            ws = self._get_workspace(nbytes, dev)
            final_trans = torch.empty(bs, 4, 4, device=dev, dtype=torch.float32)
            final_labels = torch.empty(bs, n, device=dev, dtype=torch.float32)
            call = self._forward_call(cfg, wpack, wsplit, (corr_pos, src_keypts, tgt_keypts), bs, n, num_seeds, ws)
            call.mode = _lib.FORWARD_TESTING if testing else _lib.FORWARD_VALIDATION
            call.final_trans, call.final_labels = final_trans.data_ptr(), final_labels.data_ptr()
            M = None
            if not testing:
                M = torch.empty(bs, n, n, device=dev, dtype=torch.float32)
                call.M, call.ldM = M.data_ptr(), n
            if counts is not None:
                seeds_per = [int(c * self.ratio) for c in counts]
                if min(seeds_per) < 1:
                    raise ValueError("every pair needs int(num_corr * ratio) >= 1 seeds (the reference fails on an empty seed set)")
                cnt = torch.tensor([counts, seeds_per], dtype=torch.int32).to(dev, non_blocking=False)
                if not hasattr(self, "_last_counts"):
                    self._last_counts = {}
                self._last_counts[self._ws_slot] = cnt      # (keeps the device arrays alive until the slot's next call: the launches are asynchronous)
                call.num_corr, call.num_seeds_per_pair, call.n_min = cnt[0].data_ptr(), cnt[1].data_ptr(), min(counts)
            tail = self._tail.get(self._ws_slot) if testing else None
            if tail is not None:
                # encoder on the current stream, the latency-bound tail on the slot's high-priority stream
                call.tail_stream, call.fork_event, call.join_event = tail[0].cuda_stream, tail[1].cuda_event, tail[2].cuda_event
            # "sync" range guard of a testing forward: the last launch writes the pairs' range words straight into pinned host memory
            # (pdsc_forward_call.range_report) -- no device-to-host copy of our own, only the wait
            report = None
            if (testing and wsplit is not None and not _in_fallback and (self._guard_override or self.range_guard) == "sync"
                    and self._report_ok and not torch.cuda.is_current_stream_capturing()):
                report = self._report_buffer(bs)
                call.range_report = report.data_ptr()
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib.pdsc_forward(C.byref(call), stream)
            if rc == _lib.ERR_ARG and report is not None:
                # rejected by the checks in front of the first launch, so nothing is enqueued yet: once more without the buffer.  If
                # that passes, pinned memory is not device-mapped on this platform: the copy path of _guard_after_forward from now on
                call.range_report = None
                rc = lib.pdsc_forward(C.byref(call), stream)
                if rc == 0:
                    self._report_ok, report = False, None
        _lib.check(rc, "pdsc_forward")
        res = {"final_trans": final_trans, "final_labels": final_labels, "M": M}
        if wsplit is not None and not _in_fallback:
            redo = self._guard_after_forward(ws, cfg, bs, n, num_seeds, dev, report)
            if redo:
                # exact-fp32 arithmetic from here on (kept for this module, like the range probe's fallback): same inputs, same call
                return self._run(corr_pos, src_keypts, tgt_keypts, testing, counts, _in_fallback=True)
        return res

    # ------------------------------------------------------------------------------------------
    def _flag_view(self, ws, cfg, bs, n, num_seeds):
        off = int(_lib.load().pdsc_workspace_offset(C.byref(cfg), bs, n, num_seeds, b"range_flag"))
        if off < 0:
            raise RuntimeError("libpointdsc_hip.so has no 'range_flag' workspace entry (library older than the module)")
        return ws[off:off + 4 * bs].view(torch.int32)

    def _to_exact_fp32(self, why: str) -> None:
        warnings.warn("pointdsc_amd: " + why + "; this module now uses attention_precision='fp32', layer_gemm='f32' (exact fp32, ~3.5x "
                      "slower; set the attributes back after fixing the input scale or the checkpoint)", RuntimeWarning)
        self.layer_gemm = "f32"
        self.attention_precision = "fp32"

    def _report_buffer(self, bs: int) -> torch.Tensor:
        if self._report_host is None or self._report_host.numel() < bs:
            self._report_host = torch.zeros(max(bs, 32), dtype=torch.int32).pin_memory()
        return self._report_host

    def _guard_after_forward(self, ws, cfg, bs, n, num_seeds, dev, report=None) -> bool:
        """Range sentinel of the forward just enqueued (see range_guard in __init__).  True = re-run this call in exact fp32."""
        mode = self._guard_override or self.range_guard
        if mode not in ("sync", "lazy", "off"):
            raise ValueError(f"range_guard must be 'sync', 'lazy' or 'off', got {mode!r}")
        self._calls += 1
        if mode == "off" or torch.cuda.is_current_stream_capturing():
            return False          # (inside a graph capture nothing of the guard can run: the library's NaN poses remain)
        self._poll_range(block=False)
        if report is not None:
            torch.cuda.current_stream(dev).synchronize()
            bad = report[:bs].numpy().nonzero()[0].tolist()
            if not bad:
                return False
            self.range_fallbacks += 1
            self._to_exact_fp32(f"activations of pair(s) {bad} of this batch reached the fp16 range (|x| >= 65504) of the split-precision "
                                "arithmetic; re-running this call in exact fp32")
            return True
        flags = self._flag_view(ws, cfg, bs, n, num_seeds)
        host = next((t for t in self._range_pool if t.numel() >= bs), None)
        if host is not None:
            self._range_pool.remove(host)
        else:
            host = torch.empty(max(bs, 32), dtype=torch.int32).pin_memory()
        host[:bs].copy_(flags, non_blocking=True)
        if mode == "lazy":
            ev = torch.cuda.Event()
            ev.record()
            self._range_pending.append((ev, host, bs, self._calls))
            return False
        torch.cuda.current_stream(dev).synchronize()
        bad = host[:bs].numpy().nonzero()[0].tolist()
        self._range_pool.append(host)
        if not bad:
            return False
        self.range_fallbacks += 1
        self._to_exact_fp32(f"activations of pair(s) {bad} of this batch reached the fp16 range (|x| >= 65504) of the split-precision "
                            "arithmetic; re-running this call in exact fp32")
        return True

    def _poll_range(self, block: bool) -> None:
        keep = []
        for ev, host, bs, call in self._range_pending:
            if block:
                ev.synchronize()
            if not ev.query():
                keep.append((ev, host, bs, call))
                continue
            bad = host[:bs].numpy().nonzero()[0].tolist()
            self._range_pool.append(host)
            if bad and self.attention_precision != "fp32":
                self.range_fallbacks += 1
                self._to_exact_fp32(f"forward number {call} of this module left the fp16 range (|x| >= 65504) of the split-precision arithmetic on "
                                    f"pair(s) {bad}: the poses it returned for them are NaN")
        self._range_pending = keep

    def check_range(self) -> int:
        """Wait for the forwards whose range words are still in flight ('lazy' guard) and apply them; returns range_fallbacks."""
        self._poll_range(block=True)
        return self.range_fallbacks

    RANGE_KINDS = ("layer0", "PointCN", "q|k|v", "message", "fc_message hidden 1", "fc_message hidden 2", "feature")

    def _h3_range_probe(self, corr_pos, src_keypts, tgt_keypts, counts=None) -> None:
        """layer_gemm = "h3" carries every operand of the fc_message / PointCN GEMMs as fp16 hi + lo, and (r05) so do the split-precision
        attention and q|k|v projection: EVERY activation of the chain, hidden ones included, must stay below 65504.  Once per weight packing, before the first forward: the encoder with the fp32
        GEMMs, one launch per conv, and the largest |value| of every activation kind over all layers (pdsc_forward, PDSC_FORWARD_PROBE;
        one device -> host copy of 8 floats).  Out of range (or NaN): warn and keep layer_gemm = "f32" for this module.
        A heuristic, not a proof: it sees the first input only -- a later input with much larger activations is not re-checked
        (set model.layer_gemm = "f32" yourself for checkpoints whose activations approach 1e4)."""
        lib = _lib.load()
        dev = corr_pos.device
        bs, n = corr_pos.shape[0], corr_pos.shape[1]
        num_seeds = max(int(n * self.ratio), 1)
        cfg = self._config()
        if counts is not None:
            # ragged batch: the probe runs the padded layout as a uniform batch, so the padding rows (any values, NaN included, by
            # contract) are replaced by zeros in copies -- nothing of the probe may depend on them
            keep = (torch.arange(n, device=dev)[None, :] < torch.tensor(counts, device=dev)[:, None])[:, :, None]
            corr_pos, src_keypts, tgt_keypts = (torch.where(keep, t, torch.zeros_like(t)) for t in (corr_pos, src_keypts, tgt_keypts))
        with torch.cuda.device(dev):
            wpack = self.packed_weights(dev)
            if self.attention_precision == "fp32":   # (the weight check at packing already fell back)
                return
            wsplit = self.split_weights(dev)
            nbytes = int(lib.pdsc_workspace_bytes(C.byref(cfg), bs, n, num_seeds))
            if nbytes == 0:
                return                               # (the forward itself reports the unsupported size)
            ws = self._get_workspace(nbytes, dev)
            absmax = torch.zeros(8, device=dev, dtype=torch.float32)
            call = self._forward_call(cfg, wpack, wsplit, (corr_pos, src_keypts, tgt_keypts), bs, n, num_seeds, ws)
            call.mode, call.absmax = _lib.FORWARD_PROBE, absmax.data_ptr()
            rc = lib.pdsc_forward(C.byref(call), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pdsc_forward")
        vals = absmax[: len(self.RANGE_KINDS)].tolist()
        self.last_range_probe = dict(zip(self.RANGE_KINDS, vals))
        bad = [(k, v) for k, v in zip(self.RANGE_KINDS, vals) if not v < 3.0e4]
        if bad and self.layer_gemm == "h3":
            warnings.warn("pointdsc_amd: activations reach " + ", ".join(f"{v:.3g} ({k})" for k, v in bad) + ", outside the fp16 range of "
                          "layer_gemm='h3'; using layer_gemm='f32' (kept for this module)", RuntimeWarning)
            self.layer_gemm = "f32"
        # r05: the attention's Q / K / V / P operands and the q|k|v projection's activations (= the PointCN output) are fp16 hi + lo
        bad_att = [(k, v) for k, v in bad if k in ("PointCN", "q|k|v")] or [(k, v) for k, v in bad if not v == v]
        if bad_att:
            warnings.warn("pointdsc_amd: activations reach " + ", ".join(f"{v:.3g} ({k})" for k, v in bad_att) + ", outside the fp16 range of "
                          "the split-precision attention; using attention_precision='fp32' (kept for this module)", RuntimeWarning)
            self.attention_precision = "fp32"

    def workspace_view(self, name: str, bs: int, n: int, dtype=torch.float32) -> torch.Tensor:
        """Intermediate of the LAST forward (parity tests): flat view into the workspace from `name` on."""
        lib = _lib.load()
        cfg = self._config()
        off = int(lib.pdsc_workspace_offset(C.byref(cfg), bs, n, int(n * self.ratio), name.encode()))
        if off < 0 or self._workspace is None:
            raise KeyError(name)
        return self._workspace[off:].view(torch.uint8)[: (self._workspace.numel() - off) // 4 * 4].view(dtype)
