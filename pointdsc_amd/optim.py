"""The trainer's update on the device: ``DeviceAdam`` and ``DeviceSGD``.

Both are ``torch.optim.Optimizer`` subclasses (parameter groups and ``ExponentialLR`` work unchanged) whose ``step()`` enqueues the
library's multi-tensor launches (include/pointdsc_hip.h, "the trainer's update on the device": the rule, bit for bit) on the
current stream and reads nothing back: the reference's guard -- skip the update when any gradient has a non-finite element,
libs/trainer.py:123-130 -- is decided on the device and counted in a device counter (``skipped_steps()``).  A step costs
3 ceil(tensors / ops.optim_tensors_per_launch()) launches per parameter group whatever the tensors' sizes, and parameters and
gradients stay where autograd put them (``zero_grad(set_to_none=True)``, the default, is fine).

``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam`` / ``torch.optim.SGD``'s format both ways.  They replace the
base class's versions: the moments and step counts live in the device state buffer, so ``optimizer.state`` is NOT populated
(``optimizer.state[p]`` is empty; read ``state_dict()`` instead) and the base class's state_dict hooks do not fire.
"""
from __future__ import annotations

import copy
from typing import Dict, List

import numpy as np
import torch

from . import _lib, ops

__all__ = ["DeviceAdam", "DeviceSGD"]

_STEP_BYTES = 32          # per-tensor step state {b1pow, b2pow (fp64), step (int64), unused} at the head of a group's state buffer


class _DeviceOptimizer(torch.optim.Optimizer):
    _KIND = -1
    _REFUSED: Dict[str, object] = {}          # option -> the only value it may have

    def __init__(self, params, defaults, guard: bool):
        self.guard = bool(guard)
        self._groups: List[dict] = []         # per parameter group: state buffer, numels, float offsets of m / buf
        self._guard_block = None              # device int32 [4]: flag, skipped steps, calls, unused
        self._device = None
        super().__init__(params, defaults)

    # ---- construction ---------------------------------------------------------------------------------------------------------
    def _check_group(self, group: dict) -> None:
        raise NotImplementedError

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            for name, only in self._REFUSED.items():
                if group.get(name, only) != only:
                    raise ValueError(f"{type(self).__name__}: {name}={group[name]!r} is not supported (only {only!r})")
            self._check_group(group)
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"{type(self).__name__}: parameters must be torch.float32, got {p.dtype}")
                if not p.is_contiguous():
                    raise ValueError(f"{type(self).__name__}: parameters must be contiguous")
                if p.numel() < 1:
                    raise ValueError(f"{type(self).__name__}: a parameter without elements")
        except Exception:
            self.param_groups.pop()
            raise
        self._groups.append(None)          # its device state is allocated when first needed: _ensure_state

    def _ensure_state(self) -> None:
        """Allocate the guard block and the state buffer of every group that has none yet (zero-filled = fresh)."""
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            if self._groups[gi] is not None:
                continue
            params = group["params"]
            for p in params:
                if not p.is_cuda:
                    raise RuntimeError(f"{name}: parameters must live on the GPU (pointdsc_amd has no CPU path)")
                if self._device is None:
                    self._device = p.device
                elif p.device != self._device:
                    raise ValueError(f"{name}: parameters on {p.device} and {self._device}; one device per optimiser")
            numels = [p.numel() for p in params]
            with torch.cuda.device(self._device):
                nbytes = ops.optim_state_bytes(self._KIND, numels)
                buf = torch.zeros(nbytes, dtype=torch.uint8, device=self._device)
                if self._guard_block is None:
                    self._guard_block = torch.zeros(4, dtype=torch.int32, device=self._device)
            per = 2 if self._KIND == _lib.OPTIM_ADAM else 1
            offs, off = [], _STEP_BYTES * len(numels) // 4
            for n in numels:
                offs.append(off)
                off += per * ((n + 3) // 4 * 4)
            assert off * 4 == nbytes, (off * 4, nbytes)
            self._groups[gi] = dict(buf=buf, numels=numels, offs=offs, rows=np.zeros((len(numels), 3), dtype=np.int64))

    def _hyper(self, group: dict) -> dict:
        raise NotImplementedError

    def _call(self, gi: int, group: dict) -> _lib.PdscOptimCall:
        rec = self._groups[gi]
        call = _lib.PdscOptimCall()
        call.kind, call.count = self._KIND, len(rec["numels"])
        call.tensors = rec["rows"].ctypes.data
        call.state, call.state_bytes = rec["buf"].data_ptr(), rec["buf"].numel()
        call.guard, call.use_guard = self._guard_block.data_ptr(), int(self.guard)
        for k, v in self._hyper(group).items():
            setattr(call, k, float(v))
        return call

    # ---- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """Enqueue one guarded update of every parameter that has a gradient, on the current stream; nothing is read back.
        A tensor whose ``.grad`` is None is left out (its step count does not advance); when no parameter has a gradient nothing
        is launched and no call is counted.  A gradient that is not contiguous is made contiguous (a copy) first.  ``lr`` and the
        other options are read from the parameter groups at every call.  Closures are refused."""
        if closure is not None:
            raise NotImplementedError(f"{type(self).__name__}.step takes no closure")
        self._ensure_state()
        calls, touched, keep = [], [], []
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            params, rec = group["params"], self._groups[gi]
            gptr, any_grad = [], False
            for p in params:
                g = p.grad
                if g is None:
                    gptr.append(0)
                    continue
                if g.dtype != torch.float32 or not g.is_cuda or g.is_sparse:
                    raise TypeError(f"{name}: gradients must be dense torch.float32 on the GPU, got {g.dtype} on {g.device}")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                gptr.append(g.data_ptr())
                touched.append(p)
                any_grad = True
            if not any_grad:
                continue
            rows = rec["rows"]
            rows[:, 0] = [p.data_ptr() for p in params]
            rows[:, 1] = gptr
            rows[:, 2] = rec["numels"]
            calls.append(self._call(gi, group))
        if not calls:
            return None
        with torch.cuda.device(self._device):
            if self.guard:
                for call in calls:          # every group's check before any group's update
                    ops.optim_check(call)
            for call in calls:
                ops.optim_update(call)
            for i, call in enumerate(calls):
                ops.optim_finish(call, last=i == len(calls) - 1)
        # the raw-pointer update is invisible to autograd: without this PointDSC's packed-weight fingerprint (the sum of
        # t._version, model.py) would not move and model.eval()(data) would run on stale packed weights
        torch.autograd.graph.increment_version(touched)
        return None

    def skipped_steps(self, sync: bool = False):
        """Calls of step() that the guard turned into no-ops: a device scalar (a snapshot in stream order, no synchronisation), or
        with ``sync=True`` an int (one read-back)."""
        self._ensure_state()
        v = self._guard_block[1].clone()
        return int(v.item()) if sync else v

    def steps_taken(self, sync: bool = False):
        """Calls of step() that launched, less the skipped ones; a device scalar, or with ``sync=True`` an int."""
        self._ensure_state()
        v = self._guard_block[2] - self._guard_block[1]
        return int(v.item()) if sync else v

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def _header(self, gi: int) -> torch.Tensor:
        rec = self._groups[gi]
        return rec["buf"][: _STEP_BYTES * len(rec["numels"])]

    def _moment(self, gi: int, li: int, which: int) -> torch.Tensor:
        """View of tensor li's m / buf (which = 0) or v (1) in group gi's state buffer, shaped like the parameter."""
        rec = self._groups[gi]
        n = rec["numels"][li]
        start = (rec["offs"][li] + which * ((n + 3) // 4 * 4)) * 4
        return rec["buf"][start: start + 4 * n].view(torch.float32).view_as(self.param_groups[gi]["params"][li])

    def _steps(self, gi: int) -> List[int]:
        return self._header(gi).view(torch.int64).view(-1, 4)[:, 2].cpu().tolist()

    def _tensor_state(self, gi: int, li: int, step: int, group: dict):
        raise NotImplementedError

    def _load_tensor_state(self, gi: int, li: int, saved, group: dict):
        """-> (step, b1pow, b2pow) after copying the saved moments in (zeros when there is no saved state)."""
        raise NotImplementedError

    def state_dict(self):
        """``torch.optim``'s format: {"state": {index: {...}}, "param_groups": [...]}, tensors cloned; a tensor that never took a
        step has no entry, as in torch.  Reads the per-tensor step counts back (one copy per group)."""
        self._ensure_state()
        state, groups, idx = {}, [], 0
        for gi, group in enumerate(self.param_groups):
            steps = self._steps(gi)
            packed = {k: copy.deepcopy(v) for k, v in group.items() if k != "params"}
            packed["params"] = list(range(idx, idx + len(group["params"])))
            groups.append(packed)
            for li, step in enumerate(steps):
                if step > 0:
                    s = self._tensor_state(gi, li, step, group)
                    if s:
                        state[idx + li] = s
            idx += len(group["params"])
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """Takes a state_dict of this class or of the torch optimiser it stands for.  The bias-correction products are rebuilt as
        beta ** step in Python floats (the running product differs from that in the last bits of an fp64)."""
        self._ensure_state()
        saved_groups, saved_state = state_dict["param_groups"], state_dict["state"]
        if len(saved_groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for group, saved in zip(self.param_groups, saved_groups):
            if len(saved["params"]) != len(group["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for name, only in self._REFUSED.items():
                if saved.get(name, only) != only:
                    raise ValueError(f"{type(self).__name__}: {name}={saved[name]!r} is not supported (only {only!r})")
        for gi, (group, saved) in enumerate(zip(self.param_groups, saved_groups)):
            for k, v in saved.items():
                if k != "params":
                    group[k] = copy.deepcopy(v)
            self._check_group(group)
            hdr = np.zeros((len(group["params"]), 4), dtype=np.float64)
            for li, pid in enumerate(saved["params"]):
                step, b1, b2 = self._load_tensor_state(gi, li, saved_state.get(pid), group)
                hdr[li, 0], hdr[li, 1] = b1, b2
                hdr[li].view(np.int64)[2] = step
            self._header(gi).copy_(torch.from_numpy(hdr.view(np.uint8).reshape(-1)))


def _torch_defaults(cls, **kw) -> dict:
    """The defaults dict of the torch optimiser `cls` for these options, checked by torch's own constructor: what a state_dict of
    ours must carry to load into it."""
    return dict(cls([torch.zeros(1)], **kw).defaults)


class DeviceAdam(_DeviceOptimizer):
    """``torch.optim.Adam`` (L2 weight_decay added to the gradient, no amsgrad, no maximize) with the trainer's finite-gradient
    guard, on the device.  ``guard=False`` applies the rule to whatever the gradients hold."""
    _KIND = _lib.OPTIM_ADAM
    _REFUSED = {"amsgrad": False, "maximize": False, "decoupled_weight_decay": False}

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, guard=True, *, amsgrad=False,
                 maximize=False):
        if amsgrad or maximize:
            raise ValueError("DeviceAdam: amsgrad and maximize are not supported")
        super().__init__(params, _torch_defaults(torch.optim.Adam, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), guard)

    def _check_group(self, group):
        _torch_defaults(torch.optim.Adam, lr=float(group["lr"]), betas=group["betas"], eps=group["eps"],
                        weight_decay=group["weight_decay"])

    def _hyper(self, group):
        return dict(lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                    weight_decay=group["weight_decay"], momentum=0.0)

    def _tensor_state(self, gi, li, step, group):
        return {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": self._moment(gi, li, 0).clone(),
                "exp_avg_sq": self._moment(gi, li, 1).clone()}

    def _load_tensor_state(self, gi, li, saved, group):
        m, v = self._moment(gi, li, 0), self._moment(gi, li, 1)
        if not saved:
            m.zero_()
            v.zero_()
            return 0, 0.0, 0.0
        step = int(round(float(saved["step"])))
        m.copy_(saved["exp_avg"])
        v.copy_(saved["exp_avg_sq"])
        b1, b2 = (float(b) for b in group["betas"])
        return step, b1 ** step, b2 ** step


class DeviceSGD(_DeviceOptimizer):
    """``torch.optim.SGD`` (momentum, L2 weight_decay; dampening 0, no nesterov, no maximize) with the trainer's finite-gradient
    guard, on the device."""
    _KIND = _lib.OPTIM_SGD
    _REFUSED = {"dampening": 0, "nesterov": False, "maximize": False}

    def __init__(self, params, lr, momentum=0, weight_decay=0, guard=True, *, dampening=0, nesterov=False, maximize=False):
        if dampening != 0 or nesterov or maximize:
            raise ValueError("DeviceSGD: dampening, nesterov and maximize are not supported")
        super().__init__(params, _torch_defaults(torch.optim.SGD, lr=lr, momentum=momentum, weight_decay=weight_decay), guard)

    def _check_group(self, group):
        _torch_defaults(torch.optim.SGD, lr=float(group["lr"]), momentum=group["momentum"], weight_decay=group["weight_decay"])

    def _hyper(self, group):
        return dict(lr=group["lr"], beta1=0.0, beta2=0.0, eps=0.0, weight_decay=group["weight_decay"], momentum=group["momentum"])

    def _tensor_state(self, gi, li, step, group):
        # torch.optim.SGD keeps a momentum_buffer only, and none without momentum
        return {"momentum_buffer": self._moment(gi, li, 0).clone()} if group["momentum"] != 0 else None

    def _load_tensor_state(self, gi, li, saved, group):
        buf = self._moment(gi, li, 0)
        if not saved or saved.get("momentum_buffer") is None:
            buf.zero_()
            return 0, 0.0, 0.0
        buf.copy_(saved["momentum_buffer"])
        return 1, 0.0, 0.0          # not the tensor's first step: the buffer is multiplied, not replaced
