"""The trainer's update on the device (pdsc_optim_*, ops.optim_*, pointdsc_amd.DeviceAdam / DeviceSGD, harness.train_epoch with
them).

Bit for bit: tests/optimizer_oracle.py holds the rule in numpy float32 (one rounding per product and per sum, correctly rounded
`/` and sqrt, the scalars rounded once) and asserts that no intermediate is a denormal; parameters, moments and step counts must
equal it after EVERY step.  Every parameter and every gradient is a view that starts one element into a 16-byte aligned buffer;
the sizes table, the model's table and two guard positions run again ON the boundary, through the 16-byte paths.
Against fp64: the UPDATE p_K - p_0 under linear_train_oracle.errors (err(X) = max|X - X64| / max|X64|) and train_oracle.bound
(max(4 e32, 128 2^-24)), e32 the same measure of torch.optim.Adam(foreach=False) / torch.optim.SGD in fp32 on the device from the
same inputs, truth the fp64 oracle.  Whole model: tests/test_train_forward.py's two-layer model.  Every figure is printed before it
is asserted.

Figures on one MI355X: profiles/f25_optimizer_errors.txt."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_train_oracle as LO  # noqa: E402
import optimizer_oracle as OO  # noqa: E402
import train_oracle as TO  # noqa: E402
import test_train_forward as TF  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("pdsc_optim_state_bytes", "pdsc_optim_tensors_per_launch", "pdsc_optim_check", "pdsc_optim_update", "pdsc_optim_finish")
SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 16384)
GAMMA = 0.99
STEPS = 5


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_signatures_and_defaults():
    import pointdsc_amd
    from pointdsc_amd import ops, optim
    for name in ("DeviceAdam", "DeviceSGD"):
        assert getattr(pointdsc_amd, name) is getattr(optim, name) and name in pointdsc_amd.__all__
        assert issubclass(getattr(optim, name), torch.optim.Optimizer)
    par = inspect.signature(optim.DeviceAdam.__init__).parameters
    assert list(par)[:7] == ["self", "params", "lr", "betas", "eps", "weight_decay", "guard"]
    assert (par["lr"].default, par["betas"].default, par["eps"].default, par["weight_decay"].default, par["guard"].default) == \
        (1e-3, (0.9, 0.999), 1e-8, 0, True)
    par = inspect.signature(optim.DeviceSGD.__init__).parameters
    assert list(par)[:6] == ["self", "params", "lr", "momentum", "weight_decay", "guard"]
    assert par["lr"].default is inspect.Parameter.empty
    assert (par["momentum"].default, par["weight_decay"].default, par["guard"].default) == (0, 0, True)
    for cls in (optim.DeviceAdam, optim.DeviceSGD):
        for fn in (cls.skipped_steps, cls.steps_taken):
            assert inspect.signature(fn).parameters["sync"].default is False
    for name in ("optim_state_bytes", "optim_tensors_per_launch", "optim_check", "optim_update", "optim_finish"):
        assert callable(getattr(ops, name))


def test_header_signatures_exports_and_struct_layout_agree(tmp_path):
    from pointdsc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert len(_lib.SIGNATURES[name][1]) == n, name
        assert hasattr(lib, name)
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 10
    assert (_lib.OPTIM_ADAM, _lib.OPTIM_SGD) == (0, 1) and re.search(r"PDSC_OPTIM_ADAM = 0, PDSC_OPTIM_SGD = 1", header)
    structs = {"pdsc_optim_tensor": _lib.PdscOptimTensor, "pdsc_optim_call": _lib.PdscOptimCall}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pointdsc_hip.h"', 'int main(void) {']
    want = []
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
        want.append((cname, "sizeof", str(C.sizeof(cls))))
        want += [(cname, f, str(getattr(cls, f).offset)) for f, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [tuple(ln.split()) for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
    assert C.sizeof(_lib.PdscOptimTensor) == 24


def _numels(*ns):
    return (C.c_longlong * len(ns))(*ns)


def test_size_queries():
    from pointdsc_amd import _lib, ops
    lib = _lib.load()
    q = lib.pdsc_optim_state_bytes
    cap = lib.pdsc_optim_tensors_per_launch()
    assert cap == ops.optim_tensors_per_launch() and 8 <= cap <= 160          # the rows must fit 4 KB of kernel arguments
    arr = _numels(5, 1024)
    ptr = C.cast(arr, C.c_void_p)
    assert q(2, ptr, 2) == 0 and q(-1, ptr, 2) == 0 and q(0, None, 2) == 0 and q(0, ptr, 0) == 0 and q(0, ptr, -1) == 0
    assert q(0, C.cast(_numels(5, 0), C.c_void_p), 2) == 0 and q(1, C.cast(_numels(-1), C.c_void_p), 1) == 0
    assert q(0, C.cast(_numels(1 << 31), C.c_void_p), 1) == 0
    last = {0: 0, 1: 0}
    for n in (1, 4, 5, 1024, 16384):
        for kind, per in ((0, 2), (1, 1)):
            got = q(kind, C.cast(_numels(n), C.c_void_p), 1)
            print(f"state bytes kind {kind} numel {n}: {got}")
            assert got >= per * 4 * n + 24 and got % 16 == 0 and got > last[kind] - (n == 4)
            last[kind] = got
    assert q(0, ptr, 2) > q(1, ptr, 2) > 0
    assert ops.optim_state_bytes(0, [5, 1024]) == q(0, ptr, 2)
    with pytest.raises(ValueError):
        ops.optim_state_bytes(0, [0])


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """Pointers that nobody may dereference: every rule returns PDSC_ERR_ARG with its text before the first HIP call."""
    from pointdsc_amd import _lib
    lib = _lib.load()
    dev = 4096          # a "device" address, never dereferenced
    inf, nan = float("inf"), float("nan")

    def attempt(entry, kind=0, count=2, rows=((dev, dev + 64, 5), (dev + 1024, 0, 1024)), state=dev, state_bytes=1 << 30, guard=dev,
                null_table=False, null_call=False, **hyper):
        table = (_lib.PdscOptimTensor * max(len(rows), 1))(*[_lib.PdscOptimTensor(*r) for r in rows])
        call = _lib.PdscOptimCall()
        call.kind, call.count = kind, count
        call.tensors = None if null_table else C.cast(table, C.c_void_p)
        call.state, call.state_bytes, call.guard, call.use_guard = state, state_bytes, guard, 1
        values = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, momentum=0.0)
        values.update(hyper)
        for k, v in values.items():
            setattr(call, k, v)
        ref = None if null_call else C.byref(call)
        rc = lib.pdsc_optim_finish(ref, 1, None) if entry == "finish" else getattr(lib, "pdsc_optim_" + entry)(ref, None)
        return rc, lib.pdsc_last_error()

    need = lib.pdsc_optim_state_bytes(0, C.cast(_numels(5, 1024), C.c_void_p), 2)
    cases = [
        (dict(null_call=True), b"null pointer"), (dict(null_table=True), b"null pointer"), (dict(state=None), b"null pointer"),
        (dict(guard=None), b"null pointer"), (dict(rows=((0, dev, 5), (dev, 0, 4))), b"null pointer"),
        (dict(rows=((dev + 2, dev, 5), (dev, 0, 4))), b"aligned"), (dict(rows=((dev, dev + 1, 5), (dev, 0, 4))), b"aligned"),
        (dict(state=dev + 4), b"aligned"), (dict(guard=dev + 2), b"aligned"),
        (dict(count=0), b"count=0"), (dict(count=-3), b"count=-3"),
        (dict(rows=((dev, dev, 0), (dev, 0, 4))), b"numel=0"), (dict(rows=((dev, dev, -7), (dev, 0, 4))), b"numel=-7"),
        (dict(state_bytes=need - 1), b"state of"), (dict(kind=2), b"unknown kind 2"), (dict(kind=-1), b"unknown kind -1"),
        (dict(lr=-1e-3), b"lr="), (dict(lr=nan), b"lr="), (dict(lr=inf), b"lr="),
        (dict(beta1=1.0), b"beta1="), (dict(beta1=-0.1), b"beta1="), (dict(beta1=nan), b"beta1="),
        (dict(beta2=1.0), b"beta2="), (dict(beta2=nan), b"beta2="), (dict(eps=-1e-8), b"eps="), (dict(eps=inf), b"eps="),
        (dict(weight_decay=-1e-6), b"weight_decay="), (dict(weight_decay=nan), b"weight_decay="),
        (dict(kind=1, momentum=-0.5), b"momentum="), (dict(kind=1, momentum=nan), b"momentum="),
        (dict(kind=1, lr=-1.0), b"lr="), (dict(kind=1, weight_decay=inf), b"weight_decay="),
    ]
    for entry in ("check", "update", "finish"):
        for kw, text in cases:
            rc, msg = attempt(entry, **kw)
            assert rc == _lib.ERR_ARG and text in msg and b"pdsc_optim_" + entry.encode() in msg, (entry, kw, rc, msg)
    assert attempt("finish", state_bytes=need - 1)[0] == _lib.ERR_ARG
    # `last` of the finish, with an otherwise good call
    table = (_lib.PdscOptimTensor * 1)(_lib.PdscOptimTensor(dev, dev, 5))
    call = _lib.PdscOptimCall()
    call.kind, call.count, call.tensors, call.state, call.state_bytes, call.guard = 0, 1, C.cast(table, C.c_void_p), dev, 1 << 20, dev
    call.lr, call.beta1, call.beta2, call.eps = 1e-3, 0.9, 0.999, 1e-8
    assert lib.pdsc_optim_finish(C.byref(call), 2, None) == _lib.ERR_ARG and b"last=2" in lib.pdsc_last_error()


def test_python_classes_refuse_what_they_cannot_do():
    from pointdsc_amd import DeviceAdam, DeviceSGD
    w = torch.nn.Parameter(torch.zeros(4, 3))
    w.grad = torch.ones(4, 3)
    for opt in (DeviceAdam([w]), DeviceSGD([w], lr=0.1)):
        with pytest.raises(NotImplementedError, match="closure"):
            opt.step(lambda: 0.0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            opt.step()
        with pytest.raises(RuntimeError, match="no CPU path"):
            opt.state_dict()
    for bad in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="torch.float32"):
            DeviceAdam([torch.nn.Parameter(torch.zeros(4, dtype=bad))])
        with pytest.raises(TypeError, match="torch.float32"):
            DeviceSGD([torch.nn.Parameter(torch.zeros(4, dtype=bad))], lr=0.1)
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError):
            DeviceAdam([w], **kw)
        with pytest.raises(ValueError):
            DeviceAdam([dict(params=[w], **kw)])
    for kw in (dict(nesterov=True, momentum=0.9), dict(dampening=0.1), dict(maximize=True)):
        with pytest.raises(ValueError):
            DeviceSGD([w], lr=0.1, **kw)
        with pytest.raises(ValueError):
            DeviceSGD([dict(params=[w], **kw)], lr=0.1)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            DeviceAdam([w], **kw)
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-1.0), dict(lr=0.1, weight_decay=-1.0)):
        with pytest.raises(ValueError):
            DeviceSGD([w], **kw)
    with pytest.raises(TypeError):
        DeviceSGD([w])          # lr has no default, as in torch


def test_exponential_lr_drives_the_groups():
    from pointdsc_amd import DeviceAdam, DeviceSGD
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2))
    for opt in (DeviceAdam([dict(params=[a]), dict(params=[b], lr=1e-2)], lr=1e-3),
                DeviceSGD([dict(params=[a]), dict(params=[b], lr=1e-2)], lr=1e-3, momentum=0.9)):
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
        assert [g["lr"] for g in opt.param_groups] == [1e-3, 1e-2]
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # "scheduler.step() before optimizer.step()": no CPU step exists
            sched.step()
        assert [g["lr"] for g in opt.param_groups] == [1e-3 * GAMMA, 1e-2 * GAMMA]


def _host_case(numels, seed):
    rng = np.random.default_rng(seed)
    params = []
    for n in numels:
        p = 0.1 * rng.standard_normal(n)
        p = np.where(np.abs(p) < 1e-3, 1e-3, p)
        params.append(p.astype(np.float32))
    return params


def _host_grads(numels, seed, zeros=True):
    """randn 10^U(-6, 0), |g| floored at 1e-12, every seventh element an exact zero."""
    rng = np.random.default_rng(seed)
    out = []
    for n in numels:
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 0.0, n)
        g = np.where(np.abs(g) < 1e-12, np.copysign(1e-12, g), g)
        if n > 8:
            g[:2] = (1e-12, -1e-12)
        if zeros:
            g[3::7] = 0.0
        out.append(g.astype(np.float32))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-6])
@pytest.mark.parametrize("kind", [OO.ADAM, OO.SGD])
def test_oracle_is_torchs_rule_in_fp64(kind, wd):
    """The fp64 oracle against torch.optim.Adam / SGD on the CPU in fp64, 5 steps, one tensor absent at step 2, lr under
    ExponentialLR: 1e-12 relative on parameters and moments -- the rule is torch's."""
    numels = (1, 7, 300)
    params = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in _host_case(numels, 3)]
    hyper = dict(lr=1e-3, weight_decay=wd)
    if kind == OO.ADAM:
        opt = torch.optim.Adam(params, foreach=False, **hyper)
    else:
        opt = torch.optim.SGD(params, momentum=0.9, foreach=False, **hyper)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
    orc = OO.Oracle(kind, [p.detach().numpy() for p in params], dtype=np.float64)
    worst = 0.0
    for s in range(5):
        grads = [g.astype(np.float64) for g in _host_grads(numels, 50 + s)]
        if s == 2:
            grads[1] = None
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.tensor(g)
        lr = opt.param_groups[0]["lr"]
        opt.step()
        orc.step(grads, lr=lr, weight_decay=wd, momentum=0.9)
        sched.step()
        for i, p in enumerate(params):
            pairs = [(p.detach().numpy(), orc.p[i])]
            st = opt.state[p]
            if kind == OO.ADAM:
                pairs += [(st["exp_avg"].numpy(), orc.m[i]), (st["exp_avg_sq"].numpy(), orc.v[i])]
                assert int(st["step"]) == orc.steps[i]
            else:
                pairs.append((st["momentum_buffer"].numpy(), orc.m[i]))
            for a, b in pairs:
                worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    print(f"oracle ({kind}, weight_decay {wd}) against torch in fp64: worst relative difference {worst:.3e}")
    assert orc.steps == [5, 4, 5] and worst <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the harness of the bit-for-bit tests
# ---------------------------------------------------------------------------------------------------------------------------
def _views(arrays, lead=1):
    """One device buffer; array i becomes a view that starts `lead` elements past a 16-byte boundary: ONE for the tests of the
    4-byte paths, none for the 16-byte paths that torch's own allocations take."""
    offs, off = [], 0
    for a in arrays:
        offs.append(off + lead)
        off += (a.size + lead + 3) // 4 * 4
    flat = np.zeros(off, dtype=np.float32)
    for a, o in zip(arrays, offs):
        flat[o:o + a.size] = a
    dev = torch.from_numpy(flat).to("cuda:0")
    assert dev.data_ptr() % 16 == 0
    return [dev[o:o + a.size] for a, o in zip(arrays, offs)]


def _bits(arrays):
    return np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]).view(np.uint32)


class Case:
    """Device optimiser and oracle side by side.  `groups`: list of lists of numel; `hypers`: per-group options."""

    def __init__(self, kind, groups, hypers, seed=1, guard=True, strict=True, common=None, lead=1):
        from pointdsc_amd import DeviceAdam, DeviceSGD
        self.kind, self.groups, self.hypers = kind, groups, hypers
        self.numels = [n for grp in groups for n in grp]
        host = _host_case(self.numels, seed)
        self.lead = lead
        self.params = [torch.nn.Parameter(v) for v in _views(host, lead)]
        assert all(p.data_ptr() % 16 == 4 * lead for p in self.params)
        at, spec = 0, []
        for grp, hy in zip(groups, hypers):
            spec.append(dict(params=self.params[at:at + len(grp)], **hy))
            at += len(grp)
        common = dict(common or {})
        if kind == OO.ADAM:
            self.opt = DeviceAdam(spec, guard=guard, **common)
        else:
            self.opt = DeviceSGD(spec, guard=guard, **dict(dict(lr=1e-3), **common))
        self.sched = torch.optim.lr_scheduler.ExponentialLR(self.opt, gamma=GAMMA)
        self.oracles = []
        at = 0
        for grp in groups:
            self.oracles.append(OO.Oracle(kind, host[at:at + len(grp)], guard=False, strict=strict))
            at += len(grp)
        self.guard = guard
        self.skipped = 0

    def step(self, grads):
        """grads: one numpy array or None per tensor (all groups, flat)."""
        present = [g for g in grads if g is not None]
        views = iter(_views(present, self.lead)) if present else iter(())
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else next(views)
            assert p.grad is None or p.grad.data_ptr() % 16 == 4 * self.lead
        self.opt.step()
        bad = any(not np.isfinite(g).all() for g in present)
        if self.guard and bad:
            self.skipped += 1
        elif present:
            at = 0
            for orc, grp, group in zip(self.oracles, self.groups, self.opt.param_groups):
                hy = dict(lr=group["lr"], weight_decay=group["weight_decay"])
                if self.kind == OO.ADAM:
                    hy.update(betas=group["betas"], eps=group["eps"])
                else:
                    hy.update(momentum=group["momentum"])
                orc.step(grads[at:at + len(grp)], **hy)
                at += len(grp)
        self.sched.step()

    def device_state(self):
        """-> (bits of p, bits of m / buf, bits of v, step counts), all groups flat."""
        def flat(tensors):
            return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy().view(np.uint32)
        self.opt._ensure_state()
        where = [(gi, li) for gi, grp in enumerate(self.groups) for li in range(len(grp))]
        p = flat(self.params)
        m = flat([self.opt._moment(gi, li, 0) for gi, li in where])
        v = flat([self.opt._moment(gi, li, 1) for gi, li in where]) if self.kind == OO.ADAM else np.zeros(0, np.uint32)
        return p, m, v, [s for gi in range(len(self.groups)) for s in self.opt._steps(gi)]

    def oracle_state(self):
        p = _bits([x for o in self.oracles for x in o.p])
        m = _bits([x for o in self.oracles for x in o.m])
        v = _bits([x for o in self.oracles for x in o.v]) if self.kind == OO.ADAM else np.zeros(0, np.uint32)
        return p, m, v, [s for o in self.oracles for s in o.steps]

    def compare(self, what):
        got, want = self.device_state(), self.oracle_state()
        diff = [int((g != w).sum()) for g, w in zip(got[:3], want[:3])]
        print(f"{what}: elements that differ from the oracle: p {diff[0]} of {got[0].size}, m {diff[1]}, v {diff[2]}; steps "
              f"{'equal' if got[3] == want[3] else 'DIFFER'}; skipped {self.opt.skipped_steps(sync=True)} (expected {self.skipped})")
        assert diff == [0, 0, 0] and got[3] == want[3], what
        assert self.opt.skipped_steps(sync=True) == self.skipped
        return got


def _absent(i, s, count):
    """The absence pattern of the tables: tensor 1 misses the first step, tensor 2 every step, the rest a pattern that moves."""
    if count < 4:
        return False
    return (i == 1 and s == 0) or i == 2 or (i > 3 and (i + s) % 5 == 4)


def _run_table(kind, numels, hyper, steps=STEPS, seed=1, common=None, lead=1):
    case = Case(kind, [list(numels)], [hyper], seed=seed, common=common, lead=lead)
    before = case.device_state()
    p0 = before[0]
    for s in range(steps):
        grads = _host_grads(numels, 1000 * seed + s)
        if s == 0:
            grads[0] = np.zeros_like(grads[0])          # an all-zero gradient on a fresh state: d = eps, p must not move
        grads = [None if _absent(i, s, len(numels)) else g for i, g in enumerate(grads)]
        case.step(grads)
        after = case.compare(f"{kind} {len(numels)} tensors {hyper}{' 16-byte aligned' if lead == 0 else ''} step {s + 1}")
        if s == 0:
            n0 = numels[0]
            assert np.array_equal(after[0][:n0], p0[:n0]) or hyper.get("weight_decay", 0) != 0
        if len(numels) >= 4:           # the absent neighbour stands still while the present ones moved
            lo, hi = sum(numels[:2]), sum(numels[:3])
            assert np.array_equal(after[0][lo:hi], before[0][lo:hi]) and after[3][2] == 0
            assert not np.array_equal(after[0][hi:hi + numels[3]], before[0][hi:hi + numels[3]])
        before = after
    return case


@functools.lru_cache(maxsize=None)
def _model_numels():
    from pointdsc_amd import training
    return tuple(p.numel() for p in training.TrainablePointDSC(num_layers=12).parameters() if p.requires_grad)


def _table(name):
    from pointdsc_amd import ops
    cap = ops.optim_tensors_per_launch()
    if name == "sizes":
        return SIZES
    if name == "model":
        numels = _model_numels()
        assert len(numels) == 249 and sum(numels) > 1_000_000
        return numels
    count = {"one": 1, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1}[name]
    return tuple((1, 3, 5, 300, 4, 1030, 17)[i % 7] for i in range(count))


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 1e-6])
@pytest.mark.parametrize("table", ["sizes", "one", "cap-1", "cap", "cap+1", "model"])
def test_adam_equals_the_oracle_bit_for_bit(table, wd):
    _run_table(OO.ADAM, _table(table), dict(lr=1e-3, weight_decay=wd))


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 1e-6])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_equals_the_oracle_bit_for_bit(momentum, wd):
    case = _run_table(OO.SGD, SIZES, dict(lr=1e-2, weight_decay=wd, momentum=momentum))
    assert case.oracles[0].steps[0] == STEPS and case.oracles[0].steps[1:3] == [STEPS - 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,table", [(OO.ADAM, "sizes"), (OO.ADAM, "model"), (OO.SGD, "sizes")])
def test_aligned_tensors_equal_the_oracle_bit_for_bit(kind, table):
    """The tables again with every parameter and gradient ON a 16-byte boundary: the 16-byte loads and stores that real training
    takes (torch's allocations are aligned), with the ragged last four of the sizes that are no multiple of 4."""
    hyper = dict(lr=1e-3, weight_decay=1e-6) if kind == OO.ADAM else dict(lr=1e-2, weight_decay=1e-6, momentum=0.9)
    _run_table(kind, _table(table), hyper, lead=0)


GUARD_SIZES = (257, 1) + SIZES[1:]          # the first tensor has many elements; the one-element tensor is the second
GUARD_GROUPS = [list(GUARD_SIZES), [5, 300]]
# where -> (tensor, element, elements between a 16-byte boundary and every tensor's start)
POSITIONS = {"first of first": (0, 0, 1), "last of last": (len(GUARD_SIZES) + 1, -1, 1), "one-element tensor": (1, 0, 1),
             "second group": (len(GUARD_SIZES) + 1, 17, 1),
             "aligned, element 4k+3": (0, 7, 0), "aligned, ragged end": (0, 256, 0)}          # the check's 16-byte branch and its tail


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [OO.ADAM, OO.SGD])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", list(POSITIONS))
def test_guard_skips_the_whole_step(where, value, kind):
    """[good, bad, good] over two parameter groups: the bad call changes nothing anywhere, counts one skipped step, advances no
    step count, and the result equals the oracle's two good steps (the bias correction did not advance)."""
    numels = [n for grp in GUARD_GROUPS for n in grp]
    extra = {} if kind == OO.ADAM else dict(momentum=0.9)
    ti, ei, lead = POSITIONS[where]
    case = Case(kind, GUARD_GROUPS, [dict(lr=1e-3, weight_decay=1e-6, **extra), dict(lr=3e-3, weight_decay=0.0, **extra)], seed=2,
                lead=lead)
    case.step(_host_grads(numels, 70))
    case.compare(f"guard {where} {value} {kind}: good step 1")
    before = case.device_state()
    bad = _host_grads(numels, 71)
    assert ti < len(numels) and (where != "one-element tensor" or numels[ti] == 1) and (where != "first of first" or numels[ti] > 1)
    assert where != "last of last" or ti == len(numels) - 1
    bad[ti][ei] = value
    case.step(bad)
    after = case.device_state()
    same = [bool(np.array_equal(a, b)) for a, b in zip(before[:3], after[:3])]
    print(f"guard {where} {value} {kind}: unchanged p {same[0]} m {same[1]} v {same[2]}, steps {after[3] == before[3]}, "
          f"skipped {case.opt.skipped_steps(sync=True)}, taken {case.opt.steps_taken(sync=True)}")
    assert all(same) and after[3] == before[3] == [1] * len(numels)
    assert case.opt.skipped_steps(sync=True) == 1 and case.opt.steps_taken(sync=True) == 1
    case.step(_host_grads(numels, 72))
    case.compare(f"guard {where} {value} {kind}: good step 2 after the skipped call")
    assert case.device_state()[3] == [2] * len(numels) and case.opt.steps_taken(sync=True) == 2


@pytest.mark.gpu
def test_a_nan_parameter_does_not_skip_and_guard_off_applies_the_rule():
    numels = list(SIZES)
    case = Case(OO.ADAM, [numels], [dict(lr=1e-3)], seed=4, strict=False)
    with torch.no_grad():
        case.params[3][7] = float("nan")
    case.oracles[0].p[3][7] = np.nan
    case.step(_host_grads(numels, 80))
    got, want = case.device_state(), case.oracle_state()
    nan_at = sum(numels[:3]) + 7
    ok = got[0] == want[0]
    print(f"NaN parameter: skipped {case.opt.skipped_steps(sync=True)}, p differs at {np.flatnonzero(~ok).tolist()} (NaN at {nan_at})")
    assert case.opt.skipped_steps(sync=True) == 0 and got[3] == [1] * len(numels)
    assert np.flatnonzero(~ok).tolist() in ([], [nan_at]) and np.isnan(got[0].view(np.float32)[nan_at])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])

    for kind, hyper in ((OO.ADAM, dict(lr=1e-3, weight_decay=1e-6)), (OO.SGD, dict(lr=1e-2, momentum=0.9))):
        off = Case(kind, [numels], [hyper], seed=5, guard=False)
        for s in range(3):
            off.step(_host_grads(numels, 90 + s))
            off.compare(f"guard=False {kind} step {s + 1}")
        assert off.opt.steps_taken(sync=True) == 3


@pytest.mark.gpu
def test_no_gradient_no_launch_and_repeat_runs_are_bit_identical():
    numels = _table("model")
    case = Case(OO.ADAM, [list(numels)], [dict(lr=1e-3)], seed=6)
    case.opt.step()          # no gradient anywhere: nothing launched, no call counted
    assert case.opt.steps_taken(sync=True) == 0 and int(case.opt._guard_block[2]) == 0
    runs = []
    for _ in range(2):
        c = Case(OO.ADAM, [list(numels)], [dict(lr=1e-3, weight_decay=1e-6)], seed=6)
        for s in range(3):
            c.step(_host_grads(numels, 100 + s))
        runs.append(c.device_state())
    same = [bool(np.array_equal(a, b)) for a, b in zip(runs[0][:3], runs[1][:3])]
    print(f"repeat: p {same[0]} m {same[1]} v {same[2]} steps {runs[0][3] == runs[1][3]}")
    assert all(same) and runs[0][3] == runs[1][3]
    # a gradient that is not contiguous is copied; the parameters' version counters move
    w = torch.nn.Parameter(torch.ones(6, 4, device="cuda:0"))
    from pointdsc_amd import DeviceSGD
    opt = DeviceSGD([w], lr=0.5)
    w.grad = torch.arange(24.0, device="cuda:0").view(4, 6).t()
    assert not w.grad.is_contiguous()
    version = w._version
    opt.step()
    assert torch.equal(w.detach(), 1.0 - 0.5 * torch.arange(24.0, device="cuda:0").view(4, 6).t()) and w._version > version


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("kind,wd", [(OO.ADAM, 1e-6), (OO.ADAM, 0.0), (OO.SGD, 1e-6)])
def test_update_against_fp64(kind, wd, K):
    from pointdsc_amd import DeviceAdam, DeviceSGD
    numels = [n for n in SIZES if n > 1] + [4099]
    host = _host_case(numels, 8)
    grads = [_host_grads(numels, 200 + s, zeros=False) for s in range(K)]
    lr = 1e-3 if kind == OO.ADAM else 1e-2
    truth = OO.Oracle(kind, host, dtype=np.float64, strict=False)

    def make(cls, **kw):
        params = [torch.nn.Parameter(torch.from_numpy(h.copy()).to("cuda:0")) for h in host]
        return params, cls(params, lr=lr, weight_decay=wd, **kw)

    if kind == OO.ADAM:
        sides = {"torch": make(torch.optim.Adam, foreach=False), "device": make(DeviceAdam)}
    else:
        sides = {"torch": make(torch.optim.SGD, momentum=0.9, foreach=False), "device": make(DeviceSGD, momentum=0.9)}
    scheds = {k: torch.optim.lr_scheduler.ExponentialLR(o, gamma=GAMMA) for k, (_, o) in sides.items()}
    for s in range(K):
        truth.step([g.astype(np.float64) for g in grads[s]], lr=lr * GAMMA ** s, weight_decay=wd, momentum=0.9)
        for k, (params, opt) in sides.items():
            for p, gr in zip(params, grads[s]):
                p.grad = torch.from_numpy(gr.copy()).to("cuda:0")
            opt.step()
            scheds[k].step()
    names = list(range(len(numels)))
    ref = {i: torch.from_numpy(truth.p[i] - host[i].astype(np.float64)) for i in names}
    errs = {}
    for k, (params, _) in sides.items():
        upd = {i: params[i].detach().double().cpu() - torch.from_numpy(host[i]).double() for i in names}
        errs[k] = LO.errors(upd, ref, names)
    e32 = max(errs["torch"].values())
    worst = max(errs["device"].values())
    print(f"update p_K - p_0 against fp64, {kind} weight_decay {wd} K {K}: e32 {e32:.3e} bound {TO.bound(e32):.3e} "
          f"device worst {worst:.3e}; per tensor " + " ".join(f"{numels[i]}:{errs['device'][i]:.2e}/{errs['torch'][i]:.2e}" for i in names))
    for i in names:
        assert errs["device"][i] <= TO.bound(e32), (numels[i], errs["device"][i], TO.bound(e32))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: state round trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [OO.ADAM, OO.SGD])
def test_state_round_trip_with_torch(kind):
    from pointdsc_amd import DeviceAdam, DeviceSGD
    numels = [1, 3, 257, 1025]
    host = _host_case(numels, 9)
    hyper = dict(lr=1e-3, weight_decay=1e-6)
    if kind == OO.SGD:
        hyper.update(momentum=0.9)
    tcls, dcls = (torch.optim.Adam, DeviceAdam) if kind == OO.ADAM else (torch.optim.SGD, DeviceSGD)
    tparams = [torch.nn.Parameter(torch.from_numpy(h.copy()).to("cuda:0")) for h in host]
    topt = tcls(tparams, foreach=False, **hyper)
    for s in range(3):
        for p, gr in zip(tparams, _host_grads(numels, 300 + s)):
            p.grad = torch.from_numpy(gr).to("cuda:0")
        topt.step()
    sd = topt.state_dict()

    case = Case(kind, [numels], [hyper], seed=9)
    with torch.no_grad():
        for p, t in zip(case.params, tparams):
            p.copy_(t)
    case.opt.load_state_dict(sd)
    back = case.opt.state_dict()
    keys = ("exp_avg", "exp_avg_sq") if kind == OO.ADAM else ("momentum_buffer",)
    assert sorted(back["state"]) == sorted(sd["state"]) == list(range(len(numels)))
    for i in back["state"]:
        assert sorted(back["state"][i]) == sorted(sd["state"][i])
        for k in keys:
            assert torch.equal(back["state"][i][k], sd["state"][i][k]) and back["state"][i][k].shape == tparams[i].shape
        if kind == OO.ADAM:
            assert float(back["state"][i]["step"]) == float(sd["state"][i]["step"]) == 3.0
    # ("initial_lr" is what this Case's own ExponentialLR wrote into the group; torch's optimiser above has no scheduler)
    assert [{k: v for k, v in grp.items() if k != "initial_lr"} for grp in back["param_groups"]] == sd["param_groups"]

    # the next device step equals the oracle seeded from that state
    orc = case.oracles[0]
    for i, p in enumerate(tparams):
        orc.p[i] = p.detach().cpu().numpy().copy()
        st = sd["state"][i]
        if kind == OO.ADAM:
            orc.seed(i, 3, st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        else:
            orc.seed(i, 1, st["momentum_buffer"].cpu().numpy())
    # (torch's SGD keeps no step count: after a load the device and the seeded oracle both count a tensor with a buffer from 1)
    case.step(_host_grads(numels, 310))
    case.compare(f"{kind}: the step after load_state_dict")

    # and back into a fresh torch optimiser
    fresh = tcls([torch.nn.Parameter(p.detach().clone()) for p in case.params], foreach=False, **hyper)
    out = case.opt.state_dict()
    fresh.load_state_dict(out)
    again = fresh.state_dict()
    for i in out["state"]:
        for k in keys:
            assert torch.equal(again["state"][i][k], out["state"][i][k])
        if kind == OO.ADAM:
            assert float(again["state"][i]["step"]) == 4.0
    for p in fresh.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    fresh.step()          # torch runs on with it


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: whole model
# ---------------------------------------------------------------------------------------------------------------------------
def _epoch_model(state):
    from pointdsc_amd import training
    return TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS), state).to("cuda:0").train()


@pytest.mark.gpu
def test_train_epoch_with_device_adam_learns_is_deterministic_skips_and_reads_nothing_back(monkeypatch):
    from pointdsc_amd import DeviceAdam, PointDSC, harness, synthetic
    state = synthetic.make_state_dict(PointDSC(num_layers=TF.LAYERS).state_dict(), seed=5)
    batch = synthetic.make_batch(4, 256, seed=60)
    steps = 30

    def run():
        model = _epoch_model(state)
        opt = DeviceAdam(model.parameters(), lr=1e-3)
        out = harness.train_epoch(model, [batch] * steps, opt)
        return out, {k: v.clone() for k, v in model.state_dict().items()}, opt.state_dict()

    first, sd1, od1 = run()
    second, sd2, od2 = run()
    print(f"train_epoch with DeviceAdam: loss {first['loss_first']:.6f} -> {first['loss_last']:.6f}, steps {first['steps']}, "
          f"skipped {first['skipped']}")
    assert first["steps"] == steps and first["skipped"] == 0 and first["loss_last"] < first["loss_first"]
    assert repr(first) == repr(second) and all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert sorted(od1["state"]) == sorted(od2["state"]) and len(od1["state"]) > 0
    for i in od1["state"]:
        assert all(torch.equal(od1["state"][i][k], od2["state"][i][k]) for k in od1["state"][i])

    # a non-finite gradient: skipped on the device; parameters and moments untouched
    model = _epoch_model(state)
    model.classification[4].bias.register_hook(lambda grad: torch.full_like(grad, float("nan")))
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = DeviceAdam(model.parameters(), lr=1e-3)
    out = harness.train_epoch(model, [batch], opt)
    print(f"NaN hook: skipped {out['skipped']} steps {out['steps']}")
    assert out["skipped"] == 1 and out["steps"] == 1
    assert all(torch.equal(params[k], v.detach()) for k, v in model.named_parameters())
    assert opt.state_dict()["state"] == {}
    for li in range(len(opt.param_groups[0]["params"])):
        assert not bool(opt._moment(0, li, 0).any()) and not bool(opt._moment(0, li, 1).any())

    # no read-back inside the loop: one .cpu() on a device tensor, nothing else
    model = _epoch_model(state)
    opt = DeviceAdam(model.parameters(), lr=1e-3)
    counts = {"cpu": 0, "item": 0, "tolist": 0, "__bool__": 0}
    for name in counts:
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                counts[_name] += 1
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, spy)
    out = harness.train_epoch(model, [batch] * 3, opt)
    monkeypatch.undo()
    print(f"device -> host inside train_epoch with DeviceAdam: {counts}")
    assert counts == {"cpu": 1, "item": 0, "tolist": 0, "__bool__": 0} and out["steps"] == 3 and out["skipped"] == 0


@pytest.mark.gpu
def test_eval_after_a_device_step_runs_on_the_new_weights():
    """The lines of test_train_forward.py that pin the packed weights to the step, with DeviceAdam: a raw-pointer update that left
    the version counters alone would run eval() on stale packed weights."""
    from pointdsc_amd import DeviceAdam, PointDSC, training
    state, data, W1, W2 = TF.setup()
    corr, src, tgt = (TF.g(data[k]) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    model = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS), state).to("cuda:0")
    d = {"corr_pos": corr, "src_keypts": src, "tgt_keypts": tgt}
    with torch.no_grad():
        model.eval()(d)          # packs the weights once, before the step
    opt = DeviceAdam(model.parameters(), lr=1e-3)
    TO.objective_run(model, corr, src, tgt, TF.g(W1), TF.g(W2), forward=TF.device_forward({}))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt.step()
    assert not torch.equal(before["encoder.layer0.weight"], model.state_dict()["encoder.layer0.weight"])
    model.eval()
    fresh = PointDSC(num_layers=TF.LAYERS)
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").eval()
    with torch.no_grad():
        for extra in ({}, {"testing": True}):
            a, f = model(dict(d, **extra)), fresh(dict(d, **extra))
            assert torch.equal(a["final_trans"], f["final_trans"]) and torch.equal(a["final_labels"], f["final_labels"])
            assert (a["M"] is None and f["M"] is None) or torch.equal(a["M"], f["M"])


@pytest.mark.gpu
def test_three_model_steps_against_fp64_adam():
    """The same 3 steps of L = <W1, logits> + <W2, M> with torch.optim.Adam and with DeviceAdam on the device model; the weights
    after step 3 under test_train_forward's measure and bound: truth the fp64 model stepped by fp64 Adam, yardstick torch's run."""
    from pointdsc_amd import DeviceAdam, training
    state, data, W1, W2 = LO.model_setup()
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]

    def weights(model):
        return {"weight:" + k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad}

    m64 = TF.load(TO.TorchPointDSC(num_layers=TF.LAYERS).double(), state)
    o64 = torch.optim.Adam([p for p in m64.parameters() if p.requires_grad], lr=1e-3, foreach=False)
    for _ in range(3):
        TO.objective_run(m64, corr.double(), src.double(), tgt.double(), W1.double(), W2.double())
        o64.step()
    ref64 = weights(m64)
    errs = {}
    for side in ("torch", "device"):
        model = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS), state).to("cuda:0")
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3) if side == "torch" else DeviceAdam(params, lr=1e-3)
        for _ in range(3):
            TO.objective_run(model, TF.g(corr), TF.g(src), TF.g(tgt), TF.g(W1), TF.g(W2), forward=TF.device_forward({}))
            opt.step()
        # train_oracle.errors' measure, max|X - X64| / max|X64| per tensor, through linear_train_oracle.errors: the former looks up
        # its zero-in-exact-arithmetic GRADIENT names and cannot take a dict of weights alone
        errs[side] = LO.errors(weights(model), ref64, list(ref64))
    e32 = max(errs["torch"].values())
    worst = max(errs["device"], key=errs["device"].get)
    print(f"weights after 3 Adam steps against the fp64 model: e32 {e32:.3e} (worst {max(errs['torch'], key=errs['torch'].get)}) "
          f"bound {TO.bound(e32):.3e}; DeviceAdam worst {errs['device'][worst]:.3e} ({worst})")
    for name in sorted(errs["device"]):
        print(f"  {name}: {errs['device'][name]:.2e} (torch.optim.Adam: {errs['torch'][name]:.2e})")
    for name, e in errs["device"].items():
        assert e <= TO.bound(e32), (name, e, TO.bound(e32))
