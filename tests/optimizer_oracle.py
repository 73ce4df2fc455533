"""Oracle of the trainer's update on the device (pointdsc_amd.optim, include/pointdsc_hip.h "the trainer's update on the device").

``Oracle(kind, shapes, dtype)`` holds THE RULE in numpy: with dtype np.float32 every product and every sum is one fp32 rounding (no
fused multiply-add exists in numpy), `/` and sqrt are correctly rounded, and the scalars are Python floats rounded once -- what the
kernels do, so the kernels must match it BIT FOR BIT.  It asserts that every intermediate is finite and either zero or normal
(``strict``; the kernels keep denormals, but no test may depend on that).  With dtype np.float64 the same rule is the truth the
fp32 results are measured against (scalars unrounded).

Per tensor: p, m, v (Adam) or buf (SGD), step, b1pow, b2pow; ``step(grads, ...)`` takes one gradient or None per tensor and
applies the guard: any non-finite element of any present gradient leaves everything untouched and counts one skipped step."""
import math

import numpy as np

ADAM, SGD = "adam", "sgd"
TINY = float(np.finfo(np.float32).tiny)


class Oracle:
    def __init__(self, kind, params, dtype=np.float32, guard=True, strict=True):
        assert kind in (ADAM, SGD)
        self.kind, self.dtype, self.guard, self.strict = kind, dtype, guard, strict
        self.p = [np.array(p, dtype=dtype).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]          # Adam's exp_avg, SGD's momentum_buffer
        self.v = [np.zeros_like(p) for p in self.p]
        self.steps = [0] * len(self.p)
        self.b1pow = [1.0] * len(self.p)
        self.b2pow = [1.0] * len(self.p)
        self.skipped = 0
        self.calls = 0

    def seed(self, i, step, m, v=None, betas=(0.9, 0.999)):
        """State as load_state_dict builds it: the products are beta ** step in Python floats."""
        self.steps[i] = int(step)
        self.m[i] = np.array(m, dtype=self.dtype).copy()
        if v is not None:
            self.v[i] = np.array(v, dtype=self.dtype).copy()
        self.b1pow[i], self.b2pow[i] = betas[0] ** int(step), betas[1] ** int(step)

    def _ok(self, *xs):
        if not self.strict:
            return
        tiny = TINY if self.dtype == np.float32 else float(np.finfo(np.float64).tiny)
        for x in xs:
            x = np.asarray(x)
            assert np.isfinite(x).all(), "non-finite intermediate"
            assert ((x == 0) | (np.abs(x) >= tiny)).all(), "denormal intermediate"

    def _r(self, x):
        """A scalar of the rule, rounded once to the working precision."""
        return self.dtype(x)

    def step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0):
        assert len(grads) == len(self.p)
        present = [g is not None for g in grads]
        if not any(present):
            return
        self.calls += 1
        if self.guard and any(not np.isfinite(np.asarray(g)).all() for g in grads if g is not None):
            self.skipped += 1
            return
        r = self._r
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = np.array(g, dtype=self.dtype)
            p = self.p[i]
            g1 = g
            if weight_decay != 0:
                wp = r(weight_decay) * p
                g1 = g + wp
                self._ok(wp)
            self._ok(g1)
            if self.kind == ADAM:
                b1pow, b2pow = self.b1pow[i] * betas[0], self.b2pow[i] * betas[1]
                step32, sq32 = r(lr / (1.0 - b1pow)), r(math.sqrt(1.0 - b2pow))
                a, b = r(betas[0]) * self.m[i], r(1.0 - betas[0]) * g1
                m = a + b
                c, e = r(betas[1]) * self.v[i], r(1.0 - betas[1]) * g1
                f = e * g1
                v = c + f
                s = np.sqrt(v)
                q = s / sq32
                d = q + r(eps)
                h = m / d
                u = step32 * h
                self._ok(a, b, m, c, e, f, v, s, q, d, h, u)
                self.p[i], self.m[i], self.v[i] = p - u, m, v
                self.b1pow[i], self.b2pow[i] = b1pow, b2pow
            else:
                buf = g1
                if momentum != 0:
                    if self.steps[i] > 0:
                        a = r(momentum) * self.m[i]
                        buf = a + g1
                        self._ok(a, buf)
                    self.m[i] = buf
                u = r(lr) * buf
                self._ok(u)
                self.p[i] = p - u
            self._ok(self.p[i])
            self.steps[i] += 1
