"""f-23: test infrastructure of tests/test_discrete_edges.py -- the crafted cases, the integer oracles and a switchable numpy model
of the four discrete decisions of the forward's tail: NMS (nms_flags_kernel; nms_grid_kernel + nms_window_kernel), seed ranking
(seed_select_kernel), the seed kNN (knn_select_kernel, knn_fused_kernel) and the vote (score_kernel, select_best_kernel,
refine_kernel's inlier count).

EXACTNESS RULE.  Every crafted case lives on a dyadic lattice: coordinates are integer multiples ("units") of a quantum 2^-m,
feature rows integer multiples of 2^-6.  The checks in this file redo every intermediate of the kernels' fp32 chains -- dx*dx, the
two fmafs of the radicand, R p + t, the 128-term dot, 2 - 2 dot -- in integers on the case's quantum and assert that it is
representable in fp32 (`is_f32`).  The truth is then integer arithmetic: independent of the order of summation and of fma
contraction, no margin condition, nothing excused.  One relaxation, written down here because a cloud 8 wide on a 2^-15 lattice
cannot avoid it: a squared distance whose chain is NOT exact must be FAR from the threshold radicand x*, |d2 - x*| >
2^-20 max(d2, x*).  The chain has three roundings of non-negative partial sums, so the computed value is within 3 * 2^-24 < 2^-22
relative of the integer one and the comparison with x* comes out as the integers say.  `radicand_check` enforces "exact or far"
pair by pair; every pair that DECIDES a case (at x*, one ulp below, one ulp above) is exact.

The only rounding in the truth is one correctly rounded np.sqrt on float32 where the product calls norm3 (`vote_truth`).

The MODEL restates what the kernels do -- cell grid and 3 x 3 window, radix ranking, fast / radix path of the matrix-form kNN, the
rounds and list cuts of the fused form, padded hypothesis groups and the argmax -- with the constants read from the sources by
regex, and takes seeded DEFECTS.  It serves two CPU checks: every case reaches the branch it is listed for, and every defect is
rejected by at least one case (a defect that no case rejects means a case is missing).
"""
from __future__ import annotations

import functools
import itertools
import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointdsc_amd" / "csrc"

F32 = np.float32
FAR_MARGIN = 2.0 ** -20             # "exact or far": see the module docstring


# ---------------------------------------------------------------------------------------------------------------------------
# constants of the sources, by regex: a changed constant fails the branch-reach test instead of silently moving a case
# ---------------------------------------------------------------------------------------------------------------------------
def _const(text, name):
    m = re.search(rf"\b{name}\s*=\s*(\d+)\s*[,;]", text)
    assert m, name
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def source_constants():
    seeds = (CSRC / "seeds.hip").read_text()
    score = (CSRC / "score_kernel.h").read_text()
    names = ("NMS2_ROWS", "NMS2_MAX_SLICE", "GRID_MAX", "SEL_THREADS", "KNN_THREADS", "KNN_FAST_CAP", "KF_ROWS", "KF_CAP", "KF_KEEP",
             "KF_MAX_WANT")
    c = {n: _const(seeds, n) for n in names}
    c["SC_SEEDS"] = _const(score, "SC_SEEDS")
    margin = re.search(r"const float rm = radius \* ([0-9.]+)f;", seeds)
    assert margin
    c["CELL_MARGIN"] = margin.group(1)                    # kept as text: the model multiplies in float32 as the kernel does
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 representability on a lattice, and the radicand chain
# ---------------------------------------------------------------------------------------------------------------------------
def is_f32(n) -> bool:
    """An integer number of quanta (any power-of-two quantum inside the normal range) is an fp32 value iff its odd part has at
    most 24 bits."""
    n = abs(int(n))
    return n == 0 or (n >> ((n & -n).bit_length() - 1)) < (1 << 24)


def is_f32_array(a):
    a = np.abs(np.asarray(a, np.int64))
    low = a & -a
    return (a == 0) | (a // np.maximum(low, 1) < (1 << 24))


def chain_exact(d):
    """d [...,3] int64 differences in units -> (d2, exact): d2 = dx^2 + dy^2 + dz^2 and whether dx*dx, fma(dy,dy,.) and fma(dz,dz,.)
    are all fp32 values (an fma rounds once, so dy*dy and dz*dz alone need not be)."""
    d = np.asarray(d, np.int64)
    assert np.abs(d).max(initial=0) < (1 << 30)                   # squares and their sums stay inside int64
    a = d[..., 0] * d[..., 0]
    ab = a + d[..., 1] * d[..., 1]
    abc = ab + d[..., 2] * d[..., 2]
    return abc, is_f32_array(a) & is_f32_array(ab) & is_f32_array(abc)


def radicand_check(d, n_star):
    """The exactness rule for a block of differences against the threshold radicand n_star (units^2): returns d2 and the number
    of exact entries; raises if an entry is neither exact nor far."""
    d2, exact = chain_exact(d)
    far = np.abs(d2 - n_star) > FAR_MARGIN * np.maximum(d2, n_star)
    bad = ~(exact | far)
    assert not bad.any(), f"{int(bad.sum())} radicands neither exact nor far, e.g. {d2[bad][:3]} against {n_star}"
    near = np.abs(d2 - n_star) <= FAR_MARGIN * np.maximum(d2, n_star)
    assert exact[near].all()
    return d2, int(exact.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# A. thresholds: x*, its neighbours, and lattice offsets that realise all three
# ---------------------------------------------------------------------------------------------------------------------------
def x_star(thr):
    """The smallest float32 x with np.sqrt(x) >= thr, by brute force over the 129 floats around float32(thr * thr)."""
    thr = F32(thr)
    centre = int(np.array(thr * thr, F32).view(np.int32))
    cand = (centre + np.arange(-64, 65)).astype(np.int32).view(np.float32)
    ok = np.sqrt(cand) >= thr                                     # correctly rounded, monotone
    first = int(np.argmax(ok))
    assert ok.any() and 0 < first and not ok[:first].any() and ok[first:].all()
    return cand[first]


def _two_squares(r):
    a = 0
    while 2 * a * a <= r:
        b = math.isqrt(r - a * a)
        if a * a + b * b == r:
            return a, b
        a += 1
    return None


def three_squares(n):
    """(a, b, c) with a^2 + b^2 + c^2 == n, c the large one, such that the fma chain is exact in the order a, b, c (a^2, a^2 + b^2
    and n are fp32 values; for n = 2 mod 4 above 2^24 no order with c first can be).  None if the 400 largest c give nothing (n of
    the form 4^a (8 b + 7) has no solution at all)."""
    c = math.isqrt(n)
    for _ in range(400):
        ab = _two_squares(n - c * c)
        if ab is not None and min(ab) > 0:
            a, b = ab
            if all(is_f32(v) for v in (a * a, b * b, a * a + b * b, n)):
                return a, b, c
        c -= 1
    return None


def threshold_case(thr):
    """thr -> dict: x* as a float32, the quantum exponent m (units of 2^-m), the three radicands in units^2 (n_in = x* - ulp,
    n_at = x*, n_out = x* + ulp) and an offset triple for each.  None if one of them is not realisable."""
    thr = F32(thr)
    xs = x_star(thr)
    mant, exp = math.frexp(float(xs))                            # xs = mant * 2^exp, mant in [0.5, 1)
    M, e = int(mant * (1 << 24)), exp - 24                        # xs = M * 2^e, M a 24-bit integer
    assert M * 2.0 ** e == float(xs)
    if M == 1 << 23:                                              # a power of two: the float below is only half an ulp away
        return None
    s = e & 1                                                     # 2 m = s - e must be even
    m, step = (s - e) // 2, 1 << s
    n_at = M << s
    out = {"thr": thr, "x_star": xs, "m": m, "step": step, "n": (n_at - step, n_at, n_at + step), "offsets": []}
    for n in out["n"]:
        t = three_squares(n)
        if t is None:
            return None
        out["offsets"].append(t)
    below, above = np.nextafter(xs, F32(0)), np.nextafter(xs, F32(np.inf))
    assert float(below) == out["n"][0] * 4.0 ** -m and float(above) == out["n"][2] * 4.0 ** -m
    return out


def search_thresholds(want=36):
    """How THRESHOLDS was found: the three named thresholds first, then k / 40 * 2^j over ten binades, keeping what
    `threshold_case` realises."""
    found = [0.1, 0.6, 1.2]
    assert all(threshold_case(t) is not None for t in found)
    for j in range(-6, 4):
        got = 0
        for k in range(21, 40):
            t = float(F32(k / 40.0 * 2.0 ** j))
            if got < 4 and threshold_case(t) is not None and all(F32(t) != F32(u) for u in found):
                found.append(t)
                got += 1
    return found[:want]


# The fixed list, as `search_thresholds` found it (decimal literals that round to the float32 values used): 36 thresholds over nine
# binades; 0.1f, 0.6f and 1.2f -- the library's NMS radius and the inlier thresholds of 3DMatch and KITTI -- come first.
THRESHOLDS = (0.1, 0.6, 1.2, 0.00859375, 0.009375, 0.01015625, 0.0109375, 0.0171875, 0.01875, 0.0203125, 0.021875, 0.034375, 0.0375,
              0.040625, 0.04375, 0.06875, 0.075, 0.08125, 0.0875, 0.1375, 0.15, 0.1625, 0.175, 0.275, 0.3, 0.325, 0.35, 0.55, 0.65,
              0.7, 0.8, 1.1, 1.3, 1.4, 1.6, 2.2)


@functools.lru_cache(maxsize=None)
def threshold_cases():
    return tuple(threshold_case(t) for t in THRESHOLDS)


def signed_permutations():
    """The 48 signed axis permutations as int64 3 x 3 matrices (24 of them rotations; the kernels never ask)."""
    mats = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), np.int64)
            for r in range(3):
                R[r, perm[r]] = signs[r]
            mats.append(R)
    return mats


SIGNED_PERMS = signed_permutations()


def offset_variants(triple, count):
    """`count` signed axis permutations of an offset triple whose fma chain stays exact, the first one (a, b, c) itself; taken in
    a fixed scrambled order of the 48 so that signs and axes vary."""
    t = np.asarray(triple, np.int64)
    out = []
    for p in [(17 * i) % 48 for i in range(48)]:
        v = SIGNED_PERMS[p] @ t
        if chain_exact(v)[1]:
            out.append(v)
    assert len(out) >= count
    return out[:count]


# ---------------------------------------------------------------------------------------------------------------------------
# NMS: truth and exactness
# ---------------------------------------------------------------------------------------------------------------------------
def suppressed_key(conf):
    with np.errstate(invalid="ignore"):
        return (np.asarray(conf, F32) * F32(0.0)).astype(F32)


def nms_truth_units(P, conf, n_star):
    """P [N,3] int64 units, conf [N] float32, n_star = x* in units^2 -> (keys float32, number of exact pairs).  Row i is
    suppressed iff some j has conf_i < conf_j and d2(i, j) < x* -- the complement of `(s_i >= s_j) | (d >= R)` over all j."""
    P = np.asarray(P, np.int64)
    conf = np.asarray(conf, F32)
    keep = np.ones(len(P), bool)
    exact = 0
    for lo in range(0, len(P), 512):
        d = P[lo:lo + 512, None, :] - P[None, :, :]
        d2, ne = radicand_check(d, n_star)
        exact += ne
        ok = (conf[lo:lo + 512, None] >= conf[None, :]) | (d2 >= n_star)
        keep[lo:lo + 512] = ok.all(axis=1)
    return np.where(keep, conf, suppressed_key(conf)).astype(F32), exact


def nms_truth_float(P, conf, xs):
    """The same predicate in float64 on float32 inputs, for the clouds with a non-finite coordinate (no lattice there): every finite
    difference of lattice points is exact in fp64, and a NaN / Inf distance compares as IEEE says -- a NaN distance is not >= R, so
    it suppresses i whenever `conf_i >= conf_j` fails."""
    P = np.asarray(P, F32).astype(np.float64)
    conf = np.asarray(conf, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = P[:, None, :] - P[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        ok = (conf[:, None] >= conf[None, :]) | (d2 >= float(xs))
    return np.where(ok.all(axis=1), conf, suppressed_key(conf)).astype(F32)


def same_key_bits(got, want):
    """Keys as int32 bits; a NaN key (-inf * 0) is compared as 'NaN on both sides': the payload of a generated NaN is the
    processor's, not the predicate's."""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    nan = np.isnan(want)
    return int(((got.view(np.int32) != want.view(np.int32)) & ~nan).sum() + (np.isnan(got) != nan).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# NMS: the model (float32 grid header and cell index as nms_grid_kernel computes them; the predicate on exact radicands)
# ---------------------------------------------------------------------------------------------------------------------------
NMS_DEFECTS = ("le_threshold", "radicand_low", "radicand_high", "fp64_square", "eight_cells", "narrow_cell", "trunc_index")


def grid_header(P, R, defects=()):
    c = source_constants()
    P = np.asarray(P, F32)
    bad = not np.isfinite(P).all()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xmn, xmx = np.fmin.reduce(P[:, 0]), np.fmax.reduce(P[:, 0])
        ymn, ymx = np.fmin.reduce(P[:, 1]), np.fmax.reduce(P[:, 1])
        rm = F32(R) * (F32(0.75) if "narrow_cell" in defects else F32(c["CELL_MARGIN"]))
        rx, ry = F32(xmx - xmn), F32(ymx - ymn)
        fx, fy = np.floor(F32(rx / rm)), np.floor(F32(ry / rm))
    nbx = int(min(fx, c["GRID_MAX"])) if fx >= 1 and not bad else 1
    nby = int(min(fy, c["GRID_MAX"])) if fy >= 1 and not bad else 1
    wx = F32(rx / F32(nbx)) if nbx > 1 else F32(1.0)
    wy = F32(ry / F32(nby)) if nby > 1 else F32(1.0)
    return {"xmin": xmn, "ymin": ymn, "nbx": nbx, "nby": nby, "wx": wx, "wy": wy, "floor_x": float(fx), "floor_y": float(fy),
            "bad": bad, "rm": rm}


def grid_cells(P, h, defects=()):
    """Cell (cx, cy) of every point: floorf((v - vmin) / w) in float32, clamped to [0, nb).  Defect `trunc_index`: the index taken
    as trunc(v / w) - trunc(vmin / w), truncation toward zero in place of the floor of the shifted coordinate."""
    P = np.asarray(P, F32)

    def axis(v, vmin, w, nb):
        with np.errstate(invalid="ignore", over="ignore"):
            if "trunc_index" in defects:
                q = np.trunc((v / w).astype(F32)) - np.trunc(F32(vmin / w))
            else:
                q = np.floor(((v - vmin).astype(F32) / w).astype(F32))
        out = np.zeros(len(v), np.int64)
        pos = q >= 0                                                  # NaN -> cell 0
        out[pos] = np.where(q[pos] < nb, q[pos], nb - 1).astype(np.int64)
        return out
    return axis(P[:, 0], h["xmin"], h["wx"], h["nbx"]), axis(P[:, 1], h["ymin"], h["wy"], h["nby"])


def grid_cells_exact(units, m, h):
    """floor((v - vmin) / w) in exact rational arithmetic for a finite lattice cloud (w and vmin are fp32 values, hence
    rationals), clamped as the kernel clamps."""
    from fractions import Fraction
    out = []
    for ax, (vmin, w, nb) in enumerate(((h["xmin"], h["wx"], h["nbx"]), (h["ymin"], h["wy"], h["nby"]))):
        vmin, w = Fraction(float(vmin)), Fraction(float(w))
        col = [min(max(math.floor((Fraction(int(u), 1 << m) - vmin) / w), 0), nb - 1) for u in units[:, ax]]
        out.append(np.array(col, np.int64))
    return out


def nms_model(case, defects=()):
    """Keys as the grid kernels produce them (the N^2 kernel: the same with one cell), with seeded defects -> (keys, info)."""
    P, conf, thr = case["P"], np.asarray(case["conf"], F32), F32(case["R"])
    xs = x_star(thr)
    if "radicand_low" in defects:
        xs = np.nextafter(xs, F32(0))
    if "radicand_high" in defects:
        xs = np.nextafter(xs, F32(np.inf))
    bound = float(thr) * float(thr) if "fp64_square" in defects else float(xs)
    h = grid_header(P, thr, defects)
    cx, cy = grid_cells(P, h, defects)
    Pd = np.asarray(P, F32).astype(np.float64)
    keep = np.ones(len(Pd), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(Pd), 512):
            sl = slice(lo, lo + 512)
            d = Pd[sl, None, :] - Pd[None, :, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]         # exact in fp64 on the lattice
            far_enough = d2 > bound if "le_threshold" in defects else d2 >= bound
            ok = (conf[sl, None] >= conf[None, :]) | far_enough
            ddx, ddy = cx[None, :] - cx[sl, None], cy[None, :] - cy[sl, None]
            window = (np.abs(ddx) <= 1) & (np.abs(ddy) <= 1)
            if "eight_cells" in defects:
                window &= ~((ddx == 1) & (ddy == 1))
            keep[sl] = (ok | ~window).all(axis=1)
    occupancy = np.bincount(cy * h["nbx"] + cx, minlength=h["nbx"] * h["nby"])
    info = dict(h, cx=cx, cy=cy, max_per_cell=int(occupancy.max()), cells_used=int((occupancy > 0).sum()))
    return np.where(keep, conf, suppressed_key(conf)).astype(F32), info


def n2_launch(N, bs=1):
    """Rows blocks, column slices and slice length of pdsc_nms_keys' launch."""
    c = source_constants()
    row_blocks = -(-N // c["NMS2_ROWS"])
    splits = max(-(-1024 // (row_blocks * bs)), -(-N // c["NMS2_MAX_SLICE"]))
    splits = min(splits, N)
    slice_ = -(-N // splits)
    return row_blocks, -(-N // slice_), slice_


# ---------------------------------------------------------------------------------------------------------------------------
# NMS cases.  Section A clouds: one per threshold, on that threshold's own quantum.  Section B clouds: R = 0.1f, quantum 2^-15
# ---------------------------------------------------------------------------------------------------------------------------
PAIR_PITCH = 1 << 15                 # units between the pairs of a section A cloud: > 4 c for every c < 5793 = sqrt(2^25)


def to_f32(units, m):
    out = (np.asarray(units, np.int64).astype(np.float64) * 2.0 ** -m).astype(F32)
    assert np.array_equal(out.astype(np.float64) * 2.0 ** m, np.asarray(units, np.float64)), "a coordinate is not an fp32 value"
    return out


def nms_threshold_cloud(tc):
    """Twelve isolated pairs (i, j), conf_i < conf_j: four signed axis permutations of each of the three offsets.  Odd pairs put j
    before i in memory; every third i has a negative confidence (its suppressed key is -0.0)."""
    pts, conf, expect = [], [], []
    p = 0
    for kind in range(3):
        for v in offset_variants(tc["offsets"][kind], 4):
            base = np.array([(p % 4) * PAIR_PITCH + 4096, (p // 4) * PAIR_PITCH + 4096, 8192], np.int64)
            ci = F32((-1 if p % 3 == 0 else 1) * (0.5 + p / 64.0))
            cj = F32(2.0 + p / 64.0)
            pair = [(base, ci, kind == 0), (base + v, cj, False)]
            for point, c, sup in (pair[::-1] if p % 2 else pair):
                pts.append(point)
                conf.append(c)
                expect.append(sup)
            p += 1
    units = np.array(pts, np.int64)
    return {"name": f"A thr={float(tc['thr']):.9g}", "units": units, "m": tc["m"], "P": to_f32(units, tc["m"]),
            "conf": np.array(conf, F32), "R": tc["thr"], "n_star": tc["n"][1], "expect_suppressed": np.array(expect)}


B_M = 15                                                        # quantum of section B / E: 2^-15
B_R = F32(0.1)
B_NSTAR = 10737418                                              # x*(0.1f) in units^2 (asserted by the CPU tests)
B_IN, B_AT, B_OUT = (79, 110, 3274), (39, 61, 3276), (65, 87, 3275)      # the issue's offsets for 0.1f: inside, at x*, one ulp above
U = 1 << B_M                                                    # 1.0 in units


def _b_case(name, units, conf, branch, **kw):
    units = np.asarray(units, np.int64)
    case = {"name": name, "units": units, "m": B_M, "P": to_f32(units, B_M), "conf": np.asarray(conf, F32), "R": B_R,
            "n_star": B_NSTAR, "branch": branch}
    case.update(kw)
    return case


def _planted(rs, n, extent_xy, extent_z, pairs, z_only=False):
    """n random lattice points in a box plus `pairs` planted (i, j) pairs at the three edge distances (j = i + a signed permutation
    of an edge offset; z_only: the large component stays in z, so that x and y keep their extent); confidences from nine values
    (ties everywhere), some negative."""
    units = np.stack([rs.randint(0, extent_xy, n), rs.randint(0, extent_xy, n), rs.randint(0, extent_z, n)], 1).astype(np.int64)
    order = rs.permutation(n)
    for t in range(min(pairs, n // 2)):
        i, j = order[2 * t], order[2 * t + 1]
        off = SIGNED_PERMS[rs.randint(8 if z_only else 48)] @ np.array((B_IN, B_AT, B_OUT)[t % 3], np.int64)
        units[j] = units[i] + off
        if z_only:                                                # the small components reflected back into the box
            units[j, :2] = units[i, :2] + off[:2] if (0 <= units[i, :2] + off[:2]).all() and (units[i, :2] + off[:2] < extent_xy).all() \
                else units[i, :2] - off[:2]
    conf = (rs.randint(-4, 5, n) / 4.0).astype(F32)
    return units, conf


@functools.lru_cache(maxsize=None)
def nms_geometry_cases():
    rs = np.random.RandomState(2301)
    cases = []
    tin, tat, tout = (np.array(t, np.int64) for t in (B_IN, B_AT, B_OUT))
    anchors8 = [(0, 0, 0), (8 * U, 8 * U, 0)]

    # B1: extent 8 -> floor(8 / 0.1001) = 79 -> capped at 64 cells of 0.125 = 4096 units
    pts, conf = list(anchors8), [0.0, 0.0]
    for k in (1, 2, 31, 63):                                     # points exactly on cell faces and one quantum below them
        for dx, dy in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
            pts.append((k * 4096 + dx, (k + 1) * 4096 + dy, 100))
            conf.append(1.0)
    pair_specs = [((5 * 4096 - 40, 5 * 4096 + 2000, 0), (1, 0, 2)),      # large component in z; x crosses the face at 5 * 4096
                  ((9 * 4096 + 2000, 9 * 4096 - 60, 0), (0, 1, 2)),      # y crosses
                  ((13 * 4096 - 30, 13 * 4096 - 30, 0), (0, 1, 2)),      # both cross: j in the diagonal cell (+1, +1)
                  ((17 * 4096 - 1600, 17 * 4096 + 100, 50), (2, 0, 1)),  # large component in x, crossing
                  ((21 * 4096 + 100, 21 * 4096 - 1600, 50), (0, 2, 1))]  # large component in y, crossing
    for base, perm in pair_specs:
        for t, trip in enumerate((tin, tat, tout)):
            b = np.array(base, np.int64) + np.array([0, 0, 20000 * (t + 1)], np.int64)       # the three kinds far apart in z
            pts += [tuple(b), tuple(b + trip[list(perm)])]
            conf += [0.25 if t else -0.25, 0.75]
    cases.append(_b_case("B1 faces and straddles, 64-cell cap", pts, conf, {"nbx": 64, "nby": 64, "floor_x": 79, "wx": 0.125}))

    # B2: floor(rx / rm) exactly 64 (6.5 / 0.1001 = 64.9): cells of 6.5 / 64 = 3328 units; pairs two cells apart just above R
    pts, conf = [(0, 0, 0), (13 * U // 2, 13 * U // 2, 0)], [0.0, 0.0]
    for k in (3, 20, 40):
        x0 = (k + 1) * 3328 - 1                                  # last quantum of cell k
        pts += [(x0, k * 3328 + 7, 0), (x0 + 3330, k * 3328 + 7, 0)]                           # cell k + 2, d = 3330 > 3276.8
        conf += [0.5, 1.0]
        pts += [(k * 3328 + 7, x0, 0), (k * 3328 + 7, x0 + 3330, 0)]
        conf += [0.5, 1.0]
        pts += [(x0, (k + 7) * 3328 + 9, 64), tuple(np.array((x0, (k + 7) * 3328 + 9, 64)) + tin[[2, 0, 1]])]     # one cell apart, inside
        conf += [-0.5, 1.0]
    cases.append(_b_case("B2 floor exactly 64, two cells apart", pts, conf, {"nbx": 64, "nby": 64, "floor_x": 64}))

    # B3: uncapped grid (extent 1 -> 9 cells): a line of inside-pairs whose large component runs along x, then along y
    pts, conf = [(0, 0, 0), (U, U, 0)], [0.0, 0.0]
    for t in range(24):
        b = np.array((1000 + t * 997, 2000 + (t % 5) * 6000, 40000 * (t % 2)), np.int64)
        pts += [tuple(b), tuple(b + tin[[2, 0, 1]])]
        conf += [0.5, 1.0]
        b = b[[1, 0, 2]] + np.array((0, 0, 80000), np.int64)
        pts += [tuple(b), tuple(b + tin[[0, 2, 1]])]
        conf += [-0.5, 1.0]
    cases.append(_b_case("B3 uncapped 9 x 9 cells, inside pairs along x and y", pts, conf, {"nbx": 9, "nby": 9}))

    # B4: floor 0 (extent 0.05), floor 1 (0.15): one cell each, the planted pairs' large component in z; a flat cloud (ry = 0)
    for name, ex, want in (("B4a floor 0: one cell", U // 20, {"nbx": 1, "nby": 1, "floor_x": 0, "floor_y": 0}),
                           ("B4b floor 1: one cell", 4915, {"nbx": 1, "nby": 1, "floor_x": 1, "floor_y": 1})):
        units, conf = _planted(rs, 300, ex, 20000, 60, z_only=True)
        cases.append(_b_case(name, units, conf, want))
    units, conf = _planted(rs, 300, 2 * U, 2000, 0)
    units[:, 1] = 777
    for t in range(40):                                          # planted pairs without a y component: 3276^2 < x* <= 3276^2 + 61^2
        units[2 * t + 1] = units[2 * t] + np.array((3276, 0, 61 if t % 2 else 0))
    cases.append(_b_case("B4c flat cloud, ry = 0", units, conf, {"nby": 1, "floor_y": 0, "nbx": 20}))
    cases.append(_b_case("B4d all points equal", np.tile(np.array([[12345, -777, 31]], np.int64), (130, 1)),
                         (rs.randint(0, 3, 130) / 2.0).astype(F32), {"nbx": 1, "nby": 1, "floor_x": 0}))

    # B5: a cell holding more than 1024 points (1100 points inside one 4096-unit cell of the capped grid, planted pairs among them)
    units, conf = _planted(rs, 1100, 4000, 4000, 60)
    units[:, :2] += 20 * 4096 + 40
    units = np.concatenate([np.array(anchors8, np.int64), units])
    cases.append(_b_case("B5 a cell with more than 1024 points", units, np.concatenate([[0.0, 0.0], conf]).astype(F32),
                         {"nbx": 64, "min_per_cell": 1025}))

    # B6: negative coordinates, and an offset of 256 (2^23 units: still 24 bits with the 18 of the cloud)
    units, conf = _planted(rs, 400, 2 * U, 3000, 60)
    cases.append(_b_case("B6a negative coordinates", units - np.array((U + 5, U // 2 + 3, 1500)), conf, {"negative": True}))
    cases.append(_b_case("B6b offset 256", units + np.array((256 * U, -256 * U, 256 * U)), conf, {"offset": True}))

    # B7: confidences.  Equal confidences at equal positions: nothing suppressed; the same with one larger: every other one is
    same = np.tile(np.array([[500, 600, 700]], np.int64), (70, 1))
    cases.append(_b_case("B7a equal confidences at equal positions", same, np.full(70, 0.5, F32), {"suppressed": 0}))
    c = np.full(70, -0.5, F32)
    c[41] = -0.25
    cases.append(_b_case("B7b equal confidences, one larger", same, c, {"suppressed": 69}))
    units, conf = _planted(rs, 300, U, 3000, 40)
    conf[::11], conf[5::13] = F32(np.inf), F32(-np.inf)
    cases.append(_b_case("B7c +-inf confidences", units, conf, {"inf_conf": True}))

    # B8: sizes around the row blocks (512 rows, two per thread), the 256-thread window blocks and the 2048-column slices
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049):
        units, conf = _planted(rs, n, U, 8000, max(n // 8, 1))
        cases.append(_b_case(f"B8 N={n}", units, conf, {"size": n}))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def nms_batch_case():
    rs = np.random.RandomState(2302)
    clouds = [_planted(rs, 513, U, 8000, 60), _planted(rs, 513, 8 * U, 8000, 60), _planted(rs, 513, U // 20, 20000, 60, z_only=True)]
    return [_b_case(f"B9 bs=3 pair {b}", u, c, {}) for b, (u, c) in enumerate(clouds)]


@functools.lru_cache(maxsize=None)
def nms_nonfinite_cases():
    """One non-finite coordinate: the grid must fall back to one cell and agree with the N^2 kernel and the float truth."""
    rs = np.random.RandomState(2303)
    out = []
    for name, col, value in (("B10a NaN in x", 0, np.nan), ("B10b NaN in z only", 2, np.nan), ("B10c +inf in x", 0, np.inf),
                             ("B10d -inf in z only", 2, -np.inf)):
        units, conf = _planted(rs, 300, U, 3000, 40)
        case = _b_case(name, units, conf, {"nbx": 1, "nby": 1, "bad": True})
        P = case["P"].copy()
        P[17, col] = value
        case["P"], case["units"], case["bad_row"] = P, None, 17
        out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# C. seed ranking
# ---------------------------------------------------------------------------------------------------------------------------
RANK_DEFECTS = ("highest_index_tie", "negative_zero_below")


def desc_bits(keys, canonical_zero=True):
    k = np.asarray(keys, F32).copy()
    if canonical_zero:
        k[k == 0] = F32(0.0)
    u = k.view(np.uint32).astype(np.uint64)
    asc = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return (~asc) & 0xFFFFFFFF


def rank_truth(keys, S):
    """sorted(range(N), key=(-key with -0.0 == +0.0, index))[:S] -- plain Python on floats, no bit tricks."""
    vals = [0.0 if float(v) == 0.0 else float(v) for v in np.asarray(keys, F32)]
    return np.array(sorted(range(len(vals)), key=lambda i: (-vals[i], i))[:S], np.int32)


def rank_model(keys, S, defects=()):
    """seed_select_kernel: radix select on descending key bits, lowest indices among the keys equal to the S-th value -> (seeds,
    info): info has the S-th value's run of equal keys (first index, last index, how many are taken) in 1024-key chunks."""
    c = source_constants()
    u = desc_bits(keys, canonical_zero="negative_zero_below" not in defects)
    idx = np.arange(len(u))
    order = np.lexsort((-idx if "highest_index_tie" in defects else idx, u))
    seeds = order[:S].astype(np.int32)
    prefix = u[order[S - 1]]
    run = np.flatnonzero(u == prefix)
    taken = int(S - (u < prefix).sum())
    chunk = c["SEL_THREADS"]
    info = {"run": len(run), "taken": taken, "first_chunk": int(run[0] // chunk), "last_chunk": int(run[-1] // chunk),
            "last_taken_chunk": int(run[taken - 1] // chunk), "chunks": -(-len(u) // chunk)}
    return seeds, info


@functools.lru_cache(maxsize=None)
def rank_cases():
    rs = np.random.RandomState(2304)
    cases = []

    def add(name, keys, S, **branch):
        cases.append({"name": name, "keys": np.asarray(keys, F32), "S": int(S), "branch": branch})

    for n in (1023, 1024, 1025, 2049, 4097):                     # thousands of equals; the boundary inside a run that crosses chunks
        keys = np.full(n, 0.5, F32)
        keys[rs.permutation(n)[: n // 8]] = F32(0.75)
        keys[rs.permutation(n)[: n // 8]] = F32(0.25)
        keys[0] = keys[-1] = F32(0.5)                            # the run spans the whole array: every chunk edge is inside it
        above = int((keys > 0.5).sum())
        add(f"C1 N={n} boundary inside the run", keys, above + (n - above) // 2 + 1, crosses=n > 1024)
    keys = np.full(4097, -1.0, F32)                              # the wanted value's run starts in chunk 1 and ends in chunk 3
    keys[1500:3500] = F32(0.125)
    keys[:40] = F32(3.0)
    add("C2 run from chunk 1 to chunk 3, cut in chunk 2", keys, 40 + 700, first_chunk=1, last_chunk=3, last_taken_chunk=2)
    add("C2 run from chunk 1 to chunk 3, cut in chunk 3", keys, 40 + 1900, first_chunk=1, last_chunk=3, last_taken_chunk=3)
    z = np.where(rs.randint(0, 2, 2049) == 1, F32(-0.0), F32(0.0)).astype(F32)
    z[rs.permutation(2049)[:50]] = F32(1.0)
    z[rs.permutation(2049)[:50]] = F32(-1.0)
    add("C3 mixed -0.0 and +0.0", z, 1000, zeros=True)
    add("C4 all keys equal", np.full(1025, -2.5, F32), 513)
    low = (np.uint32(0x3F000000) + rs.randint(0, 256, 1500).astype(np.uint32)).view(F32)
    add("C5 keys differing in the lowest byte", low, 700, low_byte=True)
    top = np.array([1.0e-30, 1.0e-10, 1.0, 1.0e10, 1.0e30, -1.0e-30, -1.0, -1.0e30], F32)[rs.randint(0, 8, 1500)]
    add("C5 keys differing in the top byte", top, 700, top_byte=True)
    wild = rs.standard_normal(1300).astype(F32)
    wild[::7] = (rs.randint(1, 1 << 22, len(wild[::7])).astype(np.uint32) | (rs.randint(0, 2, len(wild[::7])).astype(np.uint32) << 31)).view(F32)
    wild[3::50], wild[4::50] = F32(np.inf), F32(-np.inf)
    add("C6 negative, denormal and +-inf keys", wild, 650, denormal=True)
    small = (rs.randint(-3, 4, 37) / 2.0).astype(F32)
    for S in (1, 2, 36, 37):
        add(f"C7 N=37 S={S}", small, S)
    big = (rs.randint(-3, 4, 2500) / 2.0).astype(F32)
    for S in (1, 2, 2499, 2500):
        add(f"C7 N=2500 S={S}", big, S)
    add("C8 S = N = 16384", (rs.randint(-50, 51, 16384) / 8.0).astype(F32), 16384, lds_limit=True)
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------------------
# D. seed kNN
# ---------------------------------------------------------------------------------------------------------------------------
KNN_DEFECTS = ("self_dropped", "cut_ignores_index", "fast_cap_lost", "k_off_by_one")
FQ = 64                                                           # feature entries are multiples of 2^-6
DIST_ONE = FQ * FQ                                                # 1.0 in distance units (2^-12)


@functools.lru_cache(maxsize=None)
def codebook():
    """Twelve 128-entry integer rows (units of 2^-6, |entry| <= 64), deliberately not unit-norm: 0 has entries within +-0.5 and
    1 = 2 * row 0 (a larger dot with row 0 than row 0 itself); 2 has squared norm exactly 1 (distance 0 to itself); 3 is all +-1
    (dots up to 128: negative distances); the rest are random."""
    rs = np.random.RandomState(2305)
    C = rs.randint(-FQ, FQ + 1, (12, 128)).astype(np.int64)
    C[0] = rs.randint(-FQ // 2, FQ // 2 + 1, 128)
    C[1] = 2 * C[0]
    C[2] = 0
    C[2, :64] = 8
    C[3] = np.where(rs.randint(0, 2, 128) == 1, FQ, -FQ)
    return C


def levels_of(code):
    """The codewords ordered by their distance from codeword `code` (ascending, ties by codeword number): level 0 is the nearest."""
    C = codebook()
    d = 2 * DIST_ONE - 2 * (C @ C[code])
    return np.lexsort((np.arange(len(C)), d)), np.sort(d, kind="stable")


def knn_distances(rows, seeds):
    """rows [N,128] int64 units, seeds [S] -> [S,N] int64 distances 2 - 2 dot in units of 2^-12, with the exactness rule: every
    partial sum of the dot is bounded by sum |a b| (asserted < 2^24 units, so any order and any fma contraction is exact) and
    2 - 2 dot is an fp32 value."""
    rows = np.asarray(rows, np.int64)
    A = rows[np.asarray(seeds)]
    assert (np.abs(A) @ np.abs(rows).T).max() < (1 << 24)
    d = 2 * DIST_ONE - 2 * (A @ rows.T)
    assert is_f32_array(d).all() and np.abs(d).max() < (1 << 24)
    return d


def knn_truth(dist, k):
    """Stable sort of (distance, index) per seed, ranks 1 .. k (rank 0 is dropped, whoever it is)."""
    return np.argsort(dist, axis=1, kind="stable")[:, 1:k + 1].astype(np.int32)


def _composites(d, N):
    return d.astype(np.int64) * (1 << 20) + np.arange(N)          # order of (distance, index); N < 2^20


def knn_matrix_model(d, k, seed_index=None, defects=()):
    """knn_select_kernel for one seed's distance row d [N] -> (neighbours [k], info).  Fast path: 64 group minima (group of column
    j = (j // 4) % 64), their (k+1)-th smallest bounds the answer; more than KNN_FAST_CAP survivors, or fewer than k + 1 groups,
    go to the radix select."""
    c = source_constants()
    N, want = len(d), k + 1
    comp = _composites(d, N)
    order = np.argsort(comp)
    info = {"path": "radix", "survivors": None}
    if min(64, -(-N // 4)) >= want:
        grp = (np.arange(N) // 4) % 64
        gmin = np.full(64, np.iinfo(np.int64).max)
        np.minimum.at(gmin, grp, comp)
        bound = np.sort(gmin)[want - 1]
        surv = np.flatnonzero(comp <= bound)
        info["survivors"] = len(surv)
        if len(surv) <= c["KNN_FAST_CAP"]:
            info["path"] = "fast"
        elif "fast_cap_lost" in defects:
            surv = surv[: c["KNN_FAST_CAP"]]                      # the candidates past the cap never reach the ranking
            order = surv[np.argsort(comp[surv])]
            info["path"] = "fast (overflowed)"
    return _pick(order, k, seed_index, defects), info


def _pick(order, k, seed_index, defects):
    if "self_dropped" in defects:
        order = order[order != seed_index]
        return order[:k].astype(np.int32)
    if "k_off_by_one" in defects:
        return order[2:k + 2].astype(np.int32) if len(order) >= k + 2 else np.r_[order[2:], order[:1]].astype(np.int32)[:k]
    return order[1:k + 1].astype(np.int32)


def knn_fused_model(d, k, seed_index=None, defects=()):
    """knn_fused_kernel for one seed: rounds of 128 columns; a column enters the list iff its distance <= tau; a list longer than
    KF_CAP - 128 is cut to the entries <= the (k+1)-th smallest of the 64 lane minima (lane l owns list entries l, l + 64, ..);
    more than KF_KEEP survivors: exact ranking, the k + 1 smallest stay.  List order: columns in ascending order within a round
    (each wave's 32 columns take consecutive slots; the waves in order) -- the order changes which entries a bound keeps, never
    the final ranks.  -> (neighbours, info with the rounds of the cuts)."""
    c = source_constants()
    cap, keep_max = c["KF_CAP"], c["KF_KEEP"]
    N, want = len(d), k + 1
    comp = _composites(d, N)
    lst = np.zeros(0, np.int64)
    tau = None                                                    # +inf
    nblocks = -(-N // 32)
    rounds = -(-nblocks // 4)
    info = {"rounds": rounds, "bound_cuts": [], "exact_cuts": [], "max_list": 0, "late_ties": 0,
            "partial_last_round": N % 128 != 0}
    for rd in range(rounds):
        cols = np.arange(rd * 128, min(N, rd * 128 + 128))
        passing = cols if tau is None else cols[d[cols] <= tau]
        if tau is not None:
            info["late_ties"] += int((d[passing] == tau).sum())
        lst = np.concatenate([lst, comp[passing]])
        n = len(lst)
        info["max_list"] = max(info["max_list"], n)
        assert n <= cap
        if n <= cap - 128:
            continue
        pad = np.full(cap, np.iinfo(np.int64).max)
        pad[:n] = lst
        lane_min = pad.reshape(cap // 64, 64).min(axis=0)
        ub = np.sort(lane_min)[want - 1]
        kept = lst[lst <= ub]
        info["bound_cuts"].append(rd)
        if len(kept) > keep_max:
            info["exact_cuts"].append(rd)
            if "cut_ignores_index" in defects:                    # equal distances ranked without the index: the highest survive
                key = (kept >> 20) * (1 << 20) + ((1 << 20) - 1 - (kept & ((1 << 20) - 1)))
                kept = kept[np.argsort(key)][:want]
                ub = kept.max()
            else:
                kept = np.sort(kept)[:want]
                ub = kept[-1]
        lst = kept
        tau = ub >> 20
    order = (np.sort(lst) & ((1 << 20) - 1))
    return _pick(order, k, seed_index, defects), info


def pf_image(x):
    """[bs,N,128] float32 rows -> the point-fragment image [bs, round_up(N, 32), 128] (split_layout.h: tile = [q = 0..15][h][l31][4
    floats], channel 8 q + 4 h + e of row l31; rows past N zero)."""
    bs, n, _ = x.shape
    tiles = -(-n // 32)
    padded = np.zeros((bs, tiles * 32, 128), F32)
    padded[:, :n] = x
    img = padded.reshape(bs, tiles, 32, 16, 2, 4).transpose(0, 1, 3, 4, 2, 5)
    return np.ascontiguousarray(img).reshape(bs, tiles * 32, 128)


def _rows_from_levels(seed_code, levels):
    order, _ = levels_of(seed_code)
    return order[np.asarray(levels)]


def _knn_case(name, codes, seeds, k, forms, branch, pf=False):
    """codes [bs,N] codeword per row, seeds [bs,S]."""
    codes, seeds = np.asarray(codes, np.int64), np.asarray(seeds, np.int32)
    return {"name": name, "codes": codes, "seeds": seeds, "k": int(k), "forms": tuple(forms), "branch": branch, "pf": pf}


def knn_rows(case):
    return codebook()[case["codes"]]                              # [bs,N,128] int64 units


def knn_features(case):
    return (knn_rows(case).astype(np.float64) / FQ).astype(F32)


def _seeds_with_code(codes, code, S, rs, repeat=False):
    pool = np.flatnonzero(codes == code)
    assert len(pool)
    return rs.choice(pool, S, replace=repeat or len(pool) < S)


@functools.lru_cache(maxsize=None)
def knn_cases():
    rs = np.random.RandomState(2306)
    cases = []
    BOTH, MAT, FUS = ("matrix", "fused", "auto"), ("matrix", "auto"), ("fused",)

    # D1: rank 0 is not "self": seeds of codeword 0 (codeword 1 = 2 x row 0 is nearer than row 0 itself) and seeds that are the
    # second, third .. copy of their codeword (a duplicate at a lower index is rank 0)
    codes = rs.randint(0, 12, (1, 300))
    codes[0, :6] = (0, 1, 0, 2, 2, 3)
    seeds = np.array([[0, 2, 3, 4, 5, 1, 2, 2]], np.int32)        # incl. repeated seeds
    cases.append(_knn_case("D1 rank 0 is not self", codes, seeds, 10, BOTH, {"self_not_rank0": True}))

    # D2: more than KNN_FAST_CAP columns at or below the fast-path bound: 47 of the 64 column groups hold only the nearest codeword,
    # and the last 256 columns of those groups an even nearer one (the true neighbours sit at the END of the row)
    N, k = 4097, 47
    grp = (np.arange(N) // 4) % 64
    lev = np.where(grp < 47, 1, 5)
    lev[(np.arange(N) >= N - 257) & (grp < 47)] = 0
    codes = _rows_from_levels(4, lev)[None]
    seeds = _seeds_with_code(codes[0], levels_of(4)[0][1], 5, rs)[None]      # seeds whose own codeword is level 1 of codeword 4 ...
    codes[0, seeds[0]] = 4                                                   # ... replaced by codeword 4 itself
    cases.append(_knn_case("D2 fast-path overflow into the radix path", codes, seeds, k, MAT, {"path": "radix", "min_survivors": 1025}))

    # D3: the boundary min(64, ceil(N / 4)) >= k + 1 at k = 40
    for n in (160, 161, 164, 165):
        codes = rs.randint(0, 12, (1, n))
        cases.append(_knn_case(f"D3 fast-path boundary N={n} k=40", codes, rs.permutation(n)[:9][None], 40, MAT,
                               {"path": "fast" if -(-n // 4) >= 41 else "radix"}))

    # D4: matrix-form sizes and k
    for n in (2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097):
        ks = sorted({kk for kk in (1, 2, n - 1 if n <= 65 else 0, 47, 48, 64) if 1 <= kk <= min(n - 1, 64)})
        if n > 65:
            ks = [ks[(n + i) % len(ks)] for i in range(2)] if n < 4097 else [1, 64]
        codes = rs.randint(0, 12, (1, n))
        S = (1, 31, 32, 33, 65)[n % 5]
        for kk in dict.fromkeys(ks):
            cases.append(_knn_case(f"D4 matrix N={n} k={kk} S={S}", codes, rs.randint(0, n, (1, S)), kk, MAT, {}))
    for kk in (47, 48, 64):                                                  # the k values on one mid-sized cloud
        codes = rs.randint(0, 12, (1, 1025))
        cases.append(_knn_case(f"D4 matrix N=1025 k={kk} S=33", codes, rs.randint(0, 1025, (1, 33)), kk, MAT, {}))

    # D5: fused-form sizes, k, S, batch
    sizes = (256, 257, 287, 288, 289, 383, 384, 385, 1000)
    for i, n in enumerate(sizes):
        kk, S, bs = (1, 2, 40, 46, 47)[i % 5], (1, 31, 32, 33, 65)[(i + 2) % 5], (1, 3, 8, 16)[i % 4]
        codes = rs.randint(0, 12, (bs, n))
        for b in range(bs):                                                  # pairs that differ
            codes[b, : 20 + b] = b % 12
        seeds = np.stack([rs.randint(0, n, S) for _ in range(bs)])
        cases.append(_knn_case(f"D5 fused N={n} k={kk} S={S} bs={bs}", codes, seeds, kk, BOTH, {"block_map": bs % 8 == 0},
                               pf=i % 2 == 0))
    for kk in (1, 2, 40, 46, 47):
        codes = rs.randint(0, 12, (1, 385))
        cases.append(_knn_case(f"D5 fused N=385 k={kk} S=33", codes, rs.randint(0, 385, (1, 33)), kk, BOTH, {}, pf=kk % 2 == 1))

    # D6: list cuts.  Distances that fall with the column index: every column passes, the list is cut after round 1 (the earliest
    # round a list can pass KF_CAP - 128: a round adds at most 128), in middle rounds and in the last, partial round
    for n, kk in ((1000, 40), (383, 47), (289, 2)):
        lev = 11 - (np.arange(n) * 12) // n
        codes = _rows_from_levels(5, lev)[None]
        seeds = _seeds_with_code(codes[0], 5, 7, rs)[None]
        cases.append(_knn_case(f"D6 falling distances N={n} k={kk}", codes, seeds, kk, BOTH,
                               {"cut_rounds": ("first", "middle", "last") if n == 1000 else ("first", "last") if n == 383 else ("first",)}, pf=n == 383))

    # D7: more than KF_KEEP entries at or below the cut bound.  Column residues mod 32 map to fixed lanes of the cutting wave:
    # (k+1-1)//2 residues hold the nearest codeword, one residue the second, the rest a far one -- the (k+1)-th smallest lane
    # minimum is then a "second" entry whatever the order of the waves, and every "nearest" entry is at or below it
    for kk in (40, 46, 47):
        n0 = kk // 2
        res = np.arange(512) % 32
        lev = np.where(res < n0, 0, np.where(res == n0, 2, 9))
        codes = _rows_from_levels(6, lev)[None]
        seeds = _seeds_with_code(codes[0], 6, 5, rs)[None]
        cases.append(_knn_case(f"D7 exact-ranking cut k={kk}", codes, seeds, kk, BOTH, {"exact_cut": True}))

    # D8: the tie run of the (k+1)-th distance goes on through every later round (equal distance, larger index)
    codes = np.full((1, 1000), 7, np.int64)
    codes[0, ::97] = 8
    cases.append(_knn_case("D8 one codeword: ties through every round", codes, rs.randint(0, 1000, (1, 33)), 40, BOTH, {"late_ties": True}))
    # ... and in the matrix form with thousands of equals
    codes = np.full((1, 4097), 7, np.int64)
    codes[0, ::97] = 8
    cases.append(_knn_case("D8 one codeword, N=4097", codes, rs.randint(0, 4097, (1, 5)), 64, MAT, {}))

    # D9: negative distances and distance exactly 0
    codes = rs.randint(0, 12, (1, 300))
    codes[0, :40] = 3
    codes[0, 40:80] = 2
    seeds = np.concatenate([_seeds_with_code(codes[0], 3, 4, rs), _seeds_with_code(codes[0], 2, 4, rs)])[None]
    cases.append(_knn_case("D9 negative and zero distances", codes, seeds, 47, BOTH, {"negative": True, "zero": True}))
    return tuple(cases)


def knn_case_truth(case):
    rows = knn_rows(case)
    dist = [knn_distances(rows[b], case["seeds"][b]) for b in range(len(rows))]
    return dist, np.stack([knn_truth(d, case["k"]) for d in dist])


@functools.lru_cache(maxsize=None)
def knn_nan_case():
    """A few rows contain a NaN of either sign; no seed is such a row; every seed keeps at least k + 1 finite distances.  Truth
    ranks NaN last, as torch.sort does."""
    rs = np.random.RandomState(2307)
    n, k = 300, 40
    codes = rs.randint(0, 12, (1, n))
    nan_rows = np.array([0, 1, 2, 3, 64, 130, 131, 299])
    seeds = np.setdiff1d(rs.permutation(n)[:40], nan_rows)[:33][None].astype(np.int32)
    case = _knn_case("D10 NaN rows of either sign", codes, seeds, k, ("matrix", "fused", "auto"), {})
    x = knn_features(case)
    pos, neg = np.array([0x7FC00000], np.uint32).view(F32)[0], np.array([0xFFC00000], np.uint32).view(F32)[0]
    for i, r in enumerate(nan_rows):
        x[0, r, (7 * i) % 128] = pos if i % 2 else neg
    d = knn_distances(knn_rows(case)[0], seeds[0]).astype(np.float64)
    d[:, nan_rows] = np.inf                                       # NaN last; among themselves by index, but never inside rank k
    assert ((np.isfinite(d)).sum(axis=1) >= k + 1).all()
    return case, x, knn_truth(d, k), nan_rows


# ---------------------------------------------------------------------------------------------------------------------------
# A / E. voting: hypotheses that are signed axis permutations with dyadic translations
# ---------------------------------------------------------------------------------------------------------------------------
VOTE_DEFECTS = ("argmax_last", "padded_counted")


def residual_units(R, t, P, Q):
    """R [S,3,3] int64, t [S,3], P, Q [N,3] units -> d [S,N,3] = R p + t - q, with R p + t asserted an fp32 value (each product is
    0 or +-p, so the two fmafs and the add of the translation are exact as soon as their result is)."""
    X = np.einsum("sij,nj->sni", R, P) + t[:, None, :]
    assert is_f32_array(X).all() and is_f32_array(P).all() and is_f32_array(Q).all() and is_f32_array(t).all()
    return X - Q[None]


def vote_truth(R, t, P, Q, n_star, m, thr):
    """counts [S] (integer radicand < x*), best (lowest index among the highest counts), labels of the winner through the norm3 form:
    np.sqrt of the float32 radicand < thr -- the radicand is exact for every row near the threshold, one correctly rounded
    square root is the only rounding."""
    d = residual_units(R, t, P, Q)
    d2, exact = radicand_check(d, n_star)
    counts = (d2 < n_star).sum(axis=1).astype(np.int32)
    best = int(np.argmax(counts))                                  # numpy's argmax: the first maximum
    rad = (d2[best].astype(np.float64) * 4.0 ** -m).astype(F32)
    labels = (np.sqrt(rad) < F32(thr)).astype(F32)
    return counts, best, labels, exact


def vote_model(counts, defects=()):
    """select_best on the counts of score_kernel's groups of SC_SEEDS hypotheses."""
    c = source_constants()
    counts = np.asarray(counts, np.int64).copy()
    if "padded_counted" in defects:                               # the clamped copies of hypothesis S - 1 in the last group add up
        counts[-1] *= 1 + (-len(counts)) % c["SC_SEEDS"]
    if "argmax_last" in defects:
        return counts, len(counts) - 1 - int(np.argmax(counts[::-1]))
    return counts, int(np.argmax(counts))


def transforms_f32(R, t, m):
    T = np.zeros((len(R), 4, 4), F32)
    T[:, :3, :3] = R.astype(F32)
    T[:, :3, 3] = to_f32(t, m)
    T[:, 3, 3] = 1.0
    return T


def vote_threshold_case(tc, winner):
    """Section A: three edge hypotheses (distinct signed permutations, translations 2^17 units apart) and two fillers.  Under edge
    hypothesis g its own rows sit at x* - ulp (a_g rows), at x* (3 rows), at x* + ulp (3 rows) and at 0 (1 row); under every other
    hypothesis they are far.  `winner` gets the most rows inside."""
    rs = np.random.RandomState(100 + winner)
    Rs = np.stack([SIGNED_PERMS[i] for i in (3, 20, 41, 0, 29)])
    ts = np.array([[g << 17, (g % 2) << 12, -(g << 10)] for g in range(5)], np.int64)
    P, Q = [], []
    for g in range(3):
        inside = 6 if g == winner else 3 + g % 2
        offs = offset_variants(tc["offsets"][0], 12)[:inside] + offset_variants(tc["offsets"][1], 3) + \
            offset_variants(tc["offsets"][2], 3) + [np.zeros(3, np.int64)]
        for off in offs:
            p = rs.randint(-(1 << 13), 1 << 13, 3).astype(np.int64)
            P.append(p)
            Q.append(Rs[g] @ p + ts[g] - off)
    order = rs.permutation(len(P))
    return {"R": Rs, "t": ts, "P": np.array(P)[order], "Q": np.array(Q)[order], "m": tc["m"], "thr": tc["thr"], "n_star": tc["n"][1],
            "winner": winner}


def refine_threshold_case(tc, kind):
    """Section A, post_refinement: 64 rows that all sit at x* (kind 1), at x* - ulp (kind 0) or at x* + ulp (kind 2) under the pose."""
    rs = np.random.RandomState(7)
    R, t = SIGNED_PERMS[20][None], np.array([[1 << 12, -(1 << 11), 1 << 10]], np.int64)
    offs = offset_variants(tc["offsets"][kind], 12)
    P = rs.randint(-(1 << 13), 1 << 13, (64, 3)).astype(np.int64)
    Q = np.stack([R[0] @ p + t[0] - offs[i % 12] for i, p in enumerate(P)])
    return {"R": R, "t": t, "P": P, "Q": Q, "m": tc["m"], "thr": tc["thr"], "n_star": tc["n"][1]}


def vote_size_case(S, N, seed, mode="mixed"):
    """Section E (thr = 0.1f, quantum 2^-15): hypotheses = one signed permutation with translations t* + delta_s; delta_s is 0, a
    difference of two edge offsets (rows move between inside / at / outside) or far.  Rows sit at 0 or at one of the three edge
    offsets under delta = 0."""
    rs = np.random.RandomState(seed)
    R0 = SIGNED_PERMS[26]
    tstar = np.array([1 << 12, 1 << 11, -(1 << 12)], np.int64)
    edge = [np.asarray(o, np.int64) for trip in (B_IN, B_AT, B_OUT) for o in offset_variants(trip, 3)]
    deltas = [np.zeros(3, np.int64)] + [edge[i] - edge[j] for i, j in ((0, 3), (3, 0), (0, 6), (6, 3), (1, 4), (4, 1))]
    P = rs.randint(-(1 << 13), 1 << 13, (N, 3)).astype(np.int64)
    if mode == "all":
        off = np.zeros((N, 3), np.int64)
    else:
        off = np.stack([edge[i] if i < 9 else np.zeros(3, np.int64) for i in rs.randint(0, 12, N)])
    Q = P @ R0.T + tstar - off
    pick = rs.randint(0, 3 * len(deltas), S)
    far = np.stack([rs.randint(1, 9, S) << 16, rs.randint(-8, 9, S) << 12, rs.randint(-8, 9, S) << 12], 1).astype(np.int64)
    d = np.stack([deltas[i] if i < len(deltas) else far[s] for s, i in enumerate(pick)])
    if mode == "zero":
        d = far
    if mode == "all":
        d[S // 2] = 0
    if mode == "tie":                                             # the same best transform at s and s + 1024
        s0 = 5
        d[:] = far
        d[s0] = d[s0 + 1024] = 0
    if mode == "mixed":
        d[S - 1] = deltas[1 + (seed % 3)]                         # the last hypothesis (next to the padded slots) counts something
    return {"R": np.tile(R0[None], (S, 1, 1)), "t": tstar[None] + d, "P": P, "Q": Q, "m": B_M, "thr": B_R, "n_star": B_NSTAR,
            "mode": mode}


VOTE_SIZES = ((1, 1), (3, 63), (4, 64), (5, 65), (1023, 255), (1024, 256), (1025, 257), (2049, 1000), (5, 1000), (2049, 1))
