"""CPU oracle of the batched correspondence construction (pointdsc_amd.correspondences.build_correspondences_batch).
TEST INFRASTRUCTURE ONLY.

It loops ``oracle.correspondence_oracle.build_correspondences`` (the numpy restatement of datasets/ThreeDMatch.py:283-290, :299-308)
over the pairs of a pool and adds the data loader's ground-truth label lines (datasets/ThreeDMatch.py:293-297) as numpy runs them:
``gt_trans`` is a float64 matrix there (np.linalg.inv), so ``transform`` promotes the float32 points and everything after it is fp64.
"""
from __future__ import annotations

import numpy as np

from oracle import correspondence_oracle as CO


def label_lines(src_sel: np.ndarray, tgt_sel: np.ndarray, gt_trans: np.ndarray, thr: float):
    """frag1_warp = transform(frag1, gt_trans); distance = sqrt(sum((frag1_warp - frag2)^2, axis=1)); labels = distance < thr."""
    T = np.asarray(gt_trans, dtype=np.float64)
    warp = (T[:3, :3] @ src_sel.T + T[:3, 3:4]).T                       # float32 points x float64 matrix -> float64
    dist = np.sqrt(np.sum(np.power(warp - tgt_sel, 2), axis=1))
    return dist, (dist < thr).astype(np.float32)


def build_correspondences_batch(desc, keypts, pairs, use_mutual=False, gt_trans=None, inlier_threshold=None):
    """Per pair the dict of CO.build_correspondences, plus gt_dist (fp64) and gt_labels when gt_trans [P,4,4] is given."""
    out = []
    for p, (s, t) in enumerate(pairs):
        r = CO.build_correspondences(desc[s], desc[t], keypts[s], keypts[t], use_mutual=use_mutual)
        if gt_trans is not None:
            r["gt_dist"], r["gt_labels"] = label_lines(r["src_keypts"], r["tgt_keypts"], gt_trans[p], inlier_threshold)
        out.append(r)
    return out


def rigid64(seed: int, max_angle: float = 0.3, max_trans: float = 0.3) -> np.ndarray:
    """A seeded float64 rigid motion [4,4]: a rotation of up to max_angle rad about a random axis (Rodrigues) and a shift."""
    rs = np.random.RandomState(seed)
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rs.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = rs.uniform(-max_trans, max_trans, 3)
    return T


def make_pool(d: int):
    """The pool of the GPU tests: clouds of 1, 77, 131, 257 and 700 points from CO.make_descriptors seeds (131 / 77 and 700 / 257 are
    each other's noisy partners, so the mutual check keeps a real share).  -> (desc list, keypts list), float32 numpy."""
    s700, t257, k700, k257 = CO.make_descriptors(700, 257, d, seed=1)
    s131, t77, k131, k77 = CO.make_descriptors(131, 77, d, seed=2)
    s1, _, k1, _ = CO.make_descriptors(1, 1, d, seed=3)
    return [s1, t77, s131, t257, s700], [k1, k77, k131, k257, k700]


# about nine pairs over make_pool: (a,b) and (b,a), a self pair, one pair twice, the 1-point cloud as source and as target, and
# 257 rows (three source tiles) directly in front of 1 row (one tile): tile-table boundaries next to each other
POOL_PAIRS = [(4, 3), (3, 4), (2, 2), (2, 1), (2, 1), (4, 0), (3, 1), (0, 2), (1, 4)]

# the label test: pairs of make_pool(33) with seeded float64 poses.  The pool's keypoints are uniform in a 3 m cube, so a threshold of
# 1.5 m (not the data sets' 0.10) leaves both labels well represented.  LABEL_SEED was chosen on the CPU so that no distance lies
# within 1e-9 of the threshold (test_label_seed_keeps_its_margin asserts it).
LABEL_PAIRS = [(2, 1), (4, 3), (3, 4), (1, 2)]
LABEL_THR = 1.5
LABEL_SEED = 11


def label_poses():
    return np.stack([rigid64(LABEL_SEED + i) for i in range(len(LABEL_PAIRS))])


def threshold_case():
    """Identity pose, thr = 0.10 (a double; np.float32(0.1) is greater): sources at the origin, target 0 at distance float32(0.1) -> an
    outlier, target 1 one float32 step closer -> an inlier.  Orthogonal unit descriptors pair source i with target i."""
    desc = np.eye(2, 4, dtype=np.float32)
    src_kp = np.zeros((2, 3), np.float32)
    tgt_kp = np.zeros((2, 3), np.float32)
    tgt_kp[0, 0] = np.float32(0.1)
    tgt_kp[1, 0] = np.nextafter(np.float32(0.1), np.float32(0))
    return [desc, desc.copy()], [src_kp, tgt_kp], np.eye(4)[None], 0.10, np.array([0.0, 1.0], np.float32)
