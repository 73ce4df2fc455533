"""CPU side of tests/test_pmc_search.py: the instances on which the branch and bound of csrc/pmc.hip has real work to do, and numpy
restatements of what DESIGN.md section 8 f-10 fixes about the device's answer: first without replaying its colouring (the greedy
bound, the tie rules, which pass a root takes), then with it (replay: the whole call, node for node), and an exact oracle of the
per-root clique sizes that shares nothing with the replay.

Everything here is an integer, a set or a bit pattern.  The edge rule is tests/test_pmc.py's ``oracle_adjacency``; networkx is imported
only inside the functions that the CPU tests call, the GPU tests read the table below (which a CPU test recomputes) or numpy results.
"""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))
from test_pmc import THR, oracle_adjacency, oracle_clique_size  # noqa: E402,F401

from pointdsc_amd import synthetic  # noqa: E402

POOL_WORDS = 6144                                                 # PMC_POOL_WORDS of csrc/pmc.hip: 48 KiB of LDS


def ball(n, scale):
    """No inliers in a small cube: every pair is within reach of the squared-distance rule, the graph is dense and random-like."""
    return dict(num_corr=n, inlier_ratio=0.0, scale=scale, seed=900 + n)


def noisy(n, ratio, noise):
    """Inliers with centimetres of noise: the inlier subgraph is no longer a clique."""
    return dict(num_corr=n, inlier_ratio=ratio, noise=noise, seed=500 + n)


def fixture(n, ratio, seed):
    return dict(num_corr=n, inlier_ratio=ratio, seed=seed)


# name -> synthetic.make_pair keywords
RECIPES = {
    "B1": ball(120, 0.6), "B2": ball(120, 0.45), "B3": ball(200, 0.6), "B4": ball(150, 0.35), "B5": ball(400, 0.6), "B6": ball(1000, 0.8),
    "B7": dict(num_corr=120, inlier_ratio=0.0, scale=0.5, seed=1021),
    "Z1": noisy(200, 0.5, 0.03), "Z2": noisy(300, 0.5, 0.03), "Z3": noisy(300, 0.4, 0.04),
    "W5": dict(num_corr=1400, inlier_ratio=0.0, scale=0.8, seed=7002), "W6": ball(2400, 0.9),
    "F70": fixture(70, 0.3, 1), "F257": fixture(257, 0.2, 2), "F600": fixture(600, 0.2, 3), "F1000": fixture(1000, 0.1, 4),
}
# name -> (maximum clique size, greedy bound, earliest root among the maximum cliques' last members (None: not enumerated));
# tests/test_pmc_search.py::test_instance_table recomputes every entry
TABLE = {
    "B1": (15, 14, 109), "B2": (26, 24, None), "B3": (19, 16, None), "B4": (67, 64, None), "B5": (29, 24, None), "B6": (20, 18, None),
    "B7": (23, 21, 60),
    "Z1": (19, 17, 43), "Z2": (17, 15, 72), "Z3": (13, 11, None),
    "W5": (26, 23, 1240), "W6": (24, 21, 1896),
    "F70": (13, 13, None), "F257": (39, 39, None), "F600": (82, 81, None), "F1000": (52, 52, None),
}
SEARCH = ("B1", "B2", "B3", "B4", "B5", "B6", "B7", "Z1", "Z2", "Z3", "W5", "W6")  # the instances whose greedy clique is not a maximum clique
EARLIEST_ROOT = ("Z1", "Z2", "B1", "B7")                          # maximum cliques enumerated: the winner's root is predicted
WIDE = {"W5": 256, "W6": 320}                                    # the one root with a maximum clique has more candidates than this
SEARCH_ALL = SEARCH + ("F600", "F1000")                           # every instance on which some root branches
TIED_GREEDY = ("F70", "F257")                                     # several maximum cliques, the greedy clique one of them


AMPLE = 1 << 22                                                   # tests/test_pmc_search.py's ample budget
# name -> the position in the order of the winning root at a budget that does not bind: the earliest root whose largest clique is a
# maximum clique (test_replay_agrees_with_the_exact_oracle: from the exact oracle, root by root).  F1000: the greedy clique wins.
WINNING_ROOT = {"B1": 109, "B2": 93, "B3": 155, "B4": 128, "B5": 271, "B6": 445, "B7": 60, "Z1": 43, "Z2": 72, "Z3": 72, "W5": 1240,
                "W6": 1896, "F600": 104}
# (name, max_nodes, lds_words) -> replay()'s (clique_size, members of the labelled clique, proven, (nodes, roots that branched, roots
# not exhausted, greedy bound)) for every setting a GPU test runs; tests/test_pmc_search.py::test_predicted_table recomputes every row
PREDICTED = {
    ("B1", AMPLE, 0): (15, (2, 8, 19, 23, 25, 26, 42, 55, 68, 71, 76, 77, 92, 93, 99), 1, (35, 13, 0, 14)),
    ("B2", AMPLE, 0): (26, (2, 7, 15, 19, 24, 29, 33, 35, 38, 47, 51, 52, 56, 58, 60, 63, 70, 71, 76, 85, 87, 102, 107, 109, 111, 118), 1, (2005,
        67, 0, 24)),
    ("B3", AMPLE, 0): (19, (5, 7, 23, 29, 36, 41, 78, 94, 97, 103, 110, 121, 129, 140, 142, 149, 153, 154, 186), 1, (2233, 145, 0, 16)),
    ("B4", AMPLE, 0): (67, (1, 5, 8, 9, 10, 11, 14, 21, 23, 27, 29, 30, 31, 32, 33, 34, 35, 36, 37, 39, 40, 41, 42, 45, 48, 51, 53, 54, 56, 58, 63,
        66, 67, 70, 75, 77, 80, 83, 88, 89, 90, 92, 94, 97, 100, 101, 102, 103, 104, 105, 107, 111, 112, 113, 118, 123, 127, 130, 133, 136, 137,
        141, 144, 145, 146, 147, 148), 1, (1226, 43, 0, 64)),
    ("B5", AMPLE, 0): (29, (5, 26, 43, 68, 90, 111, 120, 122, 126, 142, 178, 202, 218, 228, 252, 264, 271, 278, 315, 320, 322, 323, 324, 332, 337,
        358, 369, 380, 392), 1, (41346, 321, 0, 24)),
    ("B6", AMPLE, 0): (20, (90, 101, 113, 114, 191, 194, 326, 369, 482, 486, 540, 561, 674, 775, 781, 796, 798, 917, 924, 946), 1, (73934, 878, 0,
        18)),
    ("B7", AMPLE, 0): (23, (3, 7, 9, 10, 16, 17, 25, 29, 36, 40, 52, 59, 68, 72, 83, 92, 97, 105, 107, 108, 110, 113, 115), 1, (167, 32, 0, 21)),
    ("Z1", AMPLE, 0): (19, (15, 31, 33, 36, 43, 45, 55, 76, 90, 102, 135, 149, 157, 165, 169, 178, 191, 195, 198), 1, (186, 28, 0, 17)),
    ("Z2", AMPLE, 0): (17, (20, 21, 45, 52, 62, 63, 84, 89, 111, 139, 144, 148, 169, 188, 227, 239, 271), 1, (704, 74, 0, 15)),
    ("Z3", AMPLE, 0): (13, (21, 45, 63, 66, 97, 111, 148, 150, 156, 195, 227, 266, 272), 1, (49, 11, 0, 11)),
    ("W5", AMPLE, 0): (26, (98, 205, 221, 228, 247, 283, 289, 325, 361, 420, 525, 593, 616, 620, 628, 651, 695, 843, 1101, 1108, 1122, 1127, 1132,
        1140, 1278, 1279), 1, (266396, 1278, 0, 23)),
    ("W6", AMPLE, 0): (24, (20, 155, 226, 235, 298, 299, 348, 666, 674, 692, 712, 723, 1065, 1134, 1233, 1360, 1362, 1537, 1879, 1905, 1909, 1993,
        2121, 2167), 1, (753096, 2253, 0, 21)),
    ("F600", AMPLE, 0): (82, (8, 9, 36, 42, 66, 67, 81, 88, 90, 91, 95, 108, 117, 124, 125, 129, 132, 137, 139, 152, 168, 172, 178, 186, 189, 196,
        201, 208, 218, 219, 226, 227, 230, 239, 240, 241, 246, 249, 268, 269, 276, 285, 289, 298, 301, 306, 309, 327, 329, 345, 351, 352, 363, 377,
        383, 385, 393, 399, 421, 424, 432, 434, 435, 451, 454, 461, 463, 472, 473, 502, 503, 517, 518, 525, 526, 539, 551, 565, 568, 578, 587, 599),
        1, (120, 5, 0, 81)),
    ("F1000", AMPLE, 0): (52, (6, 14, 66, 67, 70, 71, 109, 183, 264, 265, 272, 282, 284, 296, 315, 339, 361, 383, 399, 410, 417, 423, 428, 454, 459,
        470, 480, 487, 494, 514, 562, 575, 580, 596, 602, 618, 643, 648, 659, 678, 712, 722, 735, 751, 756, 762, 768, 881, 913, 952, 953, 992), 1,
        (11, 1, 0, 52)),
    ("W5", AMPLE, 1024): (26, (98, 205, 221, 228, 247, 283, 289, 325, 361, 420, 525, 593, 616, 620, 628, 651, 695, 843, 1101, 1108, 1122, 1127,
        1132, 1140, 1278, 1279), 1, (266396, 1278, 0, 23)),
    ("W5", AMPLE, 1): (26, (98, 205, 221, 228, 247, 283, 289, 325, 361, 420, 525, 593, 616, 620, 628, 651, 695, 843, 1101, 1108, 1122, 1127, 1132,
        1140, 1278, 1279), 1, (266396, 1278, 0, 23)),
    ("B2", 1, 0): (24, (7, 11, 25, 34, 35, 38, 39, 51, 54, 57, 59, 64, 70, 71, 75, 80, 89, 93, 94, 102, 107, 111, 115, 117), 0, (67, 67, 60, 24)),
    ("B2", 8, 0): (24, (7, 11, 25, 34, 35, 38, 39, 51, 54, 57, 59, 64, 70, 71, 75, 80, 89, 93, 94, 102, 107, 111, 115, 117), 0, (438, 67, 45, 24)),
    ("B2", 64, 0): (26, (2, 7, 15, 19, 24, 29, 33, 35, 38, 47, 51, 52, 56, 58, 60, 63, 70, 71, 76, 85, 87, 102, 107, 109, 111, 118), 0, (1638, 67,
        11, 24)),
    ("B2", 512, 0): (26, (2, 7, 15, 19, 24, 29, 33, 35, 38, 47, 51, 52, 56, 58, 60, 63, 70, 71, 76, 85, 87, 102, 107, 109, 111, 118), 1, (2005, 67,
        0, 24)),
    ("B2", 4096, 0): (26, (2, 7, 15, 19, 24, 29, 33, 35, 38, 47, 51, 52, 56, 58, 60, 63, 70, 71, 76, 85, 87, 102, 107, 109, 111, 118), 1, (2005, 67,
        0, 24)),
    ("B4", 1, 0): (64, (2, 8, 9, 11, 14, 27, 28, 29, 31, 32, 33, 34, 35, 36, 39, 40, 41, 42, 44, 51, 53, 54, 56, 58, 65, 66, 67, 70, 75, 77, 78, 80,
        84, 88, 89, 90, 92, 94, 95, 97, 100, 102, 103, 104, 105, 107, 111, 113, 120, 123, 127, 129, 130, 133, 136, 137, 141, 142, 143, 144, 145,
        146, 147, 148), 0, (43, 43, 38, 64)),
    ("B4", 8, 0): (64, (2, 8, 9, 11, 14, 27, 28, 29, 31, 32, 33, 34, 35, 36, 39, 40, 41, 42, 44, 51, 53, 54, 56, 58, 65, 66, 67, 70, 75, 77, 78, 80,
        84, 88, 89, 90, 92, 94, 95, 97, 100, 102, 103, 104, 105, 107, 111, 113, 120, 123, 127, 129, 130, 133, 136, 137, 141, 142, 143, 144, 145,
        146, 147, 148), 0, (214, 43, 15, 64)),
    ("B4", 64, 0): (65, (1, 5, 8, 9, 10, 14, 21, 23, 27, 29, 31, 32, 33, 34, 35, 36, 37, 39, 40, 41, 42, 45, 48, 51, 53, 54, 56, 58, 63, 66, 67, 70,
        75, 77, 80, 83, 88, 89, 90, 92, 94, 97, 100, 101, 102, 103, 104, 105, 107, 111, 112, 113, 118, 123, 127, 130, 133, 136, 137, 141, 144, 145,
        146, 147, 148), 0, (754, 43, 8, 64)),
    ("B4", 512, 0): (67, (1, 5, 8, 9, 10, 11, 14, 21, 23, 27, 29, 30, 31, 32, 33, 34, 35, 36, 37, 39, 40, 41, 42, 45, 48, 51, 53, 54, 56, 58, 63,
        66, 67, 70, 75, 77, 80, 83, 88, 89, 90, 92, 94, 97, 100, 101, 102, 103, 104, 105, 107, 111, 112, 113, 118, 123, 127, 130, 133, 136, 137,
        141, 144, 145, 146, 147, 148), 1, (1226, 43, 0, 64)),
    ("B4", 4096, 0): (67, (1, 5, 8, 9, 10, 11, 14, 21, 23, 27, 29, 30, 31, 32, 33, 34, 35, 36, 37, 39, 40, 41, 42, 45, 48, 51, 53, 54, 56, 58, 63,
        66, 67, 70, 75, 77, 80, 83, 88, 89, 90, 92, 94, 97, 100, 101, 102, 103, 104, 105, 107, 111, 112, 113, 118, 123, 127, 130, 133, 136, 137,
        141, 144, 145, 146, 147, 148), 1, (1226, 43, 0, 64)),
    ("B5", 1, 0): (24, (7, 15, 45, 60, 126, 129, 132, 169, 180, 195, 202, 208, 214, 215, 271, 284, 315, 320, 324, 330, 358, 360, 384, 392), 0, (321,
        321, 319, 24)),
    ("B5", 8, 0): (24, (7, 15, 45, 60, 126, 129, 132, 169, 180, 195, 202, 208, 214, 215, 271, 284, 315, 320, 324, 330, 358, 360, 384, 392), 0,
        (2471, 321, 298, 24)),
    ("B5", 64, 0): (27, (14, 15, 26, 43, 53, 68, 90, 120, 126, 178, 202, 218, 228, 252, 264, 278, 315, 320, 323, 324, 332, 337, 354, 358, 369, 384,
        392), 0, (15740, 321, 181, 24)),
    ("B5", 512, 0): (29, (5, 26, 43, 68, 90, 111, 120, 122, 126, 142, 178, 202, 218, 228, 252, 264, 271, 278, 315, 320, 322, 323, 324, 332, 337,
        358, 369, 380, 392), 0, (41026, 321, 6, 24)),
    ("B5", 4096, 0): (29, (5, 26, 43, 68, 90, 111, 120, 122, 126, 142, 178, 202, 218, 228, 252, 264, 271, 278, 315, 320, 322, 323, 324, 332, 337,
        358, 369, 380, 392), 1, (41346, 321, 0, 24)),
    ("Z2", 1, 0): (15, (21, 35, 45, 52, 63, 84, 89, 111, 120, 148, 169, 177, 231, 234, 271), 0, (74, 74, 60, 15)),
    ("Z2", 8, 0): (15, (21, 35, 45, 52, 63, 84, 89, 111, 120, 148, 169, 177, 231, 234, 271), 0, (317, 74, 16, 15)),
    ("Z2", 64, 0): (17, (20, 21, 45, 52, 62, 63, 84, 89, 111, 139, 144, 148, 169, 188, 227, 239, 271), 0, (626, 74, 3, 15)),
    ("Z2", 512, 0): (17, (20, 21, 45, 52, 62, 63, 84, 89, 111, 139, 144, 148, 169, 188, 227, 239, 271), 1, (704, 74, 0, 15)),
    ("Z2", 4096, 0): (17, (20, 21, 45, 52, 62, 63, 84, 89, 111, 139, 144, 148, 169, 188, 227, 239, 271), 1, (704, 74, 0, 15)),
    ("W5", 1, 0): (23, (144, 197, 205, 228, 269, 289, 325, 414, 467, 540, 575, 593, 616, 620, 651, 695, 719, 824, 921, 1093, 1127, 1187, 1279), 0,
        (1278, 1278, 1259, 23)),
    ("W5", 8, 0): (23, (144, 197, 205, 228, 269, 289, 325, 414, 467, 540, 575, 593, 616, 620, 651, 695, 719, 824, 921, 1093, 1127, 1187, 1279), 0,
        (9892, 1278, 1206, 23)),
    ("W5", 64, 0): (25, (98, 156, 205, 221, 247, 256, 283, 289, 325, 420, 421, 585, 593, 631, 651, 670, 695, 714, 727, 843, 881, 1027, 1122, 1140,
        1161), 0, (70244, 1278, 970, 23)),
    ("W5", 512, 0): (26, (98, 205, 221, 228, 247, 283, 289, 325, 361, 420, 525, 593, 616, 620, 628, 651, 695, 843, 1101, 1108, 1122, 1127, 1132,
        1140, 1278, 1279), 0, (242242, 1278, 93, 23)),
    ("W5", 4096, 0): (26, (98, 205, 221, 228, 247, 283, 289, 325, 361, 420, 525, 593, 616, 620, 628, 651, 695, 843, 1101, 1108, 1122, 1127, 1132,
        1140, 1278, 1279), 1, (266396, 1278, 0, 23)),
    ("B3", 256, 1): (18, (7, 23, 29, 36, 41, 78, 94, 97, 103, 110, 121, 129, 140, 141, 142, 149, 154, 186), 0, (1703, 138, 40, 16)),
    ("B5", 2048, 1): (28, (14, 15, 26, 43, 53, 61, 68, 90, 120, 126, 142, 178, 202, 218, 228, 252, 264, 278, 315, 320, 323, 324, 332, 337, 354, 358,
        369, 392), 0, (16356, 208, 175, 24)),
}


@functools.lru_cache(maxsize=None)
def pair(name):
    return synthetic.make_pair(**RECIPES[name])


@functools.lru_cache(maxsize=None)
def adjacency(name):
    adj = oracle_adjacency(pair(name)["corr_pos"][0].numpy(), THR)
    adj.setflags(write=False)
    return adj


def search_order(adj):
    """order[position] = vertex: degree descending, index ascending (pmc_order_kernel)."""
    deg = adj.sum(1)
    return np.lexsort((np.arange(len(deg)), -deg))


class Greedy:
    """DESIGN's lower bound restated.  In the search order, from every start position take the first common neighbour until none is
    left; the bound is the largest of these cliques, from the earliest start position that reaches it.
    size: the bound; start: that position; members: the clique as sorted vertex indices; sizes[position]: every start's size."""

    def __init__(self, adj):
        n = adj.shape[0]
        order = search_order(adj)
        padj = adj[np.ix_(order, order)]
        P = padj.copy()
        member = np.eye(n, dtype=bool)
        rows = np.arange(n)
        for _ in range(n):
            live = P.any(1)
            if not live.any():
                break
            u = P.argmax(1)                                       # the first set bit of every row
            member[rows[live], u[live]] = True
            P[live] &= padj[u[live]]
        self.order = order
        self.padj = padj
        self.sizes = member.sum(1)
        self.size = int(self.sizes.max())
        self.start = int(self.sizes.argmax())                     # argmax returns the first maximum
        self.members = np.sort(order[member[self.start]])
        sub = adj[np.ix_(self.members, self.members)]
        assert sub.sum() == self.size * (self.size - 1)
        # candidates of root q: its neighbours earlier in the order
        self.candidates = np.tril(padj, -1).sum(1)
        self._colours = {}

    def colours(self, q):
        if q not in self._colours:
            self._colours[q] = root_colours(self, q)
        return self._colours[q]


@functools.lru_cache(maxsize=None)
def greedy(name):
    return Greedy(adjacency(name))


def density(adj):
    n = adj.shape[0]
    return adj.sum() / (n * (n - 1))


def maximum_cliques(adj):
    """Every maximum clique as a frozenset of vertex indices (networkx.find_cliques: all maximal cliques, the largest kept)."""
    import networkx as nx
    best, out = 0, []
    for c in nx.find_cliques(nx.from_numpy_array(adj)):
        if len(c) > best:
            best, out = len(c), []
        if len(c) == best:
            out.append(frozenset(c))
    return out


@functools.lru_cache(maxsize=None)
def cliques(name):
    return tuple(maximum_cliques(adjacency(name)))


def roots_of(cliques, order):
    """Sorted distinct roots (the position of a clique's last member in the order) of the given cliques."""
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    return sorted({int(max(pos[v] for v in c)) for c in cliques})


def searched_roots(gr, lb=None):
    """Candidate counts of the roots that are not cut at once: a root with n candidates holds cliques of at most n + 1."""
    lb = gr.size if lb is None else lb
    return gr.candidates[gr.candidates + 1 > lb]


def fits_lds(n_loc, pool_words):
    """The layout rule of pmc_search_root: the n x Wl local matrix and two stack levels (4 Wl words) against the pool."""
    wl = (n_loc + 63) // 64
    return n_loc * wl + 4 * wl <= pool_words


def root_colours(gr, q):
    """Colours of root q's first node, as pmc_search_root counts them: all candidates (q's neighbours earlier in the order, order
    kept), colour classes in sequence, each grown by taking the first vertex left and dropping its neighbours.  The incumbent plays
    no part in the count."""
    cand = np.flatnonzero(gr.padj[q, :q])
    mat = gr.padj[np.ix_(cand, cand)]
    left = np.ones(len(cand), dtype=bool)
    colours = 0
    while left.any():
        colours += 1
        Q = left.copy()
        while Q.any():
            v = int(Q.argmax())
            Q &= ~mat[v]
            Q[v] = False
            left[v] = False
    return colours


def searched_in_lds(gr, pool_words, max_depth=1024):
    """Per root that the greedy bound does not cut (ascending position): True where the first search pass keeps it with a pool of
    `pool_words`, False where it goes to the slab pass.  pmc_search_root's whole rule: the layout rule, then the levels left after the
    matrix, levels = (pool - n Wl) / (2 Wl) capped at PMC_MAX_DEPTH, must hold min(n, colours of the root) + 1."""
    out = []
    for q in np.flatnonzero(gr.candidates + 1 > gr.size):
        n = int(gr.candidates[q])
        wl = (n + 63) // 64
        if not fits_lds(n, pool_words):
            out.append(False)
            continue
        levels = min((pool_words - n * wl) // (2 * wl), max_depth)
        out.append(min(n, gr.colours(int(q))) + 1 <= levels)
    return np.array(out, dtype=bool)



# ---- the replay: pdsc_pmc_baseline_ex restated from its documented rules (csrc/pmc.hip's header) ----------
PMC_MAX_LOCAL = 4096
PMC_MAX_DEPTH = 1024
SLAB_WGS = 64                                                     # PMC_SLAB_WGS
SLAB_NODE_COST = 8                                                # PMC_SLAB_NODE_COST
ST_DONE, ST_BUDGET, ST_SLAB = 0, 1, 2


def local_matrix(gr, q):
    """(candidates of root q as ascending positions, their adjacency as one Python-int bitset per candidate; bit j = candidate j)."""
    if not hasattr(gr, "_local"):
        gr._local = {}
    if q not in gr._local:
        cand = np.flatnonzero(gr.padj[q, :q])
        packed = np.packbits(gr.padj[np.ix_(cand, cand)], axis=1, bitorder="little")
        gr._local[q] = (cand, [int.from_bytes(row.tobytes(), "little") for row in packed])
    return gr._local[q]


def replay_root(mat, n, lb, max_nodes, levels):
    """pmc_search_root's loop on a root of n candidates: the private incumbent starts at lb; mode 0 expands a node (incumbent, the
    s + cnt <= best cut, sequential colouring with k = best - s, B = the candidates of colour > k), mode 1 takes the LAST member of B
    (the nodes >= max_nodes stop comes before it), mode 2 returns to the parent.  One node per branching step.
    Returns (status, nodes, best, path of local indices or None, colours of the first node, loop iterations).
    Only the first k colour classes are built below the first node: whatever is left after them is B, and no later class changes it.
    The first node is coloured to the end, because its number of colours decides between LDS and slab."""
    best, bestp, nodes, it = lb, None, 0, 0
    cap = 4 * max_nodes + 8
    stP, stB, cur = [0] * (n + 2), [0] * (n + 2), [0] * (n + 2)
    Pw = (1 << n) - 1
    d, s, mode, colours0 = 0, 1, 0, 0
    while it < cap:
        it += 1
        if mode == 0:
            if s > best:
                best, bestp = s, cur[:d]
            cnt = Pw.bit_count() if hasattr(Pw, "bit_count") else bin(Pw).count("1")
            if cnt == 0 or s + cnt <= best:
                mode = 2
                continue
            k = best - s
            U, c, Bw = Pw, 0, None
            while U:
                if c == k:
                    Bw = U
                    if d:
                        break
                c += 1
                Q = U
                while Q:
                    low = Q & -Q
                    Q &= ~(mat[low.bit_length() - 1] | low)
                    U ^= low
            if Bw is None:
                Bw = 0
            if d == 0:
                colours0 = c
                if min(n, c) + 1 > levels:
                    return ST_SLAB, 0, lb, None, c, it
            if Bw == 0:
                mode = 2
                continue
            stP[d], stB[d] = Pw, Bw
            mode = 1
            continue
        if mode == 1:
            Pw, Bw = stP[d], stB[d]
            if Bw == 0 or s + bin(Pw).count("1") <= best:
                mode = 2
                continue
            if nodes >= max_nodes:
                return ST_BUDGET, nodes, best, bestp, colours0, it
            assert d + 2 <= levels, "the stack guard is never taken after the check at the root"
            nodes += 1
            v = Bw.bit_length() - 1
            m = 1 << v
            Pw &= ~m
            stP[d], stB[d] = Pw, Bw & ~m
            cur[d] = v
            Pw &= mat[v]
            d += 1
            s += 1
            mode = 0
            continue
        if d == 0:
            return ST_DONE, nodes, best, bestp, colours0, it
        d -= 1
        s -= 1
        mode = 1
    raise AssertionError(f"the iteration cap 4 max_nodes + 8 = {cap} binds (nodes {nodes})")


class Replay:
    """What replay() returns.  members: sorted vertex indices of the labelled clique; counters: (nodes, roots with nodes > 0, roots
    not exhausted, greedy bound); rsize / rstat / rnodes: per root position, as the finish kernel reads them; root: the winning root's
    position (None: the greedy clique is returned)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def row(self):
        """The committed form (PREDICTED)."""
        return (self.clique_size, tuple(int(v) for v in self.members), self.proven, self.counters)


def _root_search(gr, q, max_nodes, levels):
    """replay_root on root q, through a memo.  A search that ended DONE after `nodes` nodes never met the budget stop, and it would
    not have met it with any budget >= nodes either (the stop is looked at only right before a node is counted): that result is reused
    for such budgets.  `levels` enters only through the check at the first node, which is redone here from the recorded colours."""
    cand, mat = local_matrix(gr, q)
    n = len(cand)
    if not hasattr(gr, "_memo"):
        gr._memo = {}
    hit = gr._memo.get(q)
    if hit is not None and hit[1] <= max_nodes:
        if min(n, hit[4]) + 1 > levels:
            return ST_SLAB, 0, gr.size, None, hit[4], 0
        assert hit[5] <= 4 * max_nodes + 8
        return hit
    r = replay_root(mat, n, gr.size, max_nodes, levels)
    if r[0] == ST_DONE:
        gr._memo[q] = r
    return r


def replay_graph(gr, max_nodes, lds_words=0):
    """The replay on a Greedy (which holds the order, the ordered adjacency and the bound)."""
    N = len(gr.order)
    lb = gr.size
    pool = lds_words if lds_words else POOL_WORDS
    rsize, rstat, rnodes = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    path = {}

    def record(q, r):
        status, nodes, best, bestp, _, _ = r
        rstat[q], rnodes[q] = status, nodes
        rsize[q] = best if best > lb else 0
        path.pop(q, None)
        if best > lb:
            path[q] = bestp

    searched = [int(q) for q in np.flatnonzero(gr.candidates + 1 > lb)]      # every other root: DONE, size 0, no nodes
    # first pass: one workgroup per root, max_nodes each
    for q in searched:
        n = int(gr.candidates[q])
        wl = (n + 63) // 64
        assert n <= PMC_MAX_LOCAL, "PMC_ST_UNSERVED is out of scope"
        if n * wl + 4 * wl > pool:
            rstat[q] = ST_SLAB
            continue
        record(q, _root_search(gr, q, max_nodes, min((pool - n * wl) // (2 * wl), PMC_MAX_DEPTH)))
    # slab pass: workgroup g serves the roots q = g (mod 64) left with ST_SLAB, ascending, from one budget of max_nodes // 8
    nl_max = min(max(N - 1, 1), PMC_MAX_LOCAL)
    wl_max = (nl_max + 63) // 64
    slab_words = nl_max * wl_max + 2 * wl_max * (min(nl_max, PMC_MAX_DEPTH) + 1)
    unreached, interrupted, ran_out = 0, 0, set()
    for g in range(SLAB_WGS):
        left = max_nodes // SLAB_NODE_COST
        for q in range(g, N, SLAB_WGS):
            if rstat[q] != ST_SLAB:
                continue
            if left <= 0:
                rstat[q] = ST_BUDGET
                unreached += 1
                ran_out.add(g)
                continue
            n = int(gr.candidates[q])
            wl = (n + 63) // 64
            assert n * wl + 4 * wl <= slab_words
            r = _root_search(gr, q, left, min((slab_words - n * wl) // (2 * wl), PMC_MAX_DEPTH))
            assert r[0] != ST_SLAB, "PMC_ST_UNSERVED is out of scope"
            record(q, r)
            interrupted += r[0] == ST_BUDGET
            left -= r[1]
    # finish: the largest root clique, the earliest root among equals; the greedy clique unless a root is strictly larger
    win = int(rsize.max())
    if win > 0:
        root = int(rsize.argmax())
        cand, _ = local_matrix(gr, root)
        members = np.sort(gr.order[[root] + [int(cand[i]) for i in path[root]]])
        assert len(members) == win
    else:
        root, members = None, gr.members
    open_roots = int((rstat != ST_DONE).sum())
    return Replay(clique_size=win if win > 0 else lb, members=members, proven=int(open_roots == 0), root=root,
                  counters=(int(rnodes.sum()), int((rnodes > 0).sum()), open_roots, lb), rsize=rsize, rstat=rstat, rnodes=rnodes,
                  slab_unreached=unreached, slab_interrupted=interrupted, slab_wgs_ran_out=len(ran_out))


def replay(adj, max_nodes, lds_words=0):
    """pdsc_pmc_baseline_ex(max_nodes, lds_words) on the graph `adj`, integers and bitsets only."""
    return replay_graph(Greedy(adj), max_nodes, lds_words)


@functools.lru_cache(maxsize=None)
def replayed(name, max_nodes, lds_words=0):
    return replay_graph(greedy(name), max_nodes, lds_words)


# ---- an exact oracle that shares nothing with the replay but the definition of a root ----------------------------------------------
def exact_root_sizes(adj):
    """{root position: size of the largest clique whose last member in the search order is that root}, for the roots where that size
    exceeds the greedy bound.  A branch and bound of its own (Tomita's MCQ: the candidates of a root renumbered by ascending degree
    inside the root, colour classes grown from the highest number down, a colour-sorted list per node, branched from the highest colour down, pruned where size + colour cannot exceed
    the best so far); none of the replay's functions, vertex orders or data structures is used."""
    import sys as _sys
    gr = Greedy(adj)
    pos = np.empty(len(gr.order), dtype=np.int64)
    pos[gr.order] = np.arange(len(gr.order))
    nbrs = [set(pos[np.flatnonzero(adj[v])].tolist()) for v in gr.order]       # by position
    out = {}
    limit = _sys.getrecursionlimit()
    _sys.setrecursionlimit(max(limit, 10000))
    try:
        for q in range(len(gr.order)):
            cand = sorted(u for u in nbrs[q] if u < q)
            if len(cand) + 1 <= gr.size:
                continue
            inside = {u: nbrs[u].intersection(cand) for u in cand}
            by_degree = sorted(cand, key=lambda u: (len(inside[u]), -u))    # colour classes start from the highest degree
            index = {u: i for i, u in enumerate(by_degree)}
            masks = [sum(1 << index[w] for w in inside[u]) for u in by_degree]
            best = [gr.size]

            def expand(R, P):
                # colour sort: (vertex, colour) in ascending colour
                seq, colour, U = [], 0, P
                while U:
                    colour += 1
                    Q = U
                    while Q:
                        v = Q.bit_length() - 1
                        Q &= ~masks[v] & ~(1 << v)
                        U &= ~(1 << v)
                        seq.append((v, colour))
                for v, col in reversed(seq):
                    if R + col <= best[0]:
                        return
                    child = P & masks[v]
                    if child:
                        expand(R + 1, child)
                    elif R + 1 > best[0]:
                        best[0] = R + 1
                    P &= ~(1 << v)

            expand(1, (1 << len(cand)) - 1)
            if best[0] > gr.size:
                out[q] = best[0]
    finally:
        _sys.setrecursionlimit(limit)
    return out


@functools.lru_cache(maxsize=None)
def exact(name):
    return exact_root_sizes(adjacency(name))
