"""CPU side of tests/test_pmc_search.py: the instances on which the branch and bound of csrc/pmc.hip has real work to do, and numpy
restatements of what DESIGN.md section 8 f-10 fixes about the device's answer without replaying its colouring.

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
    "F70": fixture(70, 0.3, 1), "F257": fixture(257, 0.2, 2), "F600": fixture(600, 0.2, 3), "F1000": fixture(1000, 0.1, 4),
}
# name -> (maximum clique size, greedy bound, earliest root among the maximum cliques' last members (None: not enumerated));
# tests/test_pmc_search.py::test_instance_table recomputes every entry
TABLE = {
    "B1": (15, 14, 109), "B2": (26, 24, None), "B3": (19, 16, None), "B4": (67, 64, None), "B5": (29, 24, None), "B6": (20, 18, None),
    "B7": (23, 21, 60),
    "Z1": (19, 17, 43), "Z2": (17, 15, 72), "Z3": (13, 11, None),
    "F70": (13, 13, None), "F257": (39, 39, None), "F600": (82, 81, None), "F1000": (52, 52, None),
}
SEARCH = ("B1", "B2", "B3", "B4", "B5", "B6", "B7", "Z1", "Z2", "Z3")  # the instances whose greedy clique is not a maximum clique
EARLIEST_ROOT = ("Z1", "Z2", "B1", "B7")                          # maximum cliques enumerated: the winner's root is predicted
TIED_GREEDY = ("F70", "F257")                                     # several maximum cliques, the greedy clique one of them


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

