"""The branch and bound of csrc/pmc.hip (pmc_search_root) where the greedy clique is NOT a maximum clique.

tests/test_pmc.py's fixtures are planted near-cliques in sparse graphs: the greedy bound is the answer in three of four and the search
expands 120 nodes at most.  The instances here (tests/pmc_oracle.py) are dense random-like graphs ("ball": no inliers in a small cube)
and noisy inlier sets, where the search has to find 1 to 5 vertices more than the greedy clique, in roots of up to 205 candidates
(four words per bitset), thousands of nodes deep.  The oracle is tests/test_pmc.py's: numpy's fp32 edge rule and
networkx.max_weight_clique; the CPU tests recompute the table that the GPU tests read, and assert that the instance set has the
properties that keep the GPU tests from going vacuous.  Every comparison is an integer, a set or a bit pattern.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))
import pmc_oracle as PO  # noqa: E402
from test_pmc import FIXTURES, THR, assert_clique, bits_equal, g  # noqa: E402

from pointdsc_amd import synthetic  # noqa: E402

AMPLE = 1 << 22                                                   # max_nodes with which every instance below is proven
LADDER = (1, 8, 64, 512, 4096, AMPLE)
# words of the LDS pool for the first search pass: 1 sends every root to the slab pass, 1024 and 3072 keep every root of B3, B4, B5 in
# LDS, and in between each instance has a setting with roots in both passes (SPLITS; test_lds_settings_split_the_roots).  B4's roots
# have more than 64 candidates and need 56 or more stack levels, so nothing below 384 words keeps any of them.
LDS_WORDS = (1, 128, 256, 384, 1024, 3072)
SPLITS = {"B3": 128, "B4": 384, "B5": 256}
KEYS = ("pred_trans", "pred_labels", "clique_size", "proven", "counters")
HARD = dict(num_corr=1000, inlier_ratio=0.5, seed=5)              # tools/pmc_bench.py's hard instance: no CPU oracle finishes it


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_greedy_restatement_gives_the_published_bounds():
    """DESIGN.md f-10's table: greedy bounds 13 / 39 / 81 / 52 on the fixtures of tests/test_pmc.py, which are the F entries here."""
    for name, fx, want in zip(("F70", "F257", "F600", "F1000"), FIXTURES, (13, 39, 81, 52)):
        assert PO.RECIPES[name] == dict(num_corr=fx[0], inlier_ratio=fx[1], seed=fx[2])
        gr = PO.greedy(name)
        assert gr.size == want and PO.TABLE[name][:2] == (FIXTURES[fx], want)
        assert gr.sizes[gr.start] == want and (gr.sizes[:gr.start] < want).all()
        assert len(gr.members) == want


@pytest.mark.parametrize("name", list(PO.RECIPES))
def test_instance_table(name):
    adj = PO.adjacency(name)
    omega, bound, root = PO.TABLE[name]
    assert PO.oracle_clique_size(adj) == omega
    assert PO.greedy(name).size == bound
    if name in PO.EARLIEST_ROOT + PO.TIED_GREEDY:
        assert {len(c) for c in PO.cliques(name)} == {omega}
        if name in PO.EARLIEST_ROOT:
            assert PO.roots_of(PO.cliques(name), PO.greedy(name).order)[0] == root
    else:
        assert root is None


def test_instance_set_conditions():
    """What the GPU tests rely on, from the recomputed graphs (test_instance_table ties TABLE to them)."""
    gap = {n: PO.TABLE[n][0] - PO.TABLE[n][1] for n in PO.TABLE}
    assert set(PO.TABLE) == set(PO.RECIPES) and all(gap[n] > 0 for n in PO.SEARCH) and all(gap[n] == 0 for n in PO.TIED_GREEDY)
    assert sum(gap[n] > 0 for n in PO.SEARCH) >= 6 and sum(gap[n] >= 3 for n in PO.SEARCH) >= 2
    dens = {n: PO.density(PO.adjacency(n)) for n in PO.SEARCH}
    assert min(dens.values()) < 0.5 < max(dens.values()) and max(dens.values()) >= 0.9
    # a root of more than one / more than two words that is not cut at once by the greedy bound
    widest = {n: int(PO.greedy(n).candidates.max()) for n in PO.SEARCH}
    for words in (1, 2):
        wide = [n for n in PO.SEARCH if widest[n] > 64 * words]
        assert wide and all(widest[n] > PO.TABLE[n][1] for n in wide)
    assert max(widest.values()) <= 256                            # no instance with a CPU oracle has a five-word root
    # maximum cliques under several roots while the greedy clique is smaller; several maximum cliques where it is one of them
    several_roots = []
    for n in PO.EARLIEST_ROOT:
        roots = PO.roots_of(PO.cliques(n), PO.greedy(n).order)
        assert roots[0] == PO.TABLE[n][2]
        several_roots.append(len(roots) >= 2)
    assert any(several_roots)
    assert all(len(PO.cliques(n)) > 1 for n in PO.TIED_GREEDY)


@pytest.mark.parametrize("name", ["B3", "B4", "B5"])
def test_lds_settings_split_the_roots(name):
    """pmc_search_root's whole rule for keeping a root in the first pass, restated (PO.searched_in_lds: the matrix and two levels
    must fit the pool, and the levels left after the matrix must hold the root's colours + 1), on the roots the greedy bound does not
    cut: some setting of test_lds_and_slab_mixed leaves roots of this instance in BOTH passes, `1` leaves none in LDS, the largest
    setting and the full pool none in the slab."""
    gr = PO.greedy(name)
    in_lds = {w: PO.searched_in_lds(gr, w) for w in LDS_WORDS + (PO.POOL_WORDS,)}
    total = len(in_lds[1])
    assert total == len(PO.searched_roots(gr)) > 0
    assert not in_lds[1].any() and in_lds[3072].all() and in_lds[PO.POOL_WORDS].all()
    counts = {w: int(v.sum()) for w, v in in_lds.items()}
    print(f"{name}: roots searched in LDS of {total}: {counts}")
    assert 0 < counts[SPLITS[name]] < total, counts
    # a larger pool never moves a root to the slab
    assert all((in_lds[a] <= in_lds[b]).all() for a, b in zip(LDS_WORDS, LDS_WORDS[1:]))


# ---- GPU ------------------------------------------------------------------------------------------------------------
def run(p, max_nodes=AMPLE, lds_words=0):
    """baselines.pmc_run with its outputs on the host (KEYS)."""
    from pointdsc_amd import baselines
    r = baselines.pmc_run(g(p["corr_pos"]), g(p["src_keypts"]), g(p["tgt_keypts"]), THR, max_nodes=max_nodes, lds_words=lds_words)
    return {k: r[k].cpu() for k in KEYS}


@functools.lru_cache(maxsize=None)
def ample(name):
    """The default path at the ample budget: computed once, shared, never written to.  It is a device result, so a test that uses it
    as the expected value of another call first puts it through check_exact (the oracle's size, a clique of the oracle's graph)."""
    return run(PO.pair(name))


def same_bits(a, b):
    return bits_equal([a[k] for k in KEYS], [b[k] for k in KEYS])


def check_exact(name, r):
    """proven, the oracle's size, a clique of the oracle's graph, the pose of the labels bit for bit, the greedy bound's counter."""
    from pointdsc_amd import ops
    p = PO.pair(name)
    omega, bound, _ = PO.TABLE[name]
    assert int(r["proven"][0]) == 1 and int(r["counters"][0, 2]) == 0
    assert int(r["clique_size"][0]) == omega
    assert_clique(r["pred_labels"][0], PO.adjacency(name), omega)
    want = ops.rigid_transform_3d(g(p["src_keypts"]), g(p["tgt_keypts"]), g(r["pred_labels"])).cpu()
    assert torch.equal(r["pred_trans"].view(torch.int32), want.view(torch.int32))
    assert int(r["counters"][0, 3]) == bound == PO.greedy(name).size


@pytest.mark.gpu
@pytest.mark.parametrize("name", PO.SEARCH)
def test_exact_where_greedy_is_not_optimal(name):
    r = ample(name)
    check_exact(name, r)
    print(f"{name}: nodes {int(r['counters'][0, 0])} roots that branched {int(r['counters'][0, 1])}")
    assert int(r["counters"][0, 0]) > 0 and int(r["counters"][0, 1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", PO.EARLIEST_ROOT)
def test_winner_is_the_earliest_root(name):
    """TIE RULE: among roots with equally large cliques the root earliest in the order wins, so the labelled clique's last member in
    the order is the earliest of all maximum cliques' last members.  (Which clique wins inside a root depends on the colouring.)"""
    r = ample(name)
    members = np.flatnonzero(r["pred_labels"][0].numpy() == 1.0)
    assert PO.roots_of([members], PO.greedy(name).order) == [PO.TABLE[name][2]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PO.TIED_GREEDY)
def test_winner_is_the_first_greedy_clique(name):
    """TIE RULE: a root's clique replaces the greedy one only when strictly larger, and among greedy cliques of equal size the start
    vertex earliest in the order wins: with several maximum cliques the labelled one is exactly the restated greedy clique."""
    r = ample(name)
    check_exact(name, r)
    members = np.flatnonzero(r["pred_labels"][0].numpy() == 1.0)
    assert np.array_equal(members, PO.greedy(name).members)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B2", "B4", "B5", "Z2"])
def test_budget_ladder(name):
    p = PO.pair(name)
    omega, bound, _ = PO.TABLE[name]
    n = PO.RECIPES[name]["num_corr"]
    sizes = []
    for budget in LADDER:
        r = run(p, max_nodes=budget)
        assert same_bits(r, run(p, max_nodes=budget)), f"max_nodes={budget}: two calls differ"
        size, proven, nodes = int(r["clique_size"][0]), int(r["proven"][0]), int(r["counters"][0, 0])
        print(f"{name} max_nodes={budget}: clique {size} proven {proven} nodes {nodes} open roots {int(r['counters'][0, 2])}")
        assert_clique(r["pred_labels"][0], PO.adjacency(name), size)
        assert bound <= size <= omega
        assert proven in (0, 1) and (proven == 0 or size == omega)
        assert proven == (int(r["counters"][0, 2]) == 0)
        assert 0 <= nodes <= n * budget
        assert int(r["counters"][0, 3]) == bound
        sizes.append(size)
    # a root's search with a larger budget extends the same depth-first prefix
    assert sizes == sorted(sizes), sizes
    assert same_bits(r, ample(name)) and sizes[-1] == omega and proven == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B3", "B4", "B5"])
def test_lds_and_slab_mixed(name):
    """Roots split between the LDS pass and the slab pass (test_lds_settings_split_the_roots) give the default call's bits in every
    output and counter: the two passes run the same search, and at this budget the slab workgroups' shared budget does not bind.
    The default call is itself the device's, hence check_exact on it before it serves as the expected value."""
    want = ample(name)
    check_exact(name, want)
    for words in LDS_WORDS:
        got = run(PO.pair(name), lds_words=words)
        for k in KEYS:
            assert bits_equal([got[k]], [want[k]]), f"lds_words={words}: {k} differs from the default call"


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [None, AMPLE], ids=["default", "ample"])
def test_batch_equals_single_calls(budget):
    from pointdsc_amd import baselines
    budget = baselines.PMC_DEFAULT_MAX_NODES if budget is None else budget
    names = ("B1", "B2", "B7")
    cat = {k: torch.cat([PO.pair(n)[k] for n in names]) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    batch = run(cat, max_nodes=budget)
    assert batch["counters"].shape == (3, 4) and batch["pred_labels"].shape == (3, 120)
    for i, n in enumerate(names):
        single = run(PO.pair(n), max_nodes=budget)
        for k in KEYS:
            assert bits_equal([batch[k][i:i + 1]], [single[k]]), f"{n}: {k} differs inside the batch"
        if budget == AMPLE:
            assert same_bits(single, ample(n))
    if budget == AMPLE:
        assert batch["clique_size"].tolist() == [PO.TABLE[n][0] for n in names] and batch["proven"].tolist() == [1, 1, 1]


@pytest.mark.gpu
def test_hard_instance_properties():
    """make_pair(1000, inlier_ratio=0.5, seed=5) at the default budget: 65 000 nodes, and no CPU oracle finishes it, so its size has no
    independent source and is not asserted; what can be checked is."""
    from pointdsc_amd import baselines
    p = synthetic.make_pair(**HARD)
    adj = PO.oracle_adjacency(p["corr_pos"][0].numpy(), THR)
    gr = PO.Greedy(adj)
    a = run(p, max_nodes=baselines.PMC_DEFAULT_MAX_NODES)
    assert same_bits(a, run(p, max_nodes=baselines.PMC_DEFAULT_MAX_NODES))
    size = int(a["clique_size"][0])
    print(f"hard: clique {size} proven {int(a['proven'][0])} greedy {gr.size} nodes {int(a['counters'][0, 0])}")
    assert_clique(a["pred_labels"][0], adj, size)
    assert size >= gr.size
    assert int(a["counters"][0, 3]) == gr.size
    assert int(a["counters"][0, 0]) > 0
