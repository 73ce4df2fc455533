"""The branch and bound of csrc/pmc.hip (pmc_search_root) where the greedy clique is NOT a maximum clique.

tests/test_pmc.py's fixtures are planted near-cliques in sparse graphs: the greedy bound is the answer in three of four and the search
expands 120 nodes at most.  The instances here (tests/pmc_oracle.py) are dense random-like graphs ("ball": no inliers in a small cube)
and noisy inlier sets, where the search has to find 1 to 5 vertices more than the greedy clique, in roots of up to 205 candidates
(four words per bitset), thousands of nodes deep.  The oracle is tests/test_pmc.py's: numpy's fp32 edge rule and
networkx.max_weight_clique; the CPU tests recompute the table that the GPU tests read, and assert that the instance set has the
properties that keep the GPU tests from going vacuous.  Every comparison is an integer, a set or a bit pattern.

The search's own work is held to a prediction as well: PO.replay restates pdsc_pmc_baseline_ex (both passes and the finish) from its
documented rules, and PO.PREDICTED holds its size, clique members, proven and four counters for every setting a GPU test runs.  CPU
tests recompute that table and anchor the replay: root by root against an exact branch and bound that shares nothing with it, through
that against networkx, and against the device's counters recorded in DESIGN.md f-10 before the replay existed.  W5 and W6 have one root
each that holds a maximum clique, of 284 and 377 candidates (five and six words per bitset).
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
LADDER_NAMES = ("B2", "B4", "B5", "Z2", "W5")
WIDE_LDS_WORDS = (1024, 1)                                        # W5: its five-word roots in the slab pass, then every root
BATCH_BUDGETS = (64, 512)                                         # the W5 rows of test_wide_batch_equals_single_calls
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
    assert PO.greedy(name).size == bound
    if name in PO.WIDE:                                           # networkx does not finish these in useful time: the exact oracle
        sizes = PO.exact(name)
        assert max(sizes.values()) == omega and min(q for q, s in sizes.items() if s == omega) == root
        return
    assert PO.oracle_clique_size(adj) == omega
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
    assert all((widest[n] > 256) == (n in PO.WIDE) for n in PO.SEARCH)   # five words and more: test_wide_instance_conditions
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


# the device's counters of DESIGN.md f-10 (profiles/f10_pmc_search_instances.txt), recorded before the replay was written:
# (name, max_nodes) -> (nodes, roots that branched, roots not exhausted)
RECORDED = {
    ("B1", AMPLE): (35, 13, 0), ("B2", AMPLE): (2005, 67, 0), ("B3", AMPLE): (2233, 145, 0), ("B4", AMPLE): (1226, 43, 0),
    ("B5", AMPLE): (41346, 321, 0), ("B6", AMPLE): (73934, 878, 0), ("B7", AMPLE): (167, 32, 0), ("Z1", AMPLE): (186, 28, 0),
    ("Z2", AMPLE): (704, 74, 0), ("Z3", AMPLE): (49, 11, 0), ("F600", AMPLE): (120, 5, 0), ("F1000", AMPLE): (11, 1, 0),
    ("B2", 1): (67, 67, 60), ("B4", 1): (43, 43, 38), ("B5", 1): (321, 321, 319), ("Z2", 1): (74, 74, 60),
    ("B2", 8): (438, 67, 45), ("B4", 8): (214, 43, 15), ("B5", 8): (2471, 321, 298), ("Z2", 8): (317, 74, 16),
    ("B2", 64): (1638, 67, 11), ("B4", 64): (754, 43, 8), ("B5", 64): (15740, 321, 181), ("Z2", 64): (626, 74, 3),
    ("B2", 512): (2005, 67, 0), ("B4", 512): (1226, 43, 0), ("B5", 512): (41026, 321, 6), ("Z2", 512): (704, 74, 0),
}
RECORDED_SIZES = {("B2", 64): 26, ("B4", 64): 65, ("B5", 64): 27, ("Z2", 64): 17, ("B5", 512): 29}   # where it is not the greedy bound
SLAB_BINDS = (("B3", 256), ("B5", 2048))                          # lds_words = 1: test_slab_budget_settings_bind


@pytest.mark.parametrize("name", list(PO.RECIPES))
def test_replay_agrees_with_the_exact_oracle(name):
    """At a budget that does not bind, root by root: the replay's size of every root equals the largest clique whose last member in
    the order is that root, as an independent branch and bound finds it (where it exceeds the greedy bound, else 0 = nothing recorded);
    hence the maximum and the earliest root that attains it.  On the instances that networkx finishes the maximum is networkx's
    (TABLE, which test_instance_table recomputes)."""
    r = PO.replayed(name, AMPLE)
    sizes = PO.exact(name)
    assert {int(q): int(s) for q, s in enumerate(r.rsize) if s} == sizes
    omega, bound, _ = PO.TABLE[name]
    assert r.proven == 1 and r.counters[2] == 0 and r.counters[3] == bound and r.clique_size == omega
    assert max(sizes.values(), default=bound) == omega
    if omega > bound:
        assert r.root == min(q for q, s in sizes.items() if s == omega) == PO.WINNING_ROOT[name]
        assert PO.roots_of([r.members], PO.greedy(name).order) == [r.root]
    else:
        assert r.root is None and np.array_equal(r.members, PO.greedy(name).members) and name not in PO.WINNING_ROOT
    sub = PO.adjacency(name)[np.ix_(r.members, r.members)]
    assert len(r.members) == omega and sub.sum() == omega * (omega - 1)
    if PO.TABLE[name][2] is not None:
        assert r.root == PO.TABLE[name][2]


@pytest.mark.parametrize("key", list(RECORDED), ids=lambda k: f"{k[0]}-{k[1]}")
def test_replay_gives_the_recorded_device_counters(key):
    """The one outside witness of the node rule: what the device counted at an earlier commit, at the ample budget and on the ladder."""
    r = PO.replayed(*key)
    assert r.counters[:3] == RECORDED[key]
    assert r.clique_size == RECORDED_SIZES.get(key, PO.TABLE[key[0]][0] if key[1] >= 512 else PO.TABLE[key[0]][1])
    assert r.proven == (RECORDED[key][2] == 0)


def predicted_names():
    return sorted({k[0] for k in PO.PREDICTED})


@pytest.mark.parametrize("name", predicted_names())
def test_predicted_table(name):
    """PO.PREDICTED, which the GPU tests read, is the replay's answer."""
    keys = [k for k in PO.PREDICTED if k[0] == name]
    assert (name, AMPLE, 0) in keys and PO.AMPLE == AMPLE
    for k in keys:
        assert PO.replayed(*k).row() == PO.PREDICTED[k], k
    if name in LADDER_NAMES:
        assert all((name, b, 0) in keys for b in LADDER)


def test_predicted_table_covers_the_gpu_tests():
    assert set(predicted_names()) == set(PO.SEARCH_ALL)
    for words in WIDE_LDS_WORDS:                                  # the slab pass's shared budget does not bind there: the default row
        assert PO.PREDICTED[("W5", AMPLE, words)] == PO.PREDICTED[("W5", AMPLE, 0)]
    assert all((n, b, 1) in PO.PREDICTED for n, b in SLAB_BINDS) and all(b in LADDER for b in BATCH_BUDGETS)


@pytest.mark.parametrize("name", list(PO.WIDE))
def test_wide_instance_conditions(name):
    """What W5 and W6 are chosen for.  Greedy < maximum; exactly ONE root holds a maximum clique and it has more than 256 (W5) / 320
    (W6) candidates, so a defect in the five- or six-word path changes clique_size itself; at the full pool every searched root stays
    in LDS; at 1024 words every five-word root goes to the slab while some four-word roots stay (251 * 4 + 16 <= 1024 < 257 * 5 + 20)."""
    gr = PO.greedy(name)
    omega, bound, root = PO.TABLE[name]
    sizes = PO.exact(name)
    assert bound < omega == max(sizes.values())
    assert [q for q, s in sizes.items() if s == omega] == [root] == [PO.WINNING_ROOT[name]]
    assert int(gr.candidates[root]) > PO.WIDE[name]
    searched = PO.searched_roots(gr)
    print(f"{name}: N {len(gr.order)} density {PO.density(PO.adjacency(name)):.3f} greedy {bound} maximum {omega} root {root} with "
          f"{int(gr.candidates[root])} candidates; searched roots {len(searched)}, over 256: {int((searched > 256).sum())}, over 320: "
          f"{int((searched > 320).sum())}, widest {int(searched.max())}")
    assert PO.searched_in_lds(gr, PO.POOL_WORDS).all()
    in_lds = PO.searched_in_lds(gr, 1024)
    assert not in_lds[searched > 256].any() and in_lds[(searched > 192) & (searched <= 256)].any()
    assert not PO.searched_in_lds(gr, 1).any()


@pytest.mark.parametrize("name,budget", SLAB_BINDS)
def test_slab_budget_settings_bind(name, budget):
    """With every root in the slab pass (lds_words = 1) and this max_nodes the replay says that workgroups run out of their shared
    budget of max_nodes / 8 before their last root: roots are left unreached (the `left <= 0` branch of pmc_search_slab_kernel),
    others are interrupted mid-search, and the clique found lies strictly between the greedy bound and the maximum."""
    r = PO.replayed(name, budget, 1)
    print(f"{name} max_nodes={budget}: workgroups that ran out {r.slab_wgs_ran_out}, roots unreached {r.slab_unreached}, interrupted "
          f"{r.slab_interrupted}, clique {r.clique_size}, counters {r.counters}")
    assert not PO.searched_in_lds(PO.greedy(name), 1).any()
    assert r.slab_wgs_ran_out >= 1 and r.slab_unreached >= 1 and r.slab_interrupted >= 1
    assert r.proven == 0 and r.counters[2] == r.slab_unreached + r.slab_interrupted
    assert r.counters[0] > 0 and PO.TABLE[name][1] < r.clique_size < PO.TABLE[name][0]
    # interrupted roots kept what they had found and unreached ones nothing
    assert (r.rnodes[r.rstat == PO.ST_BUDGET] == 0).sum() == r.slab_unreached


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


def check_predicted(key, r, row=0):
    """Row `row` of the device's result against PO.PREDICTED[key] = (name, max_nodes, lds_words): clique_size, proven, the four
    counters, the EXACT label vector, and the pose as rigid_transform_3d of those labels bit for bit."""
    from pointdsc_amd import ops
    size, members, proven, counters = PO.PREDICTED[key]
    p = PO.pair(key[0])
    got = (int(r["clique_size"][row]), int(r["proven"][row]), tuple(int(v) for v in r["counters"][row]))
    got_members = np.flatnonzero(r["pred_labels"][row].numpy() == 1.0)
    print(f"{key}: device size {got[0]} proven {got[1]} counters {got[2]} members {got_members.tolist()} | replay size {size} proven "
          f"{proven} counters {counters} members {list(members)}")
    assert got == (size, proven, counters)
    want = torch.zeros(p["corr_pos"].shape[1], dtype=torch.float32)
    want[list(members)] = 1.0
    assert torch.equal(r["pred_labels"][row].view(torch.int32), want.view(torch.int32)), "the labelled clique is not the replay's"
    pose = ops.rigid_transform_3d(g(p["src_keypts"]), g(p["tgt_keypts"]), g(want[None])).cpu()
    assert torch.equal(r["pred_trans"][row:row + 1].view(torch.int32), pose.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", PO.SEARCH)
def test_exact_where_greedy_is_not_optimal(name):
    r = ample(name)
    check_exact(name, r)
    print(f"{name}: nodes {int(r['counters'][0, 0])} roots that branched {int(r['counters'][0, 1])}")
    assert int(r["counters"][0, 0]) > 0 and int(r["counters"][0, 1]) > 0
    check_predicted((name, AMPLE, 0), r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["F600", "F1000"])
def test_fixtures_equal_the_replay(name):
    """The two fixtures of tests/test_pmc.py on which a root branches (F1000: to no avail, the greedy clique is returned)."""
    r = ample(name)
    check_exact(name, r)
    check_predicted((name, AMPLE, 0), r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PO.WIDE))
def test_wide_roots(name):
    """W5 / W6: the only root with a maximum clique has 284 / 377 candidates (test_wide_instance_conditions), so the five- and
    six-word paths decide clique_size.  Two calls return equal bits; W5 with its wide roots (1024 words) and with all roots (1 word)
    in the slab pass returns the default call's bits in every output and counter."""
    r = ample(name)
    check_exact(name, r)
    check_predicted((name, AMPLE, 0), r)
    members = np.flatnonzero(r["pred_labels"][0].numpy() == 1.0)
    gr = PO.greedy(name)
    root = PO.roots_of([members], gr.order)
    assert root == [PO.WINNING_ROOT[name]] and int(gr.candidates[root[0]]) > PO.WIDE[name]
    assert same_bits(r, run(PO.pair(name)))
    if name == "W5":
        for words in WIDE_LDS_WORDS:
            got = run(PO.pair(name), lds_words=words)
            check_predicted((name, AMPLE, words), got)
            for k in KEYS:
                assert bits_equal([got[k]], [r[k]]), f"lds_words={words}: {k} differs from the default call"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PO.WINNING_ROOT))
def test_winner_is_the_earliest_root(name):
    """TIE RULE: among roots with equally large cliques the root earliest in the order wins, so the labelled clique's last member in
    the order is the earliest of all maximum cliques' last members (PO.WINNING_ROOT: from the exact oracle root by root, and from
    networkx's enumeration on Z1, Z2, B1, B7).  Which clique wins inside a root depends on the colouring: check_predicted."""
    r = ample(name)
    members = np.flatnonzero(r["pred_labels"][0].numpy() == 1.0)
    assert PO.roots_of([members], PO.greedy(name).order) == [PO.WINNING_ROOT[name]]
    if name in PO.EARLIEST_ROOT:
        assert PO.WINNING_ROOT[name] == PO.TABLE[name][2]


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
@pytest.mark.parametrize("name", LADDER_NAMES)
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
        check_predicted((name, budget, 0), r)
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
@pytest.mark.parametrize("name,budget", SLAB_BINDS)
def test_slab_budget_binds(name, budget):
    """Every root in the slab pass and a max_nodes at which workgroups run out of their shared budget (test_slab_budget_settings_bind):
    roots the budget does not reach stay open with nothing found, interrupted ones keep their best clique."""
    r = run(PO.pair(name), max_nodes=budget, lds_words=1)
    check_predicted((name, budget, 1), r)
    size = int(r["clique_size"][0])
    assert int(r["proven"][0]) == 0 and int(r["counters"][0, 2]) > 0
    assert_clique(r["pred_labels"][0], PO.adjacency(name), size)
    assert PO.TABLE[name][1] < size < PO.TABLE[name][0]
    assert same_bits(r, run(PO.pair(name), max_nodes=budget, lds_words=1))


@pytest.mark.gpu
def test_wide_batch_equals_single_calls():
    """W5 twice in one batch, at the ample budget and at two budgets that bind: every row equals its single call bit for bit, and
    the replay."""
    p = PO.pair("W5")
    cat = {k: torch.cat([p[k], p[k]]) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    for budget in (AMPLE,) + BATCH_BUDGETS:
        batch = run(cat, max_nodes=budget)
        single = ample("W5") if budget == AMPLE else run(p, max_nodes=budget)
        assert batch["counters"].shape == (2, 4) and batch["pred_labels"].shape == (2, 1400)
        for i in range(2):
            check_predicted(("W5", budget, 0), batch, row=i)
            for k in KEYS:
                assert bits_equal([batch[k][i:i + 1]], [single[k]]), f"max_nodes={budget} row {i}: {k} differs inside the batch"


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
