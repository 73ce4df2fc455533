"""The PMC baseline (reference baseline_scripts/baseline_3DMatch.py:56-77) on the device: pointdsc_amd.baselines.PMC,
pdsc_pmc_adjacency / pdsc_pmc_baseline (csrc/pmc.hip).

The oracle lives here and is the contract: the adjacency is the reference's fp32 edge rule, vectorised in numpy, and the clique size
comes from networkx.max_weight_clique(G, weight=None) (an exact branch and bound; maximal-clique enumeration does not terminate in
useful time on these graphs).  Which maximum clique is returned is not defined by the reference, so the tests check the size, that the
labelled set is a clique of the oracle's graph, and the pose computed from it.
"""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from pointdsc_amd import synthetic

ROOT = Path(__file__).resolve().parents[1]
THR = 0.10
# (N, inlier_ratio, seed) -> maximum clique size (test_oracle_sizes recomputes them on the CPU)
FIXTURES = {(70, 0.3, 1): 13, (257, 0.2, 2): 39, (600, 0.2, 3): 82, (1000, 0.1, 4): 52}
FIXTURE_IDS = [f"n{n}" for n, _, _ in FIXTURES]


# ---- the oracle ------------------------------------------------------------------------------------------------------
def oracle_adjacency(corr: np.ndarray, thr: float) -> np.ndarray:
    """[N,N] bool: |sum((c_i[0:3]-c_j[0:3])**2) - sum((c_i[3:6]-c_j[3:6])**2)| < thr in fp32 (each sum left to right), zero diagonal."""
    c = np.asarray(corr, dtype=np.float32)
    d1 = ((c[:, None, 0:3] - c[None, :, 0:3]) ** 2).sum(-1)
    d2 = ((c[:, None, 3:6] - c[None, :, 3:6]) ** 2).sum(-1)
    assert d1.dtype == np.float32 and d2.dtype == np.float32
    adj = np.abs(d1 - d2) < np.float32(thr)
    np.fill_diagonal(adj, False)
    return adj


def oracle_clique_size(adj: np.ndarray) -> int:
    import networkx as nx
    g = nx.from_numpy_array(adj)
    if g.number_of_edges() == 0:
        return 1
    clique, weight = nx.max_weight_clique(g, weight=None)
    assert weight == len(clique)
    return len(clique)


@functools.lru_cache(maxsize=None)
def pair(n: int, ratio: float, seed: int):
    return synthetic.make_pair(n, inlier_ratio=ratio, seed=seed)


@functools.lru_cache(maxsize=None)
def pair_adjacency(n: int, ratio: float, seed: int) -> np.ndarray:
    adj = oracle_adjacency(pair(n, ratio, seed)["corr_pos"][0].numpy(), THR)
    adj.setflags(write=False)
    return adj


def unpack_bits(bits: torch.Tensor, n: int) -> np.ndarray:
    """int64 [N, ld] -> bool [N, 64 ld]."""
    b = bits.cpu().numpy().view(np.uint64)
    return ((b[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(b.shape[0], -1)


def g(t):
    return t.cuda()


def run_pmc(p, **kw):
    from pointdsc_amd import baselines
    return baselines.PMC(g(p["corr_pos"]), g(p["src_keypts"]), g(p["tgt_keypts"]), THR, return_info=True, **kw)


def assert_clique(labels: torch.Tensor, adj: np.ndarray, size: int):
    lab = labels.cpu().numpy()
    assert set(np.unique(lab)) <= {0.0, 1.0}
    members = np.flatnonzero(lab == 1.0)
    assert len(members) == size
    sub = adj[np.ix_(members, members)]
    assert sub.sum() == size * (size - 1), "the labelled set is not a clique of the oracle's graph"


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_reference_double_loop():
    """baseline_3DMatch.py:61-68 restated (np.float32 rows, np.sum, np.abs, `<` against the python float) on the N = 70 fixture."""
    corr = pair(70, 0.3, 1)["corr_pos"][0].detach().cpu().numpy()
    assert corr.dtype == np.float32
    n = corr.shape[0]
    edges = set()
    for ind_1 in range(n):
        for ind_2 in range(0, ind_1):
            diff = np.sum((corr[ind_1][0:3] - corr[ind_2][0:3]) ** 2) - np.sum((corr[ind_1][3:] - corr[ind_2][3:]) ** 2)
            if np.abs(diff) < THR:
                edges.add((ind_1, ind_2))
    adj = pair_adjacency(70, 0.3, 1)
    assert (adj == adj.T).all() and not adj.diagonal().any()
    got = {(int(i), int(j)) for i, j in zip(*np.nonzero(adj)) if i > j}
    assert got == edges and len(edges) > 100


@pytest.mark.parametrize("fx", list(FIXTURES), ids=FIXTURE_IDS)
def test_oracle_sizes(fx):
    assert oracle_clique_size(pair_adjacency(*fx)) == FIXTURES[fx]


def test_pmc_symbols_exported():
    from pointdsc_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    declared = {n for n in re.findall(r"\b(pdsc_[a-z0-9_]+)\s*\(", header) if n.startswith("pdsc_pmc_")}
    assert declared == {"pdsc_pmc_adjacency", "pdsc_pmc_workspace_bytes", "pdsc_pmc_baseline", "pdsc_pmc_baseline_ex"}
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert name in _lib.SIGNATURES and re.search(rf"\bT {name}\b", out), name
    # argument checks come before any HIP call
    assert lib.pdsc_pmc_workspace_bytes(1, 0) == 0 and lib.pdsc_pmc_workspace_bytes(3, 257) > 3 * 2 * 257 * 5 * 8
    assert lib.pdsc_pmc_adjacency(None, 0.1, None, 1, 1, 8, None) == -1 and b"null pointer" in lib.pdsc_last_error()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.pdsc_pmc_baseline(p, p, p, 0.1, 0, p, p, p, p, p, 64, 1, 8, None) == -1 and b"max_nodes" in lib.pdsc_last_error()
    assert lib.pdsc_pmc_baseline(p, p, p, 0.1, 100, p, p, p, p, p, 64, 1, 8, None) == -2 and b"workspace" in lib.pdsc_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fx", list(FIXTURES), ids=FIXTURE_IDS)
def test_adjacency_bit_exact_fixtures(fx):
    from pointdsc_amd import baselines
    n = fx[0]
    want = pair_adjacency(*fx)
    ld = (n + 63) // 64 + 1                                       # one padding word per row
    bits = baselines.pmc_adjacency(g(pair(*fx)["corr_pos"]), THR, ld_words=ld)
    assert bits.shape == (1, n, ld) and bits.dtype == torch.int64
    got = unpack_bits(bits[0], n)
    assert (got[:, :n] == want).all(), "edge set differs from numpy's fp32 rule"
    assert not got[:, n:].any(), "padding bits set"
    assert not got[:, :n].diagonal().any() and (got[:, :n] == got[:, :n].T).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_adjacency_bit_exact_small(n):
    from pointdsc_amd import baselines
    p = synthetic.make_pair(n, inlier_ratio=0.5, seed=100 + n)
    want = oracle_adjacency(p["corr_pos"][0].numpy(), THR)
    got = unpack_bits(baselines.pmc_adjacency(g(p["corr_pos"]), THR)[0], n)
    assert got.shape == (n, 64 * ((n + 63) // 64))
    assert (got[:, :n] == want).all() and not got[:, n:].any()
    assert n < 63 or want.any()


@pytest.mark.gpu
def test_adjacency_batch_equals_single_calls():
    from pointdsc_amd import baselines
    ps = [pair(257, 0.2, 2)] + [synthetic.make_pair(257, inlier_ratio=0.2, seed=s) for s in (12, 13)]
    batch = baselines.pmc_adjacency(g(torch.cat([p["corr_pos"] for p in ps])), THR)
    assert batch.shape == (3, 257, 5)
    for i, p in enumerate(ps):
        assert torch.equal(batch[i], baselines.pmc_adjacency(g(p["corr_pos"]), THR)[0])
    assert not torch.equal(batch[0], batch[1])


@pytest.mark.gpu
@pytest.mark.parametrize("fx", list(FIXTURES), ids=FIXTURE_IDS)
def test_exact_size_and_pose(fx):
    """proven at the default budget, the oracle's size, a clique of the oracle's graph; the pose is ops.rigid_transform_3d of the
    labels bit for bit and meets the RE / TE thresholds of ops.eval_stats."""
    from pointdsc_amd import ops
    p = pair(*fx)
    trans, labels, size, proven = run_pmc(p)
    assert trans.shape == (1, 4, 4) and labels.shape == (1, fx[0]) and size.shape == (1,) and proven.shape == (1,)
    assert int(proven[0]) == 1
    assert int(size[0]) == FIXTURES[fx]
    assert_clique(labels[0], pair_adjacency(*fx), FIXTURES[fx])
    want = ops.rigid_transform_3d(g(p["src_keypts"]), g(p["tgt_keypts"]), labels)
    assert torch.equal(trans.view(torch.int32), want.view(torch.int32))
    stats = ops.eval_stats(trans, g(p["gt_trans"]), labels, g(p["gt_labels"])).cpu().numpy()
    print(f"N={fx[0]} RE {stats[0, 1]:.4f} deg TE {stats[0, 2]:.4f} cm precision {stats[0, 6]:.3f}")
    assert stats[0, 0] == 1.0                                     # RE < 15 deg and TE < 30 cm


@pytest.mark.gpu
def test_deterministic_and_batch_invariant():
    from pointdsc_amd import baselines
    p600 = pair(600, 0.2, 3)
    assert bits_equal(run_pmc(p600), run_pmc(p600))
    ps = [pair(257, 0.2, 2)] + [synthetic.make_pair(257, inlier_ratio=0.2, seed=s) for s in (12, 13)]
    cat = {k: torch.cat([p[k] for p in ps]) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    batch = baselines.PMC(g(cat["corr_pos"]), g(cat["src_keypts"]), g(cat["tgt_keypts"]), THR, return_info=True)
    assert bits_equal(batch, baselines.PMC(g(cat["corr_pos"]), g(cat["src_keypts"]), g(cat["tgt_keypts"]), THR, return_info=True))
    for i, p in enumerate(ps):
        single = run_pmc(p)
        assert bits_equal([x[i:i + 1] for x in batch], single), f"pair {i} differs inside the batch"
    assert int(batch[2][0]) == 39 and int(batch[3][0]) == 1


@pytest.mark.gpu
def test_budget_of_one_node_returns_normally():
    fx = (600, 0.2, 3)
    a = run_pmc(pair(*fx), max_nodes=1)
    b = run_pmc(pair(*fx), max_nodes=1)
    assert bits_equal(a, b)
    trans, labels, size, proven = a
    s = int(size[0])
    print(f"max_nodes=1: clique_size {s} proven {int(proven[0])}")
    assert 1 <= s <= FIXTURES[fx]
    assert_clique(labels[0], pair_adjacency(*fx), s)
    assert int(proven[0]) in (0, 1) and (int(proven[0]) == 0 or s == FIXTURES[fx])
    assert torch.isfinite(trans).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [(600, 0.2, 3), (1000, 0.1, 4)], ids=["n600", "n1000"])
def test_slab_pass_gives_the_same_result(fx):
    """With one word of LDS no root fits the first search pass: every root is searched by the slab pass (matrix and stack in the
    workspace, 64 workgroups sharing roots).  Same code, so the same bits and the same node count as the default path."""
    from pointdsc_amd import baselines
    p = pair(*fx)
    args = (g(p["corr_pos"]), g(p["src_keypts"]), g(p["tgt_keypts"]), THR)
    want = baselines.pmc_run(*args)
    got = baselines.pmc_run(*args, lds_words=1)
    keys = ("pred_trans", "pred_labels", "clique_size", "proven", "counters")
    assert bits_equal([got[k] for k in keys], [want[k] for k in keys])
    assert int(got["proven"][0]) == 1 and int(got["clique_size"][0]) == FIXTURES[fx] and int(got["counters"][0, 0]) > 0
    assert_clique(got["pred_labels"][0], pair_adjacency(*fx), FIXTURES[fx])
    # a slab workgroup's roots share one budget, a node charged 8: 7 buys nothing, the greedy clique is returned unproven
    low = baselines.pmc_run(*args, max_nodes=7, lds_words=1)
    assert int(low["proven"][0]) == 0 and int(low["counters"][0, 0]) == 0
    assert int(low["clique_size"][0]) == int(want["counters"][0, 3])
    assert_clique(low["pred_labels"][0], pair_adjacency(*fx), int(low["clique_size"][0]))


@pytest.mark.gpu
def test_named_rules_and_bad_arguments():
    from pointdsc_amd import baselines, ops
    p = pair(70, 0.3, 1)
    args = (g(p["corr_pos"]), g(p["src_keypts"]), g(p["tgt_keypts"]))
    trans, labels, size, proven = baselines.PMC(*args, 0.0, return_info=True)       # `<` is strict: no edges
    assert int(size[0]) == 1 and int(proven[0]) == 1
    assert labels[0, 0] == 1 and float(labels.sum()) == 1
    assert torch.equal(trans.view(torch.int32), ops.rigid_transform_3d(args[1], args[2], labels).view(torch.int32))
    one = synthetic.make_pair(1, seed=5)
    trans, labels, size, proven = run_pmc(one)
    assert int(size[0]) == 1 and int(proven[0]) == 1 and labels.tolist() == [[1.0]]
    assert len(baselines.PMC(*args, THR)) == 2                                        # the reference's return value
    with pytest.raises(RuntimeError, match="pdsc_pmc_baseline"):                    # N = 0
        baselines.PMC(args[0][:, :0], args[1][:, :0], args[2][:, :0], THR)
    with pytest.raises(RuntimeError, match="max_nodes"):
        baselines.PMC(*args, THR, max_nodes=0)
    from pointdsc_amd import _lib
    lib = _lib.load()
    nb = int(lib.pdsc_pmc_workspace_bytes(1, 70))
    ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
    out = torch.empty(64, device="cuda", dtype=torch.float32)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.pdsc_pmc_baseline(ptr(args[0]), ptr(args[1]), ptr(args[2]), THR, 100, ptr(out), ptr(labels), ptr(size), ptr(proven), ptr(ws),
                               nb - 1, 1, 70, torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.check(rc, "pdsc_pmc_baseline")


@pytest.mark.gpu
def test_harness_baseline_model_matches_direct_calls():
    """harness.BaselineModel (tools/eval_harness.py --baseline) is the baselines' result behind the model's calling convention."""
    from pointdsc_amd import baselines, harness
    ps = [pair(70, 0.3, 1), pair(257, 0.2, 2)]
    dev = [{k: g(p[k]) for k in ("corr_pos", "src_keypts", "tgt_keypts")} for p in ps]
    for method, fn in (("PMC", baselines.PMC), ("SM", baselines.SM)):
        model = harness.BaselineModel(method, THR)
        want = [fn(d["corr_pos"], d["src_keypts"], d["tgt_keypts"], THR) for d in dev]
        one = model({**dev[0], "testing": True})
        assert torch.equal(one["final_trans"], want[0][0]) and torch.equal(one["final_labels"], want[0][1])
        rag = model({k: [d[k][0] for d in dev] for k in dev[0]})                     # pairs of different N
        assert rag["final_trans"].shape == (2, 4, 4)
        for i in range(2):
            assert torch.equal(rag["final_trans"][i], want[i][0][0]) and torch.equal(rag["final_labels"][i], want[i][1][0])
    with pytest.raises(ValueError):
        harness.BaselineModel("RANSAC")
