"""Replica-lane decide (cd_rl.hip k_rl_decide) at the boundaries of its sorting networks.

Rows of <= 16, <= 24, <= 32, <= 48 and <= 64 entries are decided by networks of that width, longer
ones by k_rl_exact.  The graph here has vertices of degree exactly 1, 15..17, 23..25, 31..33,
47..49 and 63..65, so every network sees its shortest and its longest row and the heavy path its
first one; the engine must agree with the CPU twin bit for bit on the unit-weight graph (WM_UNIT)
and on a weighted consensus graph with weights < 256 (WM_W8), for a 64-lane group part full
(33 replicas), full (64, rows read per wave and per lane) and in two banks (70), and for the
per-lane layout (6 replicas), Louvain and LPA.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.twin_graph import internal_graph

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUNDARY_DEGREES = [1, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65]
PER_DEGREE = 4            # vertices of each boundary degree
BLOCKS, BLOCK = 30, 100   # planted blocks of the base graph
SEED = 97
N_P = 20                  # labelings behind the consensus graph: weights <= 20 < 256
TAU, DELTA = 0.2, 0.02


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


def _graph():
    """Planted blocks (p_in = 0.15, one edge per vertex to another block) plus probe vertices: a
    probe of degree d has d distinct neighbours among the base vertices of one block and no other
    edge, so its degree is exactly d once the engine has deduplicated the edge list."""
    rng = np.random.default_rng(20240607)
    nb = BLOCKS * BLOCK
    edges = []
    iu = np.triu_indices(BLOCK, 1)
    for b in range(BLOCKS):
        keep = rng.random(len(iu[0])) < 0.15
        edges.append(np.stack([iu[0][keep], iu[1][keep]], 1) + b * BLOCK)
    src = np.arange(nb)
    dst = (src + BLOCK * rng.integers(1, BLOCKS, nb) + rng.integers(0, BLOCK, nb)) % nb
    edges.append(np.stack([src, dst], 1))
    v = nb
    for i, d in enumerate(BOUNDARY_DEGREES):
        for k in range(PER_DEGREE):
            b = (i * PER_DEGREE + k) % BLOCKS
            nbrs = b * BLOCK + rng.choice(BLOCK, d, replace=False)
            edges.append(np.stack([np.full(d, v), nbrs], 1))
            v += 1
    e = np.concatenate(edges).astype(np.int32)
    return v, e[e[:, 0] != e[:, 1]]


N, EDGES = _graph()


def _degrees(eng):
    u, v, _, _ = eng.get_graph()
    return np.bincount(np.concatenate([u, v]), minlength=N)


def _unit_engine(fcmod):
    eng = fcmod.Engine(seed=SEED)
    eng.set_option("cd_engine", 1)
    eng.load_graph(N, EDGES[:, 0], EDGES[:, 1])
    deg = _degrees(eng)
    for d in BOUNDARY_DEGREES:
        assert (deg == d).sum() >= PER_DEGREE, "no vertices of degree %d" % d
    return eng


def _weighted_engine(fcmod):
    """One louvain iteration of the step API on this graph, with the labelings of a first CD call
    (as test_gpu_parity._weighted_consensus_engine does with recorded ones)."""
    eng = _unit_engine(fcmod)
    eng.cd(0, 0, N_P, N_P, 1)
    eng.set_labels(eng.get_labels(N_P))
    part = torch.zeros(max(int(eng.m), 1), dtype=torch.int32, device="cuda")
    eng.consensus_partial(0, part)
    eng.consensus_apply(0, N_P, TAU, DELTA, part)
    nc = eng.closure_sample(eng.m, 0)
    cnt = torch.zeros(max(int(nc), 1), dtype=torch.int32, device="cuda")
    eng.closure_partial(cnt)
    eng.closure_apply(0, N_P, DELTA, cnt, 0)
    _, _, w, _ = eng.get_graph()
    assert 1 < w.max() < 256, "not a W8 graph"
    deg = _degrees(eng)
    for lo, hi in [(1, 16), (17, 32), (33, 48), (49, 64)]:
        assert ((deg >= lo) & (deg <= hi)).any(), "no row of %d..%d entries in the consensus graph" % (lo, hi)
    return eng


_expected = {}


def _twin(eng, algo, n_r, weighted, iteration):
    """The twin's labelings in node order, computed once per (algorithm, batch, graph)."""
    key = (algo, n_r, weighted)
    if key not in _expected:
        if weighted:
            g_int, sigma = internal_graph(eng, N)
        else:                                      # the input graph, deduplicated as the engine does
            sigma = eng.node_map()
            g_int = orc.EdgeGraph.from_lines(N, np.stack([sigma[EDGES[:, 0]], sigma[EDGES[:, 1]]], 1))
        exp, _ = orc.engine_cd(algo, g_int, n_r, 0, iteration, SEED, shared=1, coarsen=0)
        exp = exp[:, sigma]
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


# n_r, FC_RL_U1: one unit per wave at 33 / 64 / 70 replicas, the 64-replica batch per lane too,
# and the per-lane layout of 6 replicas (lane groups of 8) that shares rl_runs
LAYOUTS = [(33, None), (64, "1"), (64, "0"), (70, None), (6, None)]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "w8"])
@pytest.mark.parametrize("n_r,u1", LAYOUTS)
@pytest.mark.parametrize("algo", [0, 1], ids=["louvain", "lpa"])
def test_rl_decide_boundary_rows_bit_exact_vs_twin(fcmod, algo, n_r, u1, weighted, monkeypatch):
    if u1 is not None:
        monkeypatch.setenv("FC_RL_U1", u1)
    eng = _weighted_engine(fcmod) if weighted else _unit_engine(fcmod)
    iteration = 3 if weighted else 1
    eng.cd(algo, 0, n_r, n_r, iteration)
    exp = _twin(eng, algo, n_r, weighted, iteration)
    np.testing.assert_array_equal(eng.get_labels(n_r), exp)
    k = n_r // 2                                   # a shard [1, 1 + k) of the batch
    eng.cd(algo, 1, k, n_r, iteration)
    np.testing.assert_array_equal(eng.get_labels(k), exp[1:1 + k])
    eng.close()
