"""The cases of the Infomap twin tests: the smallest graphs that reach every path of the MODE_INFO
kernels (leiden.hip), shared by the CPU tests of the twin (tests/test_infomap_twin.py) and the GPU
comparison (tests/test_gpu_infomap_twin.py).  The graphs are those of tests/leiden_graphs.py.

The twin (oracle/fc_oracle.c orc_engine_infomap) is exact wherever it counts no ambiguous decision
and no ambiguous trial choice (DESIGN.md "Leiden and Infomap"), so every case must count none: the
generator and engine seeds below are chosen so that this and the path conditions hold
(test_infomap_twin.py asserts them from the twin's trace; tune these, not the conditions).
"""
import os

import numpy as np

from tests.leiden_graphs import HUB_D, HUB_GRAPH_SEED, HUB_NOISE, hub_cliques, internal_graph, weighted_graph_cpu

CONSENSUS_NP = 8     # LPA labelings behind the working-graph case's consensus step
# engine seed per hub graph.  d = 5000 at seed 7 has a replica whose two trials end in different
# partitions of one codelength (the cliques are interchangeable): an ambiguous trial choice
HUB_ENGINE_SEED = {5000: 9}


def karate():
    from tests import golden_io
    e = np.loadtxt(os.path.join(golden_io.GOLDEN, "karate_club.txt"), dtype=np.int64)[:, :2]
    nodes, e = np.unique(e, return_inverse=True)
    return len(nodes), e.reshape(-1, 2).astype(np.int32)


def _clique(lo, size):
    iu = np.triu_indices(size, 1)
    return np.stack([iu[0] + lo, iu[1] + lo], 1)


# threshold_gadget's integers, found by an offline search over (a, b, j, k, l, bridges) for a state
# whose map-equation change times 2M lies just below zero
THRESHOLD_A, THRESHOLD_B, THRESHOLD_C = 19, 9, 12          # clique sizes
THRESHOLD_LINKS = (4, 3, 2)                                # the middle vertex's edges into A, B, C
THRESHOLD_PAD = (30, 100, 149)                             # padding cliques, their size, bridges between them


def threshold_gadget():
    """A vertex 0 joined to 4 vertices of a 19-clique A (vertices 1..19), 3 of a 9-clique B (20..28)
    and 2 of a 12-clique C, beside a ring of 30 100-cliques joined by 149 bridges (each between two
    vertices of its own).  Once every clique is a module and vertex 0 sits in A, its move to B
    changes the map equation by S / 2M with S = sum c_i x_i log2 x_i over the integer flows and
    exit weights x_i of the state (the c_i x_i sum to zero, so 2M drops out of S): S = -2.89e-6
    here, the bridges setting the total exit weight Q = 2 * 149 + 10 that brings S this close to
    zero.  The padding sets 2M = 297 862, so the delta is -9.7e-12: a gain, inside (-1e-10, -EPS).
    The threshold -INFO_MIN_GAIN (leiden.hip) holds vertex 0 in A; `delta < 0` moves it to B, where
    it stays (the way back costs 9.7e-12), and the final labels differ in that vertex.  Whether
    vertex 0 first lands in A depends on the pass order: the case's seed is one where it does in
    every replica.  Returns (n, edges [m][2] int32)."""
    a, b, c = THRESHOLD_A, THRESHOLD_B, THRESHOLD_C
    pad, size, bridges = THRESHOLD_PAD
    n = 1 + a + b + c
    e = [_clique(1, a), _clique(1 + a, b), _clique(1 + a + b, c),
         np.array([(0, lo + p) for lo, cnt in zip((1, 1 + a, 1 + a + b), THRESHOLD_LINKS) for p in range(cnt)])]
    e += [_clique(n + p * size, size) for p in range(pad)]
    e.append(np.array([(n + (i % pad) * size + 2 * (i // pad), n + ((i + 1) % pad) * size + 2 * (i // pad) + 1)
                       for i in range(bridges)]))
    return n + pad * size, np.concatenate(e).astype(np.int32)


def dense_cliques(k=520, count=2, bridges=7, seed=1):
    """`count` k-cliques, consecutive ones joined by `bridges` seeded random edges.  Every row has
    k - 1 or more entries (past 512: k_lv_heavy), and once a clique starts to merge its vertices
    decide from inside a module that holds many of their neighbours: the own-weight accumulation
    of k_lv_heavy (s_wown).  The hub of hub_cliques never does: the map equation keeps a vertex
    with d outside edges alone, so its long row has almost never weight inside its own module.
    The cliques merge so firmly that the final labels do not depend on that weight: this case
    decides thousands of such rows but cannot tell a wrong own weight.  The d = 700 shard can (its
    hub decides with own-module weight and the labels depend on it); test_cases_reach_their_paths
    asserts that property on the shard.
    Returns (n, edges [m][2] int32)."""
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(k, 1)
    e = [np.stack([iu[0] + c * k, iu[1] + c * k], 1) for c in range(count)]
    for c in range(count - 1):
        e.append(np.stack([rng.choice(k, bridges, replace=False) + c * k,
                           rng.choice(k, bridges, replace=False) + (c + 1) * k], 1))
    return count * k, np.concatenate(e).astype(np.int32)


class InfomapCase:
    """One engine run: eng.cd(4, rbegin, count, total, iteration) with infomap_trials = trials and
    FC_OPT_BUCKETS = buckets on graph `graph` ("lfr1k", "lfr1k_consensus", "lfr1k_weighted",
    "karate", "threshold", "dense" or a hub_cliques d), engine seed `seed`.  relabel:
    FC_OPT_RELABEL (2: the community-ordered numbering, known to the engine only, so such a case
    has no CPU-only twin run).  env: library switches read once per process (the run is a fresh
    child process)."""

    def __init__(self, graph, count, seed, trials=2, rbegin=0, total=None, iteration=0, buckets=0, relabel=1,
                 env=None):
        self.graph, self.count, self.seed, self.trials, self.rbegin = graph, count, seed, trials, rbegin
        self.total, self.iteration, self.buckets, self.relabel = total or count, iteration, buckets, relabel
        self.env = env or {}
        self.d = graph if isinstance(graph, int) else 0

    @property
    def id(self):
        s = "%s-s%d-r%d+%d-t%d" % ("d%d" % self.d if self.d else self.graph, self.seed, self.rbegin, self.count,
                                   self.trials)
        s += ("-b%d" % self.buckets if self.buckets else "") + ("-it%d" % self.iteration if self.iteration else "")
        s += "-relabel%d" % self.relabel if self.relabel != 1 else ""
        return s + "".join("-%s=%s" % kv for kv in sorted(self.env.items()))

    def edges(self):
        """(n, edges) of the unweighted input graph."""
        if self.d:
            return hub_cliques(self.d, noise=HUB_NOISE.get(self.d, 0.25), seed=HUB_GRAPH_SEED[self.d])
        if self.graph == "karate":
            return karate()
        if self.graph == "threshold":
            return threshold_gadget()
        if self.graph == "dense":
            return dense_cliques()
        from tests import golden_io
        case = golden_io.load("lfr1k_lpm_np20" if self.graph == "lfr1k_consensus" else "lfr1k_louvain_np20")
        return case.N, case.edges_file


INFOMAP_CASES = (
    [InfomapCase(d, 3, seed=HUB_ENGINE_SEED.get(d, 7)) for d in HUB_D] +          # every decide variant and heavy tier
    [InfomapCase("dense", 2, seed=7)] +                                           # heavy rows with own-module weight
    [InfomapCase("lfr1k", 6, seed=13)] +
    [InfomapCase(g, 3, seed=17, buckets=b) for g in ("lfr1k", 700) for b in (1, 5)] +
    [InfomapCase("lfr1k", 6, seed=23, buckets=1500)] +                            # > ILIST_MAXB: all scans unlisted
    [InfomapCase(700, 3, seed=19, rbegin=2, total=6, iteration=4)] +              # a shard
    [InfomapCase("lfr1k", 3, seed=37, trials=3)] +
    # working graphs that are not the input.  After an lpm-style consensus step (co-membership weights,
    # weight-0 closure edges) the graph is so dense that every replica ends in ONE module: the label
    # comparison is then near-trivial, and what the case pins is that weights and weight-0 edges are
    # ignored, every level's aggregation (node count and longest row per level enter lv_heavy_bytes'
    # condition) and the number of levels.  After a Louvain-style step (the Leiden cases'
    # lfr1k_weighted: weights up to 8) some two dozen modules remain, and the labels do the work
    [InfomapCase("lfr1k_consensus", 4, seed=31, iteration=1)] +
    [InfomapCase("lfr1k_weighted", 4, seed=31, iteration=3)] +
    [InfomapCase("karate", 1, seed=3, trials=1)] +                                # empty bucket lists
    # a best delta of -9.7e-12, held by the -1e-10 threshold.  One trial: the codelengths with the
    # middle vertex on either side differ by that much, so two trials could be an ambiguous choice
    [InfomapCase("threshold", 3, seed=2, trials=1)])
RELABEL_CASE = InfomapCase("lfr1k", 3, seed=11, relabel=2)                        # GPU only
LISTS_OFF_CASE = InfomapCase("lfr1k", 6, seed=13, env={"FC_INFO_LISTS": "0"})     # unlisted scans, launch maps
G2_OFF_CASE = InfomapCase(100, 3, seed=7, env={"FC_LV_G2": "0"})                  # rows of 65..128 on <.., LWS, 1>
CHILD_CASES = {c.id: c for c in (LISTS_OFF_CASE, G2_OFF_CASE)}
CPU_CASES = INFOMAP_CASES + [LISTS_OFF_CASE, G2_OFF_CASE]                         # every case the oracle can run alone


def consensus_graph_cpu(case):
    """The working-graph case's graph computed by the oracle alone: CONSENSUS_NP LPA labelings (the
    engine twin), co-membership weights, threshold, the recorded closure pairs (weight 0) -- what
    eng.cd(1), consensus_apply and closure_apply leave on the device."""
    from oracle import oracle as orc
    from tests import golden_io
    gc = golden_io.load("lfr1k_lpm_np20")
    sigma = orc.device_sigma(gc.N, case.seed)
    g = orc.EdgeGraph.from_lines(gc.N, gc.edges_file)
    lab, _ = orc.engine_cd(orc.LPM, internal_graph(gc.N, g.u, g.v, g.w, sigma), CONSENSUS_NP, 0, 0, case.seed)
    new, _ = orc.iterate(orc.LPM, g, lab[:, sigma], gc.pair_batches[0], CONSENSUS_NP, gc.tau, gc.delta, 0)
    return gc.N, new.u, new.v, new.w


def topology(case):
    """(n, edges [m][2], weights) of the graph the case's run sees, computed by the oracle alone."""
    from oracle import oracle as orc
    if case.graph == "lfr1k_consensus":
        n, u, v, w = consensus_graph_cpu(case)
    elif case.graph == "lfr1k_weighted":
        n, u, v, w = weighted_graph_cpu(case)
    else:
        n, e = case.edges()
        g = orc.EdgeGraph.from_lines(n, e)
        u, v, w = g.u, g.v, g.w
    return n, np.stack([u, v], 1), w


_twin_cache = {}


def infomap_twin(case, graph=None, sigma=None):
    """The twin's result for a case (an orc.InfomapTwin whose label arrays are in node order).
    graph = (n, u, v, w) in node ids and sigma default to what the oracle computes alone (the input
    graph / consensus_graph_cpu, and orc.device_sigma); the GPU tests pass the engine's own."""
    from oracle import oracle as orc
    key = case.id
    if graph is None and key in _twin_cache:
        return _twin_cache[key]
    if graph is None:
        assert case.relabel == 1, "the community-ordered numbering is the engine's: pass its node map"
        n, e, w = topology(case)
        u, v = e[:, 0], e[:, 1]
    else:
        n, u, v, w = graph
    if sigma is None:
        sigma = orc.device_sigma(n, case.seed)
    tw = orc.engine_infomap(internal_graph(n, u, v, w, sigma), case.count, case.rbegin, case.iteration, case.seed,
                            trials=case.trials, buckets=case.buckets)
    tw.trial_labels = np.ascontiguousarray(tw.trial_labels[:, :, sigma])
    tw.labels = np.ascontiguousarray(tw.labels[:, sigma])
    if graph is None:
        _twin_cache[key] = tw
    return tw
