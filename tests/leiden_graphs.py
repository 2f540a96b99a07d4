"""Graphs whose rows reach every row-length path of the Leiden kernels (leiden.hip), shared by
the CPU tests of the twin (tests/test_leiden.py) and the GPU comparison
(tests/test_gpu_leiden_twin.py), and the map-equation codelength both Infomap test files use.

hub_cliques(d): `hubs` linked hubs, each joined to one vertex of each of its d 4-cliques, plus
seeded random edges between cliques.  A hub's row is d (+ hubs - 1) entries long at level 0; the
aggregate that holds it keeps a row of about d entries with about d distinct candidate
communities at level 1, and the member-row sum of its refined community exceeds d.
"""
import numpy as np


def hub_cliques(d, hubs=1, noise=0.25, seed=1):
    """Returns (n, edges [m][2] int32).  Vertices 0..hubs-1 are the hubs; hub h's clique i is the
    4 vertices from hubs + 4 * (h * d + i); noise * (number of cliques) random clique-to-clique
    edges."""
    rng = np.random.default_rng(seed)
    nc = hubs * d
    first = hubs + 4 * np.arange(nc)
    e = [np.stack([first + a, first + b], 1) for a in range(4) for b in range(a + 1, 4)]
    e.append(np.stack([np.repeat(np.arange(hubs), d), first], 1))            # hub -- clique vertex 0
    if hubs > 1:
        e.append(np.stack([np.arange(hubs - 1), np.arange(1, hubs)], 1))    # the hubs, in a path
    k = int(noise * nc)
    if k:
        ca, cb = rng.integers(0, nc, k), rng.integers(0, nc, k)
        ok = ca != cb
        # clique vertices 1..3: the hub's neighbour keeps its one outside edge
        e.append(np.stack([first[ca[ok]] + rng.integers(1, 4, int(ok.sum())),
                           first[cb[ok]] + rng.integers(1, 4, int(ok.sum()))], 1))
    return hubs + 4 * nc, np.concatenate(e).astype(np.int32)


def plogp(p):
    p = np.asarray(p, np.float64)
    out = np.zeros_like(p)
    nz = p > 0
    out[nz] = p[nz] * np.log2(p[nz])
    return out


def codelength(N, e, lab):
    """Two-level map equation (bits) of a partition of an unweighted undirected graph."""
    deg = np.bincount(e.ravel(), minlength=N).astype(np.float64)
    W = deg.sum()
    k = int(lab.max()) + 1
    tot = np.bincount(lab, weights=deg, minlength=k)
    cut = lab[e[:, 0]] != lab[e[:, 1]]
    out = np.bincount(lab[e[cut, 0]], minlength=k) + np.bincount(lab[e[cut, 1]], minlength=k)
    q, p = out / W, tot / W
    return float(plogp(q.sum()) - 2 * plogp(q).sum() - plogp(deg / W).sum() + plogp(q + p).sum())


# ------------------------------------------------------------------ the cases of the twin tests
HUB_D = (50, 100, 300, 700, 1500, 3000, 5000)   # one per decide variant and heavy tier (leiden.hip)
# generator seed per d: chosen so that the preconditions of the GPU tests hold (test_leiden.py
# asserts them from the twin's trace; tune these, not the conditions)
HUB_GRAPH_SEED = {50: 50, 100: 100, 300: 300, 700: 700, 1500: 1500, 3000: 3000, 5000: 1}
# random clique-to-clique edges per clique.  0.25 merges enough cliques that the hub aggregate's row
# shrinks by a quarter from level 2 on; d = 5000 takes 0.1, so that its row stays past 4096 entries
# (the global-table tier) on every level and the refine sweeps of levels >= 2 decide it too
HUB_NOISE = {5000: 0.1}


class LeidenCase:
    """One engine run: eng.cd(3, rbegin, count, total, iteration) with FC_OPT_BUCKETS = buckets on
    graph `graph` ("lfr1k", "lfr1k_weighted" or a hub_cliques d), engine seed `seed`."""

    def __init__(self, graph, count, seed, rbegin=0, total=None, iteration=0, buckets=0):
        self.graph, self.count, self.seed, self.rbegin = graph, count, seed, rbegin
        self.total, self.iteration, self.buckets = total or count, iteration, buckets
        self.d = graph if isinstance(graph, int) else 0

    @property
    def id(self):
        s = "%s-s%d-r%d+%d" % ("d%d" % self.d if self.d else self.graph, self.seed, self.rbegin, self.count)
        return s + ("-b%d" % self.buckets if self.buckets else "") + ("-it%d" % self.iteration if self.iteration else "")

    def edges(self):
        """(n, edges) of the unweighted input graph."""
        if self.d:
            return hub_cliques(self.d, noise=HUB_NOISE.get(self.d, 0.25), seed=HUB_GRAPH_SEED[self.d])
        from tests import golden_io
        case = golden_io.load("lfr1k_louvain_np20")
        return case.N, case.edges_file


LEIDEN_CASES = (
    [LeidenCase(d, 3, seed=7) for d in HUB_D] +
    [LeidenCase("lfr1k", 6, seed=13)] +
    [LeidenCase(g, 3, seed=17, buckets=b) for g in ("lfr1k", 700) for b in (0, 1, 5)] +
    [LeidenCase(700, 3, seed=19, rbegin=2, total=6, iteration=4)] +
    [LeidenCase("lfr1k_weighted", 4, seed=31, iteration=3)])
G2_OFF_CASE = LeidenCase(100, 3, seed=7)   # FC_LV_G2=0: rows of 65..128 entries on the one-vertex-per-wave variant
INFOMAP_D = (100, 700, 5000)
WEIGHTED_NP = 8     # Louvain labelings behind the weighted case's consensus weights


def internal_graph(n, u, v, w, sigma):
    """The engine's working graph: edges (u, v, w) in node ids -> oracle EdgeGraph in the engine's
    internal numbering sigma (fc_get_node_map)."""
    from oracle import oracle as orc
    a, b = sigma[u], sigma[v]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    o = np.lexsort((hi, lo))
    return orc.EdgeGraph(n, lo[o], hi[o], np.asarray(w)[o], np.zeros(len(o), np.int64))


def weighted_graph_cpu(case):
    """The weighted case's working graph computed by the oracle alone: WEIGHTED_NP Louvain
    labelings (the engine twin), consensus weights, threshold, the recorded closure pairs, repair
    -- what eng.cd(0), consensus_apply and closure_apply leave on the device."""
    from oracle import oracle as orc
    from tests import golden_io
    gc = golden_io.load("lfr1k_louvain_np20")
    sigma = orc.device_sigma(gc.N, case.seed)
    g = orc.EdgeGraph.from_lines(gc.N, gc.edges_file)
    lab, _ = orc.engine_cd(0, internal_graph(gc.N, g.u, g.v, g.w, sigma), WEIGHTED_NP, 0, 0, case.seed)
    new, _ = orc.iterate(0, g, lab[:, sigma], gc.pair_batches[0], WEIGHTED_NP, gc.tau, gc.delta, 0)
    return gc.N, new.u, new.v, new.w


_twin_cache = {}


def leiden_twin(case, graph=None, sigma=None):
    """The twin's (labels in node order, traces) of a case.  graph = (n, u, v, w) in node ids and
    sigma default to what the oracle computes alone (unit weights / weighted_graph_cpu, and
    orc.device_sigma); the GPU tests pass the engine's own for the weighted case."""
    from oracle import oracle as orc
    key = case.id
    if graph is None and key in _twin_cache:
        return _twin_cache[key]
    if graph is None:
        if case.graph == "lfr1k_weighted":
            n, u, v, w = weighted_graph_cpu(case)
        else:
            n, e = case.edges()
            g = orc.EdgeGraph.from_lines(n, e)
            n, u, v, w = n, g.u, g.v, g.w
    else:
        n, u, v, w = graph
    if sigma is None:
        sigma = orc.device_sigma(n, case.seed)
    lab, tr = orc.engine_leiden(internal_graph(n, u, v, w, sigma), case.count, case.rbegin, case.iteration, case.seed,
                                buckets=case.buckets)
    out = (lab[:, sigma], tr)
    if graph is None:
        _twin_cache[key] = out
    return out
