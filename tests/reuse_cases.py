"""The data of the used-engine tests (tests/test_gpu_engine_reuse.py, GPU) and of their CPU-only
preconditions (tests/test_reuse_cases.py): TARGETS, HISTORIES and the MATRIX of (history, target)
pairs that runs.

A target is one operation whose expected result comes from the CPU alone -- the oracle, the CPU
engine model (tests/cpu_engine.py) or a *_ref.py module -- and so has no history by construction.
`reference()` computes it once per process (functools.lru_cache); `run(eng, ref)` sets every option
and the seed the target depends on, loads its graph into the engine it is given, runs and asserts,
np.array_equal throughout (floats: the bound of the entry point's own GPU test).  The internal
numbering comes from orc.device_sigma, and eng.node_map() is asserted equal to it.

A history is what the same engine did before: a plain function history(fc, eng, target), `target`
the one that follows (for "the target's own graph"), which leaves the engine open with whatever
options, labelings, hierarchy, closure state and buffer contents it ended with.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_levels_ref as lref
from tests import consensus_ref as cref
from tests import golden_io, score_ref
from tests.infomap_graphs import InfomapCase, infomap_twin, karate
from tests.leiden_graphs import LeidenCase, leiden_twin, weighted_graph_cpu
from tests.twin_graph import cd_twin

# every option a history or a target touches, at the engine's default (fc_ctx.h)
DEFAULTS = {"buckets": 0, "max_sweeps": 200, "max_iters": 1000, "chunk": 16, "prune": 1, "relabel": 1,
            "tail_visits": -1, "coarsen": 8, "store": 1, "closure_rounds": 0, "prune_mark": 1, "infomap_trials": 10,
            "cd_engine": 2, "dense_div": 0}


def apply_options(eng, seed, **over):
    """The target's options, all of them and explicitly: DEFAULTS, `over` on top, and the seed."""
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    for k, v in dict(DEFAULTS, **over).items():
        eng.set_option(k, v)
    eng.set_option("seed", seed)


@functools.lru_cache(maxsize=None)
def lfr1k():
    return golden_io.load("lfr1k_louvain_np20")


def lfr1k_graph():
    case = lfr1k()
    return case.N, case.edges_file


@functools.lru_cache(maxsize=None)
def karate_graph():
    return karate()


def dev_i32(n):
    import torch
    return torch.zeros(max(int(n), 1), dtype=torch.int32, device="cuda")


def load(eng, graph, seed, relabel=1):
    """load_graph, and the node map the CPU side predicts for (n, seed, relabel)."""
    n, e = graph
    eng.load_graph(n, e[:, 0], e[:, 1])
    sigma = orc.device_sigma(n, seed) if relabel else np.arange(n, dtype=np.int32)
    assert np.array_equal(eng.node_map(), sigma), "node map after a history"
    return sigma


def same_graph(got, exp, tag):
    for name, a, b in zip(("u", "v", "w", "age"), got, exp):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


# ------------------------------------------------------------------ targets 1-3: whole runs
RUN_SEED, RUN_MAX_ITERS, RUN_DELTA = 17, 50, 0.02


class RunTarget:
    """fc_run on LFR-1k with default options == the CPU engine model driven by run_sharded."""

    def __init__(self, name, algo, n_p, tau):
        self.id, self.algo, self.n_p, self.tau = name, algo, n_p, tau
        self.replicas, self.seed = n_p, RUN_SEED
        self.graph = lfr1k_graph

    @functools.lru_cache(maxsize=None)
    def reference(self):
        from fastconsensus_amd.distributed import run_sharded
        from tests.cpu_engine import OracleEngine
        n, e = self.graph()
        cpu = OracleEngine(seed=RUN_SEED, sigma=orc.device_sigma(n, RUN_SEED))
        cpu.load_graph(n, e[:, 0], e[:, 1])
        labels, st = run_sharded(cpu, self.algo, self.n_p, self.tau, RUN_DELTA, device="cpu", max_iters=RUN_MAX_ITERS)
        return {"labels": labels.copy(), "iterations": st["iterations"], "partition_edges": st["partition_edges"],
                "hit_iter_cap": st["hit_iter_cap"], "graph": cpu.get_graph()}

    def run(self, eng, ref):
        apply_options(eng, RUN_SEED, max_iters=RUN_MAX_ITERS)
        load(eng, self.graph(), RUN_SEED)
        labels, st = eng.run(self.algo, self.n_p, self.tau, RUN_DELTA)
        assert st["iterations"] == ref["iterations"], (st["iterations"], ref["iterations"])
        assert st["partition_edges"] == ref["partition_edges"]
        assert labels.shape == ref["labels"].shape and np.array_equal(labels, ref["labels"])
        same_graph(eng.get_graph(), ref["graph"], self.id)


# ------------------------------------------------------------------ target 4: CD batches, engines 0 and 1
CD_SEED, CD_ITERATION = 99, 4
CD_REPLICAS = (3, 64)          # 64: one unit per wave in the replica-lane decide
CD_TWIN = {0: {"shared": 0}, 1: {"shared": 1, "coarsen": 0}}     # FC_OPT_CD_ENGINE -> orc.engine_cd's arguments


class CdTarget:
    """Louvain and LPA batches of 3 and of 64 replicas on one non-default CD engine == orc.engine_cd."""

    def __init__(self, name, engine):
        self.id, self.engine = name, engine
        self.replicas, self.seed = max(CD_REPLICAS), CD_SEED
        self.graph = lfr1k_graph

    def batches(self):
        # 3 then 64, then 64 then 3: the replica-lane state grows and shrinks inside the target too
        return [(0, CD_REPLICAS[0]), (0, CD_REPLICAS[1]), (1, CD_REPLICAS[1]), (1, CD_REPLICAS[0])]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        n, e = self.graph()
        sigma = orc.device_sigma(n, CD_SEED)
        return {(algo, n_r): cd_twin(sigma, algo, n, e, n_r, 0, CD_ITERATION, CD_SEED, **CD_TWIN[self.engine])[0]
                for algo, n_r in self.batches()}

    def run(self, eng, ref):
        apply_options(eng, CD_SEED, cd_engine=self.engine)
        load(eng, self.graph(), CD_SEED)
        for algo, n_r in self.batches():
            eng.cd(algo, 0, n_r, n_r, CD_ITERATION)
            assert eng.replica_info() == (n_r, 0, n_r)
            got = eng.get_labels(n_r)
            bad = [r for r in range(n_r) if not np.array_equal(got[r], ref[(algo, n_r)][r])]
            assert not bad, "engine %d algo %d, %d replicas: rows %s differ" % (self.engine, algo, n_r, bad)


# ------------------------------------------------------------------ target 5: Leiden batches
class LeidenTarget:
    """A 3-replica (hub) / 4-replica (weighted) Leiden batch == orc.engine_leiden on the graph and
    numbering the oracle computes alone."""

    def __init__(self, name, case):
        self.id, self.case, self.seed = name, case, case.seed
        self.replicas = max(case.count, 8 if case.graph == "lfr1k_weighted" else 0)
        self.graph = case.edges

    @functools.lru_cache(maxsize=None)
    def reference(self):
        lab, traces = leiden_twin(self.case)
        ref = {"labels": lab, "renumbered": orc.renumber(lab), "traces": traces}
        if self.case.graph == "lfr1k_weighted":
            ref["working"] = weighted_graph_cpu(self.case)
        return ref

    def run(self, eng, ref):
        from tests.test_gpu_leiden_twin import run_leiden
        case = self.case
        apply_options(eng, case.seed, buckets=case.buckets)
        lab, ren, st, (n, u, v, w), sigma = run_leiden(eng, case)
        assert np.array_equal(sigma, orc.device_sigma(n, case.seed)), "node map after a history"
        if "working" in ref:
            _, ru, rv, rw = ref["working"]
            assert np.array_equal(u, ru) and np.array_equal(v, rv) and np.array_equal(w, rw), "working graph"
        assert st["lv_decide_bytes"] > 0
        if case.d:
            assert (st["lv_heavy_bytes"] > 0) == (case.d > 512)
        bad = [(r, int((lab[r] != ref["labels"][r]).sum())) for r in range(case.count)
               if not np.array_equal(lab[r], ref["labels"][r])]
        assert not bad, "replicas (local index, differing vertices) %s" % bad
        assert np.array_equal(ren, ref["renumbered"])


# ------------------------------------------------------------------ target 6: Infomap batches
class InfomapTarget:
    """An Infomap batch == orc.engine_infomap (tests/test_gpu_infomap_twin.py's acceptance rule)."""

    def __init__(self, name, case):
        self.id, self.case, self.seed = name, case, case.seed
        self.replicas = case.count
        self.graph = case.edges

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return infomap_twin(self.case)

    def run(self, eng, tw):
        from tests.test_gpu_infomap_twin import run_infomap
        case = self.case
        apply_options(eng, case.seed, buckets=case.buckets, infomap_trials=case.trials)
        lab, ren, st, (n, u, v, w), sigma = run_infomap(eng, case)
        assert np.array_equal(sigma, orc.device_sigma(n, case.seed)), "node map after a history"
        assert st["lv_decide_bytes"] > 0
        if case.d:
            assert (st["lv_heavy_bytes"] > 0) == (case.d > 512)
        bad = [(r, int((lab[r] != tw.labels[r]).sum())) for r in range(case.count) if not tw.accepts(r, lab[r])]
        assert not bad, "replicas (local index, vertices differing from the chosen trial) %s" % bad
        assert np.array_equal(ren, orc.renumber(tw.labels))
        if tw.equivalent.sum() == case.count:
            assert np.array_equal(lab, tw.labels)


# ------------------------------------------------------------------ target 7: the step API, one iteration
STEP_SEED = 5


class StepTarget:
    """set_labels, consensus_partial / _apply, closure_sample / _partial / _apply on LFR-1k with the
    golden case's recorded labelings == orc.consensus / threshold / check and the CPU engine
    model's closure sampler, closure weights, repair and ages."""
    id = "step_api"
    seed = STEP_SEED
    graph = staticmethod(lfr1k_graph)

    def __init__(self):
        self.replicas = self.rows = lfr1k().n_p

    @functools.lru_cache(maxsize=None)
    def reference(self):
        import torch
        from tests.cpu_engine import OracleEngine
        case = lfr1k()
        n, e, lab, n_p = case.N, case.edges_file, case.cd_batches[0], case.n_p
        g = orc.EdgeGraph.from_lines(n, e)
        w = orc.consensus(0, g, lab, n_p)
        keep = orc.threshold(w, case.tau, n_p)
        conv, unc = orc.check(w[keep], n_p, case.delta)
        sigma = orc.device_sigma(n, STEP_SEED)
        cpu = OracleEngine(seed=STEP_SEED, sigma=sigma)
        cpu.load_graph(n, e[:, 0], e[:, 1])
        cpu.lab = np.empty_like(lab)
        cpu.lab[:, sigma] = lab                      # the model keeps labels by internal id
        cpu.r0 = 0
        part = torch.zeros(cpu.m + 1, dtype=torch.int32)
        cpu.consensus_partial(0, part)
        _, kept_m, unc_m = cpu.consensus_apply(0, n_p, case.tau, case.delta, part)
        assert (kept_m, unc_m) == (int(keep.sum()), unc)
        nc = cpu.closure_sample(g.m, 0)
        cnt = torch.zeros(max(nc, 1), dtype=torch.int32)
        cpu.closure_partial(cnt)
        conv2, m1 = cpu.closure_apply(0, n_p, case.delta, cnt, 0)
        return {"kept": (g.u[keep], g.v[keep], w[keep], g.age[keep]), "conv": bool(conv), "unc": int(unc),
                "candidates": int(nc), "conv2": bool(conv2), "m1": int(m1), "graph": cpu.get_graph(), "attempts": g.m}

    def run(self, eng, ref, reload=True):
        """reload=False: on the graph the engine already holds (loaded with this target's seed and
        options), as a caller that installs one set of labelings after another does."""
        case = lfr1k()
        if reload:
            apply_options(eng, STEP_SEED)
            load(eng, self.graph(), STEP_SEED)
        eng.set_labels(case.cd_batches[0])
        part = dev_i32(eng.m)
        eng.consensus_partial(0, part)
        conv, kept, unc = eng.consensus_apply(0, case.n_p, case.tau, case.delta, part)
        assert (conv, kept, unc) == (ref["conv"], len(ref["kept"][0]), ref["unc"])
        same_graph(eng.get_nextgraph(), ref["kept"], "kept graph")
        nc = eng.closure_sample(ref["attempts"], 0)
        assert nc == ref["candidates"]
        cnt = dev_i32(nc)
        eng.closure_partial(cnt)
        conv2, m1 = eng.closure_apply(0, case.n_p, case.delta, cnt, 0)
        assert (conv2, m1) == (ref["conv2"], ref["m1"])
        same_graph(eng.get_graph(), ref["graph"], "merged graph")


# ------------------------------------------------------------------ target 8: analysis
ANALYSIS_SEED = 7               # a node map that is not the identity
ANALYSIS_COMMUNITIES = (2, 2, 3, 3, 4, 6, 40)     # per labeling: supports spread over 0..7
ANALYSIS_CUT = 5                # a level of several hundred communities, not the consensus_partition(0.5) one


class AnalysisTarget:
    """score_partitions, consensus_partition, consensus_levels + one consensus_cut, coassociation of
    200 nodes (+ its histogram) and cluster_consensus of 7 fixed random labelings on LFR-1k ==
    the *_ref.py modules."""
    id = "analysis"
    seed = ANALYSIS_SEED
    graph = staticmethod(lfr1k_graph)
    replicas = rows = len(ANALYSIS_COMMUNITIES)

    @functools.lru_cache(maxsize=None)
    def reference(self):
        n, e = self.graph()
        rng = np.random.default_rng(2024)
        labs = np.stack([rng.integers(0, k, n) for k in ANALYSIS_COMMUNITIES]).astype(np.int32)
        u, v = cref.canonical_edges(e[:, 0], e[:, 1])
        nt = len(labs)
        sup = cref.support(labs, u, v)
        birth, up = lref.tree(n, u, v, sup, nt)
        rec = lref.level_records(n, u, v, sup, nt, birth=birth, up=up)
        nodes = rng.choice(n, 200, replace=False)
        part = rng.integers(0, 40, n)
        return {"labs": labs, "parts": [score_ref.part(l, e[:, 0], e[:, 1]) for l in labs],
                "consensus": cref.partition(n, u, v, 0.5, labels=labs),
                "birth": birth, "up": up, "records": rec, "best": lref.best_level(rec),
                "cut": lref.cut(birth, up, ANALYSIS_CUT),
                "nodes": nodes, "matrix": car.matrix(labs, nodes), "hist": car.hist(labs, nodes),
                "partition": part, "sums": ccr.sums(labs, part)}

    def run(self, eng, ref, reload=True):
        # reload=False: as StepTarget.run.  The comparisons of tests/test_gpu_score.py, test_gpu_consensus.py, test_gpu_consensus_levels.py,
        # test_gpu_coassoc.py and test_gpu_cluster_consensus.py, on references computed once
        from tests.test_gpu_consensus import same
        from tests.test_gpu_consensus_levels import same_record
        from tests.test_gpu_score import PART_INTS
        n, _ = self.graph()
        labs, nt = ref["labs"], len(ref["labs"])
        if reload:
            apply_options(eng, ANALYSIS_SEED)
            load(eng, self.graph(), ANALYSIS_SEED)
        eng.set_labels(labs)
        got = eng.score_partitions("input")
        for r, exp in enumerate(ref["parts"]):
            for f in PART_INTS:
                assert int(got[f][r]) == exp[f], (r, f, int(got[f][r]), exp[f])
            assert abs(got["entropy"][r] - exp["entropy"]) <= score_ref.float_bound(n), r
            assert abs(got["modularity"][r] - exp["modularity"]) <= 1e-15, (r, got["modularity"][r], exp["modularity"])
        same(eng.consensus_partition(0.5), ref["consensus"], "consensus_partition")
        lev = eng.consensus_levels("input")
        assert lev["n_total"] == nt and len(lev["levels"]) == nt + 1
        assert np.array_equal(lev["birth"], ref["birth"]) and np.array_equal(lev["up"], ref["up"])
        for s in range(nt + 1):
            same_record(lev["levels"][s], ref["records"][s], s)
        assert lev["best_level"] == ref["best"]
        assert lev["best_theta"] == lref.theta_of(ref["best"], nt)
        cut, k = eng.consensus_cut(ANALYSIS_CUT)
        assert cut.dtype == np.int32 and np.array_equal(cut, ref["cut"])
        assert k == ref["records"][ANALYSIS_CUT]["k"] == int(ref["cut"].max()) + 1
        mat = eng.coassociation(ref["nodes"]).cpu().numpy()
        assert mat.dtype == np.int32 and np.array_equal(mat, ref["matrix"])
        hist = eng.coassoc_hist(ref["nodes"])
        assert hist.dtype == np.int64 and np.array_equal(hist, ref["hist"])
        ids, size, pairs, item = ref["sums"]
        cc = eng.cluster_consensus(ref["partition"])
        assert cc["ids"].dtype == np.int32 and np.array_equal(cc["ids"], ids)
        assert cc["size"].dtype == np.int64 and np.array_equal(cc["size"], size)
        assert cc["cluster_pairs"].dtype == np.int64 and np.array_equal(cc["cluster_pairs"], pairs)
        assert cc["item_pairs"].dtype == np.int64 and np.array_equal(cc["item_pairs"], item)
        assert cc["k"] == len(ids) and cc["max_size"] == size.max() and cc["singletons"] == (size == 1).sum()
        assert cc["pairs_total"] == pairs.sum() == item.sum() and cc["n_r"] == nt
        own = size[np.searchsorted(ids, ref["partition"])]
        assert ccr.same_floats(cc["cluster_consensus"], ccr.cluster_consensus(pairs, size, nt))
        assert ccr.same_floats(cc["item_consensus"], ccr.item_consensus(item, own, nt))


TARGETS = [
    RunTarget("louvain_run", 0, 10, 0.2),
    RunTarget("lpm_run", 1, 6, 0.8),
    RunTarget("louvain_nc_run", 2, 10, 0.2),
    CdTarget("cd_classic", 0),
    CdTarget("cd_replica_lane", 1),
    LeidenTarget("leiden_hub700", LeidenCase(700, 3, seed=7)),
    LeidenTarget("leiden_weighted", LeidenCase("lfr1k_weighted", 4, seed=31, iteration=3)),
    InfomapTarget("infomap_hub700", InfomapCase(700, 3, seed=7)),
    InfomapTarget("infomap_lfr1k", InfomapCase("lfr1k", 6, seed=13)),
    StepTarget(),
    AnalysisTarget(),
]
TARGET = {t.id: t for t in TARGETS}
WHOLE_RUNS = ("louvain_run", "lpm_run", "louvain_nc_run")
LEVEL_BATCHES = ("leiden_hub700", "leiden_weighted", "infomap_hub700", "infomap_lfr1k")
CUTTABLE = ("cd_classic", "cd_replica_lane", "analysis")          # targets 4 and 8: the only pairs a time cut may drop


# ------------------------------------------------------------------ histories
def step_iteration(eng, algo, n_p, tau, delta, it, closure=True):
    """One iteration of the consensus loop on the labelings the engine holds."""
    part = dev_i32(eng.m)
    eng.consensus_partial(algo, part)
    eng.consensus_apply(algo, n_p, tau, delta, part)
    if not closure:
        return
    nc = eng.closure_sample(eng.graph_info()[2], it)
    cnt = dev_i32(nc)
    if nc and algo != 1:
        eng.closure_partial(cnt)
    eng.closure_apply(algo, n_p, delta, cnt if algo != 1 else None, it)


def analysis_calls(eng, n_r):
    """One analysis call of each kind on the labelings the engine holds, the hierarchy last."""
    n = eng.n
    eng.score_partitions("input")
    eng.score_partitions("working")
    eng.score_pairs([(0, n_r - 1)])
    eng.consensus_partition(0.5)
    nodes = np.arange(0, n, max(n // 300, 1))
    eng.coassociation(nodes)
    eng.coassoc_hist(nodes)
    eng.cluster_consensus(eng.get_labels(n_r)[0])
    eng.consensus_levels("input")


BIGGER_LFR = (4000, 0.3, 5)          # synth.lfr(n, mu, seed)
BIGGER_NP = 64
BIGGER_CD = 70                       # a CD batch past every target's replica count (64)
BIGGER_HUB = 1500                    # a hub graph of the Leiden twin tests with a row past every target's (700)


@functools.lru_cache(maxsize=None)
def bigger_lfr():
    from fastconsensus_amd import synth
    n, mu, seed = BIGGER_LFR
    u, v, _ = synth.lfr(n, mu, seed=seed)
    return n, np.stack([u, v], 1)


@functools.lru_cache(maxsize=None)
def bigger_hub():
    return LeidenCase(BIGGER_HUB, 3, seed=7).edges()


def bigger_graphs():
    return [bigger_lfr(), bigger_hub()]


def fresh(fc, eng, target):
    """Nothing: the control.  A failure here is a wrong target, not wrong reuse."""


def bigger_first(fc, eng, target):
    """A Louvain run of 64 replicas on LFR-4000, CD batches of 70 (the default engine and the
    replica-lane engine), one analysis call of each kind, the hierarchy; then a Leiden and an Infomap batch on the d = 1500 hub graph, whose hub row is
    longer than any target's (LFR's degrees stop at 50, the d = 700 targets have a row of 700).
    N, m, 2m, replica count, ldT, closure candidates, community count and longest row are all above
    every target's: each buffer a target uses holds foreign data inside and past its new extent."""
    n, e = bigger_lfr()
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.run(0, BIGGER_NP, 0.2, 0.02)
    eng.cd(0, 0, BIGGER_CD, BIGGER_CD, 1)
    eng.set_option("cd_engine", 1)            # the replica-lane engine's own buffers too (a bank past 64 lanes)
    eng.cd(1, 0, BIGGER_CD, BIGGER_CD, 1)
    eng.set_option("cd_engine", DEFAULTS["cd_engine"])
    analysis_calls(eng, BIGGER_CD)
    n, e = bigger_hub()
    eng.set_option("infomap_trials", 2)
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.cd(3, 0, 4, 4, 0)
    eng.cd(4, 0, 2, 2, 0)


def smaller_first(fc, eng, target):
    """Karate, an lpm run of 3 replicas: every buffer must grow (DevBuf::ensure reallocates) when
    the target runs."""
    n, e = karate_graph()
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.run(1, 3, 0.8, 0.02)


def more_replicas_same_graph(fc, eng, target):
    """On the target's graph, with the default CD engine and then the replica-lane engine (left
    selected): cd of 64 replicas, of 3, a shard [5, 8) of 10 at iteration 4; then set_labels of 20
    rows, a consensus update, reset_graph: ldT, rbase, n_p_total, the replica-lane masks and
    rep_state shrink and move."""
    n, e = target.graph()
    eng.load_graph(n, e[:, 0], e[:, 1])
    for engine in (DEFAULTS["cd_engine"], 1):
        eng.set_option("cd_engine", engine)
        for algo in (0, 1):
            eng.cd(algo, 0, 64, 64, 0)
            eng.cd(algo, 0, 3, 3, 0)
            eng.cd(algo, 5, 3, 10, 4)
    eng.set_labels(np.random.default_rng(20).integers(0, 5, (20, n)))
    step_iteration(eng, 0, 20, 0.2, 0.02, 0, closure=False)
    eng.reset_graph()


def other_algorithms(fc, eng, target):
    """On the target's graph: a Louvain run to convergence (a weighted working graph with closure
    and repair edges), reset_graph, a Leiden batch, an Infomap batch, an lpm run: clo_algo, lv[],
    mvt / mvo, tailmark, the weighted and unit-weight kernel choice, Leiden-style marks."""
    n, e = target.graph()
    eng.load_graph(n, e[:, 0], e[:, 1])
    _, st = eng.run(0, 8, 0.2, 0.02)
    assert st["exit_check"] in (1, 2) and not st["hit_iter_cap"]
    eng.cd(0, 0, 8, 8, 3)                     # one more batch on the weighted graph the run left
    eng.reset_graph()
    eng.cd(3, 0, 3, 3, 0)
    eng.set_option("infomap_trials", 2)
    eng.cd(4, 0, 2, 2, 0)
    eng.run(1, 6, 0.8, 0.02)


OTHER_OPTIONS = [("cd_engine", 0), ("cd_engine", 1), ("cd_engine", 2), ("chunk", 0), ("prune", 0), ("tail_visits", 0),
                 ("coarsen", 0), ("prune_mark", 2), ("store", 0), ("relabel", 0), ("relabel", 2)]


def other_options(fc, eng, target):
    """buckets = 5 and closure_rounds = 1, then each of OTHER_OPTIONS in turn (they accumulate), a
    load and a 3-replica Louvain batch after each, one consensus iteration with the one-block
    closure at the end; then every option back at its default.  Covers the relabel = 2 double
    ingest, order_pass and the storage order maps."""
    n, e = lfr1k_graph()
    eng.set_params(buckets=5)
    eng.set_option("closure_rounds", 1)
    for name, value in OTHER_OPTIONS:
        eng.set_option(name, value)
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(0, 0, 3, 3, 0)
    step_iteration(eng, 0, 3, 0.2, 0.02, 0)
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)


def interrupted(fc, eng, target):
    """A load that fails its endpoint check, a valid load, a consensus update whose closure never
    comes, a sharded closure sequence begun and abandoned after block 0's draw, a run cut short by
    max_iters = 1."""
    import torch
    n, e = lfr1k_graph()
    bad = e.copy()
    bad[len(bad) // 2, 1] = n
    try:
        eng.load_graph(n, bad[:, 0], bad[:, 1])
    except fc.FastConsensusError:
        pass
    else:
        raise AssertionError("an endpoint equal to n was accepted")
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.cd(0, 0, 5, 5, 0)
    step_iteration(eng, 0, 5, 0.2, 0.02, 0, closure=False)
    attempts = eng.graph_info()[2]
    blocks = eng.closure_begin(attempts, 0)
    buf = torch.empty(2 * (attempts // blocks + 1), dtype=torch.int64, device="cuda")
    eng.closure_block_sample(0, 0, attempts // blocks, buf)
    eng.set_params(max_iters=1)
    _, st = eng.run(0, 5, 0.2, 0.02)
    assert st["hit_iter_cap"] == 1
    eng.set_params(max_iters=DEFAULTS["max_iters"])


RESEEDED_CREATE_SEED = 424242        # differs from every target's seed


def reseeded(fc, eng, target):
    """The engine was created with RESEEDED_CREATE_SEED and is used with it; the target then does
    bench.py's step: set_option("seed", s), load_graph, run."""
    assert eng.seed == RESEEDED_CREATE_SEED
    n, e = lfr1k_graph()
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.run(0, 8, 0.2, 0.02)


def timed(fc, eng, target):
    """set_timing(True), a run, collect_timing(); timing stays on while the target runs (the test
    collects again afterwards): the event pool and the chained decide timers change no result."""
    n, e = lfr1k_graph()
    eng.set_timing(True)
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.run(0, 8, 0.2, 0.02)
    eng.collect_timing()


def labels_replaced(fc, eng, target):
    """For the targets that begin with set_labels: the target's graph loaded with the target's seed
    (the engine's) and default options, other labelings with the target's row count installed and
    used (consensus_partial, a score: the transposed copy exists), a consensus update without its
    closure.  The target then runs on the loaded graph, without a load of its own: only
    set_labels stands between the old labelings' derived state and the new results."""
    assert eng.seed == target.seed
    n, e = target.graph()
    eng.load_graph(n, e[:, 0], e[:, 1])
    eng.set_labels(np.random.default_rng(31).integers(0, 4, (target.rows, n)))
    step_iteration(eng, 0, target.rows, 0.2, 0.02, 0, closure=False)
    eng.score_partitions("input")
    eng.consensus_levels("input")


NO_RELOAD = {"labels_replaced": ("step_api", "analysis")}     # history -> its only targets, run with reload=False
HISTORIES = [fresh, bigger_first, smaller_first, more_replicas_same_graph, other_algorithms, other_options,
             interrupted, reseeded, timed, labels_replaced]
HISTORY = {h.__name__: h for h in HISTORIES}
# what each history is aimed at (DESIGN.md "Used engines" prints this table)
AIMS = {
    "fresh": "control: a broken target, not broken reuse",
    "bigger_first": "stale data inside and past every new extent: N, m, 2m, replicas, ldT, candidates, communities, rows",
    "smaller_first": "DevBuf::ensure reallocating every buffer; pointers taken before a later ensure",
    "more_replicas_same_graph": "ldT, rbase, n_p_total, labT_valid, replica-lane masks, rep_state shrinking and moving",
    "other_algorithms": "clo_algo, lv[], mvt / mvo stamps, tailmark, weighted vs unit-weight kernels, Leiden-style marks",
    "other_options": "options that apply at the next load (relabel, store), the relabel = 2 double ingest, order_pass",
    "interrupted": "N = 0 after a failed load, kept_m / n_cand of an unfinished iteration, clo_next, max_iters",
    "reseeded": "seed taken at the next load: set_option(seed) + load_graph == Engine(seed)",
    "timed": "the event pool and chained decide timers while results are computed",
    "labels_replaced": "labT_valid / ldT, lv_valid and kept_m across set_labels on a loaded graph (no load in between)",
}
assert set(AIMS) == set(HISTORY)

# The pairs that run: every target after every history, minus DROPPED.  A pair may be dropped only to
# keep the file's time within a third of the suite's, only from CUTTABLE targets, and never after
# bigger_first, other_algorithms or reseeded (tests/test_reuse_cases.py asserts these rules).
DROPPED = set()
MATRIX = [(h.__name__, t.id) for t in TARGETS for h in HISTORIES
          if (h.__name__, t.id) not in DROPPED and t.id in NO_RELOAD.get(h.__name__, (t.id,))]


def pair_id(pair):
    return "%s-after-%s" % (pair[1], pair[0])


def create_seed(history, target_seed):
    return RESEEDED_CREATE_SEED if history == "reseeded" else target_seed


def graph_stats(graph):
    """(N, m, maximum degree) of (n, edges) from numpy alone: distinct undirected edges, no loops."""
    n, e = graph
    e = np.asarray(e, np.int64)
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    deg = np.bincount(np.concatenate([key // n, key % n]), minlength=n)
    return n, len(key), int(deg.max())

