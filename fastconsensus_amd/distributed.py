"""Replica-sharded fast_consensus over several GPUs (one process per GPU, RCCL over xGMI).

The n_p community-detection runs of every iteration are independent given the graph, so
rank g owns the CONTIGUOUS replica range [g*n_p/W, (g+1)*n_p/W) (the Louvain consensus
rule depends on replica order, fast_consensus.py:154-159).  Every rank keeps an identical
copy of the graph; the only data-path exchanges are
  * per-edge partials: Louvain k_last (all-reduce MAX) / LPM co-membership counts (SUM);
  * per-candidate closure co-membership counts (SUM, louvain only);
both travel as uint8 when n_p <= 255 (k_last + 1 and counts are in [0, n_p]): a quarter
of the int32 bytes on every xGMI ring hop;
after which threshold, check, repair and the graph rebuild run replicated and
deterministically -- no graph broadcast.  The triadic closure runs replicated too (same
counter-based RNG on every rank) unless shard_closure=True: then each closure block's
attempts are divided over the ranks and their (pair, first attempt) lists all-gathered
(_closure_sharded, same candidates).  Measured on LFR-1M it does not pay: half the
attempts yield a candidate, and the per-candidate work (dedup, append, growing the closure
graph) stays on every rank -- 4.7 ms per rank at W = 8 against 6.0 ms replicated, before
the ~116 MB all-gathered per iteration (profiles/r03_closure_shard_time.json).  The final
partitions are all-gathered to rank 0.  The loop mirrors fc_run (capi.cpp) step for step,
so W ranks produce bit-identical results to one GPU.

The driver only needs an "engine" with the step API of fastconsensus_amd.Engine; buffers
are torch tensors on the engine's device (RCCL) or on the CPU (gloo, used by the tests).
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from .core import FINAL_PASS_ITER, check_consensus_flags, refine_consensus

LOUVAIN, LPM, LOUVAIN_NC, LEIDEN, INFOMAP = 0, 1, 2, 3, 4


def on_device(t):
    return t.device.type == "cuda"


def shard(n_p, rank, world):
    return n_p * rank // world, n_p * (rank + 1) // world


def _world():
    """The number of ranks; 1 without a process group."""
    return dist.get_world_size() if dist.is_initialized() else 1


def _devices(engine, device):
    """(the engine's device string, the device the collectives run on: the same, or "cpu" for gloo)"""
    cuda = "cuda:%d" % engine.device
    return cuda, cuda if str(device).startswith("cuda") else "cpu"


def _sum_ranks(*tensors):
    """One SUM all-reduce per tensor, in place and in argument order, when there are ranks to add;
    returns the tensors."""
    if _world() > 1:
        for t in tensors:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return tensors


def _gather_rows(block, sums, comm, axis=0):
    """All ranks' rows in rank order, and the ranks' counters added.  block: this rank's rows along
    `axis` (every other extent the same on every rank); sums: its row count, then its further
    counters.  Two all-gathers: the int64 counters, then the blocks padded along `axis` to the
    largest (one row at least) on the device `comm`.  Returns (rows on `comm`, summed counters);
    with one rank no collective is issued and (block, sums) come back as they are."""
    world = _world()
    if world <= 1:
        return block, sums
    cnt = torch.tensor(sums, dtype=torch.int64, device=comm)
    cnts = [torch.empty_like(cnt) for _ in range(world)]
    dist.all_gather(cnts, cnt)
    cnts = torch.stack(cnts).cpu()
    shape = list(block.shape)
    shape[axis] = max(int(cnts[:, 0].max()), 1)
    buf = torch.zeros(shape, dtype=block.dtype, device=comm)
    buf.narrow(axis, 0, block.shape[axis]).copy_(block)
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf)
    rows = torch.cat([bufs[g].narrow(axis, 0, int(cnts[g, 0])) for g in range(world)], dim=axis)
    return rows, cnts.sum(0).tolist()


def _all_reduce_small(t, op, n_p, world, shift):
    """In-place all-reduce of int32 values in [-shift, n_p - shift] (MAX, or SUM of per-rank
    counts whose total is <= n_p); as uint8 when n_p <= 255.  Exact: MAX commutes with the
    +shift, and every partial SUM is a count of replicas, <= n_p."""
    if world <= 1:
        return t
    if n_p > 255:
        dist.all_reduce(t, op=op)
        return t
    b = (t + shift).to(torch.uint8)
    dist.all_reduce(b, op=op)
    t.copy_(b)
    if shift:
        t.sub_(shift)
    return t


def _closure_sharded(engine, attempts, iteration, world, rank, device):
    """fast_consensus.py:175-184 / :292-300 (the growing nextgraph) over W ranks: block b's
    attempts [t0, t1) are split into W contiguous sub-ranges, each rank draws its own, and
    the ranks' pair lists (int64 key, first attempt) are all-gathered -- a count exchange,
    then the lists padded to the largest -- and added on every rank before block b + 1 draws
    from the grown graph.  Same candidates as engine.closure_sample on one rank."""
    blocks = engine.closure_begin(attempts, iteration)
    for b in range(blocks):
        t0, t1 = attempts * b // blocks, attempts * (b + 1) // blocks
        lo, hi = t0 + (t1 - t0) * rank // world, t0 + (t1 - t0) * (rank + 1) // world
        cap_pairs = (t1 - t0 + world - 1) // world + 1          # >= every rank's sub-range
        mine = torch.empty(2 * cap_pairs, dtype=torch.int64, device=device)
        k = engine.closure_block_sample(b, lo, hi, mine)
        cnt = torch.tensor([k], dtype=torch.int64, device=device)
        cnts = [torch.empty_like(cnt) for _ in range(world)]
        dist.all_gather(cnts, cnt)
        cnts = [int(x) for x in torch.cat(cnts).tolist()]
        top = max(cnts)
        if top == 0:
            engine.closure_block_add(b, None, 0)
            continue
        recv = [torch.empty(2 * top, dtype=torch.int64, device=device) for _ in range(world)]
        dist.all_gather(recv, mine[:2 * top])
        pairs = torch.cat([recv[g][:2 * cnts[g]] for g in range(world)])
        engine.closure_block_add(b, pairs, sum(cnts))
    return engine.closure_finish()


class SharedOutput:
    """The run's [n_p][n] int32 host labelings in POSIX shared memory, mapped by every rank of
    the node (collective: all ranks construct it).  Passed as run_sharded(out=..., out_shared=
    True), each rank downloads ITS replica rows over its own PCIe link straight into the
    array -- no device all-gather of n_p*n labels and no 256 MB download through rank 0.
    `array` is None on every rank (callers fall back to the gather) when /dev/shm cannot hold
    it -- tmpfs does not reserve pages, and a write past its limit would be a SIGBUS -- or when
    the ranks are not all on one node (a rank elsewhere could not map it)."""

    def __init__(self, n_p, n):
        from multiprocessing import resource_tracker, shared_memory
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.shm, self.array = None, None
        size = max(4 * int(n_p) * int(n), 4)
        name = None
        one_node = True
        if _world() > 1:
            import socket
            hosts = [None] * dist.get_world_size()
            dist.all_gather_object(hosts, socket.gethostname())
            one_node = len(set(hosts)) == 1
        if self.rank == 0 and one_node:
            try:
                st = os.statvfs("/dev/shm")
                if st.f_bavail * st.f_frsize >= size + size // 8 + (64 << 20):
                    self.shm = shared_memory.SharedMemory(create=True, size=size)
                    name = self.shm.name
            except OSError:
                name = None
        obj = [name]
        if dist.is_initialized():
            dist.broadcast_object_list(obj, src=0)
        name = obj[0]
        if name is None:
            return
        if self.rank != 0:
            self.shm = shared_memory.SharedMemory(name=name)
            resource_tracker.unregister(self.shm._name, "shared_memory")   # rank 0 owns (unlinks) it
        self.array = np.ndarray((n_p, n), np.int32, buffer=self.shm.buf)

    def close(self):
        """Collective.  Drop every view of `array` first."""
        if dist.is_initialized():
            dist.barrier()
        self.array = None
        if self.shm is not None:
            self.shm.close()
            if self.rank == 0:
                self.shm.unlink()
            self.shm = None


def _consensus(engine, theta, n_p, world, mine, device):
    """The consensus partition of the run's n_p final partitions, replicated: every rank counts
    the support of the input graph's edges over ITS replicas, one SUM all-reduce adds them, and
    every rank takes the components of the agreeing edges (identical on every rank).  theta
    "best": the hierarchy over the reduced support and the partition at its best level
    (core.best_consensus), again the same on every rank."""
    _, _, m0 = engine.graph_info()
    sup = torch.zeros(max(m0, 1), dtype=torch.int32, device=device)
    if mine > 0:
        engine.consensus_support("input", sup)
    _all_reduce_small(sup, dist.ReduceOp.SUM, n_p, world, 0)
    if isinstance(theta, str):
        from .core import best_consensus
        return best_consensus(engine, sup, n_p)
    return engine.consensus_partition(theta, "input", dev_support=sup, n_total=n_p)


def coassociation_sharded(engine, a, b=None, device="cuda"):
    """The consensus matrix of two node lists (Engine.coassociation) over every rank's replicas:
    each rank counts over ITS local labelings, one int32 SUM all-reduce adds the counts, and every
    rank returns the same int32 [na, nb] tensor on `device`.  A rank without replicas
    contributes zeros."""
    na = len(np.asarray(a).reshape(-1))
    nb = na if b is None else len(np.asarray(b).reshape(-1))
    if engine.replica_info()[0] > 0:
        mat = engine.coassociation(a, b)
        if not str(device).startswith("cuda"):
            mat = mat.cpu()
    else:
        mat = torch.zeros((na, nb), dtype=torch.int32, device=device)
    return _sum_ranks(mat.contiguous())[0]


def coassoc_hist_sharded(engine, nodes, n_total, device="cuda"):
    """int64 [n_total + 1] histogram of the counts over the position pairs i < j of `nodes`,
    over all n_total replicas of a sharded run.  A histogram of sums is not a sum of histograms
    -- a pair's count is spread over the ranks, and which bin it falls in is known only after the
    counts are added -- so Engine.coassoc_hist (fc_coassoc_hist) does not shard: this takes the
    reduced matrix of coassociation_sharded and bins its strict upper triangle with
    torch.bincount.  The matrix limits it to lists whose k * k counts fit in memory."""
    mat = coassociation_sharded(engine, nodes, None, device)
    k = mat.shape[0]
    iu = torch.triu_indices(k, k, offset=1, device=mat.device)
    return torch.bincount(mat[iu[0], iu[1]].to(torch.int64), minlength=int(n_total) + 1).cpu().numpy()


def cluster_consensus_sharded(engine, labels, n_total, device="cuda"):
    """Engine.cluster_consensus of the partition `labels` over all n_total replicas of a sharded
    run: each rank sums over ITS local labelings into int64 buffers of one shape (n entries each),
    one SUM all-reduce per buffer adds them, and every rank normalises the same integers with
    core.cluster_consensus / core.item_consensus (n_total in place of the local count).  Returns
    ids, size, cluster_pairs, item_pairs, cluster_consensus, item_consensus and slow_members (the
    ranks' sum).  A rank without replicas contributes zeros; `labels` is the same on every rank."""
    from .core import cluster_consensus, item_consensus
    n = engine.n
    labels = np.asarray(labels)
    cuda, comm = _devices(engine, device)
    pairs = torch.zeros(max(n, 1), dtype=torch.int64, device=cuda)
    item = torch.zeros(max(n, 1), dtype=torch.int64, device=cuda)
    slow = 0
    if engine.replica_info()[0] > 0:
        slow = engine.cluster_consensus(labels, dev_cluster=pairs, dev_item=item)["slow_members"]
    ids, size = np.unique(labels, return_counts=True)
    pairs, item, slow = _sum_ranks(pairs.to(comm), item.to(comm), torch.tensor([slow], dtype=torch.int64, device=comm))
    k = len(ids)
    cp, ip = pairs[:k].cpu().numpy(), item[:n].cpu().numpy()
    size = size.astype(np.int64)
    return {"ids": ids.astype(np.int32), "size": size, "cluster_pairs": cp, "item_pairs": ip,
            "cluster_consensus": cluster_consensus(cp, size, n_total),
            "item_consensus": item_consensus(ip, size[np.searchsorted(ids, labels)], n_total),
            "slow_members": int(slow.item()), "n_total": int(n_total)}


def vote_sharded(engine, labels, n_total, device="cuda"):
    """Engine.vote of the partition `labels` over all n_total replicas of a sharded run.  The ranks'
    `top` cannot be reduced (a plurality is not a sum of pluralities), so each rank maps ITS local
    labelings onto `labels` (Engine.vote_map), the int32 [n_r, n] results are all-gathered in rank
    order -- the global replica order of run_sharded's contiguous shards; a count exchange, then the
    blocks padded to the largest -- and every rank counts the votes over the same [n_total, n] buffer
    (fc_vote_count).  Returns the dict of Engine.vote, the same on every rank, with
    mapped_communities and slow_members summed over the ranks.  A rank without replicas
    contributes no rows; `labels` is the same on every rank."""
    n = engine.n
    cuda, comm = _devices(engine, device)
    n_r = engine.replica_info()[0]
    mine = torch.empty((0, n), dtype=torch.int32, device=cuda)
    sums = [n_r, 0, 0]
    if n_r > 0:
        m = engine.vote_map(labels)
        mine, sums = m["mapped"], [n_r, m["mapped_communities"], m["slow_members"]]
    mine, sums = _gather_rows(mine, sums, comm)
    mine = mine.to(cuda).contiguous()
    if mine.shape[0] != int(n_total):
        raise ValueError("the ranks hold %d labelings, n_total = %d" % (mine.shape[0], n_total))
    res = engine.vote(labels, dev_mapped=mine, n_total=int(n_total))
    res["mapped_communities"], res["slow_members"] = int(sums[1]), int(sums[2])
    return res


def _pair_sums_sharded(engine, method, key, labels, a, b, device):
    """The body of item_affinity_sharded and cluster_coassoc_sharded.  method: the engine call,
    (labels, a, b, dev_out=) -> dict with slow_lookups; key: the name of the sums in the result."""
    cuda, comm = _devices(engine, device)
    npairs = len(np.asarray(a).reshape(-1))
    buf = torch.zeros(npairs + 1, dtype=torch.int64, device=cuda)   # the sums, then slow_lookups
    if engine.replica_info()[0] > 0:
        buf[npairs] = method(labels, a, b, dev_out=buf)["slow_lookups"]
    out = _sum_ranks(buf.to(comm))[0].cpu().numpy()
    return {key: out[:npairs].copy(), "slow_lookups": int(out[npairs])}


def item_affinity_sharded(engine, labels, nodes, clusters, device="cuda"):
    """Engine.item_affinity over every rank's replicas: each rank sums over ITS local labelings, one
    int64 SUM all-reduce adds the sums, and every rank returns the same dict: aff int64[npairs] and
    slow_lookups (the ranks' sum).  A rank without replicas contributes zeros; `labels` and the
    query lists are the same on every rank."""
    return _pair_sums_sharded(engine, engine.item_affinity, "aff", labels, nodes, clusters, device)


def cluster_coassoc_sharded(engine, labels, a, b, device="cuda"):
    """Engine.cluster_coassoc over every rank's replicas, as item_affinity_sharded: x int64[npairs]
    and slow_lookups (the ranks' sum)."""
    return _pair_sums_sharded(engine, engine.cluster_coassoc, "x", labels, a, b, device)


def _sum_sq_sharded(engine, device):
    """T of core.median_refine / merge_refine: the replicas' sum_sq (score_partitions) added over
    the ranks, one SUM all-reduce."""
    t = torch.zeros(1, dtype=torch.int64, device=_devices(engine, device)[1])
    if engine.replica_info()[0] > 0:
        t[0] = int(np.asarray(engine.score_partitions()["sum_sq"], np.int64).sum())
    return int(_sum_ranks(t)[0].item())


def sharded_calls(engine, n_total, device="cuda"):
    """The `calls` of core.refine_consensus over all n_total replicas of a sharded run: every engine
    call that reads the labelings through its *_sharded counterpart, and sum_sq as the callable that
    adds it over the ranks.  What needs no labelings (community_graph, community_quality) stays the
    engine's own."""
    return {"vote": lambda lab: vote_sharded(engine, lab, n_total, device),
            "cluster_consensus": lambda lab: cluster_consensus_sharded(engine, lab, n_total, device),
            "item_affinity": lambda lab, nd, cl: item_affinity_sharded(engine, lab, nd, cl, device),
            "cluster_coassoc": lambda lab, a, b: cluster_coassoc_sharded(engine, lab, a, b, device),
            "cluster_match": lambda lab: cluster_match_sharded(engine, lab, n_total, device),
            "sum_sq": lambda: _sum_sq_sharded(engine, device)}


def median_refine_sharded(engine, labels, n_total, device="cuda", max_rounds=64, candidates=None):
    """core.median_refine over all n_total replicas of a sharded run: the vote, the cluster consensus
    and the affinities through vote_sharded, cluster_consensus_sharded and item_affinity_sharded, the
    replicas' sum_sq added over the ranks.  The selection (core.median_moves) is deterministic on
    the same integers, so every rank returns the same dict.  `labels` is the same on every rank."""
    from .core import median_refine
    c = sharded_calls(engine, n_total, device)
    return median_refine(engine, labels, max_rounds=max_rounds, candidates=candidates, vote=c["vote"],
                         cluster_consensus=c["cluster_consensus"], item_affinity=c["item_affinity"],
                         sum_sq=c["sum_sq"]())


def merge_refine_sharded(engine, labels, n_total, device="cuda", graph="input", max_rounds=64, candidates=None):
    """core.merge_refine over all n_total replicas of a sharded run: the pair co-association and the
    cluster consensus through cluster_coassoc_sharded and cluster_consensus_sharded, the replicas'
    sum_sq added over the ranks; the community graph needs no labelings and is every rank's own.
    The selection (core.merge_moves) is deterministic on the same integers, so every rank returns
    the same dict.  `labels` is the same on every rank."""
    from .core import merge_refine
    c = sharded_calls(engine, n_total, device)
    return merge_refine(engine, labels, graph=graph, max_rounds=max_rounds, candidates=candidates,
                        cluster_coassoc=c["cluster_coassoc"], cluster_consensus=c["cluster_consensus"],
                        sum_sq=c["sum_sq"]())


def cluster_match_sharded(engine, labels, n_total, device="cuda"):
    """Engine.cluster_match of the partition `labels` against all n_total replicas of a sharded run.
    A row of the two tables depends on its own replica alone, so nothing is reduced: each rank
    computes ITS rows, the int32 [n_r, K] blocks are all-gathered in rank order -- the global
    replica order of run_sharded's contiguous shards; a count exchange, then the blocks padded to
    the largest -- and every rank derives the same summary from the same [n_total, K] integers.
    Returns the dict of Engine.cluster_match, the same on every rank and identical to one rank
    holding every replica, with perfect, inter_total and slow_members summed over the ranks and
    n_r = n_total.  A rank without replicas contributes no rows; `labels` is the same on every rank."""
    from .core import match_summary
    labels = np.asarray(labels)
    cuda, comm = _devices(engine, device)
    ids, size = np.unique(labels, return_counts=True)
    k = len(ids)
    n_r = engine.replica_info()[0]
    both = torch.zeros((2, 0, k), dtype=torch.int32, device=cuda)   # inter, then csize
    sums = [n_r, 0, 0, 0]
    if n_r > 0:
        both = torch.empty((2, n_r, k), dtype=torch.int32, device=cuda)
        cm = engine.cluster_match(labels, dev_inter=both[0], dev_csize=both[1])
        sums = [n_r, cm["perfect"], cm["inter_total"], cm["slow_members"]]
    both, sums = _gather_rows(both, sums, comm, axis=1)
    if both.shape[1] != int(n_total):
        raise ValueError("the ranks hold %d labelings, n_total = %d" % (both.shape[1], n_total))
    inter, csize = both[0].cpu().numpy(), both[1].cpu().numpy()
    size = size.astype(np.int64)
    out = {"ids": ids.astype(np.int32), "size": size, "inter": inter, "csize": csize, "k": k,
           "max_size": int(size.max()), "singletons": int((size == 1).sum()), "perfect": int(sums[1]),
           "inter_total": int(sums[2]), "slow_members": int(sums[3]), "n_r": int(n_total)}
    out.update(match_summary(inter, size, csize))
    return out


def _result(res, consensus):
    labels, st = res
    return (labels, st) if consensus is None else (labels, st, st.pop("consensus"))


def run_sharded(engine, algo, n_p, tau, delta, device="cuda", max_iters=1000, gather=True, out=None,
                shard_closure=False, out_shared=False, consensus=None, vote=False, median=False, quality=False,
                merge=False, match=False):
    """Returns (labels [n_p][N] on rank 0 (None elsewhere), stats dict).  `out`: optional
    C-contiguous int32 host array [n_p][N] that rank 0 downloads into (see Engine.run).
    shard_closure: split the closure's attempts over the ranks (world > 1; same result);
    default False: every rank draws all of them (see the module docstring).
    out_shared: `out` is the same host array on every rank (SharedOutput.array): each rank
    writes its own rows, rank 0 returns it once all have.
    consensus: an agreement threshold in [0, 1]; the return value is then (labels, stats,
    consensus) with the dict of Engine.consensus_partition over all n_p final partitions on the
    input graph, the same on every rank.  consensus="best": the threshold is chosen by the
    consensus hierarchy (Engine.consensus_levels over the reduced support); the dict then also
    holds level, theta, levels, birth and up.
    vote: (needs consensus) the consensus partition refined by plurality vote of all n_p final
    partitions (core.vote_refine over vote_sharded); the dict gains voted, vote_confidence,
    vote_rounds and vote_moved, the same on every rank.
    median: (needs consensus) the consensus partition (`voted` with vote=True) refined by exact
    one-element moves towards the median partition of all n_p final partitions
    (median_refine_sharded); the dict gains median, median_objective, median_rounds, median_moved
    and median_mean_rand, the same on every rank.
    quality: (needs consensus) what the input graph says about the consensus communities
    (Engine.community_quality): the dict gains quality and, for each of voted / median the call
    produced, voted_quality / median_quality.  A property of the graph and the partition alone, so
    every rank computes it locally and no collective is needed.
    merge: (needs consensus) runs last, on median if it was produced, else on voted, else on the
    consensus partition: cluster merges towards the median partition of all n_p final partitions
    (merge_refine_sharded); the dict gains merged, merged_objective, merged_rounds, merged_accepted,
    merged_k and merged_mean_rand, the same on every rank, and with quality also merged_quality.
    match: (needs consensus) the best match, by Jaccard index, of every consensus community in all
    n_p final partitions (cluster_match_sharded); the dict gains match_inter, match_csize,
    match_stability, match_recovered and match_dissolved, the same on every rank."""
    check_consensus_flags(consensus, match=match, merge=merge, quality=quality, median=median, vote=vote)
    world = _world()
    rank = dist.get_rank() if dist.is_initialized() else 0
    if out_shared and world > 1 and out is None:
        # every rank must pass the shared array: a rank without it would take the all-gather
        # path while the others wait in the shared path's barrier
        raise ValueError("run_sharded(out_shared=True) needs the SharedOutput array on every rank")
    r0, r1 = shard(n_p, rank, world)
    louv = algo in (LOUVAIN, LOUVAIN_NC)    # louvain loop: check #1, closure counts, repair
    on_gpu = str(device).startswith("cuda")
    if not on_gpu:
        return _result(_loop(engine, algo, n_p, tau, delta, device, max_iters, gather, world, rank, r0, r1, louv,
                             out, shard_closure, out_shared, consensus, vote, median, quality, merge, match), consensus)
    # engine kernels and torch/RCCL ops on ONE explicit stream: no cross-stream races
    # (torch's default stream is the legacy null stream, which the engine cannot adopt)
    stream = torch.cuda.Stream(device=device)
    stream.wait_stream(torch.cuda.current_stream(device))
    engine.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            return _result(_loop(engine, algo, n_p, tau, delta, device, max_iters, gather, world, rank, r0, r1,
                                 louv, out, shard_closure, out_shared, consensus, vote, median, quality, merge, match),
                           consensus)
    finally:
        stream.synchronize()
        engine.set_stream(None)


def _loop(engine, algo, n_p, tau, delta, device, max_iters, gather, world, rank, r0, r1, louv, out=None,
          shard_closure=False, out_shared=False, consensus=None, vote=False, median=False, quality=False,
          merge=False, match=False):
    mine = r1 - r0
    engine.reset_graph()
    n, _, L = engine.graph_info()
    st = {"iterations": 0, "exit_check": 0, "hit_iter_cap": 0, "partition_edges": 0, "n_p": n_p}
    it = 0
    if algo == LEIDEN:
        # fast_consensus.py:204-258 on integer node ids: the str-keyed lookups (:97, :217) never
        # match, every weight stays 0 and check #1 (:229) converges on the emptied graph; the
        # loop's CD batch cannot reach the result (capi.cpp fc_run does the same)
        st["exit_check"] = 1
    while algo != LEIDEN:
        if it >= max_iters:
            st["hit_iter_cap"] = 1
            break
        m = engine.m
        part = torch.empty(max(m, 1), dtype=torch.int32, device=device)
        if mine > 0:
            engine.cd(algo, r0, mine, n_p, it)                       # :148 / :270
            engine.consensus_partial(algo, part)                     # :150-159 / :273-280
        else:
            part.fill_(-1 if algo == LOUVAIN else 0)
        # louvain: k_last in [-1, n_p-1] (MAX); lpm / new_consensus rule: counts in [0, n_p] (SUM)
        if algo == LOUVAIN:
            _all_reduce_small(part, dist.ReduceOp.MAX, n_p, world, 1)
        else:
            _all_reduce_small(part, dist.ReduceOp.SUM, n_p, world, 0)
        st["partition_edges"] += n_p * m
        conv1, kept, unc = engine.consensus_apply(algo, n_p, tau, delta, part)   # :163-173
        if louv and conv1:
            st["exit_check"] = 1
            break
        if world > 1 and shard_closure:                              # :175-184 / :292-300
            nc = _closure_sharded(engine, L, it, world, rank, device)
        else:
            nc = engine.closure_sample(L, it)
        cnt = None
        if louv and nc > 0:
            cnt = torch.zeros(nc, dtype=torch.int32, device=device)
            if mine > 0:
                engine.closure_partial(cnt)                          # :186-190
            _all_reduce_small(cnt, dist.ReduceOp.SUM, n_p, world, 0)
        conv2, _ = engine.closure_apply(algo, n_p, delta, cnt, it)   # :193-202 / :307-310
        it += 1
        if conv2:
            st["exit_check"] = 2
            break
    st["iterations"] = it + (1 if st["exit_check"] == 1 else 0)
    m = engine.m
    st["partition_edges"] += n_p * m
    st["m_final"] = m
    if mine > 0:
        engine.cd(algo, r0, mine, n_p, FINAL_PASS_ITER + it)         # final pass :383-392
    if consensus is not None:
        st["consensus"] = _consensus(engine, consensus if isinstance(consensus, str) else float(consensus), n_p, world,
                                      mine, device)
        refine_consensus(engine, st["consensus"], vote=vote, median=median, quality=quality, merge=merge, match=match,
                         calls=sharded_calls(engine, n_p, device))
    if gather and world > 1 and out_shared and out is not None:
        # every rank downloads its rows into the shared host array; the barrier orders the
        # writes before rank 0 hands the array back
        if mine > 0:
            engine.get_labels_into(out[r0:r1], renumber=True)
        dist.barrier()
        return (out if rank == 0 else None), st
    if not gather or world == 1:
        if mine > 0 and out is not None and world == 1:
            engine.get_labels_into(out, renumber=True)
            return out, st
        return (engine.get_labels(mine, renumber=True) if mine > 0 else None), st
    # final partitions: exported straight into the gather buffer (no host round trip), one
    # all-gather, one download on rank 0
    cap = max(shard(n_p, g, world)[1] - shard(n_p, g, world)[0] for g in range(world))
    buf = torch.full((cap, n), -1, dtype=torch.int32, device=device)
    if mine > 0:
        if on_device(buf):
            engine.get_labels(mine, renumber=True, dev_out=buf)
        else:
            buf[:mine].copy_(torch.from_numpy(engine.get_labels(mine, renumber=True)))
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf)
    if rank != 0:
        return None, st
    if out is None:
        out = np.empty((n_p, n), np.int32)
    host = torch.from_numpy(out)   # device -> the host array directly (no staging tensors)
    for g in range(world):
        a, b = shard(n_p, g, world)
        if b > a:
            host[a:b].copy_(bufs[g][:b - a])
    return out, st
