"""Host side of the engine: the drop-in ``fast_consensus()`` and a thin ``Engine`` over
the C-ABI.  Mirrors fast_consensus.py:129-411 (same names, argument meaning, defaults
and return types); all compute runs in the HIP library.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import (FC_ALGO_INFOMAP, FC_ALGO_LEIDEN, FC_ALGO_LOUVAIN, FC_ALGO_LOUVAIN_NC, FC_ALGO_LPM,
                   FastConsensusError, Stats, check, ptr)

ALGORITHMS = {"louvain": FC_ALGO_LOUVAIN, "lpm": FC_ALGO_LPM, "leiden": FC_ALGO_LEIDEN, "infomap": FC_ALGO_INFOMAP}
# consensus weight rules: fast_consensus.py (the named entry point) or the new_consensus.py
# fork's plain count that keeps converged edges (:155-163); louvain only
RULES = ("fast_consensus", "new_consensus")
OUT_OF_SCOPE = ("cnm",)
FINAL_PASS_ITER = 0x40000000  # iteration salt of the final pass (matches capi.cpp fc_run)


def torch_int32():
    import torch
    return torch.int32


def torch_int64():
    import torch
    return torch.int64


def algo_id(algorithm):
    if algorithm in ALGORITHMS:
        return ALGORITHMS[algorithm]
    if algorithm in OUT_OF_SCOPE:
        raise NotImplementedError("algorithm %r is outside this engine's scope (louvain, lpm, leiden and infomap only)"
                                  % algorithm)
    return None


class PinnedHost:
    """Page-locks (hipHostRegister) a caller-owned host array that the engine downloads labelings
    into (Engine.run(out=...), run_sharded(out=...)): the device -> host copy then runs as one
    direct DMA instead of being staged through the runtime's pinned bounce buffers.  A caller that
    keeps one output array pins it once, next to allocating it.  `ok` is False (and nothing is
    pinned) when the runtime refuses.  release() before the array is freed."""

    def __init__(self, array):
        import torch
        self._rt = torch._C._cudart
        self._ptr, self._n = int(array.ctypes.data), int(array.nbytes)
        self.ok = self._n > 0 and int(self._rt.cudaHostRegister(self._ptr, self._n, 0)) == 0

    def release(self):
        if self.ok:
            self._rt.cudaHostUnregister(self._ptr)
            self.ok = False


def device_bytes():
    """Device bytes currently held by this process's engines through their growable buffers
    (Engine.close() returns an engine's whole share)."""
    return int(_lib.load().fc_device_bytes())


class Engine:
    """One device-resident consensus engine (one GPU, one host thread)."""

    def __init__(self, device=0, seed=None):
        L = _lib.load()
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")  # the reference is unseeded
        self.seed = int(seed) & (2 ** 64 - 1)
        self._ctx = ctypes.c_void_p()
        check(L.fc_create(int(device), self.seed, ctypes.byref(self._ctx)))
        self._L = L
        self.device = device

    # -- lifecycle ---------------------------------------------------------------
    def close(self):
        if self._ctx:
            self._L.fc_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle):
        check(self._L.fc_set_stream(self._ctx, stream_handle))
        self._shared_stream = stream_handle is not None

    def _dev(self, t):
        """Address of a caller device buffer.  Unless the engine runs on the caller's stream
        (set_stream), the work queued on that buffer by torch (e.g. the zero fill of
        torch.zeros) is drained first: the engine's own stream is not ordered after it."""
        if t is not None and not getattr(self, "_shared_stream", False) and hasattr(t, "is_cuda") and t.is_cuda:
            import torch
            torch.cuda.current_stream(t.device).synchronize()
        return ptr(t)

    def _written(self):
        """After a native call that wrote a caller device buffer and returned without synchronising
        its stream (the step calls and fc_consensus_support): unless the engine runs on the caller's
        stream, wait for it, so that torch may read the buffer on its own.  Every other analysis call
        synchronises before it returns ("The sync rule") and is followed by none."""
        if not getattr(self, "_shared_stream", False):
            check(self._L.fc_synchronize(self._ctx))

    def set_timing(self, on=True):
        check(self._L.fc_set_timing(self._ctx, 1 if on else 0))

    def collect_timing(self):
        st = Stats()
        check(self._L.fc_collect_timing(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    def set_params(self, buckets=0, max_sweeps=0, max_iters=0):
        check(self._L.fc_set_params(self._ctx, int(buckets), int(max_sweeps), int(max_iters)))

    def set_option(self, name, value):
        if name == "seed":
            value = int(value) & (2 ** 64 - 1)
            self.seed = value
            value = value - 2 ** 64 if value >= 2 ** 63 else value   # int64_t on the C side
        check(self._L.fc_set_option(self._ctx, _lib.OPTIONS[name], int(value)))

    # -- graph -----------------------------------------------------------------------
    def load_graph(self, n, u, v):
        u = np.ascontiguousarray(u, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.int32)
        assert u.shape == v.shape
        check(self._L.fc_load_graph(self._ctx, int(n), len(u), u, v))

    def node_map(self):
        """sigma[node id] = the engine's internal vertex id."""
        out = np.empty(self.n, np.int32)
        check(self._L.fc_get_node_map(self._ctx, out))
        return out

    def reset_graph(self):
        check(self._L.fc_reset_graph(self._ctx))

    def graph_info(self):
        n, m, m0 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self._L.fc_graph_info(self._ctx, ctypes.byref(n), ctypes.byref(m), ctypes.byref(m0)))
        return n.value, m.value, m0.value

    @property
    def n(self):
        return self.graph_info()[0]

    @property
    def m(self):
        return self.graph_info()[1]

    def get_graph(self):
        _, m, _ = self.graph_info()
        u = np.empty(m, np.int32)
        v = np.empty(m, np.int32)
        w = np.empty(m, np.int32)
        age = np.empty(m, np.int64)
        check(self._L.fc_get_graph(self._ctx, ptr(u), ptr(v), ptr(w), ptr(age)))
        return u, v, w, age

    def get_nextgraph(self):
        m = ctypes.c_int64()
        check(self._L.fc_get_nextgraph(self._ctx, ctypes.byref(m), None, None, None, None))
        u, v, w = (np.empty(m.value, np.int32) for _ in range(3))
        age = np.empty(m.value, np.int64)
        check(self._L.fc_get_nextgraph(self._ctx, ctypes.byref(m), ptr(u), ptr(v), ptr(w), ptr(age)))
        return u, v, w, age

    # -- one-shot driver ------------------------------------------------------------------
    def run(self, algo, n_p, tau, delta, out=None):
        """Whole fast_consensus run; returns ([n_p][n] int32 labelings, stats).  `out`: an
        optional C-contiguous int32 host array of that shape to write into (a caller that runs
        repeatedly keeps one: a fresh 256 MB array costs ~20 ms of OS page zeroing on first
        touch, more than the PCIe download itself)."""
        n = self.n
        if out is None:
            labels = np.empty((n_p, n), np.int32)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.shape == (n_p, n)
                    and out.flags.c_contiguous):
                raise ValueError("out must be a C-contiguous int32 array of shape (n_p, n)")
            labels = out
        st = Stats()
        check(self._L.fc_run(self._ctx, int(algo), int(n_p), float(tau), float(delta), ptr(labels),
                             ctypes.byref(st)))
        return labels, st.as_dict()

    # -- step API (distributed driver, replay) ------------------------------------------
    def cd(self, algo, rbegin, rcount, n_p_total, iteration):
        check(self._L.fc_cd(self._ctx, int(algo), int(rbegin), int(rcount), int(n_p_total), int(iteration)))

    def set_labels(self, labels):
        """Install host labelings [count][n] (node order).  Any integer community ids are
        accepted: a row with ids outside [0, n) (1-based memberships, sparse or negative ids)
        is compacted first -- ids only matter through equality (fc_set_labels requires
        [0, n))."""
        labels = np.asarray(labels)
        if labels.ndim != 2 or labels.shape[1] != self.n:
            raise ValueError("labelings must have shape (count, %d)" % self.n)
        if labels.size and (labels.min() < 0 or labels.max() >= self.n):
            labels = np.stack([np.unique(row, return_inverse=True)[1].reshape(-1) for row in labels])
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        check(self._L.fc_set_labels(self._ctx, labels.shape[0], labels))

    def replica_info(self):
        """(local replica count, first global replica index, n_p of the run)."""
        n, b, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self._L.fc_replica_info(self._ctx, ctypes.byref(n), ctypes.byref(b), ctypes.byref(t)))
        return n.value, b.value, t.value

    def _check_count(self, count):
        n_r = self.replica_info()[0]
        if count != n_r:
            raise ValueError("the engine holds %d local labelings, %d requested" % (n_r, count))

    def get_labels(self, count, renumber=False, dev_out=None):
        """[count][n] labelings in node order (count must equal the local replica count): a
        new numpy array, or written into the device tensor `dev_out` (int32, >= count*n
        elements) when given."""
        self._check_count(count)
        if dev_out is not None:
            if dev_out.dtype != torch_int32() or dev_out.numel() < count * self.n:
                raise ValueError("dev_out must be an int32 tensor of >= %d elements" % (count * self.n))
            check(self._L.fc_get_labels(self._ctx, self._dev(dev_out), int(dev_out.numel()), 1 if renumber else 0))
            return dev_out
        out = np.empty((count, self.n), np.int32)
        check(self._L.fc_get_labels(self._ctx, ptr(out), out.size, 1 if renumber else 0))
        return out

    def get_labels_into(self, out, renumber=False):
        """Like get_labels(out.shape[0], ...) into a caller-owned C-contiguous int32 host array."""
        if not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.ndim == 2 and out.shape[1] == self.n
                and out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous int32 array of shape (count, %d)" % self.n)
        self._check_count(out.shape[0])
        check(self._L.fc_get_labels(self._ctx, ptr(out), out.size, 1 if renumber else 0))
        return out

    def consensus_partial(self, algo, dev_out):
        check(self._L.fc_consensus_partial(self._ctx, int(algo), self._dev(dev_out)))
        self._written()

    def consensus_apply(self, algo, n_p, tau, delta, dev_partial):
        conv, kept, unc = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        check(self._L.fc_consensus_apply(self._ctx, int(algo), int(n_p), float(tau), float(delta),
                                         self._dev(dev_partial), ctypes.byref(conv), ctypes.byref(kept),
                                         ctypes.byref(unc)))
        return bool(conv.value), kept.value, unc.value

    def closure_sample(self, attempts, iteration):
        nc = ctypes.c_int64()
        check(self._L.fc_closure_sample(self._ctx, int(attempts), int(iteration), ctypes.byref(nc)))
        return nc.value

    # sharded closure (distributed.py, world > 1): same candidates as closure_sample
    def closure_begin(self, attempts, iteration):
        """Returns the number of closure blocks; block b covers attempts
        [attempts*b//blocks, attempts*(b+1)//blocks)."""
        nb = ctypes.c_int()
        check(self._L.fc_closure_begin(self._ctx, int(attempts), int(iteration), ctypes.byref(nb)))
        return nb.value

    def closure_block_sample(self, block, t_lo, t_hi, dev_out):
        """Draws attempts [t_lo, t_hi) of `block` into dev_out (int64 tensor, (key, first
        attempt) pairs); returns the number of pairs."""
        if dev_out.dtype != torch_int64() or dev_out.numel() < 2 * max(t_hi - t_lo, 0):
            raise ValueError("dev_out must be an int64 tensor of >= %d elements" % (2 * (t_hi - t_lo)))
        k = ctypes.c_int64()
        check(self._L.fc_closure_block_sample(self._ctx, int(block), int(t_lo), int(t_hi), self._dev(dev_out),
                                              int(dev_out.numel() // 2), ctypes.byref(k)))
        self._written()
        return k.value

    def closure_block_add(self, block, dev_in, count):
        check(self._L.fc_closure_block_add(self._ctx, int(block), self._dev(dev_in) if count else None, int(count)))

    def closure_finish(self):
        nc = ctypes.c_int64()
        check(self._L.fc_closure_finish(self._ctx, ctypes.byref(nc)))
        return nc.value

    def closure_set_pairs(self, pairs, iteration):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        nc = ctypes.c_int64()
        check(self._L.fc_closure_set_pairs(self._ctx, len(pairs), ptr(pairs), int(iteration), ctypes.byref(nc)))
        return nc.value

    def closure_partial(self, dev_out):
        check(self._L.fc_closure_partial(self._ctx, self._dev(dev_out)))
        self._written()

    def closure_apply(self, algo, n_p, delta, dev_counts, iteration):
        conv, m = ctypes.c_int(), ctypes.c_int64()
        check(self._L.fc_closure_apply(self._ctx, int(algo), int(n_p), float(delta), self._dev(dev_counts),
                                       int(iteration), ctypes.byref(conv), ctypes.byref(m)))
        return bool(conv.value), m.value

    # -- scoring the local labelings (fc_score_*) ---------------------------------------
    def set_reference(self, labels):
        """Install a reference labeling [n] (node order) for score_pairs' FC_SCORE_REF index; ids
        outside [0, n) are compacted as set_labels does.  None clears it (so does load_graph)."""
        if labels is None:
            check(self._L.fc_score_set_reference(self._ctx, None))
            return
        labels = np.asarray(labels)
        if labels.shape != (self.n,):
            raise ValueError("the reference labeling must have shape (%d,)" % self.n)
        if labels.size and (not np.issubdtype(labels.dtype, np.integer) or labels.min() < 0
                            or labels.max() >= self.n):
            labels = np.unique(labels, return_inverse=True)[1].reshape(-1)   # any ids (strings too): equality only
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        check(self._L.fc_score_set_reference(self._ctx, ptr(labels)))

    def score_partitions(self, graph="input"):
        """Per local replica on `graph` ("input": the loaded G with unit weights, "working": the
        working graph with its consensus weights): a dict of numpy arrays [n_r] -- k, max_size,
        sum_sq, in_weight (int64), tot_sq (exact Python ints, dtype object), s_log, entropy,
        modularity (float64)."""
        gid = self._graph_id(graph)
        n_r = self.replica_info()[0]
        rec = np.zeros(max(n_r, 1), dtype=PART_DTYPE)
        check(self._L.fc_score_partitions(self._ctx, gid, ptr(rec)))
        rec = rec[:n_r]
        out = {k: rec[k].copy() for k in ("k", "max_size", "sum_sq", "in_weight", "s_log", "entropy", "modularity")}
        out["tot_sq"] = np.array([(int(h) << 64) | int(l) for l, h in zip(rec["tot_sq_lo"], rec["tot_sq_hi"])],
                                 dtype=object)
        return out

    def score_pairs(self, pairs=None):
        """Contingency scores of ordered pairs (a, b) of local replica indices (-1: the
        reference labeling): a structured array with fields a, b, cells, sum_sq, slow_members,
        s_log, mi, nmi, ari.  pairs=None: every a < b, then (-1, b) for every b when a
        reference is set."""
        n_r = self.replica_info()[0]
        if pairs is None:
            cap = n_r * (n_r - 1) // 2 + n_r
            parr = None
        else:
            parr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            cap = len(parr)
        rec = np.zeros(max(cap, 1), dtype=PAIR_DTYPE)
        k = ctypes.c_int64(cap)
        check(self._L.fc_score_pairs(self._ctx, ptr(parr), ctypes.byref(k), ptr(rec)))
        return rec[:k.value]

    # -- the consensus partition (fc_consensus_*) ----------------------------------------
    @staticmethod
    def _graph_id(graph):
        """The C id (FC_SCORE_GRAPH_*) of "input" / "working"."""
        if graph not in _lib.SCORE_GRAPHS:
            raise ValueError("graph must be one of %s" % (sorted(_lib.SCORE_GRAPHS),))
        return _lib.SCORE_GRAPHS[graph]

    def _graph_edges(self, graph):
        self._graph_id(graph)
        _, m, m0 = self.graph_info()
        return m0 if graph == "input" else m

    def _support_total(self, graph, dev_support, n_total):
        """n_total of a consensus call: the local replica count, or the caller's with a checked
        `dev_support`."""
        m = self._graph_edges(graph)
        if dev_support is None:
            return self.replica_info()[0]
        if n_total is None:
            raise ValueError("dev_support needs n_total, the number of replicas it was summed over")
        if dev_support.dtype != torch_int32() or dev_support.numel() < m:
            raise ValueError("dev_support must be an int32 tensor of >= %d elements" % m)
        return int(n_total)

    def _phase_timing(self, fn, names):
        """{name: device milliseconds} of the phases one fc_*_timing getter reports."""
        ms = (ctypes.c_double * len(names))()
        check(fn(self._ctx, ms))
        return dict(zip(names, ms))

    def _flat_out(self, dev_out, count, dtype="int32", name="dev_out", contiguous=True):
        """A device tensor of `dtype` ("int32" / "int64") with at least `count` elements: `dev_out`
        when given (checked; `name` is the caller's argument in the message), else a new one."""
        import torch
        if dev_out is None:
            return torch.empty(max(count, 1), dtype=getattr(torch, dtype), device="cuda:%d" % self.device)
        if dev_out.dtype != getattr(torch, dtype) or dev_out.numel() < count or \
                (contiguous and not dev_out.is_contiguous()):
            raise ValueError("%s must be %s %s tensor of >= %d elements"
                             % (name, "a contiguous" if contiguous else "an", dtype, count))
        return dev_out

    def _partition(self, labels, ids=True):
        """The partition `labels` ([n] in node order) with its shape checked: through _node_ids, or
        (ids=False) as the numpy array it is."""
        labels = np.asarray(labels)
        if labels.shape != (self.n,):
            raise ValueError("the partition must have shape (%d,)" % self.n)
        return self._node_ids(labels) if ids else labels

    def consensus_support(self, graph="input", dev_out=None):
        """Per edge of `graph`, the number of local labelings that put both ends in one community:
        an int32 device tensor [m] in the engine's edge order (consensus_partial's; the same on
        every engine that loaded the graph with the same seed and options), written into
        `dev_out` when given.  Ranks add theirs (SUM) and hand the total to consensus_partition."""
        m = self._graph_edges(graph)
        dev_out = self._flat_out(dev_out, m, contiguous=False)
        check(self._L.fc_consensus_support(self._ctx, self._graph_id(graph), self._dev(dev_out)))
        self._written()   # fc_consensus_support queues the count and returns
        return dev_out[:m]

    def consensus_partition(self, agreement=0.5, graph="input", dev_support=None, n_total=None):
        """The consensus partition: the connected components of the edges of `graph` on which at
        least agreement * n_total labelings agree, numbered by smallest node.  `dev_support`:
        None (the local labelings are counted, n_total = their number) or an int32 device tensor
        [m] already summed over `n_total` replicas.  Returns a dict: labels int32[n] (node
        order), support_hist int64[n_total + 1], node_in / node_out int64[n] (support summed over
        a node's edges inside / leaving its consensus community), stability float64[n] =
        node_in / (node_in + node_out) (1.0 for a node without support), and the
        fc_consensus_info fields (edges, kept_edges, unanimous_edges, split_edges, k, max_size,
        singletons, n_total, passes, cut)."""
        nt = self._support_total(graph, dev_support, n_total)
        n = self.n
        labels = np.empty(n, np.int32)
        hist = np.zeros(max(nt, 0) + 1, np.int64)
        nin = np.empty(n, np.int64)
        nout = np.empty(n, np.int64)
        info = _lib.ConsensusInfo()
        check(self._L.fc_consensus_partition(self._ctx, _lib.SCORE_GRAPHS[graph], self._dev(dev_support), nt,
                                             float(agreement), ptr(labels), ptr(hist), ptr(nin), ptr(nout),
                                             ctypes.addressof(info)))
        out = {"labels": labels, "support_hist": hist, "node_in": nin, "node_out": nout}
        out.update(info.as_dict())
        out["stability"] = stability(nin, nout)
        return out

    def consensus_timing(self):
        """Device milliseconds of the phases of the last consensus_partition made with timing on
        (set_timing): support, histogram, components, renumber (+ sizes), node_sums."""
        return self._phase_timing(self._L.fc_consensus_timing,
                                  ("support", "histogram", "components", "renumber", "node_sums"))

    # -- the consensus hierarchy (fc_consensus_levels / fc_consensus_cut) ------------------
    def consensus_levels(self, graph="input", dev_support=None, n_total=None):
        """Every agreement level at once: level s (0..n_total) is the connected components of
        the edges of `graph` with support >= s.  `dev_support` / `n_total` as in
        consensus_partition.  Returns a dict: birth, up int32[n] (the tree: cut_tree(birth, up, s)
        gives level s without an engine), levels (a structured array [n_total + 1] with
        bucket_edges, k, max_size, singletons, in_weight, tot_sq_lo, tot_sq_hi, modularity),
        best_level (the level of largest modularity, compared as exact integers; the highest
        among equals), best_theta = theta_of(best_level, n_total) and n_total.  The tree stays in
        the engine for consensus_cut."""
        nt = self._support_total(graph, dev_support, n_total)
        n = self.n
        birth = np.empty(n, np.int32)
        up = np.empty(n, np.int32)
        levels = np.zeros(max(nt, 0) + 1, LEVEL_DTYPE)
        best = ctypes.c_int32()
        check(self._L.fc_consensus_levels(self._ctx, _lib.SCORE_GRAPHS[graph], self._dev(dev_support), nt,
                                          ptr(birth), ptr(up), ptr(levels), ctypes.byref(best)))
        return {"birth": birth, "up": up, "levels": levels, "best_level": best.value,
                "best_theta": theta_of(best.value, nt), "n_total": nt}

    def consensus_cut(self, level):
        """(labels int32[n] in node order, k) of level `level` of the last consensus_levels."""
        labels = np.empty(self.n, np.int32)
        k = ctypes.c_int64()
        check(self._L.fc_consensus_cut(self._ctx, int(level), ptr(labels), ctypes.byref(k)))
        return labels, k.value

    def consensus_levels_timing(self):
        """Device milliseconds of the phases of the last consensus_levels made with timing on
        (set_timing): bucket, tree, statistics, join_levels."""
        return self._phase_timing(self._L.fc_consensus_levels_timing,
                                  ("bucket", "tree", "statistics", "join_levels"))

    # -- co-association (fc_coassociation / fc_coassoc_pairs / fc_coassoc_hist) -------------
    @staticmethod
    def _node_ids(ids, width=None):
        """ids as a C-contiguous int32 array with at least one element's worth of storage (so
        its address is never NULL); an id that does not fit int32 becomes -1, which the library
        rejects with its index."""
        a = np.asarray(ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("node ids must be integers (positions in node order)")
        if a.size and a.dtype != np.int32:
            a = a.astype(np.int64)
            a = np.where((a < 0) | (a > 2 ** 31 - 1), -1, a)
        a = np.ascontiguousarray(a, dtype=np.int32)
        a = a.reshape(-1) if width is None else a.reshape(-1, width)
        return a if a.size else np.zeros((1,) if width is None else (1, width), np.int32)[:0]

    def coassociation(self, a, b=None, dev_out=None):
        """The consensus matrix of two node lists: an int32 device tensor [na, nb] whose entry
        (i, j) is the number of local labelings that put node a[i] and node b[j] in one community
        (b=None: b = a).  Node ids are the caller's node order (the columns of get_labels); any
        order, duplicates allowed.  Written into `dev_out` (int32, >= na * nb elements) when
        given.  Ranks add theirs (SUM)."""
        a = self._node_ids(a)
        b = None if b is None else self._node_ids(b)
        na, nb = len(a), len(a if b is None else b)
        out = self._flat_out(dev_out, na * nb)
        check(self._L.fc_coassociation(self._ctx, na, ptr(a), nb, ptr(b), self._dev(out)))
        return out.reshape(-1)[:na * nb].view(na, nb)

    def coassoc_pairs(self, pairs, dev_out=None):
        """Per node pair (pairs[p][0], pairs[p][1]), the number of local labelings that put the
        two in one community: an int32 device tensor [npairs]."""
        pairs = self._node_ids(pairs, 2)
        out = self._flat_out(dev_out, len(pairs))
        check(self._L.fc_coassoc_pairs(self._ctx, len(pairs), ptr(pairs), self._dev(out)))
        return out.reshape(-1)[:len(pairs)]

    def coassoc_hist(self, nodes):
        """int64 [n_r + 1]: hist[s] = the number of unordered position pairs i < j of `nodes`
        that s local labelings put in one community.  No matrix is formed (k = 65536 is 2.1 G
        pairs).  pac(hist) and consensus_cdf(hist) read it.  A sharded run's histogram is not the
        sum of the ranks' histograms: see distributed.coassoc_hist_sharded."""
        nodes = self._node_ids(nodes)
        hist = np.zeros(self.replica_info()[0] + 1, np.int64)
        check(self._L.fc_coassoc_hist(self._ctx, len(nodes), ptr(nodes), hist))
        return hist

    def coassoc_timing(self):
        """Device milliseconds of the phases of the last co-association call made with timing on
        (set_timing): ids (upload and map to internal vertices), count (the kernel)."""
        return self._phase_timing(self._L.fc_coassoc_timing, ("ids", "count"))

    # -- cluster and item consensus (fc_cluster_consensus) ----------------------------------
    def cluster_consensus(self, labels, dev_cluster=None, dev_item=None):
        """Monti et al.'s cluster and item consensus of the partition `labels` ([n] in node order,
        integer ids in [0, n), not necessarily dense: a consensus cut, one of the replicas, a
        ground truth) over the local labelings, without the consensus matrix (O(n * n_r)).
        Returns a dict: ids int32[K] (the distinct ids, ascending) and size int64[K];
        cluster_pairs int64[K] (the co-association summed over the ordered member pairs of each
        cluster, diagonal included) and item_pairs int64[n] (each node's co-association summed
        over the members of its own cluster, itself included); the fc_cluster_info fields (k,
        max_size, singletons, pairs_total, slow_members, n_r); and cluster_consensus float64[K],
        item_consensus float64[n], the module-level functions of those integers with n_total =
        n_r (NaN for a cluster of one node).  `dev_cluster` / `dev_item`: int64 device tensors of
        >= n elements to write into (pairs of the K clusters, then zeros; item sums in node
        order); ranks add theirs (SUM), see distributed.cluster_consensus_sharded."""
        n = self.n
        lab = self._partition(labels)
        dev_cluster = self._flat_out(dev_cluster, n, "int64", "dev_cluster")
        dev_item = self._flat_out(dev_item, n, "int64", "dev_item")
        ids = np.empty(max(n, 1), np.int32)
        size = np.empty(max(n, 1), np.int64)
        info = _lib.ClusterInfo()
        check(self._L.fc_cluster_consensus(self._ctx, ptr(lab), ptr(ids), ptr(size), self._dev(dev_cluster),
                                           self._dev(dev_item), ctypes.addressof(info)))
        k = info.k
        ids, size = ids[:k].copy(), size[:k].copy()
        out = {"ids": ids, "size": size, "cluster_pairs": dev_cluster[:k].cpu().numpy(),
               "item_pairs": dev_item[:n].cpu().numpy()}
        out.update(info.as_dict())
        out["cluster_consensus"] = cluster_consensus(out["cluster_pairs"], size, info.n_r)
        out["item_consensus"] = item_consensus(out["item_pairs"], size[np.searchsorted(ids, lab)], info.n_r)
        return out

    def cluster_consensus_timing(self):
        """Device milliseconds of the phases of the last cluster_consensus made with timing on
        (set_timing): segments, count, fallback."""
        return self._phase_timing(self._L.fc_cluster_consensus_timing, ("segments", "count", "fallback"))

    # -- plurality vote (fc_vote_map / fc_vote_count / fc_vote) ----------------------------
    def vote_map(self, labels, dev_mapped=None):
        """Every local labeling relabelled onto the partition `labels` ([n] in node order, ids in
        [0, n), not necessarily dense): each community of replica r becomes the cluster of
        `labels` it shares the most nodes with (the smallest id among equals).  Returns a dict:
        mapped (an int32 device tensor [n_r, n], replica-major, node order, values are ids of
        `labels`; written into `dev_mapped`, contiguous int32 of >= n_r * n elements, when given)
        and k, mapped_communities, slow_members, n_total (= n_r) of fc_vote_info.  Only this
        depends on which rank holds a replica: distributed.vote_sharded all-gathers it."""
        lab = self._partition(labels)
        n_r, n = self.replica_info()[0], self.n
        out = self._flat_out(dev_mapped, n_r * n)
        info = _lib.VoteInfo()
        check(self._L.fc_vote_map(self._ctx, ptr(lab), self._dev(out), ctypes.addressof(info)))
        d = info.as_dict()
        res = {k: d[k] for k in ("k", "mapped_communities", "slow_members", "n_total")}
        res["mapped"] = out.reshape(-1)[:n_r * n].view(n_r, n)
        return res

    def vote(self, labels, dev_mapped=None, n_total=None):
        """Plurality vote of the labelings on the partition `labels` (relabel-and-vote): every
        replica votes, per node, for the cluster its community of that node maps to (vote_map).
        Returns a dict: top int32[n] (the cluster of most votes: the node's own when it is among
        several, else the smallest id), top_votes and own_votes int32[n] (the votes for `top` and
        for the node's own cluster), confidence float64[n] = own_votes / n_total ("x of n_total
        runs agree"), own_hist int64[n_total + 1] and the fc_vote_info fields (k, k_voted, moved,
        unanimous, tied, mapped_communities, slow_members, slow_nodes, n_total).
        `dev_mapped`: None (the local labelings are mapped, n_total = their number) or an int32
        device tensor [n_total, n] of vote_map's layout, from this engine or gathered over ranks;
        no labelings are needed then, and the map's three fields are 0."""
        lab = self._partition(labels)
        n = self.n
        if dev_mapped is None:
            nt = self.replica_info()[0]
        else:
            nt = int(dev_mapped.shape[0] if n_total is None else n_total)
            if dev_mapped.dtype != torch_int32() or not dev_mapped.is_contiguous() or dev_mapped.numel() < nt * n:
                raise ValueError("dev_mapped must be a contiguous int32 tensor of >= n_total * n elements")
        top, tv, own = (self._flat_out(None, n) for _ in range(3))
        hist = np.zeros(max(nt, 0) + 1, np.int64)
        info = _lib.VoteInfo()
        if dev_mapped is None:
            check(self._L.fc_vote(self._ctx, ptr(lab), self._dev(top), self._dev(tv), self._dev(own), ptr(hist),
                                  ctypes.addressof(info)))
        else:
            check(self._L.fc_vote_count(self._ctx, ptr(lab), self._dev(dev_mapped), nt, self._dev(top), self._dev(tv),
                                        self._dev(own), ptr(hist), ctypes.addressof(info)))
        out = info.as_dict()
        out.update(top=top[:n].cpu().numpy(), top_votes=tv[:n].cpu().numpy(), own_votes=own[:n].cpu().numpy(),
                   own_hist=hist)
        out["confidence"] = out["own_votes"].astype(np.float64) / np.float64(out["n_total"])
        return out

    def vote_timing(self):
        """Device milliseconds of the phases of the last vote / vote_map made with timing on
        (set_timing): segments, map, map_fallback, count (0.0 for a phase the call did not run)."""
        return self._phase_timing(self._L.fc_vote_timing, ("segments", "map", "map_fallback", "count"))

    # -- item affinity (fc_item_affinity) ---------------------------------------------------
    def item_affinity(self, labels, nodes, clusters, dev_out=None):
        """aff[p] = the co-association of node nodes[p] summed over the members of cluster
        clusters[p] of the partition `labels` ([n] in node order, ids in [0, n)), over the local
        labelings, the node itself counted where it is a member: exact integers from the
        contingency rows, no matrix, cost following the members of the queried clusters plus the
        queries.  Any order, duplicates allowed, a node may appear against many clusters; an id of
        [0, n) that does not occur in `labels` gives 0.  Returns a dict: aff int64[npairs] and the
        fc_affinity_info fields (k, queried_clusters, slow_lookups, n_r).  `dev_out`: a contiguous
        int64 device tensor of >= npairs elements to write into; ranks add theirs (SUM), see
        distributed.item_affinity_sharded."""
        lab = self._partition(labels)
        nodes, clusters = self._node_ids(nodes), self._node_ids(clusters)
        if len(nodes) != len(clusters):
            raise ValueError("nodes and clusters must have the same length")
        npairs = len(nodes)
        dev_out = self._flat_out(dev_out, npairs, "int64")
        info = _lib.AffinityInfo()
        check(self._L.fc_item_affinity(self._ctx, ptr(lab), npairs, ptr(nodes), ptr(clusters), self._dev(dev_out),
                                       ctypes.addressof(info)))
        out = info.as_dict()
        out["aff"] = dev_out.reshape(-1)[:npairs].cpu().numpy()
        return out

    def item_affinity_timing(self):
        """Device milliseconds of the phases of the last item_affinity made with timing on
        (set_timing): queries, count, fallback."""
        return self._phase_timing(self._L.fc_item_affinity_timing, ("queries", "count", "fallback"))

    def item_consensus(self, nodes, labels, clusters):
        """int64 [len(nodes), len(clusters)]: entry (i, c) is the co-association of node nodes[i]
        summed over the members of cluster clusters[c] of the partition `labels` ([n] in node
        order), the node itself included where it is a member -- the numerator of Monti et al.'s
        item consensus m_i(k) with any cluster, not only the node's own.  A thin helper over
        coassociation: its columns are the clusters' members (in chunks, no matrix above 2^26
        entries), segment-summed on the device with torch.  The cost is co-association's,
        len(nodes) * (members of the clusters) * n_r: meant for a list of doubtful nodes against a
        few candidate clusters; cluster_consensus gives every node's own-cluster sum in O(n * n_r)."""
        import torch
        nodes = self._node_ids(nodes)
        labels = self._partition(labels, ids=False)
        clusters = np.asarray(clusters).reshape(-1)
        members = [np.flatnonzero(labels == c).astype(np.int32) for c in clusters]
        cols = np.concatenate(members) if members else np.zeros(0, np.int32)
        seg = np.repeat(np.arange(len(members), dtype=np.int64), [len(x) for x in members])
        if len(nodes) > ITEM_CHUNK:
            raise ValueError("item_consensus takes at most %d nodes" % ITEM_CHUNK)
        dev = "cuda:%d" % self.device
        out = torch.zeros((len(nodes), len(clusters)), dtype=torch.int64, device=dev)
        width = max(1, ITEM_CHUNK // max(len(nodes), 1))
        for c0 in range(0, len(cols) if len(nodes) else 0, width):
            mat = self.coassociation(nodes, cols[c0:c0 + width])
            out.index_add_(1, torch.as_tensor(seg[c0:c0 + width], device=dev), mat.to(torch.int64))
        return out.cpu().numpy()

    # -- community quality on the graph (fc_community_quality) ------------------------------
    def community_quality(self, labels, graph="input", split=True, nodes=True):
        """What `graph` ("input": G, "working": the consensus graph with its weights) says about
        every cluster of the partition `labels` ([n] in node order, integer ids in [0, n), not
        necessarily dense), where cluster_consensus says what the labelings say.  Needs no
        labelings.  Returns a dict: ids, size, volume (the members' weighted degrees), in_weight
        and in_edges (the edges inside, each once), min_in_degree, components (connected parts of
        the induced subgraph), largest_component and cut = volume - 2 in_weight, int64[K] in id
        order; with `nodes`, node_in / node_out int64[n] (the weight a node sends inside / outside
        its cluster) and mixing float64[n]; with `split`, split int32[n] (the partition refined to
        the connected parts, numbered by smallest node); the fc_quality_info fields (k, max_size,
        singletons, parts, disconnected, in_weight_total, cut_weight, total_degree); and
        conductance, density and modularity_share float64[K], the module-level functions of those
        integers."""
        gid = self._graph_id(graph)
        n = self.n
        lab = self._partition(labels)
        rec = np.empty(max(n, 1), _lib.COMMUNITY_RECORD)
        nin = np.empty(n, np.int64) if nodes else None
        nout = np.empty(n, np.int64) if nodes else None
        sp = np.empty(n, np.int32) if split else None
        info = _lib.QualityInfo()
        check(self._L.fc_community_quality(self._ctx, gid, ptr(lab), ptr(rec), ptr(nin), ptr(nout), ptr(sp),
                                           ctypes.addressof(info)))
        rec = rec[:info.k]
        out = {("ids" if f == "id" else f): rec[f].copy() for f in rec.dtype.names}
        out["cut"] = out["volume"] - 2 * out["in_weight"]
        # `in_weight` is the per-cluster array: the info's total takes another name
        out.update(("in_weight_total" if k == "in_weight" else k, v) for k, v in info.as_dict().items())
        if nodes:
            out.update(node_in=nin, node_out=nout, mixing=mixing(nin, nout))
        if split:
            out["split"] = sp
        out["conductance"] = conductance(out["cut"], out["volume"], info.total_degree)
        out["density"] = density(out["in_edges"], out["size"])
        out["modularity_share"] = modularity_share(out["in_weight"], out["volume"], info.total_degree)
        return out

    def community_quality_timing(self):
        """Device milliseconds of the phases of the last community_quality made with timing on
        (set_timing): labels, rows, fold, components."""
        return self._phase_timing(self._L.fc_community_quality_timing, ("labels", "rows", "fold", "components"))

    # -- cluster merges (fc_community_graph / fc_cluster_coassoc) ---------------------------
    def community_graph(self, labels, graph="input"):
        """The community graph (quotient graph) of the partition `labels` ([n] in node order,
        integer ids in [0, n), not necessarily dense) on `graph` ("input": G, "working": the
        consensus graph with its weights): which clusters touch, and how strongly.  Needs no
        labelings.  Returns a dict: a, b int32[npairs] (the distinct cluster pairs a < b joined by
        at least one edge, ascending by (a, b)), weight int64[npairs] (the sum of w over the joining
        edges), edges int64[npairs] (their number) and npairs."""
        cap = max(self._graph_edges(graph), 1)   # every edge its own pair at the most; the pages stay untouched
        lab = self._partition(labels)
        a, b = np.empty(cap, np.int32), np.empty(cap, np.int32)
        w, e = np.empty(cap, np.int64), np.empty(cap, np.int64)
        cnt = ctypes.c_int64(0)
        check(self._L.fc_community_graph(self._ctx, self._graph_id(graph), ptr(lab), cap, ptr(a), ptr(b), ptr(w),
                                         ptr(e), ctypes.byref(cnt)))
        k = cnt.value
        return {"a": a[:k].copy(), "b": b[:k].copy(), "weight": w[:k].copy(), "edges": e[:k].copy(), "npairs": int(k)}

    def community_graph_timing(self):
        """Device milliseconds of the phases of the last community_graph made with timing on
        (set_timing): labels, emit, sort, pairs."""
        return self._phase_timing(self._L.fc_community_graph_timing, ("labels", "emit", "sort", "pairs"))

    def cluster_coassoc(self, labels, a, b, dev_out=None):
        """x[p] = X(a[p], b[p]): the co-association summed over the member pairs (i in a[p], j in
        b[p]) of two clusters of the partition `labels` ([n] in node order, ids in [0, n)), over the
        local labelings: exact integers from the contingency rows, no matrix.  Duplicates, both
        orders and a[p] == b[p] are allowed (X(a, a) is cluster_consensus' cluster_pairs); an id of
        [0, n) that does not occur in `labels` gives 0.  Returns a dict: x int64[npairs] and the
        fc_cluster_pair_info fields (k, listed_clusters, walked_members, slow_lookups, n_r).
        `dev_out`: a contiguous int64 device tensor of >= npairs elements to write into; ranks add
        theirs (SUM), see distributed.cluster_coassoc_sharded."""
        lab = self._partition(labels)
        a, b = self._node_ids(a), self._node_ids(b)
        if len(a) != len(b):
            raise ValueError("a and b must have the same length")
        npairs = len(a)
        dev_out = self._flat_out(dev_out, npairs, "int64")
        info = _lib.ClusterPairInfo()
        check(self._L.fc_cluster_coassoc(self._ctx, ptr(lab), npairs, ptr(a), ptr(b), self._dev(dev_out),
                                         ctypes.addressof(info)))
        out = info.as_dict()
        out["x"] = dev_out.reshape(-1)[:npairs].cpu().numpy()
        return out

    def cluster_coassoc_timing(self):
        """Device milliseconds of the phases of the last cluster_coassoc made with timing on
        (set_timing): pairs, count, fallback."""
        return self._phase_timing(self._L.fc_cluster_coassoc_timing, ("pairs", "count", "fallback"))

    # -- cluster-wise Jaccard best match (fc_cluster_match) ---------------------------------
    def _match_out(self, dev_out, rows, k, name):
        """An int32 device tensor [>= rows, ld >= k] for one of cluster_match's tables: `dev_out`
        when given (checked), else a new [rows, k]."""
        import torch
        if dev_out is None:
            return torch.empty((max(rows, 1), max(k, 1)), dtype=torch.int32, device="cuda:%d" % self.device)
        if dev_out.dtype != torch_int32() or dev_out.dim() != 2 or not dev_out.is_contiguous() or \
                dev_out.shape[0] < rows or dev_out.shape[1] < k:
            raise ValueError("%s must be a contiguous int32 tensor [>= %d, >= %d]" % (name, rows, k))
        return dev_out

    def cluster_match(self, part, other=None, dev_inter=None, dev_csize=None):
        """The best match, by Jaccard index, of every cluster of the partition `part` ([n] in node
        order, integer ids in [0, n), not necessarily dense) in every local labeling -- or, with
        `other` ([n] in node order, ids in [0, n)), in that one labeling alone, which needs no
        labelings and leaves them untouched (found against planted, one cut against another).
        For cluster k (size s) and row r the community d of r with the largest
        C / (s + t - C), C = |k and d|, t = |d|, chosen on integers (cross-multiplied; among
        equal fractions the larger C), so the pair (C, t) is unique.  Returns a dict: ids int32[K]
        (the distinct ids, ascending) and size int64[K]; inter and csize int32[rows, K] (C and t
        of the match; rows = n_r, or 1 with `other`); the fc_match_info fields (k, max_size,
        singletons, perfect, inter_total, slow_members, n_r); and the module-level functions of
        those integers: jaccard and f1 float64[rows, K], stability float64[K] (Hennig's cluster-wise
        stability: the mean Jaccard over the rows), recovered and dissolved int64[K] (rows with
        J >= 3/4, with J <= 1/2).  `dev_inter` / `dev_csize`: contiguous int32 device tensors
        [>= rows, ld >= K] of one shape to write into (row r's first K entries; the rest is left
        alone); distributed.cluster_match_sharded gathers the ranks' rows."""
        lab = self._partition(part)
        oth = None if other is None else self._partition(other)
        rows = 1 if other is not None else self.replica_info()[0]
        k = len(np.unique(lab))
        dev_inter = self._match_out(dev_inter, rows, k, "dev_inter")
        dev_csize = self._match_out(dev_csize, rows, k, "dev_csize")
        if dev_inter.shape[1] != dev_csize.shape[1]:
            raise ValueError("dev_inter and dev_csize must have one row length")
        n = self.n
        ids = np.empty(max(n, 1), np.int32)
        size = np.empty(max(n, 1), np.int64)
        info = _lib.MatchInfo()
        check(self._L.fc_cluster_match(self._ctx, ptr(lab), ptr(oth), dev_inter.shape[1], ptr(ids), ptr(size),
                                       self._dev(dev_inter), self._dev(dev_csize), ctypes.addressof(info)))
        k = info.k
        out = {"ids": ids[:k].copy(), "size": size[:k].copy(), "inter": dev_inter[:info.n_r, :k].cpu().numpy(),
               "csize": dev_csize[:info.n_r, :k].cpu().numpy()}
        out.update(info.as_dict())
        out.update(match_summary(out["inter"], out["size"], out["csize"]))
        return out

    def cluster_match_timing(self):
        """Device milliseconds of the phases of the last cluster_match made with timing on
        (set_timing): segments, sizes, match, fallback."""
        return self._phase_timing(self._L.fc_cluster_match_timing, ("segments", "sizes", "match", "fallback"))

    def nmi_matrix(self):
        """Symmetric [n_r, n_r] float64 NMI between the local replicas (unit diagonal)."""
        return self._pair_matrices()[0]

    def _pair_matrices(self):
        n_r = self.replica_info()[0]
        iu = np.triu_indices(n_r, 1)
        rec = self.score_pairs(np.stack(iu, 1)) if n_r > 1 else np.zeros(0, PAIR_DTYPE)
        out = []
        for f in ("nmi", "ari"):
            mat = np.eye(n_r, dtype=np.float64)
            mat[iu] = rec[f]
            mat.T[iu] = rec[f]
            out.append(mat)
        return out


PART_DTYPE = np.dtype([(k, np.dtype(t)) for k, t in _lib.PartScore._fields_], align=True)
PAIR_DTYPE = np.dtype([(k, np.dtype(t)) for k, t in _lib.PairScore._fields_], align=True)
assert PART_DTYPE.itemsize == ctypes.sizeof(_lib.PartScore) and PAIR_DTYPE.itemsize == ctypes.sizeof(_lib.PairScore)
CONSENSUS_INFO_DTYPE = np.dtype([(k, np.dtype(t)) for k, t in _lib.ConsensusInfo._fields_], align=True)
assert CONSENSUS_INFO_DTYPE.itemsize == ctypes.sizeof(_lib.ConsensusInfo)
LEVEL_DTYPE = np.dtype([(k, np.dtype(t)) for k, t in _lib.LevelScore._fields_], align=True)
assert LEVEL_DTYPE.itemsize == ctypes.sizeof(_lib.LevelScore)


ITEM_CHUNK = 1 << 26    # Engine.item_consensus: entries of the largest co-association matrix it forms


def cluster_consensus(pairs, size, n_total):
    """Monti et al.'s cluster consensus m(k), float64 [K]: the mean consensus-matrix entry over
    the pairs i != j of cluster k, (pairs - n_total * size) / (n_total * size * (size - 1)) from
    the integers of Engine.cluster_consensus (`pairs` counts ordered pairs with the diagonal,
    which is n_total per node).  NaN where size = 1, as ConsensusClusterPlus gives."""
    pairs, size = np.asarray(pairs, np.int64), np.asarray(size, np.int64)
    nt = np.int64(n_total)
    out = np.full(pairs.shape, np.nan, np.float64)
    m = size > 1
    out[m] = (pairs[m] - nt * size[m]) / (nt * size[m] * (size[m] - 1))
    return out


def item_consensus(item, size_of_own, n_total):
    """Monti et al.'s item consensus m_i(k) of every node with its own cluster, float64 [n]:
    (item - n_total) / (n_total * (size_of_own - 1)), `size_of_own` the size of each node's
    cluster.  NaN where that size is 1."""
    item, size = np.asarray(item, np.int64), np.asarray(size_of_own, np.int64)
    nt = np.int64(n_total)
    out = np.full(item.shape, np.nan, np.float64)
    m = size > 1
    out[m] = (item[m] - nt) / (nt * (size[m] - 1))
    return out


def cluster_result(eng, labels):
    """What fast_consensus(cluster_consensus=True) adds to the `consensus` dict."""
    cc = eng.cluster_consensus(labels)
    return {k: cc[k] for k in ("cluster_consensus", "item_consensus", "cluster_pairs", "item_pairs")}


def _match_ints(inter, size, csize):
    """inter, csize [..., K] and size [K] as int64, and the union size + csize - inter"""
    inter, size, csize = np.asarray(inter, np.int64), np.asarray(size, np.int64), np.asarray(csize, np.int64)
    return inter, size, csize, size + csize - inter


def jaccard(inter, size, csize):
    """inter / (size + csize - inter), float64: the Jaccard index of every best match from the
    integers of Engine.cluster_match (inter, csize [rows, K] or [K]; size [K])."""
    inter, _, _, union = _match_ints(inter, size, csize)
    return inter / union


def match_f1(inter, size, csize):
    """2 inter / (size + csize), float64: the F1 of every best match (precision inter / csize,
    recall inter / size); 2 J / (1 + J), so the match of largest J is the match of largest F1."""
    inter, size, csize, _ = _match_ints(inter, size, csize)
    return 2 * inter / (size + csize)


def cluster_stability(inter, size, csize):
    """Hennig's cluster-wise stability, float64 [K]: the mean over the rows of jaccard."""
    return np.atleast_2d(jaccard(inter, size, csize)).mean(axis=0)


def recovered(inter, size, csize, num=3, den=4):
    """int64 [K]: the rows in which the cluster is recovered, J >= num / den, decided on integers
    as den * inter >= num * union (Hennig's 0.75 by default)."""
    inter, _, _, union = _match_ints(inter, size, csize)
    return np.atleast_2d(den * inter >= num * union).sum(axis=0).astype(np.int64)


def dissolved(inter, size, csize, num=1, den=2):
    """int64 [K]: the rows in which the cluster is dissolved, J <= num / den, decided on integers
    as den * inter <= num * union (Hennig's 0.5 by default)."""
    inter, _, _, union = _match_ints(inter, size, csize)
    return np.atleast_2d(den * inter <= num * union).sum(axis=0).astype(np.int64)


def match_summary(inter, size, csize):
    """The derived arrays of Engine.cluster_match: jaccard, f1, stability, recovered, dissolved."""
    return {"jaccard": jaccard(inter, size, csize), "f1": match_f1(inter, size, csize),
            "stability": cluster_stability(inter, size, csize), "recovered": recovered(inter, size, csize),
            "dissolved": dissolved(inter, size, csize)}


def match_result(eng, labels, cluster_match=None):
    """What fast_consensus(match=True) adds to the `consensus` dict.  The keys carry the call's name:
    the dict's `stability` is the per-node value of consensus_partition.  `cluster_match`: the
    matching function, labels -> dict (default eng.cluster_match; the sharded driver passes its own)."""
    cm = (eng.cluster_match if cluster_match is None else cluster_match)(labels)
    return {"match_inter": cm["inter"], "match_csize": cm["csize"], "match_stability": cm["stability"],
            "match_recovered": cm["recovered"], "match_dissolved": cm["dissolved"]}


def truth_match(eng, truth, labels):
    """The per-community evaluation of the partition `labels` against the planted partition `truth`
    (both [n] in node order; truth's ids are arbitrary integers): Engine.cluster_match with P = the
    planted partition and `labels` as the one row.  ids (truth's own ids, ascending), size, inter,
    csize, jaccard, f1 [K] and mean_f1."""
    ids, dense = np.unique(np.asarray(truth), return_inverse=True)
    cm = eng.cluster_match(dense.reshape(-1).astype(np.int32), other=labels)
    out = {"ids": ids, "size": cm["size"]}
    out.update({k: cm[k][0] for k in ("inter", "csize", "jaccard", "f1")})
    out["mean_f1"] = float(out["f1"].mean())
    return out


def conductance(cut, volume, total_degree):
    """cut / min(volume, total_degree - volume) per cluster, float64 [K], from the integers of
    Engine.community_quality; NaN where that minimum is 0 (a cluster without edges, or one that
    holds every edge end)."""
    cut, volume = np.asarray(cut, np.int64), np.asarray(volume, np.int64)
    den = np.minimum(volume, np.int64(total_degree) - volume)
    out = np.full(cut.shape, np.nan, np.float64)
    m = den > 0
    out[m] = cut[m] / den[m]
    return out


def density(in_edges, size):
    """in_edges / (size (size - 1) / 2) per cluster, float64 [K]; NaN for a cluster of one node."""
    in_edges, size = np.asarray(in_edges, np.int64), np.asarray(size, np.int64)
    out = np.full(in_edges.shape, np.nan, np.float64)
    m = size > 1
    out[m] = 2 * in_edges[m] / (size[m] * (size[m] - 1))
    return out


def modularity_share(in_weight, volume, total_degree):
    """2 in_weight / W2 - (volume / W2)^2 per cluster, float64 [K], W2 = total_degree: the terms
    whose sum is the partition's modularity (zeros on a graph without edges, like the scorer)."""
    in_weight, volume = np.asarray(in_weight, np.int64), np.asarray(volume, np.int64)
    if total_degree == 0:
        return np.zeros(in_weight.shape, np.float64)
    w2 = float(total_degree)
    return 2.0 * in_weight / w2 - (volume / w2) ** 2


def mixing(node_in, node_out):
    """node_out / (node_in + node_out) per node, float64 [n]: the share of a node's weight that
    leaves its cluster (on an LFR graph with its planted partition, the node's empirical mu); NaN
    for a node without incident weight."""
    node_in, node_out = np.asarray(node_in, np.int64), np.asarray(node_out, np.int64)
    tot = node_in + node_out
    out = np.full(tot.shape, np.nan, np.float64)
    m = tot != 0
    out[m] = node_out[m] / tot[m]
    return out


def split_disconnected(eng, labels, graph="input"):
    """`labels` refined to the connected parts of each of its clusters on `graph`, int32[n], the parts
    numbered by their smallest node (Engine.community_quality's `split` alone)."""
    labels = eng._partition(labels, ids=False)
    gid = eng._graph_id(graph)
    lab = eng._node_ids(labels)
    sp = np.empty(len(lab), np.int32)
    check(eng._L.fc_community_quality(eng._ctx, gid, ptr(lab), None, None, None, ptr(sp), None))
    return sp


def quality_result(eng, cons, community_quality=None):
    """What fast_consensus(quality=True) adds to the `consensus` dict: `quality` for its labels and
    `voted_quality` / `median_quality` for the refinements the same call made.  `community_quality`:
    labels -> dict (default eng.community_quality)."""
    cq = eng.community_quality if community_quality is None else community_quality
    out = {"quality": cq(cons["labels"])}
    out.update((k + "_quality", cq(cons[k])) for k in ("voted", "median") if k in cons)
    return out


def vote_refine(eng, labels, max_rounds=16, vote=None):
    """labels <- top of Engine.vote(labels), repeated until a vote moves no node or `max_rounds`
    reassignments were made: unlike the components of the agreement graph, the vote can move a node
    out of the cluster it fell into and empty a fragment cluster.  Returns the dict of the last
    vote, plus `labels` (int32[n], the partition that vote was made on: a fixpoint, top == labels,
    when its moved is 0), `rounds` (the reassignments made) and `moved_per_round` (their sizes).
    `vote`: the voting function, labels -> dict (default eng.vote; the sharded driver passes its own)."""
    vote = eng.vote if vote is None else vote
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    moved = []
    while True:
        res = vote(labels)
        res["labels"] = labels
        if res["moved"] == 0 or len(moved) >= max_rounds:
            break
        moved.append(res["moved"])
        labels = np.ascontiguousarray(res["top"], dtype=np.int32)
    res["rounds"] = len(moved)
    res["moved_per_round"] = moved
    return res


def vote_result(ref):
    """What fast_consensus(vote=True) adds to the `consensus` dict, from vote_refine's result."""
    return {"voted": ref["labels"], "vote_confidence": ref["confidence"], "vote_rounds": ref["rounds"],
            "vote_moved": ref["moved_per_round"]}


def median_objective(pairs_total, size, n_total):
    """F(P) = 2 * agree(P) - R * sum_k s_k^2 as a Python int: `pairs_total` = agree(P), the sum of
    cluster_consensus' cluster_pairs over all R = n_total replicas, `size` the cluster sizes.  The
    summed Mirkin distance of P to the replicas is (T - F) / 2 with T the replicas' summed
    sum_sq (score_partitions), so the median partition is the P of largest F."""
    return 2 * int(pairs_total) - int(n_total) * sum(int(s) * int(s) for s in np.asarray(size).reshape(-1))


def mean_rand(objective, sum_sq, n, n_total):
    """The mean Rand index of P with the R = n_total replicas from F(P) and T: 1 - (T - F) / (R n (n - 1))."""
    if n < 2:
        return 1.0
    return 1.0 - (int(sum_sq) - int(objective)) / (int(n_total) * n * (n - 1))


def median_moves(labels, nodes, clusters, aff, item_pairs, n_total):
    """One round of one-element moves towards the median partition, selected so that their gains
    add exactly.  labels int[n] (ids in [0, n)); (nodes[p], clusters[p]) the candidate targets with
    aff[p] = aff(node, cluster) over all R = n_total replicas (Engine.item_affinity, ranks summed);
    item_pairs[v] = aff(v, P(v)) (cluster_consensus).  With s the cluster sizes,
        pull_own(v) = 2 (item_pairs[v] - R) - R (s_P(v) - 1),   pull(v, b) = 2 aff(v, b) - R s_b,
        gain(v -> b) = pull(v, b) - pull_own(v),   gain(v alone) = -pull_own(v) when s_P(v) > 1,
    and a move of v alone changes F (median_objective) by exactly 2 gain.
    1. Per node (every node, listed or not), the targets are the distinct b != P(v) among its pairs,
       plus "alone" when its cluster has other members; the best has the largest gain, among equals
       the smallest cluster id, "alone" losing a tie to a cluster; it is kept when its gain is > 0.
    2. The kept moves in (gain descending, node ascending) order: winner(c) is the first whose
       source or target is c.  A move is accepted iff it is winner(source) and goes alone or is
       also winner(target): the accepted moves touch pairwise disjoint clusters, so F changes by
       twice the sum of their gains.
    3. The accepted "alone" movers, by ascending node, take the ids of [0, n) that `labels` does
       not use, ascending.
    Every candidate cluster must occur in `labels` (ValueError).  Returns a dict: labels (int32, new),
    gain (int, the sum over the accepted moves), proposed (the kept moves), accepted, alone."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    n = len(labels)
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    clusters = np.asarray(clusters, np.int64).reshape(-1)
    aff = np.asarray(aff, np.int64).reshape(-1)
    item = np.asarray(item_pairs, np.int64).reshape(-1)
    R = np.int64(n_total)
    if not (len(nodes) == len(clusters) == len(aff)) or len(item) != n:
        raise ValueError("nodes, clusters and aff must have one length, item_pairs the length of labels")
    size = np.bincount(labels, minlength=n).astype(np.int64)
    if len(clusters) and (clusters.min() < 0 or clusters.max() >= n or (size[clusters] == 0).any()):
        raise ValueError("a candidate cluster does not occur in labels")
    own = labels
    pull_own = 2 * (item - R) - R * (size[own] - 1)
    # the candidates: (node, target, gain); "alone" is target n, so that it loses ties to every id
    other = clusters != own[nodes]
    cv, cb = nodes[other], clusters[other]
    cg = 2 * aff[other] - R * size[cb] - pull_own[cv]
    lone = np.flatnonzero(size[own] > 1)
    cv = np.concatenate([cv, lone])
    cb = np.concatenate([cb, np.full(len(lone), n, np.int64)])
    cg = np.concatenate([cg, -pull_own[lone]])
    order = np.lexsort((cb, -cg, cv))
    cv, cb, cg = cv[order], cb[order], cg[order]
    first = np.ones(len(cv), bool)
    first[1:] = cv[1:] != cv[:-1]
    keep = first & (cg > 0)
    mv, mb, mg = cv[keep], cb[keep], cg[keep]
    order = np.lexsort((mv, -mg))
    mv, mb, mg = mv[order], mb[order], mg[order]
    m = len(mv)
    pos = np.arange(m, dtype=np.int64)
    src = own[mv]
    win = np.full(n + 1, m, np.int64)
    np.minimum.at(win, src, pos)
    np.minimum.at(win, mb, pos)   # slot n collects the "alone" movers and is not read
    alone = mb == n
    acc = (win[src] == pos) & (alone | (win[np.minimum(mb, n - 1)] == pos))
    new = labels.copy()
    go = acc & ~alone
    new[mv[go]] = mb[go]
    solo = np.sort(mv[acc & alone])
    free = np.flatnonzero(size == 0)
    new[solo] = free[:len(solo)]
    return {"labels": new.astype(np.int32), "gain": int(mg[acc].sum()), "proposed": int(m),
            "accepted": int(acc.sum()), "alone": int(len(solo))}


def median_refine(eng, labels, max_rounds=64, candidates=None, vote=None, cluster_consensus=None,
                  item_affinity=None, sum_sq=None):
    """One-element-move refinement of `labels` towards the median partition of the replicas (the
    partition of largest mean Rand index with them; Filkov & Skiena, Goder & Filkov).  A round:
    the vote gives every node's plurality cluster `top` and the replica total R; the candidates are
    (v, top[v]) for the nodes with top != P (or `candidates`: a pair (nodes, clusters) or a
    callable labels -> (nodes, clusters)); cluster_consensus gives item_pairs, the sizes and
    agree(P); item_affinity the candidates' affinities; median_moves selects and applies.  The loop
    ends when a round accepts nothing (converged) or after `max_rounds` rounds.  A round accepts at
    most one move per cluster: a refinement, not a from-scratch optimiser.
    vote, cluster_consensus, item_affinity: the three engine calls, labels -> dict and
    (labels, nodes, clusters) -> dict (defaults: eng's; the sharded driver passes its own);
    sum_sq: T, the replicas' summed sum_sq (default: from eng.score_partitions).
    Returns a dict: labels (int32[n]), rounds, converged, objective (F before the first round and
    after each, Python ints), proposed_per_round, accepted_per_round, alone_per_round, gain_per_round,
    mean_rand (before, after) and n_total."""
    vote = eng.vote if vote is None else vote
    cluster_consensus = eng.cluster_consensus if cluster_consensus is None else cluster_consensus
    item_affinity = eng.item_affinity if item_affinity is None else item_affinity
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    n = len(labels)
    objective, proposed, accepted, alone, gains = [], [], [], [], []
    converged = False
    R = None
    while True:
        cc = cluster_consensus(labels)
        if R is None or len(accepted) < max_rounds:
            v = vote(labels)
            R = int(v["n_total"])
        F = median_objective(int(np.asarray(cc["cluster_pairs"], np.int64).sum()), cc["size"], R)
        objective.append(F)
        if len(accepted) >= max_rounds:
            break
        if candidates is None:
            top = np.asarray(v["top"])
            nodes = np.flatnonzero(top != labels)
            clusters = top[nodes]
        else:
            nodes, clusters = candidates(labels) if callable(candidates) else candidates
        nodes, clusters = np.asarray(nodes, np.int32).reshape(-1), np.asarray(clusters, np.int32).reshape(-1)
        aff = item_affinity(labels, nodes, clusters)["aff"]
        mv = median_moves(labels, nodes, clusters, aff, cc["item_pairs"], R)
        if mv["accepted"] == 0:
            converged = True
            break
        proposed.append(mv["proposed"]); accepted.append(mv["accepted"]); alone.append(mv["alone"])
        gains.append(mv["gain"])
        labels = mv["labels"]
    if sum_sq is None:
        sum_sq = int(np.asarray(eng.score_partitions()["sum_sq"], np.int64).sum())
    T = int(sum_sq() if callable(sum_sq) else sum_sq)
    return {"labels": labels, "rounds": len(accepted), "converged": converged, "objective": objective,
            "proposed_per_round": proposed, "accepted_per_round": accepted, "alone_per_round": alone,
            "gain_per_round": gains, "n_total": R,
            "mean_rand": (mean_rand(objective[0], T, n, R), mean_rand(objective[-1], T, n, R))}


def median_result(ref):
    """What fast_consensus(median=True) adds to the `consensus` dict, from median_refine's result."""
    return {"median": ref["labels"], "median_objective": ref["objective"], "median_rounds": ref["rounds"],
            "median_moved": ref["accepted_per_round"], "median_mean_rand": ref["mean_rand"]}


def between_consensus(x, size_a, size_b, n_total):
    """x / (n_total s_a s_b) as float64: the mean consensus between two clusters from
    Engine.cluster_coassoc's integers summed over all n_total replicas, the between-cluster
    counterpart of cluster_consensus (NaN where a size is 0)."""
    x = np.asarray(x, np.float64)
    den = float(n_total) * np.asarray(size_a, np.float64) * np.asarray(size_b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, x / den, np.nan)


def merge_moves(labels, a, b, x, n_total):
    """One round of cluster merges towards the median partition, selected so that their gains add
    exactly.  labels int[n] (ids in [0, n)); (a[p], b[p]) the candidate cluster pairs with x[p] =
    X(a, b) over all R = n_total replicas (Engine.cluster_coassoc, ranks summed).  With s the
    cluster sizes, gain(a, b) = 2 X(a, b) - R s_a s_b, and joining a and b alone changes F
    (median_objective) by exactly 2 gain.
    1. Every candidate is oriented so that a < b; a == b and repeated pairs are dropped.
    2. The pairs with gain > 0 are kept.
    3. They are ordered by (gain descending, a ascending, b ascending).
    4. In that order a pair is accepted iff neither of its clusters belongs to a pair accepted
       earlier: the accepted merges touch pairwise disjoint clusters, so F changes by twice the sum
       of their gains.
    5. The members of b take the id a.
    Deterministic on identical integers, so every rank of a sharded run selects the same merges.
    Returns a dict: labels (int32, new), gain (int, the sum over the accepted merges), proposed (the
    kept pairs), accepted."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    n = len(labels)
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.asarray(b, np.int64).reshape(-1)
    x = np.asarray(x, np.int64).reshape(-1)
    if not (len(a) == len(b) == len(x)):
        raise ValueError("a, b and x must have one length")
    if len(a) and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n):
        raise ValueError("a candidate cluster id lies outside [0, n)")
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    lo, hi, x = lo[keep], hi[keep], x[keep]
    _, first = np.unique(lo * n + hi, return_index=True)
    lo, hi, x = lo[first], hi[first], x[first]
    size = np.bincount(labels, minlength=n).astype(np.int64)
    gain = 2 * x - np.int64(n_total) * size[lo] * size[hi]
    pos = gain > 0
    lo, hi, gain = lo[pos], hi[pos], gain[pos]
    order = np.lexsort((hi, lo, -gain))
    lo, hi, gain = lo[order], hi[order], gain[order]
    used = np.zeros(n, bool)
    target = np.arange(n, dtype=np.int64)
    total, accepted = 0, 0
    for ca, cb, cg in zip(lo.tolist(), hi.tolist(), gain.tolist()):
        if used[ca] or used[cb]:
            continue
        used[ca] = used[cb] = True
        target[cb] = ca
        total += cg
        accepted += 1
    return {"labels": target[labels].astype(np.int32), "gain": int(total), "proposed": int(len(lo)),
            "accepted": int(accepted)}


def merge_refine(eng, labels, graph="input", max_rounds=64, candidates=None, community_graph=None,
                 cluster_coassoc=None, cluster_consensus=None, sum_sq=None):
    """Agglomerative refinement of `labels` towards the median partition of the replicas (Filkov &
    Skiena, Goder & Filkov): the move median_refine lacks.  A round: the candidates are the pairs of
    the community graph of the current partition on `graph` (or `candidates`: a pair (a, b) of
    cluster-id lists or a callable labels -> (a, b)); cluster_coassoc gives their X; merge_moves
    selects and applies.  The loop ends when a round accepts nothing (converged) or after
    `max_rounds` rounds.  objective[0] comes from one cluster_consensus call; every later entry is
    the one before plus twice the round's gain (exact: DESIGN, "Cluster merges").  A round accepts at
    most one merge per cluster, only adjacent clusters are candidates, and nothing is ever split.
    community_graph, cluster_coassoc, cluster_consensus: the three engine calls, labels -> dict,
    (labels, a, b) -> dict and labels -> dict (defaults: eng's; the sharded driver passes its own);
    sum_sq: T, the replicas' summed sum_sq (default: from eng.score_partitions).
    Returns a dict: labels (int32[n]), rounds, converged, objective (F before the first round and
    after each), pairs_per_round, proposed_per_round, accepted_per_round, gain_per_round,
    k_per_round (the clusters before the first round and after each) and mean_rand (before, after);
    the lists hold Python ints."""
    if community_graph is None:
        def community_graph(lab):
            return eng.community_graph(lab, graph)
    cluster_coassoc = eng.cluster_coassoc if cluster_coassoc is None else cluster_coassoc
    cluster_consensus = eng.cluster_consensus if cluster_consensus is None else cluster_consensus
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    n = len(labels)
    cc = cluster_consensus(labels)
    R = int(cc["n_total"] if "n_total" in cc else cc["n_r"])
    objective = [median_objective(int(np.asarray(cc["cluster_pairs"], np.int64).sum()), cc["size"], R)]
    ks = [int(len(cc["size"]))]
    pairs, proposed, accepted, gains = [], [], [], []
    converged = False
    while len(accepted) < max_rounds:
        if candidates is None:
            cg = community_graph(labels)
            a, b = cg["a"], cg["b"]
        else:
            a, b = candidates(labels) if callable(candidates) else candidates
        a, b = np.asarray(a, np.int32).reshape(-1), np.asarray(b, np.int32).reshape(-1)
        x = cluster_coassoc(labels, a, b)["x"] if len(a) else np.zeros(0, np.int64)
        mv = merge_moves(labels, a, b, x, R)
        if mv["accepted"] == 0:
            converged = True
            break
        pairs.append(int(len(a))); proposed.append(mv["proposed"]); accepted.append(mv["accepted"])
        gains.append(mv["gain"])
        objective.append(objective[-1] + 2 * mv["gain"])
        ks.append(ks[-1] - mv["accepted"])
        labels = mv["labels"]
    if sum_sq is None:
        sum_sq = int(np.asarray(eng.score_partitions()["sum_sq"], np.int64).sum())
    T = int(sum_sq() if callable(sum_sq) else sum_sq)
    return {"labels": labels, "rounds": len(accepted), "converged": converged, "objective": objective,
            "pairs_per_round": pairs, "proposed_per_round": proposed, "accepted_per_round": accepted,
            "gain_per_round": gains, "k_per_round": ks,
            "mean_rand": (mean_rand(objective[0], T, n, R), mean_rand(objective[-1], T, n, R))}


def merge_result(ref):
    """What fast_consensus(merge=True) adds to the `consensus` dict, from merge_refine's result."""
    return {"merged": ref["labels"], "merged_objective": ref["objective"], "merged_rounds": ref["rounds"],
            "merged_accepted": ref["accepted_per_round"], "merged_k": ref["k_per_round"],
            "merged_mean_rand": ref["mean_rand"]}


def merge_start(cons):
    """The partition merge=True starts from: `median` if it was produced, else `voted`, else the
    consensus partition."""
    for k in ("median", "voted"):
        if k in cons:
            return cons[k]
    return cons["labels"]


def check_consensus_flags(consensus, **flags):
    """ValueError for a flag that needs `consensus` and is set without it -- the first of match,
    merge, quality, median, cluster_consensus, vote among the `flags` given -- then for a
    `consensus` string other than "best"."""
    for name in ("match", "merge", "quality", "median", "cluster_consensus", "vote"):
        if flags.get(name) and consensus is None:
            raise ValueError('%s=True needs consensus (a threshold or "best")' % name)
    if isinstance(consensus, str) and consensus != "best":
        raise ValueError('consensus must be a threshold in [0, 1] or "best"')


def refine_consensus(eng, cons, *, vote=False, median=False, quality=False, merge=False, match=False, calls=None):
    """The optional refinements of the `consensus` dict `cons` in their one order, each adding its
    *_result keys; returns `cons`.  vote: vote_refine of `labels`.  median: median_refine of `voted`
    when vote ran, else of `labels`.  quality: quality_result.  merge: merge_refine of
    merge_start(cons), with quality also `merged_quality`.  match: match_result of `labels`.  All but
    quality read the labelings, so the chain runs before anything replaces them.
    calls: {name: callable} in place of the engine's methods vote, cluster_consensus, item_affinity,
    community_graph, cluster_coassoc, community_quality and cluster_match, and sum_sq (T of the two
    refinements: a number, or a callable evaluated in front of each).  The sharded driver passes
    distributed.sharded_calls; with every call given, `eng` is not used."""
    get = (calls or {}).get

    def total():
        return get("sum_sq")() if callable(get("sum_sq")) else get("sum_sq")

    if vote:
        cons.update(vote_result(vote_refine(eng, cons["labels"], vote=get("vote"))))
    if median:
        cons.update(median_result(median_refine(
            eng, cons["voted"] if vote else cons["labels"], vote=get("vote"),
            cluster_consensus=get("cluster_consensus"), item_affinity=get("item_affinity"), sum_sq=total())))
    if quality:   # of the graph and the partitions alone: no labelings are read
        cons.update(quality_result(eng, cons, get("community_quality")))
    if merge:
        cons.update(merge_result(merge_refine(
            eng, merge_start(cons), community_graph=get("community_graph"), cluster_coassoc=get("cluster_coassoc"),
            cluster_consensus=get("cluster_consensus"), sum_sq=total())))
        if quality:
            cons["merged_quality"] = (get("community_quality") or eng.community_quality)(cons["merged"])
    if match:
        cons.update(match_result(eng, cons["labels"], get("cluster_match")))
    return cons


def level_of(theta, n_total):
    """The level a threshold selects: the smallest integer s that the float64 keep rule keeps,
    i.e. with not (float(s) < theta * float(n_total)).  Scalars or arrays."""
    cut = np.asarray(theta, np.float64) * np.asarray(n_total, np.float64)
    s = np.maximum(np.ceil(cut), 0.0)           # ceil of a float64 is exact: float(s) >= cut, float(s - 1) < cut
    return s.astype(np.int64) if s.ndim else int(s)


def theta_of(level, n_total):
    """A threshold that selects `level`: (level - 0.5) / n_total, and 0.0 for level 0, so that
    level_of(theta_of(s, n_total), n_total) == s.  Scalars or arrays."""
    level = np.asarray(level, np.float64)
    t = np.where(level >= 1, (level - 0.5) / np.asarray(n_total, np.float64), 0.0)
    return t if t.ndim else float(t)


def cut_tree(birth, up, level):
    """Labels int32[n] of level `level` from a consensus_levels tree, by pointer jumping in
    numpy: the same labels as Engine.consensus_cut(level)."""
    birth = np.asarray(birth)
    n = len(birth)
    idx = np.arange(n, dtype=np.int64)
    nxt = np.where(birth >= level, np.asarray(up, np.int64), idx)    # one step, or stay at root_level
    while True:
        jump = nxt[nxt]
        if np.array_equal(jump, nxt):
            break
        nxt = jump
    rank = np.cumsum(nxt == idx) - 1
    return rank[nxt].astype(np.int32)


def stability(node_in, node_out):
    """node_in / (node_in + node_out) per node, 1.0 where both are 0 (a node without support)."""
    tot = node_in + node_out
    out = np.ones(len(tot), np.float64)
    nz = tot != 0
    out[nz] = node_in[nz] / tot[nz]
    return out


def pac(hist, lo=0.1, hi=0.9):
    """Proportion of ambiguous clustering of a co-association histogram (Engine.coassoc_hist):
    with n = len(hist) - 1, the share of the pairs whose count s has lo * n < s < hi * n (float64
    comparisons); 0.0 for a histogram without pairs."""
    hist = np.asarray(hist, np.int64)
    n = len(hist) - 1
    total = int(hist.sum())
    if total == 0:
        return 0.0
    s = np.arange(n + 1, dtype=np.float64)
    mid = (s > np.float64(lo) * np.float64(n)) & (s < np.float64(hi) * np.float64(n))
    return float(int(hist[mid].sum()) / total)


def consensus_cdf(hist):
    """float64 [n + 1]: the share of the pairs with a count <= s (cumsum(hist) / hist.sum());
    zeros for a histogram without pairs."""
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    if total == 0:
        return np.zeros(len(hist), np.float64)
    return np.cumsum(hist) / total


def coassoc_nodes(n, coassoc, labels, seed):
    """Node ids (positions in node order) of fast_consensus(coassoc=...): an int k draws k of
    the n nodes without replacement by numpy.random.default_rng(seed); a list holds the
    caller's node labels."""
    if isinstance(coassoc, (int, np.integer)) and not isinstance(coassoc, bool):
        if not 0 <= coassoc <= n:
            raise ValueError("coassoc=%d: the graph has %d nodes" % (coassoc, n))
        return np.random.default_rng(seed).choice(n, size=int(coassoc), replace=False).astype(np.int32)
    index = {x: i for i, x in enumerate(np.asarray(labels).tolist())}
    try:
        return np.asarray([index[x] for x in coassoc], np.int32)
    except KeyError as e:
        raise ValueError("coassoc: %r is not a node of the graph" % (e.args[0],)) from None


def coassoc_result(eng, ids, node_labels, cons=None):
    """The `coassoc` dict of fast_consensus(coassoc=...) from the engine's local labelings."""
    node_labels = np.asarray(node_labels)
    hist = eng.coassoc_hist(ids)
    out = {"nodes": [node_labels[i] for i in ids.tolist()] if node_labels.dtype == object else node_labels[ids].tolist(),
           "matrix": eng.coassociation(ids).cpu().numpy(), "hist": hist, "pac": pac(hist), "cdf": consensus_cdf(hist)}
    if cons is not None:
        out["order"] = np.argsort(cons["labels"][ids], kind="stable")
    return out


def best_consensus(eng, dev_support=None, n_total=None):
    """consensus="best": the hierarchy (consensus_levels), then the consensus partition at the
    best level's threshold -- every field consensus_partition returns, plus level, theta, levels,
    birth and up.  dev_support: the support summed over n_total replicas (the sharded driver's);
    None: both calls count it over the engine's own labelings, which keeps the one-engine paths
    (fast_consensus, the command line) free of torch, as with a float threshold."""
    lev = eng.consensus_levels("input", dev_support=dev_support, n_total=n_total)
    cons = eng.consensus_partition(lev["best_theta"], "input", dev_support=dev_support, n_total=n_total)
    cons.update(level=lev["best_level"], theta=lev["best_theta"], levels=lev["levels"], birth=lev["birth"],
                up=lev["up"])
    return cons


def consensus_scores(eng, sc, cons, truth=None):
    """Adds to the `scores` dict what relates the n_p partitions to the consensus partition:
    nmi_consensus / ari_consensus [n_p] (the consensus labeling installed as the reference), then
    -- the engine's labelings are REPLACED by the consensus labeling as a one-replica batch, so
    the caller has downloaded them -- consensus_modularity (on the input graph) and, with
    `truth`, consensus_nmi_truth / consensus_ari_truth."""
    n_p = eng.replica_info()[0]
    eng.set_reference(cons["labels"])
    rec = eng.score_pairs(np.stack([np.full(n_p, _lib.FC_SCORE_REF), np.arange(n_p)], 1))
    sc["nmi_consensus"] = rec["nmi"].copy()
    sc["ari_consensus"] = rec["ari"].copy()
    eng.set_labels(cons["labels"][None, :])
    sc["consensus_modularity"] = float(eng.score_partitions("input")["modularity"][0])
    if truth is not None:
        eng.set_reference(truth)
        rec = eng.score_pairs([(_lib.FC_SCORE_REF, 0)])
        sc["consensus_nmi_truth"] = float(rec["nmi"][0])
        sc["consensus_ari_truth"] = float(rec["ari"][0])
    else:
        eng.set_reference(None)
    return sc


def run_scores(eng, truth=None):
    """The `scores` dict of fast_consensus(scores=True) from the engine's local labelings:
    modularity and k per partition (on the input graph), the pairwise nmi / ari matrices, their
    mean off-diagonal NMI, the medoid (largest mean NMI to the others, ties to the lowest index)
    and, with `truth` [n] in node order, nmi_truth / ari_truth."""
    n_p = eng.replica_info()[0]
    part = eng.score_partitions("input")
    nmi, ari = eng._pair_matrices()
    out = {"modularity": part["modularity"], "k": part["k"], "nmi": nmi, "ari": ari}
    if n_p > 1:
        others = (nmi.sum(1) - 1.0) / (n_p - 1)
        out["mean_pairwise_nmi"] = float(nmi[np.triu_indices(n_p, 1)].mean())
    else:
        others = np.ones(n_p)
        out["mean_pairwise_nmi"] = 1.0
    out["medoid"] = int(np.argmax(others))     # argmax returns the first of equal maxima
    if truth is not None:
        eng.set_reference(truth)
        rec = eng.score_pairs(np.stack([np.full(n_p, _lib.FC_SCORE_REF), np.arange(n_p)], 1))
        out["nmi_truth"] = rec["nmi"].copy()
        out["ari_truth"] = rec["ari"].copy()
    return out


def truth_array(truth, labels):
    """truth as an array in `labels` (node) order: a {node: community} dict or such an array."""
    if isinstance(truth, dict):
        return np.asarray([truth[x] for x in labels.tolist()])
    truth = np.asarray(truth)
    if truth.shape != (len(labels),):
        raise ValueError("truth must be a {node: community} dict or an array of %d ids in node order" % len(labels))
    return truth


# ------------------------------------------------------------------------------------ inputs
ADJ_PARALLEL_MIN = 4_000_000     # adjacency entries from which read_adjacency forks workers


def host_workers():
    """Worker processes for the host conversion: FC_HOST_WORKERS, else min(8, the CPUs this
    process may run on)."""
    env = os.environ.get("FC_HOST_WORKERS")
    if env is not None:
        return max(1, int(env))
    try:
        cpus = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cpus = os.cpu_count() or 1
    return max(1, min(8, cpus))


ADJ_DEADLINE_S = 30.0            # forked read: workers still running after this (+0.2 us per entry) are killed


def _fork_safe():
    """The forked read runs only in a process with no other Python thread (a thread could hold
    an interpreter-level lock -- import, logging, a user lock -- that a child would wait on
    forever) and when FC_HOST_FORK is not 0.  Native runtime threads (a HIP runtime started by
    an earlier Engine) do not block it: the children run dict iteration and numpy only (the
    interpreter's allocator under the GIL, glibc malloc, which resets its locks at fork), never
    touch the GPU and leave through os._exit; the deadline in _reap covers the rest."""
    import threading
    return os.environ.get("FC_HOST_FORK", "1") != "0" and threading.active_count() == 1


def _reap(pids, deadline):
    """Wait for the forked workers with WNOHANG polling until `deadline` (time.monotonic());
    past it the rest are killed and reaped.  True iff every worker exited with status 0."""
    import signal
    import time
    ok, left = True, list(pids)
    while left:
        for pid in list(left):
            done, status = os.waitpid(pid, os.WNOHANG)
            if done:
                left.remove(pid)
                ok = ok and status == 0
        if left and time.monotonic() > deadline:
            for pid in left:
                try:
                    os.kill(pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                os.waitpid(pid, 0)
            return False
        if left:
            time.sleep(0.002)
    return ok


def read_adjacency(rows, lens, key=None):
    """The keys of the dicts `rows` (row i has lens[i] keys), concatenated into int64, each
    through `key` when given.  Reading 27.5 M dict keys is CPython-bound (~0.1 us per key, most
    of it a cache miss on the key object), so large adjacencies are read by forked workers,
    each chaining a contiguous range of rows into a shared anonymous mapping (no pickling: the
    children see the parent's dicts copy-on-write).  Any worker failure, or workers still
    running at the deadline (killed), falls back to the serial read; a process with other
    Python threads reads serially (_fork_safe)."""
    import itertools
    tot = int(lens.sum())
    W = host_workers() if hasattr(os, "fork") else 1

    def serial(lo, hi, cnt):
        it = itertools.chain.from_iterable(rows[lo:hi])
        return np.fromiter(it if key is None else map(key, it), np.int64, count=cnt)

    if W <= 1 or tot < ADJ_PARALLEL_MIN or not _fork_safe():
        return serial(0, len(rows), tot)
    import mmap
    import time
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    cut = np.searchsorted(off, np.linspace(0, tot, W + 1).astype(np.int64))
    cut[0], cut[-1] = 0, len(rows)
    buf = mmap.mmap(-1, tot * 8)                   # MAP_SHARED | MAP_ANONYMOUS: children write it
    flat = np.frombuffer(buf, np.int64)
    pids = []
    try:
        for w in range(W):
            lo, hi = int(cut[w]), int(cut[w + 1])
            if hi <= lo:
                continue
            pid = os.fork()
            if pid == 0:                               # child: fill its range, leave without cleanup
                code = 1
                try:
                    flat[off[lo]:off[hi]] = serial(lo, hi, int(off[hi] - off[lo]))
                    code = 0
                finally:
                    os._exit(code)
            pids.append(pid)
    finally:
        ok = _reap(pids, time.monotonic() + ADJ_DEADLINE_S + tot * 2e-7)
    if len(pids) == 0 or not ok:
        del flat
        buf.close()
        return serial(0, len(rows), tot)
    out = flat.copy()
    del flat
    buf.close()
    return out


class IdGraph:
    """A graph in engine form: node labels in node order + edges as node-order ids, in an
    order whose per-node first occurrences reproduce networkx adjacency order."""

    def __init__(self, labels, u, v):
        lab = np.asarray(labels)
        if lab.ndim != 1:      # tuple nodes (grid graphs ...): one object per node, not a 2-D array
            lab = np.fromiter(labels, dtype=object, count=len(labels))
        self.labels = lab
        self.u = np.ascontiguousarray(u, dtype=np.int32)
        self.v = np.ascontiguousarray(v, dtype=np.int32)

    @property
    def n(self):
        return len(self.labels)

    @staticmethod
    def from_networkx(G):
        """Node order = G.nodes(); for each node x, its later neighbours are emitted in
        G.adj[x] order (that is the order G.copy() keeps, fast_consensus.py:131).  The
        adjacency is read at C speed (dict keys chained into numpy) and mapped to indices by a
        lookup array when the nodes are small non-negative integers (by a dict otherwise).
        Past ADJ_PARALLEL_MIN adjacency entries the read is split over forked workers
        (read_adjacency)."""
        if G.is_directed():
            raise TypeError("fast_consensus needs an undirected graph")
        nodes = list(G.nodes())
        n = len(nodes)
        adj = getattr(G, "_adj", None)
        rows = list(adj.values()) if isinstance(adj, dict) and len(adj) == n else None
        if rows is None or (n and (next(iter(adj)) != nodes[0] or list(adj) != nodes)):
            rows = [G.adj[x] for x in nodes]        # adjacency not keyed in node order: per node
        lens = np.fromiter(map(len, rows), np.int64, count=n)
        if n and all(type(x) is int for x in nodes[:1]) and all(isinstance(x, (int, np.integer)) for x in nodes) \
                and min(nodes) >= 0 and max(nodes) < 4 * n + 1024:
            lut = np.full(max(nodes) + 1, -1, np.int64)
            lut[np.asarray(nodes, np.int64)] = np.arange(n, dtype=np.int64)
            nbr = lut[read_adjacency(rows, lens)]
        else:
            idx = {x: i for i, x in enumerate(nodes)}
            nbr = read_adjacency(rows, lens, idx.__getitem__)
        src = np.repeat(np.arange(n, dtype=np.int64), lens)
        keep = nbr > src
        return IdGraph(nodes, src[keep].astype(np.int32), nbr[keep].astype(np.int32))

    @staticmethod
    def from_edgelist_file(path):
        """Native parser (nx.read_edgelist(path, nodetype=int) semantics, :434)."""
        L = _lib.load()
        n, m = ctypes.c_int64(), ctypes.c_int64()
        check(L.fc_read_edgelist(path.encode(), ctypes.byref(n), ctypes.byref(m), None, None, None))
        labels = np.empty(n.value, np.int64)
        u = np.empty(m.value, np.int32)
        v = np.empty(m.value, np.int32)
        check(L.fc_read_edgelist(path.encode(), ctypes.byref(n), ctypes.byref(m), ptr(labels), ptr(u), ptr(v)))
        return IdGraph(labels, u, v)


class Cover:
    """What ``leidenalg.find_partition(...).as_cover()`` returns (fast_consensus.py:123), as far
    as the reference uses it: iterating yields the clusters (lists of igraph vertex ids,
    ascending), ``membership[j]`` is ``[cluster of vertex j]`` (:465-466) and ``len`` is the
    number of clusters.  igraph vertex j is the j-th smallest node label (``nx_to_igraph``
    adds ``sorted(G.nodes())``, :47).  Clusters are numbered by decreasing size, as leidenalg
    renumbers its communities (ties: the cluster holding the smaller vertex first).  Parity
    unpinned: leidenalg is absent here, so this numbering (and the Leiden/Infomap partitions
    themselves) are checked only against the restatement in oracle/fc_oracle.c."""

    def __init__(self, vertex_labels):
        lab = np.asarray(vertex_labels)
        k = int(lab.max()) + 1 if lab.size else 0
        sizes = np.bincount(lab, minlength=k)
        first = np.full(k, lab.size, np.int64)
        np.minimum.at(first, lab, np.arange(lab.size))
        order = np.lexsort((first, -sizes))
        rank = np.empty(k, np.int64)
        rank[order] = np.arange(k)
        self._m = rank[lab] if lab.size else lab.astype(np.int64)
        self._k = k

    def __len__(self):
        return self._k

    def __iter__(self):
        idx = np.argsort(self._m, kind="stable")
        bounds = np.searchsorted(self._m[idx], np.arange(self._k + 1))
        for c in range(self._k):
            yield idx[bounds[c]:bounds[c + 1]].tolist()

    def __getitem__(self, c):
        return np.flatnonzero(self._m == c).tolist()

    @property
    def membership(self):
        return [[int(c)] for c in self._m]

    def sizes(self):
        return np.bincount(self._m, minlength=self._k).tolist()


def labels_to_output(algorithm, node_labels, labels):
    """Engine labelings [n_p][N] -> the reference's return type (fast_consensus.py:383-392):
    louvain: list of dict node -> community (insertion order = node order, as
    python-louvain builds it); lpm and infomap: list of set of frozenset of nodes; leiden:
    list of ``Cover`` (igraph vertex ids, :385-388)."""
    out = []
    nodes = list(node_labels.tolist())
    if algorithm == "leiden":
        vid = np.argsort(np.argsort(np.asarray(node_labels), kind="stable"), kind="stable")   # node -> vertex id
        for lab in labels:
            vl = np.empty(len(lab), np.int64)
            vl[vid] = lab
            out.append(Cover(vl))
        return out
    na = np.asarray(node_labels)
    # louvain: each dict is a copy of one key template (no rehashing as it grows), then its
    # values are set in node order -- ~10 % less than dict(zip(...)) per 1M-entry labeling
    tmpl = dict.fromkeys(nodes) if algorithm == "louvain" else None
    for lab in labels:
        if algorithm == "louvain":
            d = tmpl.copy()
            d.update(zip(nodes, lab.tolist()))
            out.append(d)
        else:
            # the communities as runs of one stable sort by label (C speed; a frozenset per run)
            lab = np.asarray(lab)
            order = np.argsort(lab, kind="stable")
            sl = lab[order]
            b = [0] + (np.flatnonzero(sl[1:] != sl[:-1]) + 1).tolist() + [len(sl)]
            srt = na[order].tolist()
            out.append({frozenset(srt[b[i]:b[i + 1]]) for i in range(len(b) - 1)} if len(sl) else set())
    return out


def store_order_pays(replicas, algorithm=None, cd_engine=0):
    """Label storage order (FC_OPT_STORE) for a GPU that will hold `replicas` replicas: the
    one-replica ordering pass at load costs ~4 ms on LFR-1M and saves gather misses of the
    classic CD engine (the default) in proportion to the replicas (measured: n_p=8 61.7 ms
    without vs 63.0 with, n_p=16 89.0 vs 87.0, n_p=64 saves ~20 ms).  The replica-lane engine
    (cd_engine=1) reads labels node-major and gains nothing from it for louvain / lpm."""
    if cd_engine == 1 and algorithm in (FC_ALGO_LOUVAIN, FC_ALGO_LPM, FC_ALGO_LOUVAIN_NC, "louvain", "lpm"):
        return 0
    return 1 if replicas >= 12 else 0


def relabel_for(algorithm):
    """FC_OPT_RELABEL for a run of `algorithm`: infomap's union levels gather neighbour state by
    internal id and assign buckets by a hash of it, so a community-ordered numbering (2) puts
    a vertex's in-community neighbours on shared lines (LFR-100k infomap 1.56 -> 1.46 s per
    call, same output; profiles/r06_ab.txt); every other algorithm keeps the random numbering
    (1) its chunked visit orders need."""
    return 2 if algorithm in (FC_ALGO_INFOMAP, "infomap") else 1


def fast_consensus(G, algorithm='louvain', n_p=20, thresh=0.2, delta=0.02, *, seed=None, device=0,
                   return_stats=False, rule="fast_consensus", scores=False, truth=None, consensus=None,
                   coassoc=None, cluster_consensus=False, vote=False, median=False, quality=False, merge=False,
                   match=False):
    """Drop-in for fast_consensus.py:129 ``fast_consensus(G, algorithm, n_p, thresh, delta)``.

    G: an undirected networkx Graph (weights are ignored: the reference resets them to 1,
    :135-136) or an ``IdGraph``.  Returns a list of n_p partitions -- dicts for louvain,
    sets of frozensets for lpm and infomap, ``Cover`` objects for leiden -- or None for an unknown
    algorithm (the reference's loop
    ``break``s and returns None, :380-381).  ``seed`` makes the run reproducible (the
    reference is unseeded).  ``rule="new_consensus"`` (louvain only) switches to the
    new_consensus.py fork's weight rule (:155-163).

    ``scores=True`` also scores the partitions on the device before they are converted and
    returns ``(partitions, scores)`` -- ``(partitions, stats, scores)`` with ``return_stats`` --
    where ``scores`` holds ``modularity[n_p]`` and ``k[n_p]`` (on G), the ``nmi[n_p, n_p]`` and
    ``ari[n_p, n_p]`` matrices, ``mean_pairwise_nmi``, ``medoid`` (the partition with the largest
    mean NMI to the others, ties to the lowest index) and, with ``truth`` (a ``{node: community}``
    dict or an array in node order), ``nmi_truth[n_p]`` and ``ari_truth[n_p]``.

    ``consensus=theta`` (a float in [0, 1]) appends a ``consensus`` dict to the returned tuple
    (after ``stats`` and ``scores`` when present): the consensus partition of the n_p partitions
    -- the connected components of the edges of G on which at least theta * n_p of them agree
    (``Engine.consensus_partition``) -- with ``labels``, ``support_hist``, ``node_in``,
    ``node_out``, ``stability``, the info fields and ``partition``, a ``{node: community}`` dict.
    With ``scores=True`` as well, ``scores`` gains ``nmi_consensus[n_p]`` and
    ``ari_consensus[n_p]`` (every partition against the consensus partition),
    ``consensus_modularity`` and, with ``truth``, ``consensus_nmi_truth`` / ``consensus_ari_truth``.

    ``consensus="best"`` picks the threshold itself: the consensus hierarchy over all levels
    0..n_p (``Engine.consensus_levels``) and the consensus partition at the level of largest
    modularity on G (the strictest among equals).  The ``consensus`` dict then also holds
    ``level``, ``theta``, ``levels`` (one record per level), ``birth`` and ``up`` (the tree:
    ``cut_tree(birth, up, s)`` gives any other level).

    ``coassoc=nodes`` (a list of node labels, or an int k: k nodes drawn without replacement by
    ``numpy.random.default_rng(seed)``) appends a ``coassoc`` dict to the returned tuple, after
    ``consensus`` when present: ``nodes``, ``matrix`` (numpy int32 [k, k]: how many of the n_p
    partitions put two of the nodes together), ``hist`` (the counts' histogram over the pairs
    i < j, ``Engine.coassoc_hist``), ``pac`` and ``cdf`` (``pac(hist)``, ``consensus_cdf(hist)``)
    and, with ``consensus`` also given, ``order``: the stable argsort of the nodes by consensus
    label, so that ``matrix[order][:, order]`` is the block heatmap.

    ``cluster_consensus=True`` (needs ``consensus``) adds Monti et al.'s two other summaries of the
    consensus partition to the ``consensus`` dict (``Engine.cluster_consensus``):
    ``cluster_consensus`` (float64 per community, in label order: which communities are solid),
    ``item_consensus`` (float64 per node, with its own community: which nodes are firmly placed)
    and the exact integers behind them, ``cluster_pairs`` and ``item_pairs``.

    ``vote=True`` (needs ``consensus``) refines the consensus partition by plurality vote of the
    n_p partitions (``vote_refine``) and adds to the ``consensus`` dict ``voted`` (int32 per node:
    the refined partition, ids of the consensus partition), ``vote_confidence`` (float64 per node:
    the share of the partitions that vote for the node's refined cluster), ``vote_rounds`` and
    ``vote_moved`` (the nodes reassigned in each round).

    ``median=True`` (needs ``consensus``) refines the consensus partition -- ``voted`` with
    ``vote=True`` -- by exact one-element moves towards the median partition of the n_p partitions
    (``median_refine``) and adds to the ``consensus`` dict ``median`` (int32 per node),
    ``median_objective`` (F before the first round and after each), ``median_rounds``,
    ``median_moved`` (the moves accepted in each round) and ``median_mean_rand`` (the mean Rand
    index with the partitions before and after).

    ``quality=True`` (needs ``consensus``) adds ``quality`` to the ``consensus`` dict: what G says
    about the consensus communities (``Engine.community_quality`` of ``labels``: internal weight,
    cut, volume, conductance, density, modularity share, connected parts, the split partition and
    the per-node mixing) and, for each of ``voted`` / ``median`` the same call produced,
    ``voted_quality`` / ``median_quality``.

    ``merge=True`` (needs ``consensus``) runs last, on ``median`` if it was produced, else on
    ``voted``, else on the consensus partition: cluster merges towards the median partition of the
    n_p partitions (``merge_refine``: the community graph's pairs, their exact co-association, a
    greedy matching of the positive gains).  It adds to the ``consensus`` dict ``merged`` (int32
    per node), ``merged_objective`` (F before the first round and after each), ``merged_rounds``,
    ``merged_accepted`` (the merges of each round), ``merged_k`` (the clusters before the first
    round and after each) and ``merged_mean_rand``; with ``quality=True`` also ``merged_quality``.

    ``match=True`` (needs ``consensus``) asks of every consensus community whether the n_p
    partitions contain it as a community (``Engine.cluster_match``: its best match by Jaccard index
    in each partition) and adds to the ``consensus`` dict ``match_inter`` and ``match_csize`` (int32
    [n_p, K]: the overlap with, and the size of, the matched community), ``match_stability``
    (float64 [K]: Hennig's cluster-wise stability, the mean Jaccard index), ``match_recovered`` and
    ``match_dissolved`` (int64 [K]: the partitions with J >= 3/4, with J <= 1/2).  With ``truth`` it
    also adds ``truth_match``: the planted communities against the consensus partition (``ids``,
    ``size``, ``inter``, ``csize``, ``jaccard``, ``f1`` per planted community, and ``mean_f1``).
    """
    check_consensus_flags(consensus, match=match, merge=merge, quality=quality, median=median,
                          cluster_consensus=cluster_consensus, vote=vote)
    algo = algo_id(algorithm)
    if algo is None:
        return None
    if rule not in RULES:
        raise ValueError("rule must be one of %s" % (RULES,))
    if rule == "new_consensus":
        if algo != FC_ALGO_LOUVAIN:
            raise ValueError("the new_consensus.py rule exists for louvain only")
        algo = FC_ALGO_LOUVAIN_NC
    g = G if isinstance(G, IdGraph) else IdGraph.from_networkx(G)
    if algo == FC_ALGO_LEIDEN and not np.issubdtype(np.asarray(g.labels).dtype, np.integer):
        # The engine's leiden loop is the one-iteration exit the reference takes when its
        # str(vertex id)-keyed lookup (:97) never matches an int node (:214-217).  With other
        # node types that lookup can match and the reference runs a real loop: not modelled.
        raise NotImplementedError("algorithm='leiden' is modelled for integer node labels only "
                                  "(fast_consensus.py:97, :214-217)")
    with Engine(device=device, seed=seed) as eng:
        eng.set_option("store", store_order_pays(n_p, algo))
        eng.set_option("relabel", relabel_for(algo))
        eng.load_graph(g.n, g.u, g.v)
        labels, stats = eng.run(algo, int(n_p), float(thresh), float(delta))
        tr = None if truth is None else truth_array(truth, g.labels)
        if isinstance(consensus, str):
            cons = best_consensus(eng)
        else:
            cons = eng.consensus_partition(float(consensus)) if consensus is not None else None
        if cluster_consensus:   # before consensus_scores replaces the labelings
            cons.update(cluster_result(eng, cons["labels"]))
        if cons is not None:   # before consensus_scores replaces the labelings
            refine_consensus(eng, cons, vote=vote, median=median, quality=quality, merge=merge, match=match)
        if match and tr is not None:
            cons["truth_match"] = truth_match(eng, tr, cons["labels"])
        ca = None
        if coassoc is not None:   # before consensus_scores replaces the labelings
            ca = coassoc_result(eng, coassoc_nodes(g.n, coassoc, g.labels, seed), g.labels, cons)
        sc = run_scores(eng, tr) if scores else None
        if cons is not None and scores:
            consensus_scores(eng, sc, cons, tr)
    out = labels_to_output(algorithm, g.labels, labels)
    if cons is not None:
        cons["partition"] = dict(zip(np.asarray(g.labels).tolist(), cons["labels"].tolist()))
    res = (out,) + ((stats,) if return_stats else ()) + ((sc,) if scores else ()) + \
        ((cons,) if cons is not None else ()) + ((ca,) if ca is not None else ())
    return res if len(res) > 1 else out


def check_consensus_graph(G, n_p, delta):
    """fast_consensus.py:17-37 on a networkx graph (host utility, not the hot path)."""
    count = sum(1 for w in (d.get("weight") for _, _, d in G.edges(data=True)) if w != 0 and w != n_p)
    return not (count > delta * G.number_of_edges())


def group_to_partition(partition):
    """fast_consensus.py:55-71: {node: community} -> communities in first-appearance order."""
    part = {}
    for node, c in partition.items():
        part.setdefault(c, []).append(node)
    return part.values()
