"""The engine's working graph as the CPU twin reads it (shared by the GPU parity tests)."""
import numpy as np

from oracle import oracle as orc


def cd_twin(sigma, algo, N, e, count, r0, iteration, seed, **kw):
    """The CPU twin of one CD batch on the input graph `e` in the internal numbering `sigma`
    (fc_get_node_map, or orc.device_sigma for a seed), labels returned in node order like
    fc_get_labels."""
    assert np.array_equal(np.sort(sigma), np.arange(N))
    g_int = orc.EdgeGraph.from_lines(N, np.stack([sigma[e[:, 0]], sigma[e[:, 1]]], 1))
    lab, sw = orc.engine_cd(algo, g_int, count, r0, iteration, seed, **kw)
    return lab[:, sigma], sw


def internal_graph(eng, N):
    """-> (the working graph as an EdgeGraph on the engine's internal numbering, node_map())."""
    u, v, w, _ = eng.get_graph()
    sigma = eng.node_map()
    a_, b_ = sigma[u], sigma[v]
    lo, hi = np.minimum(a_, b_), np.maximum(a_, b_)
    o = np.lexsort((hi, lo))
    return orc.EdgeGraph(N, lo[o], hi[o], w[o], np.zeros(len(o), np.int64)), sigma
