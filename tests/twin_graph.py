"""The engine's working graph as the CPU twin reads it (shared by the GPU parity tests)."""
import numpy as np

from oracle import oracle as orc


def internal_graph(eng, N):
    """-> (the working graph as an EdgeGraph on the engine's internal numbering, node_map())."""
    u, v, w, _ = eng.get_graph()
    sigma = eng.node_map()
    a_, b_ = sigma[u], sigma[v]
    lo, hi = np.minimum(a_, b_), np.maximum(a_, b_)
    o = np.lexsort((hi, lo))
    return orc.EdgeGraph(N, lo[o], hi[o], w[o], np.zeros(len(o), np.int64)), sigma
