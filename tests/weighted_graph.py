"""An engine whose working graph carries chosen int32 weights (shared by the GPU tests that need
weights no consensus run of a small graph produces).

fc_consensus_apply takes the per-edge counts from a caller's device buffer and, for FC_ALGO_LPM,
writes them as the new weights unchanged; with tau = 0 every edge is kept (a weight-0 edge too:
0 < 0 is false) and with no closure pairs the graph keeps its edges.  So the step API gives the
working graph any int32 weights, while the input graph stays the unit-weight graph that was loaded."""
import numpy as np

from tests.twin_graph import internal_graph

DELTA = 0.02


def weighted_engine(fcmod, n, edges, weight_of_edge, seed, n_p=1):
    """edges: [m][2] node ids.  weight_of_edge(u, v) -> one int32 weight per edge, for the node ids
    (u[i], v[i]) of the ends of the edges in the internal canonical order: the index space of
    fc_consensus_apply's buffer.  n_p: the n_p_total the two apply calls are given.
    Returns (engine, sigma = node_map(), (u, v, w) of the working graph read back, in node ids),
    after asserting that the graph kept its edges and carries the weights edge for edge."""
    import torch
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(n, edges[:, 0], edges[:, 1])
    u, v, w, _ = eng.get_graph()
    assert (w == 1).all()
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    # the internal canonical edge list: the index space of the partial buffer
    sigma = eng.node_map()
    lo, hi = np.minimum(sigma[u], sigma[v]), np.maximum(sigma[u], sigma[v])
    o = np.lexsort((hi, lo))
    weights = np.asarray(weight_of_edge(u[o], v[o]))
    assert weights.shape == (len(u),) and weights.dtype == np.int32 and (weights >= 0).all()
    part = torch.from_numpy(weights).to("cuda")
    eng.consensus_apply(1, n_p, 0.0, DELTA, part)           # tau 0: every edge kept, weight part[e]
    eng.closure_set_pairs(np.empty((0, 2), np.int32), 0)
    eng.closure_apply(1, n_p, DELTA, None, 0)
    g_int, sigma2 = internal_graph(eng, n)
    np.testing.assert_array_equal(sigma2, sigma)
    np.testing.assert_array_equal(g_int.u, lo[o])
    np.testing.assert_array_equal(g_int.v, hi[o])
    np.testing.assert_array_equal(g_int.w, weights)         # the weights written, edge for edge
    u2, v2, w2, _ = eng.get_graph()
    np.testing.assert_array_equal(np.bincount(np.concatenate([u2, v2]), minlength=n), deg)   # every row as it was
    return eng, sigma, (u2, v2, w2)
