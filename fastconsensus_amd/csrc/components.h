// components.h -- the consensus partition (fc_consensus_support / fc_consensus_partition): the
// connected components of the agreement graph, i.e. of the edges of G (or of the working graph)
// whose endpoints at least `agreement * n_total` labelings put in one community.
// Included at the end of consensus.hip after score.h (launch_pair_partial, the hipcub wrappers,
// ScLabT and the helpers of analysis.h are in scope).
//
// Components: a lock-free union-find over NODE ids (npos[internal vertex]).  Every vertex starts
// as its own parent; one thread per kept edge finds both roots with path halving and hooks the
// larger root under the smaller with a compare-and-swap, retrying from the value the failed swap
// returned.  A parent is only ever replaced by a smaller ancestor (parent[x] <= x throughout, a
// non-root never becomes a root again), so a stale read is still an ancestor: it costs a step,
// never a wrong answer, and the forest has no cycles.  One launch over the edge list whatever the
// graph's diameter.  After the flatten pass parent[t] is the smallest node id of t's component, so
// the labels (components numbered by their smallest node, fc_get_labels' renumber convention) do
// not depend on the order the atomics landed in.
#pragma once
#include <cstring>
#include <vector>

namespace fc {

static constexpr int CP_MAX_TOTAL = SC_MAX_REPLICAS;   // histogram bins in LDS: 4 (n_total + 2) bytes
static constexpr int CP_HIST_GRID = 1024;

// parents are read past L1 (relaxed, agent scope): a wave must not walk a stale line
__device__ __forceinline__ int32_t cp_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x as of the reads, halving the path behind it (atomicMin: parents only decrease)
__device__ __forceinline__ int32_t cp_find(int32_t* parent, int32_t x) {
    int32_t p = cp_load(parent + x);
    while (p != x) {
        const int32_t gp = cp_load(parent + p);
        if (gp == p) return p;
        atomicMin(parent + x, gp);
        x = gp;
        p = cp_load(parent + x);
    }
    return x;
}
// union the trees of a and b: find both roots, hook the larger under the smaller, and after a lost
// swap go on from the value it returned (the invariants are at the top of this file)
__device__ __forceinline__ void uf_hook(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = cp_find(parent, a);
        b = cp_find(parent, b);
        if (a == b) break;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) break;
        a = old;   // hi was hooked meanwhile: go on from its new parent
        b = lo;
    }
}

__global__ void k_cp_init(int64_t N, int32_t* parent) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) parent[t] = (int32_t)t;
}
// keep iff !((double)support < cut), the tau rule of k_consensus_apply; no kept list is built
__global__ __launch_bounds__(256) void k_cp_hook(int64_t m, const int32_t* __restrict__ eu,
                                                 const int32_t* __restrict__ ev, const int32_t* __restrict__ sup,
                                                 double cut, const int32_t* __restrict__ npos, int32_t* parent) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    if ((double)sup[e] < cut) return;
    uf_hook(parent, npos[eu[e]], npos[ev[e]]);
}
// parent[t] <- root of t; flag[t] = t is a root (flag[N] = 0 closes the scan)
__global__ void k_cp_flatten(int64_t N, int32_t* parent, int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > N) return;
    if (t == N) { flag[t] = 0; return; }
    int32_t r = (int32_t)t, p = cp_load(parent + r);
    while (p != r) { r = p; p = cp_load(parent + r); }
    __hip_atomic_store(parent + t, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[t] = r == (int32_t)t ? 1 : 0;
}
// label of node t = rank of its root among the roots in node order; the same labels by internal
// vertex for the row kernel; community sizes with one atomic per distinct label of a wave
__global__ __launch_bounds__(256) void k_cp_label(int64_t N, const int32_t* __restrict__ root,
                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ npos,
                                                  int32_t* __restrict__ lab, int32_t* __restrict__ labi,
                                                  int32_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool todo = i < N;
    int32_t l = -1;
    if (todo) {
        l = rank[root[i]];
        lab[i] = l;
        labi[i] = rank[root[npos[i]]];
    }
    for (;;) {   // wave-uniform: every lane takes every turn
        const unsigned long long rem = __ballot(todo);
        if (!rem) break;
        const int src = __ffsll((long long)rem) - 1;
        const int32_t lead = __shfl(l, src);
        const bool mine = todo && l == lead;
        const unsigned long long same = __ballot(mine);
        if (lane == src) atomicAdd(size + lead, (int32_t)__popcll(same));
        if (mine) todo = false;
    }
}
// largest community and the singletons: per block, then one sharded atomic per field
__global__ __launch_bounds__(256) void k_cp_size_stats(const int32_t* __restrict__ kp, const int32_t* __restrict__ size,
                                                       unsigned long long* counters) {
    __shared__ unsigned long long s_mx, s_one;
    if (threadIdx.x == 0) { s_mx = 0; s_one = 0; }
    __syncthreads();
    const int64_t cc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t s = cc < (int64_t)*kp ? size[cc] : 0;
    const unsigned long long ones = __ballot(s == 1);
    if (s > 1) atomicMax(&s_mx, (unsigned long long)s);
    if ((threadIdx.x & 63) == 0 && ones) atomicAdd(&s_one, (unsigned long long)__popcll(ones));
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_one && !s_mx) s_mx = 1;
        if (s_mx) atomicMax(shard(counters, 2, 0), s_mx);
        if (s_one) atomicAdd(shard(counters, 2, 1), s_one);
    }
}
// hist[s] for s in 0..nt, hist[nt + 1] = values outside [0, nt] (a caller's buffer is not trusted).
// Per-block LDS bins, one flush per block; a wave whose lanes agree adds once (consensus supports
// pile up at 0 and n_total).
__global__ __launch_bounds__(256) void k_cp_hist(int64_t m, const int32_t* __restrict__ sup, int nt,
                                                 unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned int s_cp_h[];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < nt + 2; i += blockDim.x) s_cp_h[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < m; e0 += stride) {   // block-uniform trip count
        const int64_t e = e0 + threadIdx.x;
        const bool in = e < m;
        const int bin = in ? support_bin(sup[e], nt) : -1;
        const unsigned long long act = __ballot(in);
        if (!act) continue;
        wave_bin_add(s_cp_h, in, bin, act, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt + 2; i += blockDim.x)
        if (s_cp_h[i]) atomicAdd(&hist[i], (unsigned long long)s_cp_h[i]);
}
// 16 lanes per CSR row: support through ceid, the neighbour's final label; the two sums of a row
// are folded inside its lane group (no atomics) and written at the vertex's node position
__global__ __launch_bounds__(256) void k_cp_node_sums(int64_t N, const int64_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const int32_t* __restrict__ ceid,
                                                      const int32_t* __restrict__ sup, const int32_t* __restrict__ labi,
                                                      const int32_t* __restrict__ npos, int64_t* __restrict__ nin,
                                                      int64_t* __restrict__ nout) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v = gid >> 4;
    const int l = (int)(gid & 15);
    if (v >= N) return;   // whole groups exit together
    const int64_t lo = rowptr[v], hi = rowptr[v + 1];
    const int32_t my = labi[v];
    long long a = 0, b = 0;
    for (int64_t j = lo + l; j < hi; j += 16) {
        const long long s = sup[ceid[j]];
        if (labi[col[j]] == my) a += s;
        else b += s;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 16);
        b += __shfl_xor(b, off, 16);
    }
    if (l == 0) {
        const int32_t t = npos[v];
        nin[t] = a;
        nout[t] = b;
    }
}

static const Graph& cp_graph(Ctx& c, int graph) { return graph == FC_SCORE_GRAPH_INPUT ? c.g0 : c.g; }

// support of every edge of the chosen graph over the local labelings (the count kernel of
// consensus_partial), in the graph's edge order
void consensus_support(Ctx& c, int graph, int32_t* out) {
    score_require(c);
    const Graph& g = cp_graph(c, graph);
    ScLabT lt(c);
    const int sl = timer_begin(c);
    launch_pair_partial<false>(c, g.m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), out);
    timer_end(c, TS_CONSENSUS, sl);
}

// The opening of consensus_partition and consensus_levels.  dev_support: null (counted here over the
// local labelings into cp_sup, n_total = n_r) or int32[m] reduced over n_total replicas; `what`
// names the caller in the replica-limit message.  Opens the call's consensus span and, when
// `first` is given, marks it before the count: the partition times the count as its first phase.
struct CpInput {
    const int32_t* sup;   // device, int32[m]
    int n_total;
    int span;             // timer_begin of the call
};
static CpInput cp_open(Ctx& c, const Graph& g, const int32_t* dev_support, int n_total, const char* what,
                       PhaseMarks* first = nullptr) {
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    if (!dev_support) {
        score_require(c);
        n_total = c.n_r;
    }
    FC_REQUIRE(n_total <= CP_MAX_TOTAL, FC_ELIMIT,
               std::string("the consensus ") + what + " handles at most 2048 replicas");
    CpInput in{dev_support, n_total, timer_begin(c)};
    if (first) first->mark();
    if (!in.sup) {
        int32_t* s = ensure<int32_t>(c.cp_sup, g.m + 1);
        ScLabT lt(c);
        launch_pair_partial<false>(c, g.m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), s);
        in.sup = s;
    }
    return in;
}

// dev_support as in cp_open.  Outputs (any may be null) are written only when everything succeeded.
void consensus_partition(Ctx& c, int graph, const int32_t* dev_support, int n_total, double agreement,
                         int32_t* labels_out, int64_t* hist_out, int64_t* nin_out, int64_t* nout_out,
                         fc_consensus_info* info) {
    const Graph& g = cp_graph(c, graph);
    const int64_t N = c.N, m = g.m;
    PhaseMarks ph(c, c.cp_ms);
    const CpInput in = cp_open(c, g, dev_support, n_total, "partition", &ph);
    const int32_t* sup = in.sup;
    n_total = in.n_total;
    const int sl = in.span;
    ph.mark();   // support
    const double cut = agreement * (double)n_total;   // float64 product, compared as in k_consensus_apply
    const int32_t* npos = c.npos.as<int32_t>();

    unsigned long long* hist = (unsigned long long*)ensure<uint64_t>(c.cp_hist, (size_t)n_total + 2);
    FC_HIP(hipMemsetAsync(hist, 0, sizeof(uint64_t) * ((size_t)n_total + 2), c.stream));
    if (m > 0)
        k_cp_hist<<<std::min<unsigned>(nblk(m), CP_HIST_GRID), TB, sizeof(unsigned int) * ((size_t)n_total + 2), c.stream>>>(
            m, sup, n_total, hist);
    ph.mark();   // histogram

    int32_t* parent = ensure<int32_t>(c.cp_parent, N + 1);
    int32_t* flag = ensure<int32_t>(c.cp_flag, N + 1);
    int32_t* rank = ensure<int32_t>(c.cp_rank, N + 1);
    int32_t* lab = ensure<int32_t>(c.cp_lab, N);
    int32_t* labi = ensure<int32_t>(c.cp_labi, N);
    int32_t* size = ensure<int32_t>(c.cp_size, N);
    k_cp_init<<<nblk(N), TB, 0, c.stream>>>(N, parent);
    int passes = 0;
    if (m > 0) {
        k_cp_hook<<<nblk(m), TB, 0, c.stream>>>(m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), sup, cut, npos, parent);
        passes = 1;
    }
    k_cp_flatten<<<nblk(N + 1), TB, 0, c.stream>>>(N, parent, flag);
    ph.mark();   // components
    exclusive_scan(c, (const int32_t*)flag, rank, N + 1);   // rank[N] = k
    FC_HIP(hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)N, c.stream));
    k_cp_label<<<nblk(N), TB, 0, c.stream>>>(N, parent, rank, npos, lab, labi, size);
    unsigned long long* ctr = shards_begin(c, 2);
    k_cp_size_stats<<<nblk(N), TB, 0, c.stream>>>(rank + N, size, ctr);
    ph.mark();   // renumber and sizes

    int64_t *nin = nullptr, *nout = nullptr;
    if (nin_out || nout_out) {
        nin = ensure<int64_t>(c.cp_nin, N);
        nout = ensure<int64_t>(c.cp_nout, N);
        if (m > 0)
            k_cp_node_sums<<<nblk(N * 16), TB, 0, c.stream>>>(N, g.rowptr.as<int64_t>(), g.col.as<int32_t>(),
                                                              g.ceid.as<int32_t>(), sup, labi, npos, nin, nout);
        else {
            FC_HIP(hipMemsetAsync(nin, 0, sizeof(int64_t) * (size_t)N, c.stream));
            FC_HIP(hipMemsetAsync(nout, 0, sizeof(int64_t) * (size_t)N, c.stream));
        }
    }
    ph.mark();   // node sums
    timer_end(c, TS_CONSENSUS, sl);

    std::vector<unsigned long long> h((size_t)n_total + 2);
    int32_t k = 0;
    FC_HIP(hipMemcpyAsync(h.data(), hist, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c.stream));
    FC_HIP(hipMemcpyAsync(&k, rank + N, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    int64_t st[2];
    shards_fold(c, 2, 1u, st);   // synchronises
    ph.collect();
    FC_REQUIRE(h[(size_t)n_total + 1] == 0, FC_EINVAL,
               std::to_string(h[(size_t)n_total + 1]) + " support values outside [0, n_total]");

    if (labels_out) FC_HIP(hipMemcpyAsync(labels_out, lab, sizeof(int32_t) * (size_t)N, hipMemcpyDefault, c.stream));
    if (nin_out) FC_HIP(hipMemcpyAsync(nin_out, nin, sizeof(int64_t) * (size_t)N, hipMemcpyDefault, c.stream));
    if (nout_out) FC_HIP(hipMemcpyAsync(nout_out, nout, sizeof(int64_t) * (size_t)N, hipMemcpyDefault, c.stream));
    sync(c);
    if (hist_out) std::memcpy(hist_out, h.data(), sizeof(int64_t) * ((size_t)n_total + 1));
    if (info) {
        int64_t kept = 0;
        for (int s = 0; s <= n_total; ++s)
            if (!((double)s < cut)) kept += (int64_t)h[s];
        info->edges = m;
        info->kept_edges = kept;
        info->unanimous_edges = (int64_t)h[n_total];
        info->split_edges = (int64_t)h[0];
        info->k = k;
        info->max_size = st[0];
        info->singletons = st[1];
        info->n_total = n_total;
        info->passes = passes;
        info->cut = cut;
    }
}

}  // namespace fc
