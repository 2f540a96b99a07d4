// levels.h -- the consensus hierarchy (fc_consensus_levels / fc_consensus_cut): the consensus
// partitions at EVERY agreement level from one union-find.  Level s (s = 0..n_total) is the
// connected components of the edges with support >= s; lowering s only adds edges, so the levels
// are nested and the union-find of components.h is CONTINUED from level n_total down to level 0
// instead of being restarted per threshold.
// Included at the end of consensus.hip after components.h (uf_hook, k_cp_hist, cp_graph, cp_open,
// the helpers of analysis.h and the scan wrapper are in scope).
//
// Edges are bucketed by support (counting sort on k_cp_hist's histogram).  For each nonempty
// level, from the top: one hook launch over that bucket's slice on the same parent array, then a
// flatten pass.  After a flatten parent[t] is the smallest node of t's component and
// parent[x] <= x still holds, so the next level's hooks start from a forest that satisfies every
// invariant components.h states.  The flatten also records the tree: a node that stops being a
// root at level s gets birth[t] = s, up[t] = its root, and adds its size and weighted degree sum
// into that root.  root_s(t), and with it birth, up and every label, is "the smallest node of a
// component": none of it depends on the order the atomics landed in.  The per-level integers are
// sums and maxima of terms whose total is order-independent (see k_lv_flatten).
#pragma once
#include <cstring>
#include <vector>

namespace fc {

static constexpr int LV_F = 7;          // per-level fields: absorbed roots, max size, lost singletons, 4 limbs
static constexpr int LV_GRID = 1024;    // bucket / join kernels: grid-stride blocks

// ------------------------------------------------------------------ bucket the edges by support
// bucket[cursor[bin] ...] <- edge ids, bin = support or nt + 1 for a value outside [0, nt] (its
// slice is the tail of the buffer; the host rejects the call when it is not empty).  A block
// counts its edges per bin in LDS (a wave whose lanes agree adds once), claims one range per
// touched bin, then ranks its edges inside the claimed ranges with LDS atomics.
__global__ __launch_bounds__(256) void k_lv_bucket(int64_t m, const int32_t* __restrict__ sup, int nt,
                                                   unsigned long long* __restrict__ cursor,
                                                   int32_t* __restrict__ bucket) {
    extern __shared__ unsigned int s_lv_b[];
    unsigned int* s_cnt = s_lv_b;                                                       // [nt + 2]
    unsigned long long* s_base = reinterpret_cast<unsigned long long*>(s_lv_b + ((nt + 3) & ~1));   // [nt + 2]
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < nt + 2; i += blockDim.x) s_cnt[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < m; e0 += stride) {   // block-uniform trip count
        const int64_t e = e0 + threadIdx.x;
        const bool in = e < m;
        const int bin = in ? support_bin(sup[e], nt) : -1;
        const unsigned long long act = __ballot(in);
        if (!act) continue;
        wave_bin_add(s_cnt, in, bin, act, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt + 2; i += blockDim.x) {
        const unsigned int n = s_cnt[i];
        if (n) s_base[i] = atomicAdd(&cursor[i], (unsigned long long)n);
        s_cnt[i] = 0;
    }
    __syncthreads();
    for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < m; e0 += stride) {
        const int64_t e = e0 + threadIdx.x;
        const bool in = e < m;
        const int bin = in ? support_bin(sup[e], nt) : -1;
        const unsigned long long act = __ballot(in);
        if (!act) continue;
        const unsigned int r = wave_bin_rank(s_cnt, in, bin, act, lane);
        if (in) bucket[s_base[bin] + r] = (int32_t)e;   // inside the bin's slice of [0, m)
    }
}

// ------------------------------------------------------------------ the continued union-find
// per node position of internal vertex v: its own parent, no birth, one member, its degree.
// The 128-bit sum of kdeg^2 (level "nothing merged") goes to row 0 of the statistics as limbs.
__global__ __launch_bounds__(256) void k_lv_init(int64_t N, const int32_t* __restrict__ npos,
                                                 const int64_t* __restrict__ kdeg, int32_t* __restrict__ parent,
                                                 int32_t* __restrict__ birth, int32_t* __restrict__ up,
                                                 int32_t* __restrict__ size, unsigned long long* __restrict__ tot,
                                                 unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_l[4];
    if (threadIdx.x < 4) s_l[threadIdx.x] = 0;
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < N) {
        const int32_t t = npos[v];
        const unsigned long long d = (unsigned long long)kdeg[v];
        parent[t] = t;
        birth[t] = -1;
        up[t] = t;
        size[t] = 1;
        tot[t] = d;
        if (d) {
            const unsigned long long lo = d * d, hi = __umul64hi(d, d);
            atomicAdd(&s_l[0], lo & 0xffffffffull);
            atomicAdd(&s_l[1], lo >> 32);
            atomicAdd(&s_l[2], hi & 0xffffffffull);
            atomicAdd(&s_l[3], hi >> 32);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_l[threadIdx.x]) atomicAdd(shard(stats, LV_F, 3 + threadIdx.x), s_l[threadIdx.x]);
}
// k_cp_hook over one bucket's slice of edge ids: the same union-find (uf_hook), continued
__global__ __launch_bounds__(256) void k_lv_hook(int64_t cnt, const int32_t* __restrict__ ids,
                                                 const int32_t* __restrict__ eu, const int32_t* __restrict__ ev,
                                                 const int32_t* __restrict__ npos, int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const int32_t e = ids[i];
    uf_hook(parent, npos[eu[e]], npos[ev[e]]);
}
// parent[t] <- root of t.  A node without a birth that is no root any more was a root until this
// level: it is born at s under its root and hands over its members and degree sum.  The forest
// does not change during this kernel (the hooks are a launch behind), so the receivers are the
// level's roots and the givers' totals are final.  The returned old values depend on the order of
// the adds, the level's integers do not: a receiver's last add returns its final size less the
// addend (the maximum of old + addend over all adds is the largest grown community); exactly one
// add finds a receiver that was a singleton; and the sum of old * addend over a receiver's adds is
// ((sum)^2 - sum of squares) / 2 whatever the order -- the growth of sum tot^2, kept as 32-bit
// limbs so that no 64-bit counter overflows.
__global__ __launch_bounds__(256) void k_lv_flatten(int64_t N, int32_t s, int32_t* parent, int32_t* __restrict__ birth,
                                                    int32_t* __restrict__ up, int32_t* size, unsigned long long* tot,
                                                    unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_f[LV_F];
    if (threadIdx.x < LV_F) s_f[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) {
        int32_t r = (int32_t)t, p = cp_load(parent + r);
        while (p != r) { r = p; p = cp_load(parent + r); }
        if (r != (int32_t)t) {
            __hip_atomic_store(parent + t, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (birth[t] < 0) {
                birth[t] = s;
                up[t] = r;
                const int32_t mine = size[t];
                const unsigned long long d = tot[t];
                const int32_t old = atomicAdd(size + r, mine);
                atomicAdd(&s_f[0], 1ull);
                atomicMax(&s_f[1], (unsigned long long)(old + mine));
                const unsigned long long gone = (mine == 1 ? 1ull : 0ull) + (old == 1 ? 1ull : 0ull);
                if (gone) atomicAdd(&s_f[2], gone);
                if (d) {
                    const unsigned long long o = atomicAdd(tot + r, d);
                    const unsigned long long lo = o * d, hi = __umul64hi(o, d);
                    if (lo | hi) {
                        atomicAdd(&s_f[3], lo & 0xffffffffull);
                        atomicAdd(&s_f[4], lo >> 32);
                        atomicAdd(&s_f[5], hi & 0xffffffffull);
                        atomicAdd(&s_f[6], hi >> 32);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < LV_F && s_f[threadIdx.x]) {
        if (threadIdx.x == 1) atomicMax(shard(stats, LV_F, 1), s_f[1]);
        else atomicAdd(shard(stats, LV_F, threadIdx.x), s_f[threadIdx.x]);
    }
}
// out[row][f] <- the fold of row's CSH shards (field 1: maximum); one block per row
__global__ __launch_bounds__(CSH) void k_lv_fold(const unsigned long long* __restrict__ stats,
                                                 unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s[CSH];
    const unsigned long long* base = stats + (size_t)blockIdx.x * CSH * LV_F;
    for (int f = 0; f < LV_F; ++f) {
        s[threadIdx.x] = base[(size_t)threadIdx.x * LV_F + f];
        __syncthreads();
        for (int o = CSH / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                const unsigned long long a = s[threadIdx.x], b = s[threadIdx.x + o];
                s[threadIdx.x] = f == 1 ? (a > b ? a : b) : a + b;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * LV_F + f] = s[0];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ join levels
// j(e) = the largest level at which e's ends share a component: walk the tree from both ends,
// always stepping the end that was born later (birth[up[x]] < birth[x], so at most 2 (nt + 1)
// steps); the smallest birth passed is the level of the last merge needed.  The edge's weight is
// added to bin j(e): LDS bins, one flush per block.  UNIT: no weight loads.
template <bool UNIT>
__global__ __launch_bounds__(256) void k_lv_join(int64_t m, const int32_t* __restrict__ eu,
                                                 const int32_t* __restrict__ ev, const int32_t* __restrict__ ew,
                                                 const int32_t* __restrict__ npos, const int32_t* __restrict__ birth,
                                                 const int32_t* __restrict__ up, int nt,
                                                 unsigned long long* __restrict__ jw) {
    extern __shared__ unsigned long long s_lv_j[];
    for (int i = threadIdx.x; i <= nt; i += blockDim.x) s_lv_j[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        int32_t a = npos[eu[e]], b = npos[ev[e]];
        int32_t ba = birth[a], bb = birth[b], j = nt;
        while (a != b) {
            if (ba >= bb) {
                if (ba < 0) { j = -1; break; }   // two roots of H: never joined
                j = j < ba ? j : ba;
                a = up[a];
                ba = birth[a];
            } else {
                j = j < bb ? j : bb;
                b = up[b];
                bb = birth[b];
            }
        }
        if (j >= 0) atomicAdd(&s_lv_j[j], UNIT ? 1ull : (unsigned long long)ew[e]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= nt; i += blockDim.x)
        if (s_lv_j[i]) atomicAdd(&jw[i], s_lv_j[i]);
}

// ------------------------------------------------------------------ cut
// root[t] = root_s(t): follow up while the node was born at s or above; flag[t] = t is a root
// (flag[N] = 0 closes the scan)
__global__ void k_lv_cut(int64_t N, int32_t s, const int32_t* __restrict__ birth, const int32_t* __restrict__ up,
                         int32_t* __restrict__ root, int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > N) return;
    if (t == N) { flag[t] = 0; return; }
    int32_t x = (int32_t)t;
    while (birth[x] >= s) x = up[x];
    root[t] = x;
    flag[t] = x == (int32_t)t ? 1 : 0;
}
__global__ void k_lv_label(int64_t N, const int32_t* __restrict__ root, const int32_t* __restrict__ rank,
                           int32_t* __restrict__ lab) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) lab[t] = rank[root[t]];
}

// fc_part_score's modularity from the exact integers, rounded at the division
static double lv_modularity(int64_t in_weight, unsigned __int128 tot_sq, int64_t M2) {
    if (M2 == 0) return 0.0;
    const unsigned __int128 W2 = (unsigned __int128)(uint64_t)M2;
    const __int128 num = (__int128)(2 * (unsigned __int128)(uint64_t)in_weight * W2) - (__int128)tot_sq;
    return (double)((long double)num / (long double)(W2 * W2));
}

// dev_support as in cp_open.  The tree stays in the context (lv_birth / lv_up) for
// consensus_cut; outputs (any may be null) are written only when everything succeeded.
void consensus_levels(Ctx& c, int graph, const int32_t* dev_support, int n_total, int32_t* birth_out, int32_t* up_out,
                      fc_level_score* levels_out, int32_t* best_out) {
    const Graph& g = cp_graph(c, graph);
    const int64_t N = c.N, m = g.m;
    const CpInput in = cp_open(c, g, dev_support, n_total, "hierarchy");   // the count is outside the phases
    const int32_t* sup = in.sup;
    const int nt = in.n_total, sl = in.span;
    PhaseMarks ph(c, c.lv_ms);
    ph.mark();
    const int32_t* npos = c.npos.as<int32_t>();
    const int32_t *eu = g.eu.as<int32_t>(), *ev = g.ev.as<int32_t>();

    // histogram -> slice offsets (the scan wrapper) -> scatter
    unsigned long long* hist = (unsigned long long*)ensure<uint64_t>(c.cp_hist, (size_t)nt + 3);
    unsigned long long* cursor = (unsigned long long*)ensure<uint64_t>(c.lv_cursor, (size_t)nt + 3);
    int32_t* bucket = ensure<int32_t>(c.lv_bucket, m + 1);
    FC_HIP(hipMemsetAsync(hist, 0, sizeof(uint64_t) * ((size_t)nt + 3), c.stream));
    const unsigned egrid = std::min<unsigned>(nblk(m), LV_GRID);
    if (m > 0)
        k_cp_hist<<<std::min<unsigned>(nblk(m), CP_HIST_GRID), TB, sizeof(unsigned int) * ((size_t)nt + 2), c.stream>>>(
            m, sup, nt, hist);
    exclusive_scan(c, (const int64_t*)hist, (int64_t*)cursor, (int64_t)nt + 3);
    if (m > 0)
        k_lv_bucket<<<egrid, TB, sizeof(unsigned int) * (size_t)((nt + 3) & ~1) + sizeof(uint64_t) * ((size_t)nt + 2),
                      c.stream>>>(m, sup, nt, cursor, bucket);
    std::vector<unsigned long long> h((size_t)nt + 2);
    FC_HIP(hipMemcpyAsync(h.data(), hist, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c.stream));
    sync(c);   // the host skips the empty levels
    if (h[(size_t)nt + 1] != 0) {
        timer_end(c, TS_CONSENSUS, sl);
        FC_REQUIRE(false, FC_EINVAL, std::to_string(h[(size_t)nt + 1]) + " support values outside [0, n_total]");
    }
    ph.mark();   // bucket

    std::vector<int> live;   // nonempty levels from the top
    for (int s = nt; s >= 0; --s)
        if (h[s]) live.push_back(s);
    const size_t rows = live.size() + 1;   // row 0: nothing merged
    c.lv_valid = false;
    int32_t* parent = ensure<int32_t>(c.cp_parent, N + 1);
    int32_t* birth = ensure<int32_t>(c.lv_birth, N + 1);
    int32_t* up = ensure<int32_t>(c.lv_up, N + 1);
    int32_t* size = ensure<int32_t>(c.cp_size, N);
    unsigned long long* tot = (unsigned long long*)ensure<uint64_t>(c.lv_tot, N);
    unsigned long long* stats = (unsigned long long*)ensure<uint64_t>(c.lv_stats, rows * CSH * LV_F);
    unsigned long long* folded = (unsigned long long*)ensure<uint64_t>(c.lv_fold, rows * LV_F);
    unsigned long long* jw = (unsigned long long*)ensure<uint64_t>(c.lv_jw, (size_t)nt + 1);
    FC_HIP(hipMemsetAsync(stats, 0, sizeof(uint64_t) * rows * CSH * LV_F, c.stream));
    k_lv_init<<<nblk(N), TB, 0, c.stream>>>(N, npos, g.kdeg.as<int64_t>(), parent, birth, up, size, tot, stats);
    {
        std::vector<unsigned long long> off((size_t)nt + 2, 0);
        for (int s = 0; s <= nt; ++s) off[s + 1] = off[s] + h[s];
        for (size_t i = 0; i < live.size(); ++i) {
            const int s = live[i];
            const int64_t cnt = (int64_t)h[s];
            k_lv_hook<<<nblk(cnt), TB, 0, c.stream>>>(cnt, bucket + off[s], eu, ev, npos, parent);
            k_lv_flatten<<<nblk(N), TB, 0, c.stream>>>(N, s, parent, birth, up, size, tot,
                                                       stats + (i + 1) * (size_t)CSH * LV_F);
        }
    }
    ph.mark();   // tree
    k_lv_fold<<<(unsigned)rows, CSH, 0, c.stream>>>(stats, folded);
    std::vector<unsigned long long> st(rows * LV_F);
    FC_HIP(hipMemcpyAsync(st.data(), folded, sizeof(uint64_t) * st.size(), hipMemcpyDeviceToHost, c.stream));
    ph.mark();   // statistics
    FC_HIP(hipMemsetAsync(jw, 0, sizeof(uint64_t) * ((size_t)nt + 1), c.stream));
    if (m > 0) {
        const size_t lds = sizeof(uint64_t) * ((size_t)nt + 1);
        if (unit_weights(g)) k_lv_join<true><<<egrid, TB, lds, c.stream>>>(m, eu, ev, nullptr, npos, birth, up, nt, jw);
        else k_lv_join<false><<<egrid, TB, lds, c.stream>>>(m, eu, ev, g.ew.as<int32_t>(), npos, birth, up, nt, jw);
    }
    std::vector<unsigned long long> hj((size_t)nt + 1);
    FC_HIP(hipMemcpyAsync(hj.data(), jw, sizeof(uint64_t) * hj.size(), hipMemcpyDeviceToHost, c.stream));
    ph.mark();   // join levels
    timer_end(c, TS_CONSENSUS, sl);
    sync(c);
    ph.collect();
    c.lv_valid = true;
    c.lv_nt = nt;

    // the records, from the top level down: a nonempty level applies its row, an empty one repeats
    auto limbs = [](const unsigned long long* p) {
        return (unsigned __int128)p[3] + ((unsigned __int128)p[4] << 32) + ((unsigned __int128)p[5] << 64) +
               ((unsigned __int128)p[6] << 96);
    };
    std::vector<fc_level_score> rec((size_t)nt + 1);
    int64_t k = N, mx = 1, single = N, inw = 0;
    unsigned __int128 tsq = limbs(&st[0]);
    size_t row = 0;
    int best = nt;
    __int128 best_key = 0;
    const unsigned __int128 W2 = (unsigned __int128)(uint64_t)g.M2;
    for (int s = nt; s >= 0; --s) {
        if (h[s]) {
            const unsigned long long* p = &st[(++row) * LV_F];
            k -= (int64_t)p[0];
            mx = std::max<int64_t>(mx, (int64_t)p[1]);
            single -= (int64_t)p[2];
            tsq += 2 * limbs(p);
        }
        inw += (int64_t)hj[s];
        fc_level_score& o = rec[s];
        o.bucket_edges = (int64_t)h[s];
        o.k = k; o.max_size = mx; o.singletons = single; o.in_weight = inw;
        o.tot_sq_lo = (uint64_t)tsq; o.tot_sq_hi = (uint64_t)(tsq >> 64);
        o.modularity = lv_modularity(inw, tsq, g.M2);
        const __int128 key = (__int128)(2 * (unsigned __int128)(uint64_t)inw * W2) - (__int128)tsq;
        if (s == nt || key > best_key) { best = s; best_key = key; }   // descending: ties stay at the highest level
    }

    if (birth_out) FC_HIP(hipMemcpyAsync(birth_out, birth, sizeof(int32_t) * (size_t)N, hipMemcpyDefault, c.stream));
    if (up_out) FC_HIP(hipMemcpyAsync(up_out, up, sizeof(int32_t) * (size_t)N, hipMemcpyDefault, c.stream));
    sync(c);
    if (levels_out) std::memcpy(levels_out, rec.data(), sizeof(fc_level_score) * rec.size());
    if (best_out) *best_out = best;
}

// labels of level `level` of the tree in the context (validated by the caller)
void consensus_cut(Ctx& c, int level, int32_t* labels_out, int64_t* k_out) {
    const int64_t N = c.N;
    int32_t* root = ensure<int32_t>(c.cp_parent, N + 1);
    int32_t* flag = ensure<int32_t>(c.cp_flag, N + 1);
    int32_t* rank = ensure<int32_t>(c.cp_rank, N + 1);
    int32_t* lab = ensure<int32_t>(c.cp_lab, N);
    const int sl = timer_begin(c);
    k_lv_cut<<<nblk(N + 1), TB, 0, c.stream>>>(N, level, c.lv_birth.as<int32_t>(), c.lv_up.as<int32_t>(), root, flag);
    exclusive_scan(c, (const int32_t*)flag, rank, N + 1);   // rank[N] = k
    k_lv_label<<<nblk(N), TB, 0, c.stream>>>(N, root, rank, lab);
    timer_end(c, TS_CONSENSUS, sl);
    int32_t k = 0;
    FC_HIP(hipMemcpyAsync(&k, rank + N, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    if (labels_out) FC_HIP(hipMemcpyAsync(labels_out, lab, sizeof(int32_t) * (size_t)N, hipMemcpyDefault, c.stream));
    sync(c);
    if (k_out) *k_out = k;
}

}  // namespace fc
