// quality.h -- community quality of a given partition P on a graph H (fc_community_quality): per
// cluster its volume, internal weight and edges, smallest internal degree and connected parts; per
// node the weight it sends inside and outside its cluster; P split into the connected parts.
// A property of H and P alone: no labelings are read, nothing of the context's state is written.
// Included by consensus.hip after components.h (its union-find, k_cp_init / k_cp_flatten /
// k_cp_label and cp_graph, analysis.h's PhaseMarks and the hipcub wrappers are in scope).
//
// Everything is an integer and every combination is a sum, a minimum or a maximum, so no result
// depends on the order the atomics land in.  Four phases:
//   labels      P to the device, presence flags over the id space [0, n) and their exclusive scan
//               (the rank of every id and K, no sort), then k_cp_label with root = P: dense cluster
//               ranks by node and by internal vertex, and the sizes from its leader loop.
//   rows        one pass over the CSR of H, 16 lanes per row (k_cp_node_sums' shape): weight to the
//               same cluster, weight to the others, number of same-cluster neighbours.
//   fold        the per-vertex values to per-cluster sums: a wave takes 64 vertices in STORAGE
//               order (Ctx::sinv) and adds once per distinct cluster among them (leader loop).
//   components  the union-find of components.h over the edges inside a cluster, k_cp_label once
//               more (root = the flattened parents) for the split partition and the part sizes,
//               one add and one max per part, then the records and the sharded totals.
#pragma once
#include <vector>

namespace fc {

static constexpr int QL_F = 5;   // sharded totals: max size (max), singletons, disconnected, 2 in_weight, 2 cut_weight

template <class Op> __device__ __forceinline__ long long ql_wave_fold(long long x, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = op(x, __shfl_xor(x, o));
    return x;
}
struct QlSum { __device__ long long operator()(long long a, long long b) const { return a + b; } };
struct QlMin { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };
struct QlMax { __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };

// present[id] = 1 for every id P uses (every writer stores the same value)
__global__ void k_ql_present(int64_t N, const int32_t* __restrict__ in, int32_t* present) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) present[in[t]] = 1;
}
// ids[rank of id] = id: the clusters' ids, ascending
__global__ void k_ql_ids(int64_t N, const int32_t* __restrict__ present, const int32_t* __restrict__ rank,
                         int32_t* __restrict__ ids) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N && present[t]) ids[rank[t]] = (int32_t)t;
}

// 16 lanes per CSR row; the three sums of a row are folded inside its lane group (no atomics).
// nin / nout (either may be null) at the vertex's node position, vin / vout / vcnt by internal
// vertex.  UNIT: every weight is 1, no weight loads.  A row of degree 0 writes three zeros.
template <bool UNIT>
__global__ __launch_bounds__(256) void k_ql_rows(int64_t N, const int64_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ col, const int32_t* __restrict__ cw,
                                                 const int32_t* __restrict__ labi, const int32_t* __restrict__ npos,
                                                 int64_t* __restrict__ nin, int64_t* __restrict__ nout,
                                                 int64_t* __restrict__ vin, int64_t* __restrict__ vout,
                                                 int32_t* __restrict__ vcnt) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v = gid >> 4;
    const int l = (int)(gid & 15);
    if (v >= N) return;   // whole groups exit together
    const int64_t lo = rowptr[v], hi = rowptr[v + 1];
    const int32_t my = labi[v];
    long long a = 0, b = 0;
    int n = 0;
    for (int64_t j = lo + l; j < hi; j += 16) {
        const long long w = UNIT ? 1 : (long long)cw[j];
        if (labi[col[j]] == my) { a += w; ++n; }
        else b += w;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 16);
        b += __shfl_xor(b, off, 16);
        n += __shfl_xor(n, off, 16);
    }
    if (l == 0) {
        const int32_t t = npos[v];
        if (nin) nin[t] = a;
        if (nout) nout[t] = b;
        vin[v] = a;
        vout[v] = b;
        vcnt[v] = n;
    }
}

// Per-cluster sums of the per-vertex values.  Thread i takes the vertex of storage slot i: the
// slots follow the communities of the ordering pass, so the 64 vertices of a wave lie in few
// clusters of any partition that resembles the graph's structure.  One turn per distinct cluster
// of the wave: its first lane adds the group's sums (and takes the minimum) once.
__global__ __launch_bounds__(256) void k_ql_fold(int64_t N, const int32_t* __restrict__ sinv,
                                                 const int32_t* __restrict__ labi, const int64_t* __restrict__ vin,
                                                 const int64_t* __restrict__ vout, const int32_t* __restrict__ vcnt,
                                                 unsigned long long* __restrict__ vol,
                                                 unsigned long long* __restrict__ in2,
                                                 unsigned long long* __restrict__ ie2,
                                                 unsigned long long* __restrict__ mind) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool todo = i < N;
    int32_t l = -1;
    long long a = 0, d = 0, n = 0;
    if (todo) {
        const int32_t v = sinv[i];
        l = labi[v];
        a = vin[v];
        d = a + vout[v];
        n = vcnt[v];
    }
    for (;;) {   // wave-uniform: every lane takes every turn
        const unsigned long long rem = __ballot(todo);
        if (!rem) break;
        const int src = __ffsll((long long)rem) - 1;
        const int32_t lead = __shfl(l, src);
        const bool mine = todo && l == lead;
        const unsigned long long same = __ballot(mine);
        long long sd = mine ? d : 0, sa = mine ? a : 0, sn = mine ? n : 0, mn = mine ? n : 0x7fffffffffffffffll;
        if (__popcll(same) > 1) {   // wave-uniform
            sd = ql_wave_fold(sd, QlSum());
            sa = ql_wave_fold(sa, QlSum());
            sn = ql_wave_fold(sn, QlSum());
            mn = ql_wave_fold(mn, QlMin());
        }
        if (lane == src) {
            if (sd) atomicAdd(vol + lead, (unsigned long long)sd);
            if (sa) atomicAdd(in2 + lead, (unsigned long long)sa);
            if (sn) atomicAdd(ie2 + lead, (unsigned long long)sn);
            atomicMin(mind + lead, (unsigned long long)mn);
        }
        if (mine) todo = false;
    }
}

// the edges of H inside a cluster join their ends (components.h's union-find over node ids)
__global__ __launch_bounds__(256) void k_ql_hook(int64_t m, const int32_t* __restrict__ eu,
                                                 const int32_t* __restrict__ ev, const int32_t* __restrict__ labi,
                                                 const int32_t* __restrict__ npos, int32_t* parent) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const int32_t u = eu[e], v = ev[e];
    if (labi[u] != labi[v]) return;
    uf_hook(parent, npos[u], npos[v]);
}
// Per root t (flag[t], node order): one more part of t's cluster, and the part's size against the
// cluster's largest; the roots of a wave that share a cluster add and compare once.
__global__ __launch_bounds__(256) void k_ql_parts(int64_t N, const int32_t* __restrict__ flag,
                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ lab,
                                                  const int32_t* __restrict__ psize,
                                                  unsigned long long* __restrict__ comp,
                                                  unsigned long long* __restrict__ largest) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool todo = i < N && flag[i] != 0;
    int32_t l = -1;
    long long s = 0;
    if (todo) {
        l = lab[i];
        s = psize[rank[i]];
    }
    for (;;) {   // wave-uniform
        const unsigned long long rem = __ballot(todo);
        if (!rem) break;
        const int src = __ffsll((long long)rem) - 1;
        const int32_t lead = __shfl(l, src);
        const bool mine = todo && l == lead;
        const unsigned long long same = __ballot(mine);
        long long mx = mine ? s : 0;
        if (__popcll(same) > 1) mx = ql_wave_fold(mx, QlMax());
        if (lane == src) {
            atomicAdd(comp + lead, (unsigned long long)__popcll(same));
            atomicMax(largest + lead, (unsigned long long)mx);
        }
        if (mine) todo = false;
    }
}
// One record per cluster, and the totals: per wave, then per block in LDS, then one sharded atomic
// per field (counters: QL_F fields).
__global__ __launch_bounds__(256) void k_ql_records(const int32_t* __restrict__ kp, const int32_t* __restrict__ ids,
                                                    const int32_t* __restrict__ size,
                                                    const unsigned long long* __restrict__ vol,
                                                    const unsigned long long* __restrict__ in2,
                                                    const unsigned long long* __restrict__ ie2,
                                                    const unsigned long long* __restrict__ mind,
                                                    const unsigned long long* __restrict__ comp,
                                                    const unsigned long long* __restrict__ largest,
                                                    fc_community_record* __restrict__ rec,
                                                    unsigned long long* counters) {
    __shared__ unsigned long long s_t[QL_F];
    if (threadIdx.x < QL_F) s_t[threadIdx.x] = 0;
    __syncthreads();
    const int64_t cc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = cc < (int64_t)*kp;
    long long sz = 0, one = 0, dis = 0, a = 0, cut = 0;
    if (in) {
        fc_community_record r;
        r.id = ids[cc];
        r.size = sz = size[cc];
        r.volume = (int64_t)vol[cc];
        r.in_weight = (int64_t)(in2[cc] >> 1);
        r.in_edges = (int64_t)(ie2[cc] >> 1);
        r.min_in_degree = (int64_t)mind[cc];
        r.components = (int64_t)comp[cc];
        r.largest_component = (int64_t)largest[cc];
        rec[cc] = r;
        one = sz == 1;
        dis = r.components > 1;
        a = (long long)in2[cc];
        cut = (long long)(vol[cc] - in2[cc]);
    }
    sz = ql_wave_fold(sz, QlMax());
    one = ql_wave_fold(one, QlSum());
    dis = ql_wave_fold(dis, QlSum());
    a = ql_wave_fold(a, QlSum());
    cut = ql_wave_fold(cut, QlSum());
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&s_t[0], (unsigned long long)sz);
        if (one) atomicAdd(&s_t[1], (unsigned long long)one);
        if (dis) atomicAdd(&s_t[2], (unsigned long long)dis);
        if (a) atomicAdd(&s_t[3], (unsigned long long)a);
        if (cut) atomicAdd(&s_t[4], (unsigned long long)cut);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_t[0]) atomicMax(shard(counters, QL_F, 0), s_t[0]);
#pragma unroll
        for (int f = 1; f < QL_F; ++f)
            if (s_t[f]) atomicAdd(shard(counters, QL_F, f), s_t[f]);
    }
}

// labels: host int32[N] in node order, ids in [0, N), validated by the caller.  Any output may be
// null; a phase nothing asks for does not run.  Outputs are written only when everything succeeded.
void community_quality(Ctx& c, int graph, const int32_t* labels, fc_community_record* out, int64_t* nin_out,
                       int64_t* nout_out, int32_t* split_out, fc_quality_info* info) {
    const Graph& g = cp_graph(c, graph);
    const int64_t N = c.N, m = g.m;
    const bool want_rec = out || info, want_rows = want_rec || nin_out || nout_out, want_comp = want_rec || split_out;
    const int32_t* npos = c.npos.as<int32_t>();
    PhaseMarks ph(c, c.ql_ms);
    const int sl = timer_begin(c);
    ph.mark();

    int32_t* in = ensure<int32_t>(c.st_lab, N + 1);
    FC_HIP(hipMemcpyAsync(in, labels, 4 * (size_t)N, hipMemcpyHostToDevice, c.stream));
    int32_t* present = ensure<int32_t>(c.ql_present, N + 1);
    int32_t* idrank = ensure<int32_t>(c.ql_rank, N + 1);
    int32_t* ids = ensure<int32_t>(c.ql_ids, N);
    int32_t* lab = ensure<int32_t>(c.ql_lab, N);
    int32_t* labi = ensure<int32_t>(c.ql_labi, N);
    int32_t* size = ensure<int32_t>(c.ql_size, N);
    FC_HIP(hipMemsetAsync(present, 0, sizeof(int32_t) * (size_t)(N + 1), c.stream));
    k_ql_present<<<nblk(N), TB, 0, c.stream>>>(N, in, present);
    exclusive_scan(c, (const int32_t*)present, idrank, N + 1);   // idrank[N] = K
    k_ql_ids<<<nblk(N), TB, 0, c.stream>>>(N, present, idrank, ids);
    FC_HIP(hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)N, c.stream));
    k_cp_label<<<nblk(N), TB, 0, c.stream>>>(N, in, idrank, npos, lab, labi, size);   // root = P: ranks and sizes
    ph.mark();   // labels

    int64_t *nin = nullptr, *nout = nullptr, *vin = nullptr, *vout = nullptr;
    int32_t* vcnt = nullptr;
    if (want_rows) {
        if (nin_out) nin = ensure<int64_t>(c.ql_nin, N);
        if (nout_out) nout = ensure<int64_t>(c.ql_nout, N);
        vin = ensure<int64_t>(c.ql_vin, N);
        vout = ensure<int64_t>(c.ql_vout, N);
        vcnt = ensure<int32_t>(c.ql_vcnt, N);
        if (m == 0) {
            if (nin) FC_HIP(hipMemsetAsync(nin, 0, sizeof(int64_t) * (size_t)N, c.stream));
            if (nout) FC_HIP(hipMemsetAsync(nout, 0, sizeof(int64_t) * (size_t)N, c.stream));
            FC_HIP(hipMemsetAsync(vin, 0, sizeof(int64_t) * (size_t)N, c.stream));
            FC_HIP(hipMemsetAsync(vout, 0, sizeof(int64_t) * (size_t)N, c.stream));
            FC_HIP(hipMemsetAsync(vcnt, 0, sizeof(int32_t) * (size_t)N, c.stream));
        } else if (unit_weights(g))
            k_ql_rows<true><<<nblk(N * 16), TB, 0, c.stream>>>(N, g.rowptr.as<int64_t>(), g.col.as<int32_t>(), nullptr,
                                                               labi, npos, nin, nout, vin, vout, vcnt);
        else
            k_ql_rows<false><<<nblk(N * 16), TB, 0, c.stream>>>(N, g.rowptr.as<int64_t>(), g.col.as<int32_t>(),
                                                                g.cw.as<int32_t>(), labi, npos, nin, nout, vin, vout,
                                                                vcnt);
    }
    ph.mark();   // rows

    // per-cluster accumulators: volume, 2 in_weight, 2 in_edges, components, largest part (zeroed), min degree (all ones)
    unsigned long long* acc = nullptr;
    if (want_rec) {
        acc = (unsigned long long*)ensure<uint64_t>(c.ql_acc, (size_t)6 * N);
        FC_HIP(hipMemsetAsync(acc, 0, sizeof(uint64_t) * (size_t)5 * N, c.stream));
        FC_HIP(hipMemsetAsync(acc + 5 * N, 0xff, sizeof(uint64_t) * (size_t)N, c.stream));
        k_ql_fold<<<nblk(N), TB, 0, c.stream>>>(N, c.sinv.as<int32_t>(), labi, vin, vout, vcnt, acc, acc + N, acc + 2 * N,
                                                acc + 5 * N);
    }
    ph.mark();   // fold

    int32_t *rank = nullptr, *split = nullptr;
    if (want_comp) {
        int32_t* parent = ensure<int32_t>(c.cp_parent, N + 1);
        int32_t* flag = ensure<int32_t>(c.cp_flag, N + 1);
        rank = ensure<int32_t>(c.cp_rank, N + 1);
        split = ensure<int32_t>(c.ql_split, N);
        int32_t* spliti = ensure<int32_t>(c.cp_labi, N);   // k_cp_label's labels by internal vertex: not used here
        int32_t* psize = ensure<int32_t>(c.ql_psize, N);
        k_cp_init<<<nblk(N), TB, 0, c.stream>>>(N, parent);
        if (m > 0) k_ql_hook<<<nblk(m), TB, 0, c.stream>>>(m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), labi, npos, parent);
        k_cp_flatten<<<nblk(N + 1), TB, 0, c.stream>>>(N, parent, flag);
        exclusive_scan(c, (const int32_t*)flag, rank, N + 1);   // rank[N] = parts
        FC_HIP(hipMemsetAsync(psize, 0, sizeof(int32_t) * (size_t)N, c.stream));
        k_cp_label<<<nblk(N), TB, 0, c.stream>>>(N, parent, rank, npos, split, spliti, psize);
        if (want_rec) k_ql_parts<<<nblk(N), TB, 0, c.stream>>>(N, flag, rank, lab, psize, acc + 3 * N, acc + 4 * N);
    }
    fc_community_record* rec = nullptr;
    if (want_rec) {
        rec = (fc_community_record*)ensure<uint64_t>(c.ql_rec, (size_t)N * (sizeof(fc_community_record) / 8));
        unsigned long long* ctr = shards_begin(c, QL_F);
        k_ql_records<<<nblk(N), TB, 0, c.stream>>>(idrank + N, ids, size, acc, acc + N, acc + 2 * N, acc + 5 * N,
                                                   acc + 3 * N, acc + 4 * N, rec, ctr);
    }
    ph.mark();   // components
    timer_end(c, TS_CONSENSUS, sl);

    int32_t k = 0, parts = 0;
    int64_t st[QL_F] = {};
    FC_HIP(hipMemcpyAsync(&k, idrank + N, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    if (want_comp) FC_HIP(hipMemcpyAsync(&parts, rank + N, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    if (want_rec) shards_fold(c, QL_F, 1u, st);   // synchronises
    else sync(c);
    ph.collect();

    if (out) FC_HIP(hipMemcpyAsync(out, rec, sizeof(fc_community_record) * (size_t)k, hipMemcpyDeviceToHost, c.stream));
    if (nin_out) FC_HIP(hipMemcpyAsync(nin_out, nin, sizeof(int64_t) * (size_t)N, hipMemcpyDefault, c.stream));
    if (nout_out) FC_HIP(hipMemcpyAsync(nout_out, nout, sizeof(int64_t) * (size_t)N, hipMemcpyDefault, c.stream));
    if (split_out) FC_HIP(hipMemcpyAsync(split_out, split, sizeof(int32_t) * (size_t)N, hipMemcpyDefault, c.stream));
    sync(c);
    if (info) {
        *info = fc_quality_info{};
        info->k = k;
        info->max_size = st[0];
        info->singletons = st[1];
        info->parts = parts;
        info->disconnected = st[2];
        info->in_weight = st[3] / 2;
        info->cut_weight = st[4] / 2;
        info->total_degree = g.M2;
    }
}

}  // namespace fc
