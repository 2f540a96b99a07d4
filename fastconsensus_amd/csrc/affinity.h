// affinity.h -- co-association of a node summed over the members of ANY cluster of a given
// partition P (fc_item_affinity): with C_r[k][d] = the members of cluster k that replica r labels d,
//     aff(v, k) = sum_r C_r[k][lab_r(v)] = sum over the members j of k of coassoc(v, j)
// (v itself counted when P(v) = k), for a list of (node, cluster) queries: the numerator of Monti's
// item consensus m_i(k) for any k, and what a one-element move of the median-partition objective
// needs.  Exact integers, sums over replicas (ranks add theirs), no matrix.
// Included at the end of consensus.hip after vote.h (cluster.h's cell_chunks, score.h's segments,
// cell-kernel pieces, fallback plan and ScLabT, coassoc.h's k_ca_map and analysis.h's PhaseMarks are
// in scope).
//
// Queries: a query's cluster id becomes its rank among P's ascending ids (a binary search of
// score_segments' unique labels; an id that does not occur gets rank k), the query indices are
// sorted by rank, and the run lengths of the sorted ranks are the queried clusters with their query
// segments.
// Count: one wave per QUERIED cluster, LANES ARE REPLICAS.  Pass 1 (sc_list_walk) builds the
// lane's (label, count) list of the cluster's members in SC_D registers; pass 2 walks the cluster's
// queries instead of its members, looks each query node's label up in the list (sc_gather4,
// sc_list_count) and adds the four wave sums of sc_sum4 to out[query].  A cluster no query names
// is never touched.
// Fallback: a lane with a ninth label, and every lane of a cluster past the length cap, is flagged
// in ovf[bank * k + cluster] (score.h's entries); cell_chunks sorts and run-length encodes their
// keys chunk by chunk, and one thread per (query, replica) whose lane is flagged binary-searches
// the chunk's unique keys for (slot, lab_r(v)).  A slot lies in exactly one chunk, so no cell is split.
#pragma once
#include <algorithm>
#include <vector>

namespace fc {

// Ctx::ia_ctr slots: queries whose cluster does not occur, (query, replica) pairs of the fallback,
// the run count of the sorted ranks (an int32 in the slot's low half)
enum { IA_ABSENT, IA_SLOW, IA_NRUNS, IA_CTRS };

// key[p] = the rank of clusters[p] among ulab[0 .. k) (ascending), k when it does not occur; idx[p] = p
__global__ __launch_bounds__(256) void k_ia_rank(int64_t np, const int32_t* __restrict__ clusters, int64_t k,
                                                 const uint32_t* __restrict__ ulab, uint32_t* __restrict__ key,
                                                 int32_t* __restrict__ idx, unsigned long long* __restrict__ ctr) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool absent = false;
    if (p < np) {
        const uint32_t id = (uint32_t)clusters[p];
        int64_t a = 0, b = k;   // the first rank with ulab >= id
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (ulab[mid] < id) a = mid + 1;
            else b = mid;
        }
        absent = a >= k || ulab[a] != id;
        key[p] = absent ? (uint32_t)k : (uint32_t)a;
        idx[p] = (int32_t)p;
    }
    const unsigned long long m = __ballot(absent);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctr[IA_ABSENT], (unsigned long long)__popcll(m));
}

// ------------------------------------------------------------------ count kernel (lanes are replicas)
// qc[i]: the rank of the i-th queried cluster (k: the queries of ids that do not occur, skipped);
// its queries are qidx[qoff[i] .. qoff[i + 1]), query q asking for internal vertex qv[q].
// lcap: score_list_cap with sum32.  ovf[bank * k + cluster], zeroed by the caller: the lanes left to the
// fallback.  out[query] zeroed by the caller.
__global__ __launch_bounds__(256) void k_ia_count(int64_t nq, const uint32_t* __restrict__ qc,
                                                  const int32_t* __restrict__ qoff, const int32_t* __restrict__ qidx,
                                                  const int32_t* __restrict__ qv, int64_t k,
                                                  const int32_t* __restrict__ seg, const int32_t* __restrict__ sval,
                                                  const int32_t* __restrict__ labT, int ldT, int n_r, int lcap,
                                                  unsigned long long* __restrict__ ovf,
                                                  unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int bank = blockIdx.y;
    const int r = bank * 64 + lane;
    const bool act = r < n_r;
    const int32_t* col = labT + (act ? r : 0);
    for (int64_t i = (int64_t)blockIdx.x * 4 + w; i < nq; i += (int64_t)gridDim.x * 4) {
        const int64_t cc = (int64_t)qc[i];
        if (cc >= k) continue;   // wave-uniform: the ids that do not occur
        const int32_t s0 = seg[cc], s1 = seg[cc + 1], len = s1 - s0;
        bool ov = act && len > lcap;
        if (len <= lcap) {   // wave-uniform
            int32_t key[SC_D];
            int32_t cnt[SC_D];
            // pass 1: the list of (label, count) of this lane's replica over the cluster's members
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            const bool live = act && !ov;
            // pass 2: the cluster's queries against the lists still in registers
            if (__any(live)) {   // wave-uniform
                const int32_t q0 = qoff[i], q1 = qoff[i + 1];
                for (int32_t b0 = q0; b0 < q1; b0 += 64) {
                    const int nb = q1 - b0 < 64 ? q1 - b0 : 64;
                    const int32_t myq = b0 + lane < q1 ? qidx[b0 + lane] : 0;
                    const int32_t myv = b0 + lane < q1 ? qv[myq] : 0;
                    for (int t = 0; t < nb; t += 4) {
                        int32_t l[4];
                        sc_gather4(l, myv, t, nb, col, ldT, live);
                        unsigned n[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int32_t x = sc_list_count(key, cnt, l[j]);
                            n[j] = live && t + j < nb ? (unsigned)x : 0u;
                        }
                        const unsigned tot = sc_sum4(n, lane);
                        const int tj = t + (lane >> 4);   // the query this lane's group of 16 summed
                        const int32_t q = __shfl(myq, tj < nb ? tj : nb - 1);
                        if ((lane & 15) == 0 && tj < nb && tot) atomicAdd(&out[q], (unsigned long long)tot);
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(ov);
        if (lane == 0 && mask) ovf[(int64_t)bank * k + cc] = mask;
    }
}

// ------------------------------------------------------------------ exact fallback
// *ctr[IA_SLOW] += the flagged lanes of every query's cluster: one thread per (query, bank)
__global__ __launch_bounds__(256) void k_ia_slow(int64_t np, int banks, const uint32_t* __restrict__ qrank, int64_t k,
                                                 const unsigned long long* __restrict__ ovf,
                                                 unsigned long long* __restrict__ ctr) {
    unsigned long long s = 0;
    const int64_t n = np * banks;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = g / banks, bank = g - p * banks;
        const int64_t cc = (int64_t)qrank[p];
        if (cc < k) s += (unsigned long long)__popcll(ovf[bank * k + cc]);
    }
    s = sc_wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ctr[IA_SLOW], s);
}
// One thread per (query p, replica r) of a flagged lane: the chunk's unique keys hold the cell
// ((bank * k + cluster) * 64 + lane) << 32 | lab_r(v) when the slot lies in this chunk and some
// member carries that label; its run length is C_r[cluster][lab_r(v)].
__global__ __launch_bounds__(256) void k_ia_lookup(int64_t np, int banks, int n_r, const uint32_t* __restrict__ qrank,
                                                   const int32_t* __restrict__ qv, int64_t k,
                                                   const unsigned long long* __restrict__ ovf,
                                                   const int32_t* __restrict__ labT, int ldT,
                                                   const int32_t* __restrict__ nruns,
                                                   const unsigned long long* __restrict__ ukeys,
                                                   const int32_t* __restrict__ counts,
                                                   unsigned long long* __restrict__ out) {
    const int64_t nr = *nruns, per = (int64_t)banks * 64, n = np * per;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = g / per, r = g - p * per, bank = r >> 6;
        const int lane = (int)(r & 63);
        const int64_t cc = (int64_t)qrank[p];
        if (r >= n_r || cc >= k) continue;
        const int64_t i = bank * k + cc;
        if (!((ovf[i] >> lane) & 1ull)) continue;
        const unsigned long long key = (((unsigned long long)i * 64ull + (unsigned long long)lane) << 32) |
                                       (unsigned long long)(uint32_t)labT[(int64_t)qv[p] * ldT + r];
        int64_t a = 0, b = nr;   // the first run with ukeys >= key
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (ukeys[mid] < key) a = mid + 1;
            else b = mid;
        }
        if (a < nr && ukeys[a] == key) atomicAdd(&out[p], (unsigned long long)counts[a]);
    }
}
static void affinity_fallback(Ctx& c, const ScSeg& s, int banks, const unsigned long long* ovf, int64_t np,
                              const uint32_t* qrank, const int32_t* qv, unsigned long long* out) {
    const ScPlan p = score_fallback_plan(c, s, (int64_t)banks * s.k, ovf,
                                         "too many (cluster, replica) slots for the item-affinity fallback");
    if (p.T == 0) return;
    const int64_t threads = np * banks * 64;
    cell_chunks<false>(c, s, p, ovf, c.labT.as<int32_t>(), c.ldT, [&](const CellChunk& ch) {
        k_ia_lookup<<<std::min<unsigned>(nblk(threads), 8192u), TB, 0, c.stream>>>(
            np, banks, c.n_r, qrank, qv, s.k, ovf, c.labT.as<int32_t>(), c.ldT, ch.nruns, ch.ukeys, ch.counts, out);
    });
}

// labels: host int32[N] in node order; nodes, clusters: host int32[np]; all ids in [0, N),
// validated by the caller; np >= 1.  Synchronises; dev_out is written last.
void item_affinity(Ctx& c, const int32_t* labels, int64_t np, const int32_t* nodes, const int32_t* clusters,
                   int64_t* dev_out, fc_affinity_info* info) {
    score_require(c);
    const int banks = (c.n_r + 63) / 64;
    PhaseMarks ph(c, c.ia_ms);
    ph.clear();
    ScLabT lt(c);
    ph.mark();
    const ScSeg s = partition_segments(c, partition_upload(c, labels));
    // the lists: nodes -> internal vertices, cluster ids -> ranks, query indices by rank
    int32_t* ids = ensure<int32_t>(c.ia_ids, (size_t)2 * np);
    FC_HIP(hipMemcpyAsync(ids, nodes, 4 * (size_t)np, hipMemcpyHostToDevice, c.stream));
    FC_HIP(hipMemcpyAsync(ids + np, clusters, 4 * (size_t)np, hipMemcpyHostToDevice, c.stream));
    int32_t* qv = ensure<int32_t>(c.ia_qv, (size_t)np);
    k_ca_map<<<nblk(np), TB, 0, c.stream>>>(np, ids, 1, c.sigma.as<int32_t>(), qv);
    uint32_t* key = ensure<uint32_t>(c.ia_key, (size_t)2 * np);   // ranks by query, then sorted
    int32_t* idx = ensure<int32_t>(c.ia_idx, (size_t)2 * np);     // 0 .. np, then by rank
    uint32_t* qc = ensure<uint32_t>(c.ia_qc, (size_t)np);
    int32_t* qcnt = ensure<int32_t>(c.ia_qcnt, (size_t)np + 1);
    int32_t* qoff = ensure<int32_t>(c.ia_qoff, (size_t)np + 1);
    unsigned long long* ctr = (unsigned long long*)ensure<uint64_t>(c.ia_ctr, IA_CTRS);
    unsigned long long* out = (unsigned long long*)ensure<uint64_t>(c.ia_out, (size_t)np);
    FC_HIP(hipMemsetAsync(ctr, 0, sizeof(uint64_t) * IA_CTRS, c.stream));
    FC_HIP(hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)np, c.stream));
    FC_HIP(hipMemsetAsync(qcnt, 0, sizeof(int32_t) * ((size_t)np + 1), c.stream));   // run lengths past the last run: 0
    k_ia_rank<<<nblk(np), TB, 0, c.stream>>>(np, ids + np, s.k, c.sc_ulab.as<uint32_t>(), key, idx, ctr);
    int end_bit = 1;
    while (end_bit < 32 && ((int64_t)1 << end_bit) <= s.k) ++end_bit;   // rank k included
    sort_pairs_public(c, (const uint32_t*)key, key + np, (const int32_t*)idx, idx + np, np, end_bit);
    run_length(c, (const uint32_t*)(key + np), qc, qcnt, (int32_t*)(ctr + IA_NRUNS), np);
    FC_HIP(hipMemcpyAsync(c.hpin, ctr, sizeof(uint64_t) * IA_CTRS, hipMemcpyDeviceToHost, c.stream));
    sync(c);
    const int64_t absent = c.hpin[IA_ABSENT], nq = c.hpin[IA_NRUNS];
    exclusive_scan(c, (const int32_t*)qcnt, qoff, nq + 1);
    ph.mark();   // queries
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)banks * s.k + 1);
    FC_HIP(hipMemsetAsync(ovf, 0, sizeof(uint64_t) * ((size_t)banks * s.k + 1), c.stream));
    k_ia_count<<<dim3(score_count_grid(nq), banks), TB, 0, c.stream>>>(nq, qc, qoff, idx + np, qv, s.k, s.seg, s.sval,
                                                                      c.labT.as<int32_t>(), c.ldT, c.n_r,
                                                                      score_list_cap(c, true), ovf, out);
    ph.mark();   // count
    k_ia_slow<<<std::min<unsigned>(nblk(np * banks), 1024u), TB, 0, c.stream>>>(np, banks, key, s.k, ovf, ctr);
    affinity_fallback(c, s, banks, ovf, np, key, qv, out);
    ph.mark();   // fallback
    const int64_t slow = read_i64(c, (const int64_t*)(ctr + IA_SLOW));   // synchronises
    ph.collect();
    FC_HIP(hipMemcpyAsync(dev_out, out, sizeof(int64_t) * (size_t)np, hipMemcpyDeviceToDevice, c.stream));
    sync(c);
    if (info) {
        *info = fc_affinity_info{};
        info->k = s.k; info->queried_clusters = nq - (absent > 0 ? 1 : 0);
        info->slow_lookups = slow; info->n_r = c.n_r;
    }
}

}  // namespace fc
