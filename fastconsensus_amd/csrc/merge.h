// merge.h -- what a merge of two clusters of a given partition P needs: the community graph of P on
// a graph H (fc_community_graph: which clusters touch, by how many edges and how much weight) and
// the co-association summed over the member pairs of two clusters (fc_cluster_coassoc): with
// C_r[k][d] = the members of cluster k that replica r labels d,
//     X(a, b) = sum_r sum_d C_r[a][d] * C_r[b][d] = sum over i in a, j in b of coassoc(i, j)
// so that joining a and b changes the median-partition objective F by 2 (2 X(a, b) - R s_a s_b).
// Exact integers, sums over replicas (ranks add theirs), no matrix.
// Included at the end of consensus.hip after affinity.h (quality.h's k_ql_present / k_ql_ids,
// components.h's cp_graph, affinity.h's k_ia_rank, cluster.h's cell_chunks, score.h's segments,
// cell-kernel pieces, fallback plan and ScLabT, analysis.h's PhaseMarks and the hipcub wrappers are
// in scope).
//
// Community graph: cluster ranks as quality.h takes them (presence flags over [0, n) and their
// scan), one pass over H's canonical edges that appends (rank_lo << 32) | rank_hi with the weight
// for every cut edge (one counter add per wave), a radix sort by key, the run lengths (= edges per
// pair) and the weights' prefix sums read at the run boundaries (= weight per pair), ranks back to
// ids.  Ranks ascend with the ids, so the sorted keys are the pairs ascending by (a, b).
//
// Pair co-association: every pair gets a LIST side and a WALK side: the larger cluster lists (a on
// equal sizes), the smaller walks, so the per-pair cost is the smaller size and the list of a
// cluster is built once for all its partners.  The pairs are sorted by list-side rank; the run
// lengths are the listed clusters with their partner segments.  Count: one wave per LISTED cluster,
// LANES ARE REPLICAS.  Pass 1 (sc_list_walk) builds the lane's (label, count) list in SC_D
// registers; pass 2 takes the partners in turn, streams each partner's members, looks the member's
// label up in the list (sc_gather4, sc_list_count) and adds the count to a 64-bit sum in the lane;
// one wave reduction and one int64 atomicAdd per (pair, bank) finish the partner.
// Fallback: a lane with a ninth label, and every lane of a listed cluster past the length cap, is
// flagged in ovf[bank * k + cluster] (score.h's entries); cell_chunks sorts and run-length encodes
// their keys chunk by chunk, and one thread per (pair, walk member) binary-searches the
// chunk's unique keys for (slot, lab_r(member)) over the flagged lanes.  A slot lies in exactly
// one chunk, so no cell is split; every path adds integers into the same cell.
#pragma once
#include <algorithm>
#include <vector>

namespace fc {

// ------------------------------------------------------------------ community graph
// labi[sigma[t]] = rank[in[t]]: dense cluster ranks by internal vertex
__global__ void k_mg_ranks(int64_t N, const int32_t* __restrict__ in, const int32_t* __restrict__ rank,
                           const int32_t* __restrict__ sigma, int32_t* __restrict__ labi) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) labi[sigma[t]] = rank[in[t]];
}
// One thread per canonical edge; a cut edge appends its key and weight at *count (one add per wave).
// UNIT: every weight is 1, no weight loads.  cap = m: every edge may be cut.
template <bool UNIT>
__global__ __launch_bounds__(256) void k_mg_emit(int64_t m, const int32_t* __restrict__ eu,
                                                 const int32_t* __restrict__ ev, const int32_t* __restrict__ ew,
                                                 const int32_t* __restrict__ labi,
                                                 unsigned long long* __restrict__ keys, int64_t* __restrict__ wts,
                                                 unsigned long long* __restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool cut = false;
    uint32_t lo = 0, hi = 0;
    if (e < m) {
        const uint32_t x = (uint32_t)labi[eu[e]], y = (uint32_t)labi[ev[e]];
        cut = x != y;
        lo = x < y ? x : y;
        hi = x < y ? y : x;
    }
    const unsigned long long mask = __ballot(cut);
    if (!mask) return;   // wave-uniform
    const int src = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == src) base = atomicAdd(count, (unsigned long long)__popcll(mask));
    base = __shfl(base, src);
    if (cut) {
        const int64_t at = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
        keys[at] = ((unsigned long long)lo << 32) | (unsigned long long)hi;
        wts[at] = UNIT ? 1 : (int64_t)ew[e];
    }
}
// One thread per run of the sorted keys: the pair's ids, its edges (the run length) and its weight
// (S = the exclusive prefix sums of the sorted weights, off those of the run lengths).
__global__ __launch_bounds__(256) void k_mg_pairs(const int32_t* __restrict__ nruns,
                                                  const unsigned long long* __restrict__ ukeys,
                                                  const int32_t* __restrict__ counts, const int32_t* __restrict__ off,
                                                  const int64_t* __restrict__ S, const int32_t* __restrict__ ids,
                                                  int32_t* __restrict__ a, int32_t* __restrict__ b,
                                                  int64_t* __restrict__ weight, int64_t* __restrict__ edges) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)*nruns) return;
    const unsigned long long key = ukeys[p];
    a[p] = ids[key >> 32];
    b[p] = ids[key & 0xffffffffull];
    edges[p] = counts[p];
    weight[p] = S[off[p + 1]] - S[off[p]];
}

// labels: host int32[N] in node order, ids in [0, N), validated by the caller.  The outputs (host
// or device, any may be null) are written only when everything succeeded; *npairs_out always.
void community_graph(Ctx& c, int graph, const int32_t* labels, int64_t capacity, int32_t* a_out, int32_t* b_out,
                     int64_t* weight_out, int64_t* edges_out, int64_t* npairs_out) {
    const Graph& g = cp_graph(c, graph);
    const int64_t N = c.N, m = g.m;
    PhaseMarks ph(c, c.mg_ms);
    ph.clear();
    ph.mark();
    int32_t* in = ensure<int32_t>(c.st_lab, N + 1);
    FC_HIP(hipMemcpyAsync(in, labels, 4 * (size_t)N, hipMemcpyHostToDevice, c.stream));
    int32_t* present = ensure<int32_t>(c.ql_present, N + 1);
    int32_t* idrank = ensure<int32_t>(c.ql_rank, N + 1);
    int32_t* ids = ensure<int32_t>(c.ql_ids, N);
    int32_t* labi = ensure<int32_t>(c.ql_labi, N);
    FC_HIP(hipMemsetAsync(present, 0, sizeof(int32_t) * (size_t)(N + 1), c.stream));
    k_ql_present<<<nblk(N), TB, 0, c.stream>>>(N, in, present);
    exclusive_scan(c, (const int32_t*)present, idrank, N + 1);   // idrank[N] = K
    k_ql_ids<<<nblk(N), TB, 0, c.stream>>>(N, present, idrank, ids);
    k_mg_ranks<<<nblk(N), TB, 0, c.stream>>>(N, in, idrank, c.sigma.as<int32_t>(), labi);
    ph.mark();   // labels
    unsigned long long* ctr = (unsigned long long*)ensure<uint64_t>(c.mg_ctr, 2);
    FC_HIP(hipMemsetAsync(ctr, 0, sizeof(uint64_t) * 2, c.stream));
    unsigned long long* k1 = (unsigned long long*)ensure<uint64_t>(c.mg_key, (size_t)2 * (m + 1));
    int64_t* w1 = ensure<int64_t>(c.mg_w, (size_t)2 * (m + 1));
    unsigned long long* k2 = k1 + (m + 1);
    int64_t* w2 = w1 + (m + 1);
    if (m > 0) {
        if (unit_weights(g))
            k_mg_emit<true><<<nblk(m), TB, 0, c.stream>>>(m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), nullptr, labi, k1, w1,
                                                          ctr);
        else
            k_mg_emit<false><<<nblk(m), TB, 0, c.stream>>>(m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), g.ew.as<int32_t>(),
                                                           labi, k1, w1, ctr);
    }
    const int64_t T = read_i64(c, (const int64_t*)ctr);   // cut edges; synchronises
    ph.mark();   // emit
    int64_t np = 0;
    int32_t *pa = nullptr, *pb = nullptr;
    int64_t *pw = nullptr, *pe = nullptr;
    if (T > 0) {
        int end_bit = 33;
        while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < N) ++end_bit;   // ranks below N in both halves
        sort_pairs_public(c, (const uint64_t*)k1, (uint64_t*)k2, (const int64_t*)w1, w2, T, end_bit);
        int32_t* cnt = ensure<int32_t>(c.mg_cnt, (size_t)2 * (T + 2));
        int32_t* off = cnt + (T + 2);
        int32_t* nr = (int32_t*)(ctr + 1);
        FC_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(T + 2), c.stream));   // run lengths past the last run: 0
        run_length(c, (const unsigned long long*)k2, k1, cnt, nr, T);
        exclusive_scan(c, (const int32_t*)cnt, off, T + 1);
        FC_HIP(hipMemsetAsync(w2 + T, 0, sizeof(int64_t), c.stream));
        int64_t* S = w1;   // the unsorted weights are spent
        exclusive_scan(c, (const int64_t*)w2, S, T + 1);   // S[T] = the cut weight
        ph.mark();   // sort
        pa = ensure<int32_t>(c.mg_ab, (size_t)2 * T);
        pb = pa + T;
        pw = ensure<int64_t>(c.mg_we, (size_t)2 * T);
        pe = pw + T;
        k_mg_pairs<<<nblk(T), TB, 0, c.stream>>>(nr, k1, cnt, off, S, ids, pa, pb, pw, pe);
        FC_HIP(hipMemcpyAsync(c.hpin, nr, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
        sync(c);
        np = *(const int32_t*)c.hpin.p;
    } else
        ph.mark();   // sort
    ph.mark();   // pairs
    sync(c);
    ph.collect();
    *npairs_out = np;
    const bool any = a_out || b_out || weight_out || edges_out;
    FC_REQUIRE(!any || capacity >= np, FC_EINVAL,
               "capacity " + std::to_string(capacity) + " is below the " + std::to_string(np) + " pairs of the community graph");
    if (np > 0) {
        if (a_out) FC_HIP(hipMemcpyAsync(a_out, pa, sizeof(int32_t) * (size_t)np, hipMemcpyDefault, c.stream));
        if (b_out) FC_HIP(hipMemcpyAsync(b_out, pb, sizeof(int32_t) * (size_t)np, hipMemcpyDefault, c.stream));
        if (weight_out) FC_HIP(hipMemcpyAsync(weight_out, pw, sizeof(int64_t) * (size_t)np, hipMemcpyDefault, c.stream));
        if (edges_out) FC_HIP(hipMemcpyAsync(edges_out, pe, sizeof(int64_t) * (size_t)np, hipMemcpyDefault, c.stream));
        sync(c);
    }
}

// ------------------------------------------------------------------ pair co-association
// Ctx::mc_ctr slots: ids of the lists that do not occur (k_ia_rank's slot 0, both sides counted),
// (walk member, replica) pairs of the fallback, the run count of the sorted list ranks (an int32 in
// the slot's low half), the walk-side members of all pairs
enum { MC_ABSENT, MC_SLOW, MC_NRUNS, MC_WALK, MC_CTRS };

// Pair p with ranks ra, rb (k: the id does not occur): the larger cluster lists, the smaller walks,
// a lists on equal sizes; a pair with an absent id gets list rank k (sorted last, skipped).
// lkey[p] / wrank[p] = the list / walk side's rank.
__global__ __launch_bounds__(256) void k_mc_orient(int64_t np, const uint32_t* __restrict__ ra,
                                                   const uint32_t* __restrict__ rb, int64_t k,
                                                   const int32_t* __restrict__ size, uint32_t* __restrict__ lkey,
                                                   uint32_t* __restrict__ wrank, unsigned long long* __restrict__ ctr) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long walk = 0;
    if (p < np) {
        const uint32_t x = ra[p], y = rb[p];
        uint32_t l = (uint32_t)k, w = (uint32_t)k;
        if ((int64_t)x < k && (int64_t)y < k) {
            const int32_t sx = size[x], sy = size[y];
            l = sx >= sy ? x : y;
            w = sx >= sy ? y : x;
            walk = (unsigned long long)(sx >= sy ? sy : sx);
        }
        lkey[p] = l;
        wrank[p] = w;
    }
    walk = sc_wave_sum(walk);
    if ((threadIdx.x & 63) == 0 && walk) atomicAdd(&ctr[MC_WALK], walk);
}

// ------------------------------------------------------------------ count kernel (lanes are replicas)
// qc[i]: the rank of the i-th listed cluster (k: the pairs of ids that do not occur, skipped); its
// partners are the pairs qidx[qoff[i] .. qoff[i + 1]), pair p walking the members of cluster
// wrank[p].  lcap: score_list_cap with sum32, on the list side only: a walk of any length is only read.
// ovf[bank * k + cluster], zeroed by the caller: the lanes left to the fallback.  out[pair] zeroed
// by the caller.
__global__ __launch_bounds__(256) void k_mc_count(int64_t nq, const uint32_t* __restrict__ qc,
                                                  const int32_t* __restrict__ qoff, const int32_t* __restrict__ qidx,
                                                  const uint32_t* __restrict__ wrank, int64_t k,
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
            // pass 1: the list of (label, count) of this lane's replica over the listed cluster's members
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            const bool live = act && !ov;
            // pass 2: the partners in turn, each partner's members against the lists still in registers
            if (__any(live)) {   // wave-uniform
                const int32_t q0 = qoff[i], q1 = qoff[i + 1];
                for (int32_t p0 = q0; p0 < q1; p0 += 64) {
                    const int npb = q1 - p0 < 64 ? q1 - p0 : 64;
                    const int32_t myp = p0 + lane < q1 ? qidx[p0 + lane] : 0;
                    const int32_t myw = p0 + lane < q1 ? (int32_t)wrank[myp] : 0;
                    for (int u = 0; u < npb; ++u) {
                        const int32_t p = __shfl(myp, u);
                        const int32_t wr = __shfl(myw, u);   // < k, as the pair's list rank is
                        const int32_t w0 = seg[wr], w1 = seg[wr + 1];
                        unsigned long long acc = 0;
                        for (int32_t b0 = w0; b0 < w1; b0 += 64) {
                            const int nb = w1 - b0 < 64 ? w1 - b0 : 64;
                            const int32_t myv = b0 + lane < w1 ? sval[b0 + lane] : 0;
                            for (int t = 0; t < nb; t += 4) {
                                int32_t l[4];
                                sc_gather4(l, myv, t, nb, col, ldT, live);
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    const int32_t x = sc_list_count(key, cnt, l[j]);
                                    acc += live && t + j < nb ? (unsigned long long)(uint32_t)x : 0ull;
                                }
                            }
                        }
                        acc = sc_wave_sum(acc);
                        if (lane == 0 && acc) atomicAdd(&out[p], acc);
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(ov);
        if (lane == 0 && mask) ovf[(int64_t)bank * k + cc] = mask;
    }
}

// ------------------------------------------------------------------ exact fallback
// work[p] = the walk side's members when some lane of pair p's listed cluster is flagged, else 0;
// *ctr[MC_SLOW] += members * flagged lanes.  work[np] = 0.
__global__ __launch_bounds__(256) void k_mc_work(int64_t np, int banks, const uint32_t* __restrict__ lrank,
                                                 const uint32_t* __restrict__ wrank, int64_t k,
                                                 const unsigned long long* __restrict__ ovf,
                                                 const int32_t* __restrict__ seg, int64_t* __restrict__ work,
                                                 unsigned long long* __restrict__ ctr) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long s = 0;
    if (p <= np) {
        int64_t wk = 0;
        if (p < np && (int64_t)lrank[p] < k) {
            const int64_t cc = (int64_t)lrank[p];
            int64_t lanes = 0;
            for (int bank = 0; bank < banks; ++bank) lanes += __popcll(ovf[(int64_t)bank * k + cc]);
            const int64_t wr = (int64_t)wrank[p], len = seg[wr + 1] - seg[wr];
            if (lanes) wk = len;
            s = (unsigned long long)(len * lanes);
        }
        work[p] = wk;
    }
    s = sc_wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ctr[MC_SLOW], s);
}
// One thread per (pair p, member t of its walk side) of the pairs with work (W = the exclusive
// prefix sums of work, W[np] = n): over every flagged lane of p's listed cluster, the chunk's
// unique keys hold the cell ((bank * k + cluster) * 64 + lane) << 32 | lab_r(member) when the slot
// lies in this chunk and some listed member carries that label; its run length is
// C_r[cluster][lab_r(member)].  A wave whose threads share one pair adds once.
__global__ __launch_bounds__(256) void k_mc_lookup(int64_t n, int64_t np, int banks, const int64_t* __restrict__ W,
                                                   const uint32_t* __restrict__ lrank,
                                                   const uint32_t* __restrict__ wrank, int64_t k,
                                                   const unsigned long long* __restrict__ ovf,
                                                   const int32_t* __restrict__ seg, const int32_t* __restrict__ sval,
                                                   const int32_t* __restrict__ labT, int ldT,
                                                   const int32_t* __restrict__ nruns,
                                                   const unsigned long long* __restrict__ ukeys,
                                                   const int32_t* __restrict__ counts,
                                                   unsigned long long* __restrict__ out) {
    const int64_t nr = *nruns;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (n + step - 1) / step;   // every lane of a wave takes every turn
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t it = 0; it < rounds; ++it, g += step) {
        unsigned long long sum = 0;
        int64_t p = -1;
        if (g < n) {
            int64_t a = 0, b = np - 1;   // the last pair with W[p] <= g (pairs without work repeat W: the last is the one with work)
            while (a < b) {
                const int64_t mid = (a + b + 1) >> 1;
                if (W[mid] <= g) a = mid;
                else b = mid - 1;
            }
            p = a;
            const int64_t cc = (int64_t)lrank[p], wr = (int64_t)wrank[p];
            const int32_t v = sval[(int64_t)seg[wr] + (g - W[p])];
            for (int bank = 0; bank < banks; ++bank) {
                const int64_t i = (int64_t)bank * k + cc;
                unsigned long long m = ovf[i];
                while (m) {
                    const int lane = __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    const unsigned long long key = (((unsigned long long)i * 64ull + (unsigned long long)lane) << 32) |
                                                   (unsigned long long)(uint32_t)labT[(int64_t)v * ldT + bank * 64 + lane];
                    int64_t lo = 0, hi = nr;   // the first run with ukeys >= key
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (ukeys[mid] < key) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < nr && ukeys[lo] == key) sum += (unsigned long long)counts[lo];
                }
            }
        }
        const int64_t p0 = __shfl(p, 0);
        if (__all(p == p0)) {   // wave-uniform
            sum = sc_wave_sum(sum);
            if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&out[p0], sum);
        } else if (sum)
            atomicAdd(&out[p], sum);
    }
}
// returns the (walk member, replica) pairs answered here
static int64_t merge_fallback(Ctx& c, const ScSeg& s, int banks, const unsigned long long* ovf, int64_t np,
                              const uint32_t* lrank, const uint32_t* wrank, unsigned long long* ctr,
                              unsigned long long* out) {
    const ScPlan p = score_fallback_plan(c, s, (int64_t)banks * s.k, ovf,
                                         "too many (cluster, replica) slots for the pair co-association fallback");
    if (p.T == 0) return 0;
    int64_t* work = ensure<int64_t>(c.mc_work, (size_t)2 * (np + 1));
    int64_t* W = work + (np + 1);
    k_mc_work<<<nblk(np + 1), TB, 0, c.stream>>>(np, banks, lrank, wrank, s.k, ovf, s.seg, work, ctr);
    exclusive_scan(c, (const int64_t*)work, W, np + 1);
    const int64_t threads = read_i64(c, W + np);
    const int64_t slow = read_i64(c, (const int64_t*)(ctr + MC_SLOW));
    if (threads == 0) return slow;   // flagged lists that no pair asks for
    cell_chunks<false>(c, s, p, ovf, c.labT.as<int32_t>(), c.ldT, [&](const CellChunk& ch) {
        k_mc_lookup<<<std::min<unsigned>(nblk(threads), 8192u), TB, 0, c.stream>>>(
            threads, np, banks, W, lrank, wrank, s.k, ovf, s.seg, s.sval, c.labT.as<int32_t>(), c.ldT, ch.nruns, ch.ukeys,
            ch.counts, out);
    });
    return slow;
}

// labels: host int32[N] in node order; a, b: host int32[np]; all ids in [0, N), validated by the
// caller; np >= 1.  Synchronises; dev_out is written last.
void cluster_coassoc(Ctx& c, const int32_t* labels, int64_t np, const int32_t* a, const int32_t* b, int64_t* dev_out,
                     fc_cluster_pair_info* info) {
    score_require(c);
    const int banks = (c.n_r + 63) / 64;
    PhaseMarks ph(c, c.mc_ms);
    ph.clear();
    ScLabT lt(c);
    ph.mark();
    const ScSeg s = partition_segments(c, partition_upload(c, labels));
    // the lists: cluster ids -> ranks, the sides, pair indices by list-side rank
    int32_t* ids = ensure<int32_t>(c.mc_ids, (size_t)2 * np);
    FC_HIP(hipMemcpyAsync(ids, a, 4 * (size_t)np, hipMemcpyHostToDevice, c.stream));
    FC_HIP(hipMemcpyAsync(ids + np, b, 4 * (size_t)np, hipMemcpyHostToDevice, c.stream));
    uint32_t* rk = ensure<uint32_t>(c.mc_rank, (size_t)3 * np);   // ranks of a, of b, of the walk side
    uint32_t* key = ensure<uint32_t>(c.mc_key, (size_t)2 * np);   // list ranks by pair, then sorted
    int32_t* idx = ensure<int32_t>(c.mc_idx, (size_t)2 * np);     // 0 .. np, then by list rank
    uint32_t* qc = ensure<uint32_t>(c.mc_qc, (size_t)np);
    int32_t* qcnt = ensure<int32_t>(c.mc_qcnt, (size_t)2 * (np + 1));
    int32_t* qoff = qcnt + (np + 1);
    unsigned long long* ctr = (unsigned long long*)ensure<uint64_t>(c.mc_ctr, MC_CTRS);
    unsigned long long* out = (unsigned long long*)ensure<uint64_t>(c.mc_out, (size_t)np);
    uint32_t* wrank = rk + 2 * np;
    FC_HIP(hipMemsetAsync(ctr, 0, sizeof(uint64_t) * MC_CTRS, c.stream));
    FC_HIP(hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)np, c.stream));
    FC_HIP(hipMemsetAsync(qcnt, 0, sizeof(int32_t) * ((size_t)np + 1), c.stream));   // run lengths past the last run: 0
    k_ia_rank<<<nblk(np), TB, 0, c.stream>>>(np, ids, s.k, c.sc_ulab.as<uint32_t>(), rk, idx, ctr);
    k_ia_rank<<<nblk(np), TB, 0, c.stream>>>(np, ids + np, s.k, c.sc_ulab.as<uint32_t>(), rk + np, idx, ctr);
    k_mc_orient<<<nblk(np), TB, 0, c.stream>>>(np, rk, rk + np, s.k, c.sc_cnt.as<int32_t>(), key, wrank, ctr);
    int end_bit = 1;
    while (end_bit < 32 && ((int64_t)1 << end_bit) <= s.k) ++end_bit;   // rank k included
    sort_pairs_public(c, (const uint32_t*)key, key + np, (const int32_t*)idx, idx + np, np, end_bit);
    run_length(c, (const uint32_t*)(key + np), qc, qcnt, (int32_t*)(ctr + MC_NRUNS), np);
    FC_HIP(hipMemcpyAsync(c.hpin, ctr, sizeof(uint64_t) * MC_CTRS, hipMemcpyDeviceToHost, c.stream));
    FC_HIP(hipMemcpyAsync(c.hpin.p + MC_CTRS, key + np + (np - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    const int64_t nq = c.hpin[MC_NRUNS], walked = c.hpin[MC_WALK];
    const bool absent = (int64_t)(*(const uint32_t*)(c.hpin.p + MC_CTRS)) >= s.k;   // the largest list rank
    exclusive_scan(c, (const int32_t*)qcnt, qoff, nq + 1);
    ph.mark();   // pairs
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)banks * s.k + 1);
    FC_HIP(hipMemsetAsync(ovf, 0, sizeof(uint64_t) * ((size_t)banks * s.k + 1), c.stream));
    k_mc_count<<<dim3(score_count_grid(nq), banks), TB, 0, c.stream>>>(nq, qc, qoff, idx + np, wrank, s.k, s.seg, s.sval,
                                                                      c.labT.as<int32_t>(), c.ldT, c.n_r,
                                                                      score_list_cap(c, true), ovf, out);
    ph.mark();   // count
    const int64_t slow = merge_fallback(c, s, banks, ovf, np, key, wrank, ctr, out);
    ph.mark();   // fallback
    sync(c);
    ph.collect();
    FC_HIP(hipMemcpyAsync(dev_out, out, sizeof(int64_t) * (size_t)np, hipMemcpyDeviceToDevice, c.stream));
    sync(c);
    if (info) {
        *info = fc_cluster_pair_info{};
        info->k = s.k; info->listed_clusters = nq - (absent ? 1 : 0);
        info->walked_members = walked; info->slow_lookups = slow; info->n_r = c.n_r;
    }
}

}  // namespace fc
