// coassoc.h -- co-association over the local labelings (fc_coassociation / fc_coassoc_pairs /
// fc_coassoc_hist): for two nodes, the number of local replicas that put them in one community.
// The consensus matrix of two node lists, the counts of arbitrary node pairs, and the
// distribution of the counts over the pairs of one list (what PAC and the consensus CDF need)
// without the matrix.
// Included at the end of consensus.hip after levels.h (ScLabT, score_require, launch_pair_partial,
// ensure and the helpers of analysis.h are in scope).
//
// Tile core: a 256-thread block owns 64 x 64 pairs.  Per bank of 64 replicas it stages the 64 + 64
// label rows of labT in LDS -- a row is 256 bytes, read by 16 lanes as one int4 each -- and every
// thread adds the equalities of a 4 x 4 block of pairs, four replicas per ds_read_b128.  The int4
// chunk c of tile row r sits at slot c ^ ((r >> 2) & 15) of its 256-byte LDS row: a 16-lane read
// group holds two values of ty (A rows 4 ty + a: two slots, broadcast inside each) or sixteen of tx
// (B rows 4 tx + b: sixteen slots), so every read is conflict-free.  Nothing is zero-filled: chunks
// past n_r are not read, the last chunk masks its dead replicas, and rows past the lists' ends
// hold whatever the LDS held and are never written out.
#pragma once
#include <cstring>
#include <vector>

namespace fc {

static constexpr int CA_T = 64;                 // tile edge = replicas per bank
static constexpr int CA_TILE_I4 = 2 * CA_T * 16;   // int4 slots of the A and B tiles (32 KB)

// out[i] = sigma[in[i * stride]]: caller node ids -> internal vertices (the rows of labT)
__global__ void k_ca_map(int64_t n, const int32_t* __restrict__ in, int stride, const int32_t* __restrict__ sigma,
                         int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sigma[in[i * stride]];
}

__device__ __forceinline__ int ca_eq4(const int4& a, const int4& b) {
    return (a.x == b.x) + (a.y == b.y) + (a.z == b.z) + (a.w == b.w);
}

// acc[a][b] += #replicas r < n_r with labT[va[i0 + 4 ty + a]][r] == labT[vb[j0 + 4 tx + b]][r]
// (tx = thread & 15, ty = thread >> 4); entries whose row lies past na / nb are undefined
__device__ __forceinline__ void ca_tile(const int32_t* __restrict__ labT, int ldT, int n_r,
                                        const int32_t* __restrict__ va, int64_t na, int64_t i0,
                                        const int32_t* __restrict__ vb, int64_t nb, int64_t j0, int4* s_t,
                                        int (&acc)[4][4]) {
    const int q = threadIdx.x & 15, r0 = threadIdx.x >> 4;   // staging: chunk q of the rows r0 + 16 p
    const int tx = q, ty = r0;
    int64_t base[8];
    bool has[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {   // rows 0..63: list a, 64..127: list b
        const int lr = (r0 + 16 * p) & (CA_T - 1);
        const int64_t g = (p < 4 ? i0 : j0) + lr;
        has[p] = g < (p < 4 ? na : nb);
        base[p] = has[p] ? (int64_t)(p < 4 ? va : vb)[g] * ldT : 0;
    }
    for (int b0 = 0; b0 < n_r; b0 += CA_T) {
        const int left = n_r - b0;
        const int nq = left >= CA_T ? 16 : (left + 3) >> 2;      // chunks with a live replica (inside ldT)
        const int nfull = left >= CA_T ? 16 : left >> 2;        // chunks whose four replicas are live
        int4 x[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            x[p] = make_int4(0, 0, 0, 0);
            if (has[p] && q < nq) x[p] = *reinterpret_cast<const int4*>(labT + base[p] + b0 + 4 * q);
        }
        if (b0) __syncthreads();   // the previous bank's reads are done
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = r0 + 16 * p;
            if (has[p] && q < nq) s_t[row * 16 + (q ^ ((row >> 2) & 15))] = x[p];
        }
        __syncthreads();
        const int4* sa = s_t + (4 * ty) * 16;
        const int4* sb = s_t + (CA_T + 4 * tx) * 16;
#pragma unroll 2
        for (int c = 0; c < nfull; ++c) {
            int4 A[4], B[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                A[k] = sa[k * 16 + (c ^ ty)];
                B[k] = sb[k * 16 + (c ^ tx)];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += ca_eq4(A[a], B[b]);
        }
        if (nfull < nq) {   // the bank's last chunk: 1..3 live replicas
            const int live = left - 4 * nfull, c = nfull;
            int4 A[4], B[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                A[k] = sa[k * 16 + (c ^ ty)];
                B[k] = sb[k * 16 + (c ^ tx)];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] += (A[a].x == B[b].x) + (live > 1 && A[a].y == B[b].y) + (live > 2 && A[a].z == B[b].z);
        }
    }
}

// out[i * nb + j] for the tile blockIdx.x = tile_i * tnb + tile_j.  One writer per entry, no
// atomics.  VEC: nb is a multiple of 4 and out is 16-byte aligned (one int4 store per row).
template <bool VEC>
__global__ __launch_bounds__(256) void k_ca_tile(const int32_t* __restrict__ labT, int ldT, int n_r,
                                                 const int32_t* __restrict__ va, int64_t na,
                                                 const int32_t* __restrict__ vb, int64_t nb, unsigned tnb,
                                                 int32_t* __restrict__ out) {
    __shared__ int4 s_t[CA_TILE_I4];
    const int64_t i0 = (int64_t)(blockIdx.x / tnb) * CA_T, j0 = (int64_t)(blockIdx.x % tnb) * CA_T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;
    ca_tile(labT, ldT, n_r, va, na, i0, vb, nb, j0, s_t, acc);
    const int64_t gj = j0 + 4 * tx;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t gi = i0 + 4 * ty + a;
        if (gi >= na || gj >= nb) continue;
        int32_t* o = out + gi * nb + gj;   // 64-bit: na * nb may pass 2^31
        if (VEC) {   // gj + 3 < nb: both are multiples of 4
            *reinterpret_cast<int4*>(o) = make_int4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (gj + b < nb) o[b] = acc[a][b];
        }
    }
}

// hist[s] += #position pairs i < j of one list with count s.  Block blockIdx.x is the tile
// (ti, tj), ti <= tj, of the upper triangle of T x T tiles (row ti starts at ti T - ti (ti - 1) / 2).
// LDS bins (n_r + 1 counters, dynamic), a wave whose lanes agree adds once (the counts pile up at
// 0 and n_r); one flush per block.  Integer sums: no dependence on the order of arrival.
__global__ __launch_bounds__(256) void k_ca_hist(const int32_t* __restrict__ labT, int ldT, int n_r,
                                                 const int32_t* __restrict__ va, int64_t k, int64_t T,
                                                 unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned int s_ca_h[];
    __shared__ int4 s_t[CA_TILE_I4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, lane = threadIdx.x & 63;
    const int64_t blk = blockIdx.x;
    const double d = (double)(2 * T + 1);
    int64_t ti = (int64_t)((d - sqrt(d * d - 8.0 * (double)blk)) * 0.5);
    ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
    while (ti + 1 < T && (ti + 1) * T - (ti + 1) * ti / 2 <= blk) ++ti;
    while (ti > 0 && ti * T - ti * (ti - 1) / 2 > blk) --ti;
    const int64_t tj = ti + (blk - (ti * T - ti * (ti - 1) / 2));
    const int64_t i0 = ti * CA_T, j0 = tj * CA_T;
    for (int i = threadIdx.x; i <= n_r; i += blockDim.x) s_ca_h[i] = 0;
    int acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;
    __syncthreads();
    ca_tile(labT, ldT, n_r, va, k, i0, va, k, j0, s_t, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {   // wave-uniform: every lane takes every turn
            const int64_t gi = i0 + 4 * ty + a, gj = j0 + 4 * tx + b;
            const bool in = gj < k && gi < gj;   // gi < gj < k
            const int bin = in ? acc[a][b] : -1;
            const unsigned long long act = __ballot(in);
            if (!act) continue;
            wave_bin_add(s_ca_h, in, bin, act, lane);
        }
    __syncthreads();
    for (int i = threadIdx.x; i <= n_r; i += blockDim.x)
        if (s_ca_h[i]) atomicAdd(&hist[i], (unsigned long long)s_ca_h[i]);
}

// host node ids (validated by the caller), every stride-th from `first` -> internal vertices in dst
static int32_t* ca_vertices(Ctx& c, DevBuf& stage, DevBuf& dst, const int32_t* host, int64_t count, int stride,
                            int first) {
    int32_t* in = ensure<int32_t>(stage, (size_t)count * stride);
    int32_t* out = ensure<int32_t>(dst, (size_t)count);
    if (first == 0)
        FC_HIP(hipMemcpyAsync(in, host, sizeof(int32_t) * (size_t)count * stride, hipMemcpyHostToDevice, c.stream));
    k_ca_map<<<nblk(count), TB, 0, c.stream>>>(count, in + first, stride, c.sigma.as<int32_t>(), out);
    return out;
}

// a, b: host node ids in [0, N), validated by the caller; b null: b = a.  Synchronises.
void coassoc_matrix(Ctx& c, int64_t na, const int32_t* a, int64_t nb, const int32_t* b, int32_t* dev_out) {
    score_require(c);
    if (!b) nb = na;
    PhaseMarks ph(c, c.ca_ms);
    ph.clear();   // an early return reports all-zero phases
    if (na <= 0 || nb <= 0) return;
    const int64_t tna = (na + CA_T - 1) / CA_T, tnb = (nb + CA_T - 1) / CA_T;
    FC_REQUIRE(tna * tnb < ((int64_t)1 << 31), FC_ELIMIT, "co-association matrix of more than 2^31 tiles");
    ScLabT lt(c);
    ph.mark();
    const int32_t* va = ca_vertices(c, c.ca_ids, c.ca_va, a, na, 1, 0);
    const int32_t* vb = b ? ca_vertices(c, c.ca_ids, c.ca_vb, b, nb, 1, 0) : va;
    ph.mark();   // ids
    const int32_t* labT = c.labT.as<int32_t>();
    const unsigned grid = (unsigned)(tna * tnb);
    if (nb % 4 == 0 && (reinterpret_cast<uintptr_t>(dev_out) & 15) == 0)
        k_ca_tile<true><<<grid, TB, 0, c.stream>>>(labT, c.ldT, c.n_r, va, na, vb, nb, (unsigned)tnb, dev_out);
    else
        k_ca_tile<false><<<grid, TB, 0, c.stream>>>(labT, c.ldT, c.n_r, va, na, vb, nb, (unsigned)tnb, dev_out);
    ph.mark();   // count
    sync(c);
    ph.collect();
}

// pairs: host [npairs][2] node ids, validated by the caller.  The count kernel of
// consensus_partial on arbitrary vertex pairs.  Synchronises.
void coassoc_pairs(Ctx& c, int64_t npairs, const int32_t* pairs, int32_t* dev_out) {
    score_require(c);
    PhaseMarks ph(c, c.ca_ms);
    ph.clear();   // an early return reports all-zero phases
    if (npairs <= 0) return;
    ScLabT lt(c);
    ph.mark();
    const int32_t* u = ca_vertices(c, c.ca_ids, c.ca_va, pairs, npairs, 2, 0);
    const int32_t* v = ca_vertices(c, c.ca_ids, c.ca_vb, pairs, npairs, 2, 1);
    ph.mark();   // ids
    launch_pair_partial<false>(c, npairs, u, v, dev_out);
    ph.mark();   // count
    sync(c);
    ph.collect();
}

// nodes: host node ids, validated by the caller; hist: host int64[n_r + 1]
void coassoc_hist(Ctx& c, int64_t k, const int32_t* nodes, int64_t* hist) {
    score_require(c);
    const int n_r = c.n_r;
    PhaseMarks ph(c, c.ca_ms);
    ph.clear();   // an early return reports all-zero phases
    std::memset(hist, 0, sizeof(int64_t) * ((size_t)n_r + 1));
    if (k < 2) return;
    const int64_t T = (k + CA_T - 1) / CA_T;
    FC_REQUIRE(T * (T + 1) / 2 < ((int64_t)1 << 31), FC_ELIMIT, "co-association histogram of more than 2^31 tiles");
    ScLabT lt(c);
    ph.mark();
    const int32_t* va = ca_vertices(c, c.ca_ids, c.ca_va, nodes, k, 1, 0);
    unsigned long long* dh = (unsigned long long*)ensure<uint64_t>(c.ca_hist, (size_t)n_r + 1);
    FC_HIP(hipMemsetAsync(dh, 0, sizeof(uint64_t) * ((size_t)n_r + 1), c.stream));
    ph.mark();   // ids
    k_ca_hist<<<(unsigned)(T * (T + 1) / 2), TB, sizeof(unsigned int) * ((size_t)n_r + 1), c.stream>>>(
        c.labT.as<int32_t>(), c.ldT, n_r, va, k, T, dh);
    ph.mark();   // count
    std::vector<unsigned long long> h((size_t)n_r + 1);
    FC_HIP(hipMemcpyAsync(h.data(), dh, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    ph.collect();
    for (size_t i = 0; i < h.size(); ++i) hist[i] = (int64_t)h[i];
}

}  // namespace fc
