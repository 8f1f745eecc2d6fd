// s2m_sc_many.hip — kernels of the many-query form of the ScanContext place query (s2m_sc_many.hpp):
// m queries against every stored descriptor of a range, a tiled all-pairs problem.  k_sc_many_prepare leaves every query's
// column norms (and an external descriptor's sector key), k_sc_many_dist<ALIGN> holds a tile of stored descriptors in LDS while
// a block of queries passes it and keeps every (query, tile group)'s K best, k_sc_many_select merges a query's lists into its
// row.  The arithmetic of a pair is s2m_sc_dist.hpp's, the functions the single query calls: a row is bit for bit the single
// query's.  Compiled with -ffp-contract=off; no fused multiply-add, no MFMA.  The order of the hits is (distance, key), a total
// order, and membership in the searched set is a predicate on the pair: the result does not depend on how tiles, query blocks
// or passes cut the work, no kernel uses atomics and none waits for another.
#include <limits.h>
#include <math.h>
#include <type_traits>

#include "s2m_sc_dist.hpp"
#include "s2m_sc_keys.hpp"
#include "s2m_sc_many.hpp"
#include "s2m_sc_rank.hpp"

namespace s2m {

namespace {

constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR, ND = NR * NS;
constexpr int T = kScManyTile, B = kScManyBlock;
constexpr int kLanes = 4;              // full alignment: thread (g, j), g < 4, owns sector j of the queries and the shifts 4 ch + g
constexpr int kChunks = NS / kLanes;   // ... of the 15 chunks
constexpr int NQ = 2;                  // ... for two queries side by side: a candidate value read from LDS serves both
constexpr int kPrepThreads = 64;
static_assert(NS % kLanes == 0 && kLanes * NS <= kScThreads, "the chunks cover the 60 shifts, one thread per (lane, sector)");
static_assert(NQ * T * kLanes <= 64, "one wave takes the sector sums of a chunk");
static_assert(B % NQ == 0 && T * NS <= kScThreads && T * kScShifts <= kScThreads, "one thread per task");
static_assert(ND % 2 == 0 && NS % 2 == 0, "descriptors and sector keys are staged two doubles at a time");
static_assert(kScManyMaxGroups == 64, "k_sc_many_select: one lane per list");

struct ScManyDev {                     // what the kernels read of ScManyArgs
    const double* store_desc; const double* store_sector;
    const int32_t* keys; const double* ext_desc; const double* ext_sector; const double* qnorm;
    int m;
    ScManySet set;
    int top_k;
    double max_dist;
};

__device__ __forceinline__ const double* sc_many_qdesc(const ScManyDev& a, int i)
{
    return a.keys ? a.store_desc + (size_t)a.keys[i] * ND : a.ext_desc + (size_t)i * ND;
}
__device__ __forceinline__ const double* sc_many_qsector(const ScManyDev& a, int i)
{
    return a.keys ? a.store_sector + (size_t)a.keys[i] * NS : a.ext_sector + (size_t)i * NS;
}

// One workgroup per query: the 60 column norms, and for an external descriptor its sector key (makeSectorkeyFromScancontext).
__global__ __launch_bounds__(kPrepThreads) void k_sc_many_prepare(ScManyDev a, double* __restrict__ ext_sector, double* __restrict__ qnorm)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (t >= NS) return;
    const double* __restrict__ q = sc_many_qdesc(a, i);
    const auto col = [&](int r) { return q[r * NS + t]; };
    qnorm[(size_t)i * NS + t] = sc_col_norm(col);
    if (!a.keys) sc_ext_keys(q, t, ext_sector + (size_t)i * NS, nullptr);
}

// the tile: T stored descriptors, their column norms and (sector-key alignment) sector keys
template <int ALIGN>
struct alignas(16) ScManyTile {
    double c[T][ND];
    double cnorm[T][NS];
    double ckey[ALIGN == S2M_SC_ALIGN_FULL ? 1 : T][NS];
};

// full alignment: two buffers of one chunk's similarities (the sums of chunk ch run beside the dot products of chunk ch + 1)
struct alignas(16) ScManyFull {
    double sim[2][NQ][T][kLanes][NS];
    unsigned char eff[2][NQ][T][kLanes][NS];
    double dist_out[NQ][T][kLanes];    // per lane g: the strict minimum over its shifts g, g + 4, ... ascending
    int    shift_out[NQ][T][kLanes];
};

// sector-key alignment: the query, staged, and distanceBtnScanContext's intermediate values for the T candidates
struct alignas(16) ScManySk {
    double q[ND], qkey[NS], qnorm[NS];
    double vnorm[T][NS];
    int    shifts[T][kScShifts];
    double sim[T][kScShifts][NS];
    unsigned char eff[T][kScShifts][NS];
    double dist[T][kScShifts];
};

template <int ALIGN>
__global__ __launch_bounds__(kScThreads) void k_sc_many_dist(ScManyDev a, double* __restrict__ part_d, int2* __restrict__ part_ks)
{
    using Scratch = typename std::conditional<ALIGN == S2M_SC_ALIGN_FULL, ScManyFull, ScManySk>::type;
    __shared__ ScManyTile<ALIGN> s_t;
    __shared__ Scratch s_m;
    __shared__ double s_hd[B][S2M_SC_QUERY_MAX_K];        // the block's lists: every query's best of this group's tiles so far
    __shared__ int    s_hk[B][S2M_SC_QUERY_MAX_K], s_hs[B][S2M_SC_QUERY_MAX_K];
    __shared__ int    s_held[B], s_qkey[B];
    const int t = threadIdx.x;
    const int q0 = blockIdx.y * B, nq = min(B, a.m - q0);
    const int n_tiles = (a.set.end - a.set.first + T - 1) / T;
    if (t < B) { s_held[t] = 0; s_qkey[t] = (a.keys && t < nq) ? a.keys[q0 + t] : -1; }
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int c0 = a.set.first + tile * T, nc = min(T, a.set.end - c0);
        __syncthreads();                                  // the previous tile is read until here
        for (int task = t; task < T * (ND / 2); task += kScThreads) {
            const int c = task / (ND / 2), k = task - c * (ND / 2);   // (slots are 9600 bytes: 16-byte aligned); a short last tile is padded with empty descriptors
            reinterpret_cast<double2*>(s_t.c[c])[k] = c < nc ? reinterpret_cast<const double2*>(a.store_desc + (size_t)(c0 + c) * ND)[k] : make_double2(0.0, 0.0);
        }
        if constexpr (ALIGN != S2M_SC_ALIGN_FULL)
            for (int task = t; task < T * NS; task += kScThreads) {
                const int c = task / NS, j = task - c * NS;
                s_t.ckey[c][j] = c < nc ? a.store_sector[(size_t)(c0 + c) * NS + j] : 0.0;
            }
        __syncthreads();
        if (t < T * NS) {
            const int c = t / NS, jc = t - c * NS;
            s_t.cnorm[c][jc] = sc_col_norm([&](int r) { return s_t.c[c][r * NS + jc]; });
        }
        __syncthreads();
        if constexpr (ALIGN == S2M_SC_ALIGN_FULL) {
            // min over s = 0..59 ascending of distDirectSC(query, circshift(cand, s)) for NQ queries x T candidates side by side
            const int g = t / NS, j = t - g * NS;
            const int su = t / (T * kLanes), sc = (t / kLanes) % T, sg = t % kLanes;   // t < NQ * T * 4: the sums of (query su, candidate sc, lane sg)
            for (int qq = 0; qq < nq; qq += NQ) {
                double qcol[NQ][NR], n1[NQ];
#pragma unroll
                for (int u = 0; u < NQ; u++) {
                    const int qi = q0 + qq + (qq + u < nq ? u : 0);      // an odd tail compares its first query again and drops the result
                    const double* __restrict__ q = sc_many_qdesc(a, qi);
                    const int jq = g < kLanes ? j : 0;
#pragma unroll
                    for (int r = 0; r < NR; r++) qcol[u][r] = q[r * NS + jq];
                    n1[u] = a.qnorm[(size_t)qi * NS + jq];
                }
                double best = 10000000; int best_shift = 0;
                for (int ch = 0; ch < kChunks; ch++) {
                    const int buf = ch & 1;
                    if (g < kLanes) {
                        int j2 = j - (ch * kLanes + g); j2 += (j2 < 0) ? NS : 0;   // circshift (:39-59)
#pragma unroll
                        for (int c = 0; c < T; c++) {
                            double b[NR];
#pragma unroll
                            for (int r = 0; r < NR; r++) b[r] = s_t.c[c][r * NS + j2];
                            const double n2 = s_t.cnorm[c][j2];
#pragma unroll
                            for (int u = 0; u < NQ; u++) {
                                const double dot = sc_col_dot([&](int r) { return qcol[u][r]; }, [&](int r) { return b[r]; });
                                s_m.eff[buf][u][c][g][j] = sc_sector_sim(dot, n1[u], n2, &s_m.sim[buf][u][c][g][j]) ? 1 : 0;
                            }
                        }
                    }
                    __syncthreads();                      // (buffer `buf` is written again two chunks on, behind the next barrier)
                    if (t < NQ * T * kLanes) {
                        const double d = sc_sector_sum_dist([&](int jj) { return s_m.eff[buf][su][sc][sg][jj] != 0; },
                                                            [&](int jj) { return s_m.sim[buf][su][sc][sg][jj]; });
                        sc_min_update(d, ch * kLanes + sg, &best, &best_shift);
                    }
                }
                if (t < NQ * T * kLanes) { s_m.dist_out[su][sc][sg] = best; s_m.shift_out[su][sc][sg] = best_shift; }
                __syncthreads();
                if (t < NQ && qq + t < nq) {
                    for (int c = 0; c < nc; c++) {
                        // the lanes' minima into the minimum over all shifts ascending: the smallest distance, at its lowest shift
                        double d = 10000000; int shift = 0;
                        for (int gg = 0; gg < kLanes; gg++) {
                            const double dg = s_m.dist_out[t][c][gg];
                            const int sgg = s_m.shift_out[t][c][gg];
                            if (dg < d || (dg == d && dg < 10000000 && sgg < shift)) { d = dg; shift = sgg; }
                        }
                        if (d < a.max_dist && sc_many_in_set(a.set, s_qkey[qq + t], c0 + c))
                            sc_hit_insert(s_hd[qq + t], s_hk[qq + t], s_hs[qq + t], &s_held[qq + t], a.top_k, d, c0 + c, shift);
                    }
                }
                // (dist_out is written again behind the barriers of the next query pair's chunks)
            }
        } else {
            // distanceBtnScanContext(query, cand) (:116-148) for one query x T candidates side by side
            for (int qq = 0; qq < nq; qq++) {
                const int qi = q0 + qq;
                __syncthreads();                          // the scratch may still be read from the previous query
                {
                    const double* __restrict__ q = sc_many_qdesc(a, qi);
                    const double* __restrict__ qk = sc_many_qsector(a, qi);
                    for (int k = t; k < ND / 2; k += kScThreads) reinterpret_cast<double2*>(s_m.q)[k] = reinterpret_cast<const double2*>(q)[k];
                    if (t < NS) { s_m.qkey[t] = qk[t]; s_m.qnorm[t] = a.qnorm[(size_t)qi * NS + t]; }
                }
                __syncthreads();
                if (t < T * NS) {                         // fastAlignUsingVkey (:94-113), one shift per thread
                    const int c = t / NS, s = t - c * NS;
                    s_m.vnorm[c][s] = sc_vkey_shift_norm([&](int jj) { return s_m.qkey[jj]; }, [&](int jj) { return s_t.ckey[c][jj]; }, s);
                }
                __syncthreads();
                if (t < T) {
                    int sp[kScShifts];
                    sc_search_shifts([&](int s) { return s_m.vnorm[t][s]; }, sp);
                    for (int k = 0; k < kScShifts; k++) s_m.shifts[t][k] = sp[k];
                }
                __syncthreads();
                for (int task = t; task < T * kScShifts * NS; task += kScThreads) {   // distDirectSC (:69-91), one sector pair per task
                    const int c = task / (kScShifts * NS), rem = task - c * (kScShifts * NS);
                    const int k = rem / NS, j = rem - k * NS;
                    int j2 = j - s_m.shifts[c][k]; j2 += (j2 < 0) ? NS : 0;
                    const double dot = sc_col_dot([&](int r) { return s_m.q[r * NS + j]; }, [&](int r) { return s_t.c[c][r * NS + j2]; });
                    s_m.eff[c][k][j] = sc_sector_sim(dot, s_m.qnorm[j], s_t.cnorm[c][j2], &s_m.sim[c][k][j]) ? 1 : 0;
                }
                __syncthreads();
                if (t < T * kScShifts) {
                    const int c = t / kScShifts, k = t - c * kScShifts;
                    s_m.dist[c][k] = sc_sector_sum_dist([&](int jj) { return s_m.eff[c][k][jj] != 0; }, [&](int jj) { return s_m.sim[c][k][jj]; });
                }
                __syncthreads();
                if (t == 0) {
                    for (int c = 0; c < nc; c++) {
                        double d = 10000000; int shift = 0;
                        for (int k = 0; k < kScShifts; k++) sc_min_update(s_m.dist[c][k], s_m.shifts[c][k], &d, &shift);
                        if (d < a.max_dist && sc_many_in_set(a.set, s_qkey[qq], c0 + c))
                            sc_hit_insert(s_hd[qq], s_hk[qq], s_hs[qq], &s_held[qq], a.top_k, d, c0 + c, shift);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int task = t; task < nq * a.top_k; task += kScThreads) {
        const int qq = task / a.top_k, k = task - qq * a.top_k;
        sc_hit_store(part_d, part_ks, ((size_t)(q0 + qq) * gridDim.x + blockIdx.x) * a.top_k + k, s_hd[qq], s_hk[qq], s_hs[qq], s_held[qq], k);
    }
}

// One wave per query: lane l holds the head of the list of tile group l (ascending, padded with (inf, INT_MAX)); every round the
// smallest head by (distance, key) is found by a butterfly, lane 0 writes it as the next hit and its owner moves on.
__global__ __launch_bounds__(kScThreads) void k_sc_many_select(const double* __restrict__ part_d, const int2* __restrict__ part_ks, int m, int groups,
                                                               int top_k, s2m_sc_hit* __restrict__ out_hits, int32_t* __restrict__ out_n)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (kScThreads / 64) + (threadIdx.x >> 6);
    if (qi >= m) return;                                  // (a whole wave: no barrier follows)
    int head = 0, n_hits = 0;
    for (int round = 0; round < top_k; round++) {
        double bd = INFINITY; int bk = INT_MAX, bs = 0, bg = -1;
        if (lane < groups && head < top_k) {
            const size_t e = ((size_t)qi * groups + lane) * top_k + head;
            const double d = part_d[e];
            const int2 ks = part_ks[e];
            if (sc_hit_less(d, ks.x, bd, bk)) { bd = d; bk = ks.x; bs = ks.y; bg = lane; }
        }
        sc_hit_wave_min(bd, bk, bs, bg);
        if (bg < 0) break;                                // every list is used up (the same for all lanes)
        if (lane == 0) out_hits[(size_t)qi * top_k + round] = sc_hit_record(bd, bk, bs);
        n_hits = round + 1;
        if (bg == lane) head++;
    }
    if (lane == 0) out_n[qi] = n_hits;
}

}  // namespace

hipError_t sc_many_launch(hipStream_t stream, const ScManyArgs& a)
{
    const int groups = sc_many_groups(a.set.end - a.set.first);
    const ScManyDev d{ a.store_desc, a.store_sector, a.keys, a.ext_desc, a.ext_sector, a.qnorm, a.m, a.set, a.top_k, a.max_dist };
    double* part_d = reinterpret_cast<double*>(a.part);
    int2* part_ks = reinterpret_cast<int2*>(a.part + sizeof(double) * (size_t)a.m * (size_t)groups * (size_t)a.top_k);
    const dim3 grid(groups, (a.m + kScManyBlock - 1) / kScManyBlock);
    hipLaunchKernelGGL(k_sc_many_prepare, dim3(a.m), dim3(kPrepThreads), 0, stream, d, a.ext_sector, a.qnorm);
    if (a.align == S2M_SC_ALIGN_FULL)
        hipLaunchKernelGGL(k_sc_many_dist<S2M_SC_ALIGN_FULL>, grid, dim3(kScThreads), 0, stream, d, part_d, part_ks);
    else
        hipLaunchKernelGGL(k_sc_many_dist<S2M_SC_ALIGN_SECTOR_KEY>, grid, dim3(kScThreads), 0, stream, d, part_d, part_ks);
    hipLaunchKernelGGL(k_sc_many_select, dim3((a.m + kScThreads / 64 - 1) / (kScThreads / 64)), dim3(kScThreads), 0, stream, (const double*)part_d,
                       (const int2*)part_ks, a.m, groups, a.top_k, a.out_hits, a.out_n);
    return hipGetLastError();
}

}  // namespace s2m
