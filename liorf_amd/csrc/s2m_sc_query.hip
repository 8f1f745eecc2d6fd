// s2m_sc_query.hip — kernels of the ScanContext place query (s2m_sc_query.hpp): one query descriptor
// against every stored descriptor of a range, the K nearest under a threshold.  k_sc_query_prepare fills the query slot,
// k_sc_query_dist<ALIGN> computes the distances (three candidates per workgroup at a time) and keeps every workgroup's K best,
// k_sc_query_select merges those lists and writes the hit records where the host reads them.  Compiled with -ffp-contract=off;
// every sum runs left to right in fp64 like the oracle's restatement of include/Scancontext.cpp:69-148, so distances are
// bit-identical to it.  The order of the hits is (distance, key), a total order: the result does not depend on how the
// searched set is cut over workgroups, and the kernels need no atomics and never wait for one another.
#include <limits.h>
#include <math.h>
#include <type_traits>

#include "s2m_sc_dist.hpp"
#include "s2m_sc_keys.hpp"
#include "s2m_sc_query.hpp"
#include "s2m_sc_rank.hpp"

namespace s2m {

namespace {

constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR, ND = NR * NS;
static_assert(ND % 2 == 0 && NS % 2 == 0, "descriptors and sector keys are staged two doubles at a time");

// the query's descriptor and sector key into the slot.  src_desc may be the slot itself (a descriptor uploaded in place).
__global__ __launch_bounds__(kScThreads) void k_sc_query_prepare(const double* src_desc, const double* src_sector, double* slot)
{
    const int t = threadIdx.x;
    if (!src_sector) sc_ext_keys(src_desc, t, slot + ND, nullptr);     // makeSectorkeyFromScancontext (:214-227) as k_sc_append
    else if (t < NS) slot[ND + t] = src_sector[t];
    if (src_desc != slot)
        for (int k = t; k < ND; k += kScThreads) slot[k] = src_desc[k];
}

template <int ALIGN>
__global__ __launch_bounds__(kScThreads) void k_sc_query_dist(const double* __restrict__ store_desc, const double* __restrict__ store_sector,
                                                              const double* __restrict__ slot, int first, int n_before, int skip, int n_s,
                                                              int top_k, double max_dist, double* __restrict__ part_d, int2* __restrict__ part_ks)
{
    using Scratch = typename std::conditional<ALIGN == S2M_SC_ALIGN_FULL, ScFullShared<kScQueryCands>, ScShared[kScQueryCands]>::type;
    __shared__ Scratch s_m;
    __shared__ int    s_cand[kScQueryCands];
    __shared__ double s_hd[S2M_SC_QUERY_MAX_K];          // this workgroup's best, ascending (distance, key)
    __shared__ int    s_hk[S2M_SC_QUERY_MAX_K], s_hs[S2M_SC_QUERY_MAX_K];
    __shared__ double s_q[ALIGN == S2M_SC_ALIGN_FULL ? 1 : ND], s_qkey[ALIGN == S2M_SC_ALIGN_FULL ? 1 : NS];   // sector-key mode: the query, staged once
    const int t = threadIdx.x;
    double qcol[NR], n1 = 0.0;                            // full mode: column t % 60 of the query and its norm
    if constexpr (ALIGN == S2M_SC_ALIGN_FULL) {
        const int j = t % NS;
#pragma unroll
        for (int r = 0; r < NR; r++) qcol[r] = slot[r * NS + j];
        n1 = sc_col_norm([&](int r) { return qcol[r]; });
    } else {
        for (int k = t; k < (ND + NS) / 2; k += kScThreads) {
            const double2 v = reinterpret_cast<const double2*>(slot)[k];
            double* dst = (k < ND / 2) ? &s_q[2 * k] : &s_qkey[2 * k - ND];
            dst[0] = v.x; dst[1] = v.y;
        }
    }
    int n_held = 0;                                       // (thread 0's)
    for (int i0 = blockIdx.x * kScQueryCands; i0 < n_s; i0 += gridDim.x * kScQueryCands) {
        const int nc = min(kScQueryCands, n_s - i0);
        if (t < kScQueryCands) {
            const int i = i0 + (t < nc ? t : 0);          // a short tail compares its first key again and drops the result
            s_cand[t] = first + i + (i >= n_before ? skip : 0);
        }
        __syncthreads();                                  // s_cand is written (and the scratch free since the previous triple's last barrier)
        if constexpr (ALIGN == S2M_SC_ALIGN_FULL) { sc_full_block(store_desc, qcol, n1, s_cand, s_m); __syncthreads(); }   // thread 0 reads three threads' results
        else sc_distance_block<kScQueryCands>(store_desc, store_sector, s_q, s_qkey, s_cand, s_m);
        if (t == 0) {
            for (int c = 0; c < nc; c++) {
                double d; int shift;
                if constexpr (ALIGN == S2M_SC_ALIGN_FULL) { d = s_m.dist_out[c]; shift = s_m.shift_out[c]; }
                else { d = s_m[c].dist_out; shift = s_m[c].shift_out; }
                if (d < max_dist) sc_hit_insert(s_hd, s_hk, s_hs, &n_held, top_k, d, s_cand[c], shift);
            }
        }
        __syncthreads();                                  // s_cand is read until here
    }
    if (t == 0)
        for (int k = 0; k < top_k; k++) sc_hit_store(part_d, part_ks, (size_t)blockIdx.x * top_k + k, s_hd, s_hk, s_hs, n_held, k);
}

// The workgroups' lists (each ascending, padded with (inf, INT_MAX)) into the final K: thread t holds the heads of lists t,
// t + 256, ...; every round the smallest head by (distance, key) is found by a butterfly inside each wave and over the four
// waves through LDS, thread 0 writes it as the next hit and its owner moves on.  `out` is pinned host memory.
__global__ __launch_bounds__(kScThreads) void k_sc_query_select(const double* __restrict__ part_d, const int2* __restrict__ part_ks, int groups,
                                                                int top_k, ScQueryOut* __restrict__ out)
{
    constexpr int kLists = kScQueryMaxGroups / kScThreads;
    __shared__ double w_d[kScThreads / 64];
    __shared__ int    w_k[kScThreads / 64], w_s[kScThreads / 64], w_g[kScThreads / 64];
    const int t = threadIdx.x;
    int head[kLists];
#pragma unroll
    for (int u = 0; u < kLists; u++) head[u] = 0;
    int n_hits = 0;
    for (int round = 0; round < top_k; round++) {
        double bd = INFINITY; int bk = INT_MAX, bs = 0, bg = -1;
#pragma unroll
        for (int u = 0; u < kLists; u++) {
            const int g = t + u * kScThreads;
            if (g < groups && head[u] < top_k) {
                const size_t e = (size_t)g * top_k + head[u];
                const double d = part_d[e];
                const int2 ks = part_ks[e];
                if (sc_hit_less(d, ks.x, bd, bk)) { bd = d; bk = ks.x; bs = ks.y; bg = g; }
            }
        }
        sc_hit_wave_min(bd, bk, bs, bg);
        if ((t & 63) == 0) { w_d[t >> 6] = bd; w_k[t >> 6] = bk; w_s[t >> 6] = bs; w_g[t >> 6] = bg; }
        __syncthreads();
        bd = w_d[0]; bk = w_k[0]; bs = w_s[0]; bg = w_g[0];
#pragma unroll
        for (int w = 1; w < kScThreads / 64; w++)
            if (sc_hit_less(w_d[w], w_k[w], bd, bk)) { bd = w_d[w]; bk = w_k[w]; bs = w_s[w]; bg = w_g[w]; }
        __syncthreads();                                  // w_* are written again in the next round
        if (bg < 0) break;                                // every list is used up (the same for all threads)
        if (t == 0) out->hits[round] = sc_hit_record(bd, bk, bs);
        n_hits = round + 1;
#pragma unroll
        for (int u = 0; u < kLists; u++)
            if (bg == t + u * kScThreads) head[u]++;
    }
    if (t == 0) out->n_hits = n_hits;
}

}  // namespace

hipError_t sc_query_launch(hipStream_t stream, const ScQueryArgs& a)
{
    const int groups = sc_query_groups(a.n_s);
    double* part_d = reinterpret_cast<double*>(a.part);
    int2* part_ks = reinterpret_cast<int2*>(a.part + sizeof(double) * (size_t)groups * (size_t)a.top_k);
    hipLaunchKernelGGL(k_sc_query_prepare, dim3(1), dim3(kScThreads), 0, stream, a.src_desc, a.src_sector, a.slot);
    if (a.align == S2M_SC_ALIGN_FULL)
        hipLaunchKernelGGL(k_sc_query_dist<S2M_SC_ALIGN_FULL>, dim3(groups), dim3(kScThreads), 0, stream, a.store_desc, a.store_sector,
                           (const double*)a.slot, a.first, a.n_before, a.skip, a.n_s, a.top_k, a.max_dist, part_d, part_ks);
    else
        hipLaunchKernelGGL(k_sc_query_dist<S2M_SC_ALIGN_SECTOR_KEY>, dim3(groups), dim3(kScThreads), 0, stream, a.store_desc, a.store_sector,
                           (const double*)a.slot, a.first, a.n_before, a.skip, a.n_s, a.top_k, a.max_dist, part_d, part_ks);
    hipLaunchKernelGGL(k_sc_query_select, dim3(1), dim3(kScThreads), 0, stream, (const double*)part_d, (const int2*)part_ks, groups, a.top_k, a.out);
    return hipGetLastError();
}

}  // namespace s2m
