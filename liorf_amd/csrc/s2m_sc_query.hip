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

namespace s2m {

namespace {

constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR, ND = NR * NS;
constexpr int kScFullChunk = 12;       // shifts of the full alignment a workgroup evaluates between two barriers
constexpr int kScFullLanes = 4;        // ... by 4 x 60 threads: thread (g, j) owns sector j of the query and the shifts g, g + 4, ... of a chunk
static_assert(NS % kScFullChunk == 0 && kScFullChunk % kScFullLanes == 0, "the chunks cover the 60 shifts");
static_assert(kScFullLanes * NS <= kScThreads && kScQueryCands * kScFullChunk <= kScThreads, "one thread per task");
static_assert(ND % 2 == 0 && NS % 2 == 0, "descriptors and sector keys are staged two doubles at a time");

__device__ __forceinline__ bool sc_hit_less(double da, int ka, double db, int kb) { return da < db || (da == db && ka < kb); }

// the query's descriptor and sector key into the slot.  src_desc may be the slot itself (a descriptor uploaded in place).
__global__ __launch_bounds__(kScThreads) void k_sc_query_prepare(const double* src_desc, const double* src_sector, double* slot)
{
    const int t = threadIdx.x;
    if (t < NS) {
        // makeSectorkeyFromScancontext (:214-227) as k_sc_append
        slot[ND + t] = src_sector ? src_sector[t] : sc_sector_key([&](int r) { return src_desc[r * NS + t]; });
    }
    if (src_desc != slot)
        for (int k = t; k < ND; k += kScThreads) slot[k] = src_desc[k];
}

// LDS of the full alignment: the three candidates, their column norms, one chunk of similarities
struct alignas(16) ScFullShared {
    double c[kScQueryCands][ND];
    double cnorm[kScQueryCands][NS];
    double sim[kScQueryCands][kScFullChunk][NS];
    unsigned char eff[kScQueryCands][kScFullChunk][NS];
    double dist[kScQueryCands][kScFullChunk];
    double dist_out[kScQueryCands];
    int    shift_out[kScQueryCands];
};

// min over s = 0..59 ascending of distDirectSC(query, circshift(cand[c], s)) (:69-91), strict, from 10000000 / shift 0, for the
// three candidates side by side.  A column's norm does not depend on the shift it is paired with: 60 norms per descriptor, then
// one independent left-to-right dot product of 20 terms per (shift, sector).  Thread (g, j) = (t / 60, t % 60), t < 240, holds
// column j of the query (qcol) and its norm (n1) in registers for the whole kernel, so a term costs one LDS read.
__device__ __forceinline__ void sc_full_block(const double* __restrict__ store_desc, const double (&qcol)[NR], double n1, const int* cand,
                                              ScFullShared& m)
{
    const int t = threadIdx.x;
    const int g = t / NS, j = t - g * NS;
    __syncthreads();                                     // the scratch may still be read from the previous triple
    for (int task = t; task < kScQueryCands * (ND / 2); task += kScThreads) {
        const int c = task / (ND / 2), k = task - c * (ND / 2);
        reinterpret_cast<double2*>(m.c[c])[k] = reinterpret_cast<const double2*>(store_desc + (size_t)cand[c] * ND)[k];   // (slots are 9600 bytes: 16-byte aligned)
    }
    if (t < kScQueryCands) { m.dist_out[t] = 10000000; m.shift_out[t] = 0; }
    __syncthreads();
    for (int task = t; task < kScQueryCands * NS; task += kScThreads) {
        const int c = task / NS, jc = task - c * NS;
        m.cnorm[c][jc] = sc_col_norm([&](int r) { return m.c[c][r * NS + jc]; });
    }
    __syncthreads();
    for (int s0 = 0; s0 < NS; s0 += kScFullChunk) {
        if (g < kScFullLanes) {
            for (int k = g; k < kScFullChunk; k += kScFullLanes) {
                int j2 = j - (s0 + k); j2 += (j2 < 0) ? NS : 0;            // circshift (:39-59)
#pragma unroll
                for (int c = 0; c < kScQueryCands; c++) {
                    const double dot = sc_col_dot([&](int r) { return qcol[r]; }, [&](int r) { return m.c[c][r * NS + j2]; });
                    m.eff[c][k][j] = sc_sector_sim(dot, n1, m.cnorm[c][j2], &m.sim[c][k][j]) ? 1 : 0;
                }
            }
        }
        __syncthreads();
        if (t < kScQueryCands * kScFullChunk) {
            const int c = t / kScFullChunk, k = t - c * kScFullChunk;
            m.dist[c][k] = sc_sector_sum_dist([&](int jj) { return m.eff[c][k][jj] != 0; }, [&](int jj) { return m.sim[c][k][jj]; });
        }
        __syncthreads();
        if (t < kScQueryCands)
            for (int k = 0; k < kScFullChunk; k++)
                sc_min_update(m.dist[t][k], s0 + k, &m.dist_out[t], &m.shift_out[t]);
        // (the next chunk writes sim / eff only; dist is written again behind its barrier)
    }
    __syncthreads();
}

template <int ALIGN>
__global__ __launch_bounds__(kScThreads) void k_sc_query_dist(const double* __restrict__ store_desc, const double* __restrict__ store_sector,
                                                              const double* __restrict__ slot, int first, int n_before, int skip, int n_s,
                                                              int top_k, double max_dist, double* __restrict__ part_d, int2* __restrict__ part_ks)
{
    using Scratch = typename std::conditional<ALIGN == S2M_SC_ALIGN_FULL, ScFullShared, ScShared[kScQueryCands]>::type;
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
        __syncthreads();
        if constexpr (ALIGN == S2M_SC_ALIGN_FULL) sc_full_block(store_desc, qcol, n1, s_cand, s_m);
        else sc_distance_block<kScQueryCands>(store_desc, store_sector, s_q, s_qkey, s_cand, s_m);
        if (t == 0) {
            for (int c = 0; c < nc; c++) {
                double d; int shift;
                if constexpr (ALIGN == S2M_SC_ALIGN_FULL) { d = s_m.dist_out[c]; shift = s_m.shift_out[c]; }
                else { d = s_m[c].dist_out; shift = s_m[c].shift_out; }
                const int key = s_cand[c];
                if (!(d < max_dist)) continue;
                if (n_held == top_k && !sc_hit_less(d, key, s_hd[top_k - 1], s_hk[top_k - 1])) continue;
                int p = (n_held < top_k) ? n_held++ : top_k - 1;
                while (p > 0 && sc_hit_less(d, key, s_hd[p - 1], s_hk[p - 1])) { s_hd[p] = s_hd[p - 1]; s_hk[p] = s_hk[p - 1]; s_hs[p] = s_hs[p - 1]; p--; }
                s_hd[p] = d; s_hk[p] = key; s_hs[p] = shift;
            }
        }
        __syncthreads();                                  // s_cand is read until here
    }
    if (t == 0)
        for (int k = 0; k < top_k; k++) {
            const bool have = k < n_held;
            part_d[(size_t)blockIdx.x * top_k + k] = have ? s_hd[k] : INFINITY;
            part_ks[(size_t)blockIdx.x * top_k + k] = make_int2(have ? s_hk[k] : INT_MAX, have ? s_hs[k] : 0);
        }
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
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int ok = __shfl_xor(bk, off, 64), os = __shfl_xor(bs, off, 64), og = __shfl_xor(bg, off, 64);
            if (sc_hit_less(od, ok, bd, bk)) { bd = od; bk = ok; bs = os; bg = og; }
        }
        if ((t & 63) == 0) { w_d[t >> 6] = bd; w_k[t >> 6] = bk; w_s[t >> 6] = bs; w_g[t >> 6] = bg; }
        __syncthreads();
        bd = w_d[0]; bk = w_k[0]; bs = w_s[0]; bg = w_g[0];
#pragma unroll
        for (int w = 1; w < kScThreads / 64; w++)
            if (sc_hit_less(w_d[w], w_k[w], bd, bk)) { bd = w_d[w]; bk = w_k[w]; bs = w_s[w]; bg = w_g[w]; }
        __syncthreads();                                  // w_* are written again in the next round
        if (bg < 0) break;                                // every list is used up (the same for all threads)
        if (t == 0) {
            s2m_sc_hit hit;
            hit.dist = bd; hit.key = bk; hit.shift = bs; hit.yaw_diff_rad = sc_shift_to_yaw(bs); hit.reserved = 0;
            out->hits[round] = hit;
        }
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
