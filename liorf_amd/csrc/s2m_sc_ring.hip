// s2m_sc_ring.hip — kernels of the ring-key prefilter of the ScanContext place query (s2m_sc_ring.hpp):
// the two-stage search of detectLoopClosureID (reference include/Scancontext.cpp:253-344) for any query, any candidate count,
// any searched set and many queries at once.  k_sc_ring_prepare leaves an external descriptor's fp32 ring key and sector key,
// k_sc_ring_select holds a tile of stored ring keys in LDS while a block of queries passes it and keeps every query's
// n_candidates nearest, k_sc_ring_dist<ALIGN> compares a query with its candidates three at a time, k_sc_ring_rank writes a
// query's row.  The ring-key distance is sc_ring_d2 (s2m_sc_keys.hpp), the statement k_sc_detect uses; the arithmetic of a
// descriptor pair is s2m_sc_dist.hpp's, the functions every other query calls.  Compiled with -ffp-contract=off; no fused
// multiply-add, no MFMA.  Both orders - (d2, key) of the neighbours, (distance, key) of the hits - are total orders and
// membership in the searched set is a predicate on the pair: the result does not depend on how tiles, query blocks or passes cut
// the work.  No kernel uses atomics, none waits for another, and no loop spins.
#include <limits.h>
#include <math.h>

#include "s2m_sc_dist.hpp"
#include "s2m_sc_keys.hpp"
#include "s2m_sc_rank.hpp"
#include "s2m_sc_ring.hpp"

namespace s2m {

namespace {

constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR, ND = NR * NS;
constexpr int NG = NR / 4;                            // float4 of a ring key
constexpr int T = kScRingTile, B = kScRingBlock, BUF = kScRingBuf;
constexpr int kSelThreads = 64;                       // k_sc_ring_select: one wave a workgroup, so every barrier is the wave's own
constexpr int kOwn = BUF / kSelThreads;               // buffer words a lane ranks in a prune
constexpr int NC = kScRingCands;
constexpr unsigned long long kRingInf = 0x7f800000ull << 32;   // bits(+inf) << 32: a word below it is a neighbour
static_assert(NR % 4 == 0 && BUF % kSelThreads == 0 && T % kSelThreads == 0, "whole float4, whole wave steps");
static_assert(S2M_SC_RING_MAX_CAND <= 4 * 64, "k_sc_ring_rank: four records a lane");
static_assert(sizeof(s2m_sc_ring_neighbour) == 8, "a neighbour is (d2, key)");

// One workgroup per external descriptor: its ring key as s2m_sc_add_descriptor stores it ((float) of the row mean) and its
// sector key (makeSectorkeyFromScancontext): sc_ext_keys.
__global__ __launch_bounds__(64) void k_sc_ring_prepare(const double* __restrict__ ext_desc, double* __restrict__ ext_sector, float* __restrict__ ext_ring)
{
    const int i = blockIdx.x;
    sc_ext_keys(ext_desc + (size_t)i * ND, threadIdx.x, ext_sector + (size_t)i * NS, ext_ring + (size_t)i * NR);
}

// buf[0, held): distinct words in any order -> buf[0, min(held, n_cand)): the smallest, ascending.  Every lane counts, for each
// of its words, the words below it; that rank is the word's place.  Returns the new fill; *thr becomes the largest word kept once
// n_cand are held: what comes later is a neighbour only below it.  (One wave: held and *thr are the same in every lane.)
__device__ __forceinline__ int sc_ring_prune(unsigned long long* buf, int held, int n_cand, unsigned long long* thr)
{
    const int lane = threadIdx.x;
    unsigned long long e[kOwn];
    int rank[kOwn];
    __syncthreads();                                      // the appends are in the buffer
#pragma unroll
    for (int u = 0; u < kOwn; u++) { const int idx = lane + u * kSelThreads; e[u] = idx < held ? buf[idx] : ~0ull; rank[u] = 0; }
    for (int k = 0; k < held; k++) {
        const unsigned long long w = buf[k];
#pragma unroll
        for (int u = 0; u < kOwn; u++) rank[u] += (w < e[u]) ? 1 : 0;
    }
    __syncthreads();                                      // every word is read
#pragma unroll
    for (int u = 0; u < kOwn; u++)
        if (lane + u * kSelThreads < held && rank[u] < n_cand) buf[rank[u]] = e[u];   // (rank < held <= BUF)
    __syncthreads();
    if (held >= n_cand) { *thr = buf[n_cand - 1]; return n_cand; }
    return held;
}

// Stage one.  d2 >= +0, so the word (bits of d2) << 32 | key orders exactly as (d2, key) and a NaN or an infinity is no word below
// kRingInf.  Per query a buffer of BUF words in LDS and a running threshold: a lane whose pair is in the searched set and below
// the threshold appends its word (ballot and prefix); a buffer that would overflow is pruned to the n_cand smallest first.  Of two
// exact, order-independent shapes this one needs no partial lists in global memory - at 256 candidates a list per (query, tile
// group) would be 2 KB each and the merge a kernel of its own - and one query's whole scan stays inside one wave.
__global__ __launch_bounds__(kSelThreads) void k_sc_ring_select(const float* __restrict__ store_ring, const int32_t* __restrict__ keys,
                                                                const float* __restrict__ ext_ring, int m, ScManySet set, int n_cand,
                                                                s2m_sc_ring_neighbour* __restrict__ cand, int32_t* __restrict__ n_out)
{
    __shared__ float4 s_tile[NG][T];                      // the tile, one float4 group after another: lanes read neighbouring slots
    __shared__ unsigned long long s_buf[B][BUF];
    const int lane = threadIdx.x;
    const int q0 = blockIdx.x * B, nq = min(B, m - q0);
    const int cap = min(BUF, 2 * n_cand + kSelThreads);   // few candidates: prune early, a prune costs held^2
    int held[B], qkey[B];
    unsigned long long thr[B];
#pragma unroll
    for (int qq = 0; qq < B; qq++) { held[qq] = 0; thr[qq] = kRingInf; qkey[qq] = (keys && qq < nq) ? keys[q0 + qq] : -1; }
    const int n_tiles = (set.end - set.first + T - 1) / T;
    for (int tile = 0; tile < n_tiles; tile++) {
        const int c0 = set.first + tile * T, nc = min(T, set.end - c0);
        __syncthreads();                                  // the previous tile is read until here
        for (int task = lane; task < T * NG; task += kSelThreads) {
            const int c = task / NG, g = task - c * NG;   // (rows are 80 bytes: 16-byte aligned); a short last tile is padded with zeros
            s_tile[g][c] = c < nc ? reinterpret_cast<const float4*>(store_ring + (size_t)(c0 + c) * NR)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int qq = 0; qq < B; qq++) {
            if (qq >= nq) continue;                       // (the same for the whole workgroup)
            const float* __restrict__ qrow = keys ? store_ring + (size_t)qkey[qq] * NR : ext_ring + (size_t)(q0 + qq) * NR;
            float4 qk[NG];
#pragma unroll
            for (int g = 0; g < NG; g++) qk[g] = reinterpret_cast<const float4*>(qrow)[g];
            for (int k0 = 0; k0 < nc; k0 += kSelThreads) {
                const int c = k0 + lane;                  // (< T: the padding is there to be read)
                float4 bk[NG];
#pragma unroll
                for (int g = 0; g < NG; g++) bk[g] = s_tile[g][c];
                const float d2 = sc_ring_d2(qk, bk);
                const unsigned long long word = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)(c0 + c);
                const bool in_set = c < nc && sc_many_in_set(set, qkey[qq], c0 + c);
                bool take = in_set && word < thr[qq];
                unsigned long long mask = __ballot(take);
                if (mask == 0) continue;
                if (held[qq] + __popcll(mask) > cap) {
                    held[qq] = sc_ring_prune(s_buf[qq], held[qq], n_cand, &thr[qq]);
                    take = in_set && word < thr[qq];
                    mask = __ballot(take);
                }
                if (take) s_buf[qq][held[qq] + __popcll(mask & ((1ull << lane) - 1ull))] = word;   // (held <= n_cand after a prune: + 64 <= cap)
                held[qq] += __popcll(mask);
            }
        }
    }
#pragma unroll
    for (int qq = 0; qq < B; qq++) {
        if (qq >= nq) continue;
        const int n = sc_ring_prune(s_buf[qq], held[qq], n_cand, &thr[qq]);
        for (int j = lane; j < n; j += kSelThreads) {
            const unsigned long long w = s_buf[qq][j];
            s2m_sc_ring_neighbour r;
            r.d2 = __uint_as_float((unsigned int)(w >> 32)); r.key = (int32_t)(unsigned int)w;
            cand[(size_t)(q0 + qq) * n_cand + j] = r;
        }
        if (lane == 0) n_out[q0 + qq] = n;
    }
}

// Stage two: workgroup (x, i) compares query i with R_i[3x .. 3x + 3).  Sector-key alignment is sc_distance_block, the
// detector's own call; full alignment is sc_full_block, the single query's: thread (g, j) holds column j of the query and its norm
// in registers as there.
template <int ALIGN>
__global__ __launch_bounds__(kScThreads) void k_sc_ring_dist(const double* __restrict__ store_desc, const double* __restrict__ store_sector,
                                                             const int32_t* __restrict__ keys, const double* __restrict__ ext_desc,
                                                             const double* __restrict__ ext_sector, int n_cand,
                                                             const s2m_sc_ring_neighbour* __restrict__ cand, const int32_t* __restrict__ n_out,
                                                             double* __restrict__ dist, int32_t* __restrict__ shift)
{
    __shared__ int s_cand[NC];
    const int t = threadIdx.x, i = blockIdx.y, j0 = blockIdx.x * NC;
    const int n = n_out[i];
    if (j0 >= n) return;                                  // (the whole workgroup: no barrier is left behind)
    const int nc = min(NC, n - j0);
    if (t < NC) s_cand[t] = cand[(size_t)i * n_cand + j0 + (t < nc ? t : 0)].key;   // a short tail compares its first key again and drops the result
    __syncthreads();
    const double* __restrict__ q = keys ? store_desc + (size_t)keys[i] * ND : ext_desc + (size_t)i * ND;
    const size_t e = (size_t)i * n_cand + j0;
    if constexpr (ALIGN == S2M_SC_ALIGN_FULL) {
        __shared__ ScFullShared<NC> m;
        const int j = t % NS;
        double qcol[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) qcol[r] = q[r * NS + j];
        sc_full_block<NC>(store_desc, qcol, sc_col_norm([&](int r) { return qcol[r]; }), s_cand, m);
        if (t < nc) { dist[e + t] = m.dist_out[t]; shift[e + t] = m.shift_out[t]; }
    } else {
        __shared__ ScShared sh[NC];
        const double* __restrict__ qs = keys ? store_sector + (size_t)keys[i] * NS : ext_sector + (size_t)i * NS;
        sc_distance_block<NC>(store_desc, store_sector, q, qs, s_cand, sh);
        if (t < nc) { dist[e + t] = sh[t].dist_out; shift[e + t] = sh[t].shift_out; }
    }
}

// One wave per query: lane l holds the records l, l + 64, ... of the row (at most four), a record that is no hit as
// (inf, INT_MAX); every round the smallest by (distance, key) is found by a butterfly, lane 0 writes it as the next hit and its
// owner drops it.  Keys of a row are distinct, so the key names the owner.
__global__ __launch_bounds__(kScThreads) void k_sc_ring_rank(int m, int n_cand, const s2m_sc_ring_neighbour* __restrict__ cand,
                                                             const int32_t* __restrict__ n_out, const double* __restrict__ dist,
                                                             const int32_t* __restrict__ shift, int top_k, double max_dist,
                                                             s2m_sc_hit* __restrict__ out_hits, int32_t* __restrict__ out_n)
{
    constexpr int U = S2M_SC_RING_MAX_CAND / 64;
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (kScThreads / 64) + (threadIdx.x >> 6);
    if (qi >= m) return;                                  // (a whole wave: no barrier follows)
    const int n = n_out[qi];
    double rd[U]; int rk[U], rs[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int j = lane + u * 64;
        rd[u] = INFINITY; rk[u] = INT_MAX; rs[u] = 0;
        if (j < n) {
            const size_t e = (size_t)qi * n_cand + j;
            const double d = dist[e];
            if (d < max_dist) { rd[u] = d; rk[u] = cand[e].key; rs[u] = shift[e]; }
        }
    }
    int n_hits = 0;
    for (int round = 0; round < top_k; round++) {
        double bd = INFINITY; int bk = INT_MAX, bs = 0;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (sc_hit_less(rd[u], rk[u], bd, bk)) { bd = rd[u]; bk = rk[u]; bs = rs[u]; }
        sc_hit_wave_min(bd, bk, bs);
        if (bk == INT_MAX) break;                         // no hit is left (the same for all lanes)
        if (lane == 0) out_hits[(size_t)qi * top_k + round] = sc_hit_record(bd, bk, bs);
        n_hits = round + 1;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (rk[u] == bk) { rd[u] = INFINITY; rk[u] = INT_MAX; }
    }
    if (lane == 0) out_n[qi] = n_hits;
}

}  // namespace

hipError_t sc_ring_launch(hipStream_t stream, const ScRingArgs& a)
{
    if (!a.keys)
        hipLaunchKernelGGL(k_sc_ring_prepare, dim3(a.m), dim3(64), 0, stream, a.ext_desc, a.ext_sector, a.ext_ring);
    hipLaunchKernelGGL(k_sc_ring_select, dim3((a.m + B - 1) / B), dim3(kSelThreads), 0, stream, a.store_ring, a.keys, (const float*)a.ext_ring, a.m, a.set,
                       a.n_cand, a.cand, a.n_out);
    if (a.dist) {
        const dim3 grid((a.n_cand + NC - 1) / NC, a.m);
        if (a.align == S2M_SC_ALIGN_FULL)
            hipLaunchKernelGGL(k_sc_ring_dist<S2M_SC_ALIGN_FULL>, grid, dim3(kScThreads), 0, stream, a.store_desc, a.store_sector, a.keys, a.ext_desc,
                               (const double*)a.ext_sector, a.n_cand, (const s2m_sc_ring_neighbour*)a.cand, (const int32_t*)a.n_out, a.dist, a.shift);
        else
            hipLaunchKernelGGL(k_sc_ring_dist<S2M_SC_ALIGN_SECTOR_KEY>, grid, dim3(kScThreads), 0, stream, a.store_desc, a.store_sector, a.keys, a.ext_desc,
                               (const double*)a.ext_sector, a.n_cand, (const s2m_sc_ring_neighbour*)a.cand, (const int32_t*)a.n_out, a.dist, a.shift);
        hipLaunchKernelGGL(k_sc_ring_rank, dim3((a.m + kScThreads / 64 - 1) / (kScThreads / 64)), dim3(kScThreads), 0, stream, a.m, a.n_cand,
                           (const s2m_sc_ring_neighbour*)a.cand, (const int32_t*)a.n_out, (const double*)a.dist, (const int32_t*)a.shift, a.top_k, a.max_dist,
                           a.out_hits, a.out_n);
    }
    return hipGetLastError();
}

}  // namespace s2m
