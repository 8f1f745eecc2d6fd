// s2m_sc_dist.hpp — the distance of two ScanContext descriptors: the arithmetic of a pair as device functions of one thread's
// share each, called by every kernel that compares descriptors, and distanceBtnScanContext (reference
// include/Scancontext.cpp:116-148) by one workgroup, shared by the detector and batched distance (s2m_sc.hip), the place query
// (s2m_sc_query.hip) and the ring-key prefilter (s2m_sc_ring.hip); beside it the full alignment over all 60 shifts by one
// workgroup (sc_full_block), shared by the last two.  Compiled with -ffp-contract=off; all sums run left to right in fp64 like
// the oracle's restatement, so distances are bit-identical to it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int kScThreads = 256;
constexpr int kScShifts = 7;           // 1 + 2 * round(0.5 * SEARCH_RATIO * 60) (:122-129, Scancontext.h:93)

struct ScShared {
    double v1[S2M_SC_NUM_SECTOR], v2[S2M_SC_NUM_SECTOR]; // the two sector keys, staged
    double vnorm[S2M_SC_NUM_SECTOR];                     // fastAlignUsingVkey: ||vkey1 - circshift(vkey2, s)||
    double sim[kScShifts][S2M_SC_NUM_SECTOR];            // per (shift, sector): cosine similarity
    int    eff[kScShifts][S2M_SC_NUM_SECTOR];            // ... and whether the sector pair counts
    double dist[kScShifts];
    int    shifts[kScShifts];
    double dist_out;                                     // the result: distance and the shift it was found at
    int    shift_out;
};

// ---- the arithmetic of one descriptor pair, stated once ----------------------------------------------------------------
// Every kernel that compares two descriptors - the detector and the batched distance (s2m_sc.hip), the place query
// (s2m_sc_query.hip) and the many-query (s2m_sc_many.hip) - calls these, so they agree bit for bit however the pairs are cut
// over threads.  Each function is one thread's work and each sum runs left to right in fp64.

// ||column||: at(r) is the column's value in ring r.  It does not depend on the shift the column is paired with.
template <typename At>
__device__ __forceinline__ double sc_col_norm(At at)
{
    double n = 0.0;
#pragma unroll
    for (int r = 0; r < S2M_SC_NUM_RING; r++) { const double b = at(r); n += b * b; }
    return sqrt(n);
}

// the 20-term dot product of two columns (distDirectSC, :69-91)
template <typename A, typename B>
__device__ __forceinline__ double sc_col_dot(A a, B b)
{
    double dot = 0.0;
#pragma unroll
    for (int r = 0; r < S2M_SC_NUM_RING; r++) dot += a(r) * b(r);
    return dot;
}

// a sector pair counts when both columns are non-empty; its cosine similarity
__device__ __forceinline__ bool sc_sector_sim(double dot, double n1, double n2, double* sim)
{
    const bool skip = (n1 == 0) | (n2 == 0);
    *sim = skip ? 0.0 : dot / (n1 * n2);
    return !skip;
}

// 1 - mean of the similarities of the sectors that count, sectors ascending.  No branch and no select on the sum's chain: a
// sector that does not count holds sim = +0.0 (sc_sector_sim), and sum + 0.0 is sum bit for bit - the sum starts at +0.0 and a
// sum in round-to-nearest is -0.0 only when both terms are, so it never is -0.0; a NaN or an infinity stays what it is - so
// adding every sector is the reference's "add the sectors that count".  0/0 = NaN when no sector counts: never a minimum.
template <typename Eff, typename Sim>
__device__ __forceinline__ double sc_sector_sum_dist(Eff eff, Sim sim)
{
    int num_eff = 0;
    double sum = 0;
#pragma unroll 20
    for (int j = 0; j < S2M_SC_NUM_SECTOR; j++) {
        sum = sum + sim(j);
        num_eff += eff(j) ? 1 : 0;
    }
    return 1.0 - sum / (double)num_eff;
}

// the strict minimum over shifts visited in ascending order, from 10000000 / shift 0
__device__ __forceinline__ void sc_min_update(double d, int shift, double* best, int* best_shift)
{
    if (d < *best) { *best = d; *best_shift = shift; }
}

// fastAlignUsingVkey (:94-113), one shift: ||vkey1 - circshift(vkey2, s)||
template <typename V1, typename V2>
__device__ __forceinline__ double sc_vkey_shift_norm(V1 v1, V2 v2, int s)
{
    double a = 0.0;
    for (int j = 0; j < S2M_SC_NUM_SECTOR; j++) {
        int j2 = j - s; j2 += (j2 < 0) ? S2M_SC_NUM_SECTOR : 0;
        const double d = v1(j) - v2(j2);
        a += d * d;
    }
    return sqrt(a);
}

// ... its argmin a0 (strict, ascending) and the search space a0, a0 +- 1..3 (mod 60), sorted ascending (:122-129)
template <typename Vn>
__device__ __forceinline__ void sc_search_shifts(Vn vnorm, int (&sp)[kScShifts])
{
    constexpr int NS = S2M_SC_NUM_SECTOR;
    int a0 = 0;
    double best = 10000000;
    for (int s = 0; s < NS; s++) sc_min_update(vnorm(s), s, &best, &a0);
    sp[0] = a0;
    for (int ii = 1; ii <= (kScShifts - 1) / 2; ii++) { sp[2 * ii - 1] = (a0 + ii + NS) % NS; sp[2 * ii] = (a0 - ii + NS) % NS; }
    for (int a = 1; a < kScShifts; a++) {            // insertion sort
        const int v = sp[a];
        int b = a - 1;
        while (b >= 0 && sp[b] > v) { sp[b + 1] = sp[b]; b--; }
        sp[b + 1] = v;
    }
}

// distanceBtnScanContext(query, cand[c]) (:116-148) for NC candidates side by side by one workgroup: every phase of the
// reference's function is spread over (candidate, shift) or (candidate, shift, sector) tasks, every sum is taken by one thread
// from left to right like the oracle's.  The query is its descriptor `sc1` and sector key `vkey1` (global memory or LDS), the
// candidates are store indices; `cand` lives in LDS; results in sh[c].dist_out / .shift_out, valid after the call.
template <int NC>
__device__ __forceinline__ void sc_distance_block(const double* __restrict__ store_desc, const double* __restrict__ store_sector,
                                                  const double* __restrict__ sc1, const double* __restrict__ vkey1, const int* cand,
                                                  ScShared* sh)
{
    constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR;
    const int t = threadIdx.x;
    __syncthreads();                                     // the scratch may still be read from a previous call
    for (int task = t; task < NC * NS; task += kScThreads) {
        const int c = task / NS, j = task - c * NS;
        sh[c].v1[j] = vkey1[j];
        sh[c].v2[j] = store_sector[(size_t)cand[c] * NS + j];
    }
    __syncthreads();
    for (int task = t; task < NC * NS; task += kScThreads) {              // fastAlignUsingVkey (:94-113), one shift per task
        const int c = task / NS, s = task - c * NS;
        sh[c].vnorm[s] = sc_vkey_shift_norm([&](int j) { return sh[c].v1[j]; }, [&](int j) { return sh[c].v2[j]; }, s);
    }
    __syncthreads();
    if (t < NC) {
        ScShared& m = sh[t];
        int sp[kScShifts];
        sc_search_shifts([&](int s) { return m.vnorm[s]; }, sp);
        for (int k = 0; k < kScShifts; k++) m.shifts[k] = sp[k];
    }
    __syncthreads();
    for (int task = t; task < NC * kScShifts * NS; task += kScThreads) {  // distDirectSC (:69-91), one sector pair per task
        const int c = task / (kScShifts * NS), rem = task - c * (kScShifts * NS);
        const int k = rem / NS, j = rem - k * NS;
        int j2 = j - sh[c].shifts[k]; j2 += (j2 < 0) ? NS : 0;            // circshift (:39-59)
        const double* __restrict__ sc2 = store_desc + (size_t)cand[c] * NR * NS;
        const auto a = [&](int r) { return sc1[r * NS + j]; };
        const auto b = [&](int r) { return sc2[r * NS + j2]; };
        sh[c].eff[k][j] = sc_sector_sim(sc_col_dot(a, b), sc_col_norm(a), sc_col_norm(b), &sh[c].sim[k][j]) ? 1 : 0;
    }
    __syncthreads();
    if (t < NC * kScShifts) {
        const int c = t / kScShifts, k = t - c * kScShifts;
        sh[c].dist[k] = sc_sector_sum_dist([&](int j) { return sh[c].eff[k][j] != 0; }, [&](int j) { return sh[c].sim[k][j]; });
    }
    __syncthreads();
    if (t < NC) {
        ScShared& m = sh[t];
        int argmin_shift = 0;
        double min_sc_dist = 10000000;
        for (int k = 0; k < kScShifts; k++) sc_min_update(m.dist[k], m.shifts[k], &min_sc_dist, &argmin_shift);
        m.dist_out = min_sc_dist; m.shift_out = argmin_shift;
    }
    __syncthreads();
}

constexpr int kScFullChunk = 12;       // shifts of the full alignment a workgroup evaluates between two barriers
constexpr int kScFullLanes = 4;        // ... by 4 x 60 threads: thread (g, j) owns sector j of the query and the shifts g, g + 4, ... of a chunk
static_assert(S2M_SC_NUM_SECTOR % kScFullChunk == 0 && kScFullChunk % kScFullLanes == 0, "the chunks cover the 60 shifts");
static_assert(kScFullLanes * S2M_SC_NUM_SECTOR <= kScThreads, "one thread per (lane, sector)");
static_assert(S2M_SC_NUM_SECTOR % 2 == 0, "descriptors are staged two doubles at a time");

// LDS of the full alignment: the NC candidates, their column norms, one chunk of similarities
template <int NC>
struct alignas(16) ScFullShared {
    double c[NC][S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR];
    double cnorm[NC][S2M_SC_NUM_SECTOR];
    double sim[NC][kScFullChunk][S2M_SC_NUM_SECTOR];
    unsigned char eff[NC][kScFullChunk][S2M_SC_NUM_SECTOR];
    double dist[NC][kScFullChunk];
    double dist_out[NC];                                 // the result: distance and the shift it was found at
    int    shift_out[NC];
};

// min over s = 0..59 ascending of distDirectSC(query, circshift(cand[c], s)) (:69-91), strict, from 10000000 / shift 0, for NC
// candidates side by side by one workgroup (the single query and the ring-key prefilter; the many-query's two queries x four
// candidates are its own arrangement of the same functions).  A column's norm does not depend on the shift it is paired with: 60
// norms per descriptor, then one independent left-to-right dot product of 20 terms per (shift, sector).  Thread (g, j) =
// (t / 60, t % 60), t < 240, holds column j of the query (qcol) and its norm (n1) in registers, so a term costs one LDS read.
// `cand` lives in LDS.  The block has no barrier at either end, the callers' own serve: one between writing `cand` (and reading the
// scratch of a previous call) and the call; thread c leaves the results in m.dist_out[c] / m.shift_out[c], and a caller in which
// another thread reads them puts one behind the call.
template <int NC>
__device__ __forceinline__ void sc_full_block(const double* __restrict__ store_desc, const double (&qcol)[S2M_SC_NUM_RING], double n1, const int* cand,
                                              ScFullShared<NC>& m)
{
    constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR, ND = NR * NS;
    static_assert(NC * kScFullChunk <= kScThreads, "one thread per sector sum");
    const int t = threadIdx.x;
    const int g = t / NS, j = t - g * NS;
    for (int task = t; task < NC * (ND / 2); task += kScThreads) {
        const int c = task / (ND / 2), k = task - c * (ND / 2);
        reinterpret_cast<double2*>(m.c[c])[k] = reinterpret_cast<const double2*>(store_desc + (size_t)cand[c] * ND)[k];   // (slots are 9600 bytes: 16-byte aligned)
    }
    if (t < NC) { m.dist_out[t] = 10000000; m.shift_out[t] = 0; }
    __syncthreads();
    for (int task = t; task < NC * NS; task += kScThreads) {
        const int c = task / NS, jc = task - c * NS;
        m.cnorm[c][jc] = sc_col_norm([&](int r) { return m.c[c][r * NS + jc]; });
    }
    __syncthreads();
    for (int s0 = 0; s0 < NS; s0 += kScFullChunk) {
        if (g < kScFullLanes) {
            for (int k = g; k < kScFullChunk; k += kScFullLanes) {
                int j2 = j - (s0 + k); j2 += (j2 < 0) ? NS : 0;            // circshift (:39-59)
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const double dot = sc_col_dot([&](int r) { return qcol[r]; }, [&](int r) { return m.c[c][r * NS + j2]; });
                    m.eff[c][k][j] = sc_sector_sim(dot, n1, m.cnorm[c][j2], &m.sim[c][k][j]) ? 1 : 0;
                }
            }
        }
        __syncthreads();
        if (t < NC * kScFullChunk) {
            const int c = t / kScFullChunk, k = t - c * kScFullChunk;
            m.dist[c][k] = sc_sector_sum_dist([&](int jj) { return m.eff[c][k][jj] != 0; }, [&](int jj) { return m.sim[c][k][jj]; });
        }
        __syncthreads();
        if (t < NC)
            for (int k = 0; k < kScFullChunk; k++)
                sc_min_update(m.dist[t][k], s0 + k, &m.dist_out[t], &m.shift_out[t]);
        // (the next chunk writes sim / eff only; dist is written again behind its barrier)
    }
}

// yaw difference of a column shift: deg2rad(float) of shift * PC_UNIT_SECTORANGLE (:17-20, :338-339)
__device__ __forceinline__ float sc_shift_to_yaw(int shift)
{
    return (float)((double)(float)((double)shift * (360.0 / 60.0)) * M_PI / 180.0);
}

}  // namespace s2m
