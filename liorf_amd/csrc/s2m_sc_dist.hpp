// s2m_sc_dist.hpp — distanceBtnScanContext (reference include/Scancontext.cpp:116-148) by one workgroup, shared by the detector
// and batched distance (s2m_sc.hip) and by the place query (s2m_sc_query.hip).  Compiled with -ffp-contract=off; all sums
// run left to right in fp64 like the oracle's restatement, so distances are bit-identical to it.
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
        double a = 0.0;
        for (int j = 0; j < NS; j++) {
            int j2 = j - s; j2 += (j2 < 0) ? NS : 0;
            const double d = sh[c].v1[j] - sh[c].v2[j2];
            a += d * d;
        }
        sh[c].vnorm[s] = sqrt(a);
    }
    __syncthreads();
    if (t < NC) {
        ScShared& m = sh[t];
        int a0 = 0;
        double best = 10000000;
        for (int s = 0; s < NS; s++) if (m.vnorm[s] < best) { a0 = s; best = m.vnorm[s]; }
        // search space a0, a0 +- 1..3 (mod 60), ascending (:122-129)
        int sp[kScShifts];
        sp[0] = a0;
        for (int ii = 1; ii <= (kScShifts - 1) / 2; ii++) { sp[2 * ii - 1] = (a0 + ii + NS) % NS; sp[2 * ii] = (a0 - ii + NS) % NS; }
        for (int a = 1; a < kScShifts; a++) {            // insertion sort
            const int v = sp[a];
            int b = a - 1;
            while (b >= 0 && sp[b] > v) { sp[b + 1] = sp[b]; b--; }
            sp[b + 1] = v;
        }
        for (int k = 0; k < kScShifts; k++) m.shifts[k] = sp[k];
    }
    __syncthreads();
    for (int task = t; task < NC * kScShifts * NS; task += kScThreads) {  // distDirectSC (:69-91), one sector pair per task
        const int c = task / (kScShifts * NS), rem = task - c * (kScShifts * NS);
        const int k = rem / NS, j = rem - k * NS;
        int j2 = j - sh[c].shifts[k]; j2 += (j2 < 0) ? NS : 0;            // circshift (:39-59)
        const double* __restrict__ sc2 = store_desc + (size_t)cand[c] * NR * NS;
        double n1 = 0.0, n2 = 0.0, dot = 0.0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const double a = sc1[r * NS + j], b = sc2[r * NS + j2];
            n1 += a * a; n2 += b * b; dot += a * b;
        }
        n1 = sqrt(n1); n2 = sqrt(n2);
        const bool skip = (n1 == 0) | (n2 == 0);
        sh[c].eff[k][j] = skip ? 0 : 1;
        sh[c].sim[k][j] = skip ? 0.0 : dot / (n1 * n2);
    }
    __syncthreads();
    if (t < NC * kScShifts) {
        const int c = t / kScShifts, k = t - c * kScShifts;
        int num_eff = 0;
        double sum = 0;
        for (int j = 0; j < NS; j++) if (sh[c].eff[k][j]) { sum = sum + sh[c].sim[k][j]; num_eff = num_eff + 1; }
        sh[c].dist[k] = 1.0 - sum / (double)num_eff;      // 0/0 = NaN when no sector counts, as in the reference
    }
    __syncthreads();
    if (t < NC) {
        ScShared& m = sh[t];
        int argmin_shift = 0;
        double min_sc_dist = 10000000;
        for (int k = 0; k < kScShifts; k++) if (m.dist[k] < min_sc_dist) { argmin_shift = m.shifts[k]; min_sc_dist = m.dist[k]; }
        m.dist_out = min_sc_dist; m.shift_out = argmin_shift;
    }
    __syncthreads();
}

// yaw difference of a column shift: deg2rad(float) of shift * PC_UNIT_SECTORANGLE (:17-20, :338-339)
__device__ __forceinline__ float sc_shift_to_yaw(int shift)
{
    return (float)((double)(float)((double)shift * (360.0 / 60.0)) * M_PI / 180.0);
}

}  // namespace s2m
