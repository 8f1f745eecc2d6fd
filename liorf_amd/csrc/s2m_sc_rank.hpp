// s2m_sc_rank.hpp — the ranking of the ScanContext place query's hits, stated once: the order (distance, key), the bounded sorted
// list a workgroup keeps, the padded entry it leaves for the merge, the wave's smallest hit and the record the host reads.  The
// single query (s2m_sc_query.hip), the many-query (s2m_sc_many.hip) and the ring-key prefilter (s2m_sc_ring.hip) call these, so a
// row of one is, as bytes, the row of another.  The kernels keep their own loops over lists and records.
#pragma once
#include <limits.h>
#include <math.h>

#include "s2m_sc_dist.hpp"

namespace s2m {

// the order of the hits: a total order, so a ranking does not depend on how the searched set was cut
__device__ __forceinline__ bool sc_hit_less(double da, int ka, double db, int kb) { return da < db || (da == db && ka < kb); }

// (d, key, shift) into a list of at most top_k, ascending (distance, key)
__device__ __forceinline__ void sc_hit_insert(double* hd, int* hk, int* hs, int* n_held, int top_k, double d, int key, int shift)
{
    int n = *n_held;
    if (n == top_k && !sc_hit_less(d, key, hd[top_k - 1], hk[top_k - 1])) return;
    int p = (n < top_k) ? n++ : top_k - 1;
    while (p > 0 && sc_hit_less(d, key, hd[p - 1], hk[p - 1])) { hd[p] = hd[p - 1]; hk[p] = hk[p - 1]; hs[p] = hs[p - 1]; p--; }
    hd[p] = d; hk[p] = key; hs[p] = shift;
    *n_held = n;
}

// entry k of such a list into element e of the partial lists the merge reads; behind the n_held entries the padding (inf, INT_MAX, 0)
__device__ __forceinline__ void sc_hit_store(double* __restrict__ part_d, int2* __restrict__ part_ks, size_t e, const double* hd, const int* hk,
                                             const int* hs, int n_held, int k)
{
    const bool have = k < n_held;
    part_d[e] = have ? hd[k] : INFINITY;
    part_ks[e] = make_int2(have ? hk[k] : INT_MAX, have ? hs[k] : 0);
}

// the smallest (d, k) of the wave's 64 lanes by a butterfly, with its shift and the owner its lane named: the same in every lane
__device__ __forceinline__ void sc_hit_wave_min(double& d, int& k, int& s, int& owner)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double od = __shfl_xor(d, off, 64);
        const int ok = __shfl_xor(k, off, 64), os = __shfl_xor(s, off, 64), og = __shfl_xor(owner, off, 64);
        if (sc_hit_less(od, ok, d, k)) { d = od; k = ok; s = os; owner = og; }
    }
}
__device__ __forceinline__ void sc_hit_wave_min(double& d, int& k, int& s)
{
    int owner = 0;
    sc_hit_wave_min(d, k, s, owner);
}

// the record of a hit as the host reads it
__device__ __forceinline__ s2m_sc_hit sc_hit_record(double d, int k, int s)
{
    s2m_sc_hit hit;
    hit.dist = d; hit.key = k; hit.shift = s; hit.yaw_diff_rad = sc_shift_to_yaw(s); hit.reserved = 0;
    return hit;
}

}  // namespace s2m
