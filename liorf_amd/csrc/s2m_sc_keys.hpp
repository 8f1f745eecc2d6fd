// s2m_sc_keys.hpp — the two keys of a ScanContext descriptor, stated once: the ring key (row mean, makeRingkeyFromScancontext,
// include/Scancontext.cpp:198-211) and the sector key (column mean, makeSectorkeyFromScancontext, :214-227).  Both sum left to
// right in fp64.  Every place that makes a key calls these - k_sc_finish and k_sc_append (s2m_sc.hip), s2m_sc_add_descriptor on
// the host (s2m_abi_sc.hip), the batch rebuild of a loaded session (k_sc_keys_batch, s2m_session.hip) and, through sc_ext_keys,
// the place query's three prepare kernels - so a store that was loaded holds bit for bit the keys the incremental adds left.  Compiled with -ffp-contract=off like everything else.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/liorf_s2m.h"

namespace s2m {

// mean of ring r's 60 sectors; at(k) is the descriptor's value at (r, k)
template <typename At>
__host__ __device__ __forceinline__ double sc_ring_key(At at)
{
    double s = 0.0;
    for (int k = 0; k < S2M_SC_NUM_SECTOR; k++) s += at(k);
    return s / 60.0;
}

// squared L2 distance of two fp32 ring keys, each held as five float4: the accumulation order of nanoflann's L2_Adaptor (groups
// of four), fp32, uncontracted.  The detector's three-neighbour search (k_sc_detect) and the ring-key prefilter of the place
// query (s2m_sc_ring.hip) both call this, so they agree bit for bit.
__device__ __forceinline__ float sc_ring_d2(const float4 (&q)[S2M_SC_NUM_RING / 4], const float4 (&b)[S2M_SC_NUM_RING / 4])
{
    float result = 0.0f;
#pragma unroll
    for (int g = 0; g < S2M_SC_NUM_RING / 4; g++) {
        const float d0 = q[g].x - b[g].x, d1 = q[g].y - b[g].y, d2 = q[g].z - b[g].z, d3 = q[g].w - b[g].w;
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    return result;
}

// mean of a sector's 20 rings; at(r) is the descriptor's value at (r, sector)
template <typename At>
__host__ __device__ __forceinline__ double sc_sector_key(At at)
{
    double a = 0.0;
    for (int r = 0; r < S2M_SC_NUM_RING; r++) a += at(r);
    return a / (double)S2M_SC_NUM_RING;
}

// The keys of an external descriptor q for a query, by threads t = 0 .. 63 of a workgroup: its sector key and, where `ring` is
// given, its ring key as s2m_sc_add_descriptor stores it ((float) of the row mean).  The prepare kernels of the place query, the
// many-query and the ring-key prefilter call this.
__device__ __forceinline__ void sc_ext_keys(const double* q, int t, double* sector, float* ring)
{
    constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR;
    if (ring && t < NR) ring[t] = (float)sc_ring_key([&](int k) { return q[t * NS + k]; });
    if (t < NS) sector[t] = sc_sector_key([&](int r) { return q[r * NS + t]; });
}

}  // namespace s2m
