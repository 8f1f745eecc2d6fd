// s2m_sc_ring.hpp — the ring-key prefilter of the ScanContext place query: per query the n_candidates stored keys whose fp32
// ring keys are nearest (stage one, all pairs over 80-byte rows), then the column-by-column distance against those only (stage
// two) and the ranking of the row.  Implemented in s2m_sc_ring.hip (own translation unit); semantics in include/liorf_s2m.h,
// design in DESIGN.md section 22.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"
#include "s2m_sc_many.hpp"             // ScManySet, kScManyScratchMax: the searched set and the scratch bound are the many-query's

namespace s2m {

constexpr int kScRingTile = 256;       // stored ring keys a workgroup of k_sc_ring_select holds in LDS (20 KB)
constexpr int kScRingBlock = 4;        // queries it walks past every tile
constexpr int kScRingBuf = 512;        // 64-bit words of a query's candidate buffer in LDS: at least S2M_SC_RING_MAX_CAND + one wave's appends
constexpr int kScRingCands = 3;        // candidates a workgroup of k_sc_ring_dist compares side by side
static_assert(kScRingBuf >= S2M_SC_RING_MAX_CAND + 64, "a pruned buffer takes the appends of one more wave step");

// bytes of one pass per query, by buffer
inline size_t sc_ring_cand_bytes(int n_cand) { return sizeof(s2m_sc_ring_neighbour) * (size_t)n_cand + sizeof(int32_t); }   // R_i | its size
inline size_t sc_ring_dist_bytes(int n_cand) { return (sizeof(double) + sizeof(int32_t)) * (size_t)n_cand; }               // distances | shifts
inline size_t sc_ring_out_bytes(int top_k) { return sizeof(s2m_sc_hit) * (size_t)top_k + sizeof(int32_t); }
constexpr size_t kScRingKeyBytes = sizeof(float) * S2M_SC_NUM_RING;                                                         // a query's fp32 ring key
constexpr size_t kScRingExtBytes = sizeof(double) * (S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR + S2M_SC_NUM_SECTOR) + kScRingKeyBytes;   // descriptor | sector key | ring key

struct ScRingArgs {
    const double* store_desc;      // the store: [n][1200] descriptors, [n][20] fp32 ring keys, [n][60] sector keys
    const float*  store_ring;
    const double* store_sector;
    const int32_t* keys;           // stored-key queries: [m] keys on the device; nullptr: external descriptors
    const double* ext_desc;        // external descriptors [m][1200] on the device (keys == nullptr)
    double*       ext_sector;      // ... room for their sector keys [m][60] and fp32 ring keys [m][20], written by k_sc_ring_prepare
    float*        ext_ring;
    int           m;               // queries of this pass, 0 < m <= 65535
    ScManySet     set;             // first < end
    int           n_cand;          // 1 .. S2M_SC_RING_MAX_CAND
    s2m_sc_ring_neighbour* cand;   // [m][n_cand]: R_i, ascending (d2, key)
    int32_t*      n_out;           // [m]: |R_i|
    // stage two and the ranking (dist == nullptr: stage one alone)
    int           top_k, align;
    double        max_dist;
    double*       dist;            // [m][n_cand]
    int32_t*      shift;           // [m][n_cand]
    s2m_sc_hit*   out_hits;        // [m][top_k] on the device
    int32_t*      out_n;           // [m]
};

// Enqueues the kernels of one pass on `stream`.
hipError_t sc_ring_launch(hipStream_t stream, const ScRingArgs& a);

}  // namespace s2m
