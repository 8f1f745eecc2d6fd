// s2m_sc_many.hpp — the ScanContext place query for many queries at once: every query against every stored descriptor of a
// range, each query's K nearest under a threshold.  Implemented in s2m_sc_many.hip (own translation unit); semantics in
// include/liorf_s2m.h, design in DESIGN.md section 20.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int kScManyTile = 4;         // T: stored descriptors a workgroup holds in LDS
constexpr int kScManyBlock = 8;        // B: queries a workgroup walks past its tiles
constexpr int kScManyMaxGroups = 64;   // tile groups (gridDim.x): one list per (query, group), one lane of k_sc_many_select each
constexpr size_t kScManyScratchMax = (size_t)64 << 20;   // lists, staged queries and results of one pass

// The searched set of query i is a predicate on (key of query i, c): c in [first, end), outside [ex_lo, ex_hi) and, for a
// stored-key query, outside [key + rel_lo, key + rel_hi) (sums in 64 bits; rel_lo >= rel_hi: no relative window).
struct ScManySet {
    int32_t first, end, ex_lo, ex_hi, rel_lo, rel_hi;
};

// c is in the searched set of a query with stored key qkey (-1: an external descriptor); shared with the ring-key prefilter
// (s2m_sc_ring.hip)
__device__ __forceinline__ bool sc_many_in_set(const ScManySet& s, int qkey, int c)
{
    if (c < s.first || c >= s.end) return false;
    if (c >= s.ex_lo && c < s.ex_hi) return false;
    if (qkey >= 0 && s.rel_lo < s.rel_hi && (long long)c >= (long long)qkey + s.rel_lo && (long long)c < (long long)qkey + s.rel_hi) return false;
    return true;
}

inline int sc_many_tiles(int n_range) { return (n_range + kScManyTile - 1) / kScManyTile; }
inline int sc_many_groups(int n_range) { const int t = sc_many_tiles(n_range); return t < kScManyMaxGroups ? t : kScManyMaxGroups; }

// bytes of one pass per query, by buffer
inline size_t sc_many_part_bytes(int groups, int top_k) { return (sizeof(double) + 2 * sizeof(int32_t)) * (size_t)groups * (size_t)top_k; }
inline size_t sc_many_out_bytes(int top_k) { return sizeof(s2m_sc_hit) * (size_t)top_k + sizeof(int32_t); }
constexpr size_t kScManyNormBytes = sizeof(double) * S2M_SC_NUM_SECTOR;                                        // column norms of a query
constexpr size_t kScManyExtBytes = sizeof(double) * (S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR + S2M_SC_NUM_SECTOR);  // descriptor | sector key

struct ScManyArgs {
    const double* store_desc;      // the store: [n][1200] descriptors, [n][60] sector keys
    const double* store_sector;
    const int32_t* keys;           // stored-key queries: [m] keys on the device; nullptr: external descriptors
    const double* ext_desc;        // external descriptors [m][1200] on the device (keys == nullptr)
    double*       ext_sector;      // ... and room for their sector keys [m][60], written by k_sc_many_prepare
    double*       qnorm;           // [m][60] column norms of the queries, written by k_sc_many_prepare
    int           m;               // queries of this pass, > 0
    ScManySet     set;             // first < end
    int           top_k, align;
    double        max_dist;
    unsigned char* part;           // m * sc_many_part_bytes(groups, top_k): distances [m][groups][top_k], then (key, shift) pairs
    s2m_sc_hit*   out_hits;        // [m][top_k] on the device
    int32_t*      out_n;           // [m]
};

// Enqueues the three kernels of one pass on `stream`.
hipError_t sc_many_launch(hipStream_t stream, const ScManyArgs& a);

}  // namespace s2m
