// s2m_sc_query.hpp — the ScanContext place query: a query descriptor against every stored descriptor of a range, the K nearest
// under a threshold ranked on the device.  Implemented in s2m_sc_query.hip (own translation unit); semantics in
// include/liorf_s2m.h, design in DESIGN.md section 17.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int    kScQueryMaxGroups = 1024;   // workgroups of k_sc_query_dist; a larger searched set is walked in several passes
constexpr int    kScQueryCands = 3;          // candidates a workgroup compares side by side
constexpr size_t kScQuerySlot = (size_t)S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR + S2M_SC_NUM_SECTOR;   // doubles: descriptor | sector key

// What k_sc_query_select leaves for the host, in pinned memory.
struct ScQueryOut {
    s2m_sc_hit hits[S2M_SC_QUERY_MAX_K];
    int32_t    n_hits;
};

inline int    sc_query_groups(int n_s) { const int g = (n_s + kScQueryCands - 1) / kScQueryCands; return g < kScQueryMaxGroups ? g : kScQueryMaxGroups; }
inline size_t sc_query_part_bytes(int n_s, int top_k) { return (sizeof(double) + 2 * sizeof(int32_t)) * (size_t)sc_query_groups(n_s) * (size_t)top_k; }

struct ScQueryArgs {
    const double* store_desc;      // the store: [n][1200] descriptors, [n][60] sector keys
    const double* store_sector;
    const double* src_desc;        // the query's descriptor on the device: a store slot, the descriptor of the cloud in hand, or `slot` itself
    const double* src_sector;      // its sector key where the store holds it, else nullptr: computed as k_sc_append computes it
    double*       slot;            // kScQuerySlot doubles
    // the searched set S, n_s > 0 keys: first + i for i < n_before, first + skip + i from there on (the exclusion window cut out)
    int           first, n_before, skip, n_s;
    int           top_k, align;
    double        max_dist;
    unsigned char* part;           // sc_query_part_bytes(n_s, top_k): the workgroups' lists, distances then (key, shift) pairs
    ScQueryOut*   out;             // pinned, written by the device
};

// Enqueues the three kernels on `stream`; *out is valid once the stream has drained.
hipError_t sc_query_launch(hipStream_t stream, const ScQueryArgs& a);

}  // namespace s2m
