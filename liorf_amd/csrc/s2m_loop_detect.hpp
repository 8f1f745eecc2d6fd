// s2m_loop_detect.hpp — detectLoopClosureDistance() for many stored keys at once: every query key against every key of a searched
// set by position and time, each query's top_k nearest that pass both gates.  Implemented in s2m_loop_detect.hip (own
// translation unit); the shape constants, the argument table and the pass plan in s2m_loop_detect_plan.hpp (host only);
// semantics in include/liorf_s2m.h, design in DESIGN.md section 23.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"
#include "s2m_loop_detect_plan.hpp"
#include "s2m_sc_many.hpp"             // ScManySet, sc_many_in_set: the searched set is the place queries'

namespace s2m {

static_assert(kLdScratchMax == kScManyScratchMax, "one scratch bound for the many-query calls");

struct LdArgs {
    const float4* pos;             // the store: [n] positions, [n] times
    const double* time;
    const int32_t* keys;           // [m] query keys on the device
    const double* time_cur;        // [m] on the device, or nullptr: a query's time is its key's
    int           m;               // queries of this pass, > 0
    ScManySet     set;             // first < end
    float         r2;              // (float)(R * R)
    double        time_diff;
    int           top_k, splits;   // 1 .. S2M_LOOP_MAX_CANDIDATES; 1 .. kLdMaxSplits
    unsigned long long* part;      // m * ld_part_bytes(splits, top_k): words [split][j][query]
    int32_t*      out_key;         // [m][top_k] on the device
    float*        out_d2;          // [m][top_k]
    int32_t*      out_n;           // [m]
};

// Enqueues the two kernels of one pass on `stream`.
hipError_t ld_launch(hipStream_t stream, const LdArgs& a);

}  // namespace s2m
