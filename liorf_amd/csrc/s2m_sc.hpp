// s2m_sc.hpp — the ScanContext descriptor, store and loop detector (SCManager, include/Scancontext.cpp): what s2m_abi_sc.hip
// needs of s2m_sc.hip (own translation unit with the kernels).  The functions that work on the handle's store
// (sc_build_descriptor, sc_append_from_out) are declared in s2m_context.hpp, where the other stages find them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace s2m {

struct ScDetectOut {                   // mirrors s2m_sc_match + loop id / yaw
    double  min_dist;
    int32_t loop_id, nn_idx, nn_align;
    float   yaw_diff_rad;
    int32_t cand_idx[3];
    float   cand_d2[3];
};

namespace host __attribute__((visibility("hidden"))) {

// k_sc_detect for the newest of n_total descriptors against the ring keys [0, n_search), on `stream`; `out` may be pinned host memory
void sc_launch_detect(hipStream_t stream, const double* store_desc, const float* store_ring, const double* store_sector, int n_total,
                      int n_search, ScDetectOut* out);
// k_sc_distance_batch: descriptor `query` against cand[0..m), one workgroup per candidate, on `stream`
void sc_launch_distance_batch(hipStream_t stream, const double* store_desc, const double* store_sector, int query, const int32_t* cand,
                              int m, double* dist, int32_t* shift);

}  // namespace host
}  // namespace s2m
