// s2m_kf_d2.hpp — the squared distance of two key positions: the one statement behind every radius test on the key-frame store
// (s2m_extract_surrounding's selection and k_loop_detect in s2m_voxel.hip, k_loop_detect_many in s2m_loop_detect.hip).
// Compiled with -ffp-contract=off in every unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace s2m {

// FLANN's L2_Simple accumulation: ((dx^2 + dy^2) + dz^2), fp32, no contraction
__device__ __forceinline__ float kf_d2(float4 a, float4 b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace s2m
