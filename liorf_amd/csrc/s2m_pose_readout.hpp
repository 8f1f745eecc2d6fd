// s2m_pose_readout.hpp — the two statements that turn an fp64 pose state {R row-major, t} into what the key-frame store keeps:
// the float pose vector of Rot3::RzRyRx, and the cached transform of that vector.  One text for the pose graph's read-out and
// correctPoses() (s2m_pose_graph.hip) and for the placement of an appended session (s2m_session.hip), so that the three leave
// the same bits.
#pragma once
#include "s2m_glibc_trig.hpp"

namespace s2m {
namespace {

// {x, y, z, roll, pitch, yaw} of Rot3::RzRyRx in float
__device__ __forceinline__ void pose_readout(const double* P, float o[6])
{
    const double s = fmin(1.0, fmax(-1.0, -P[6]));
    o[0] = (float)P[9]; o[1] = (float)P[10]; o[2] = (float)P[11];
    o[3] = (float)atan2(P[7], P[8]);
    o[4] = (float)asin(s);
    o[5] = (float)atan2(P[3], P[0]);
}

// transCur = pcl::getTransformation of the float pose vector (:317) in host_pose_to_transform's term order with the host libm's
// sinf / cosf (glibc_sincosf_both)
__device__ __forceinline__ void pose_transform(const float o[6], float T[12])
{
    float A, B, C, D, E, F;
    glibc_sincosf_both(o[5], B, A);
    glibc_sincosf_both(o[4], D, C);
    glibc_sincosf_both(o[3], F, E);
    const float DE = D * E, DF = D * F;
    T[0] = A * C; T[1] = A * DF - B * E; T[2]  = B * F + A * DE; T[3]  = o[0];
    T[4] = B * C; T[5] = A * E + B * DF; T[6]  = B * DE - A * F; T[7]  = o[1];
    T[8] = -D;    T[9] = C * F;          T[10] = C * E;          T[11] = o[2];
}

}  // namespace
}  // namespace s2m
