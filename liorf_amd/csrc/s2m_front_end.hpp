// s2m_front_end.hpp — the host halves between a raw lidar message and a registered pose that need no device:
// odomDeskewInfo() (reference src/imageProjection.cpp:411-491), the check of the positional-deskew argument, and
// updateInitialGuess() (src/mapOptmization.cpp:899-958). Plain inline C++ over s2m_host_math.hpp.
#pragma once
#include <cmath>
#include <cstring>
#include "s2m_host_math.hpp"

namespace s2m {

// Eigen 3.3 Transform<float,3,Affine>::inverse() [ext] on a row-major 3x4: the general 3x3 inverse (cofactors times 1/det, det
// from column 0's cofactors), translation -(Linv * t). The arithmetic of s2m_project.hip's proj_affine_inverse.
inline float host_cof3x4(const float m[12], int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 4 + j1] * m[i2 * 4 + j2] - m[i1 * 4 + j2] * m[i2 * 4 + j1];
}
inline void host_affine_inverse(const float m[12], float S[12])
{
    const float c0 = host_cof3x4(m, 0, 0), c1 = host_cof3x4(m, 1, 0), c2 = host_cof3x4(m, 2, 0);
    const float det = (c0 * m[0] + c1 * m[4]) + c2 * m[8];
    const float invdet = 1.0f / det;
    S[0] = c0 * invdet; S[1] = c1 * invdet; S[2] = c2 * invdet;
    for (int c = 0; c < 3; c++) { S[4 + c] = host_cof3x4(m, c, 1) * invdet; S[8 + c] = host_cof3x4(m, c, 2) * invdet; }
    for (int r = 0; r < 3; r++) S[r * 4 + 3] = -((S[r * 4 + 0] * m[3] + S[r * 4 + 1] * m[7]) + S[r * 4 + 2] * m[11]);
}

// getTransformation(x, y, z, roll, pitch, yaw) of six doubles narrowed to float (pcl::getTransformation takes floats)
inline void host_transformation_xyzrpy(double x, double y, double z, double roll, double pitch, double yaw, float T[12])
{
    const float t[6] = { (float)roll, (float)pitch, (float)yaw, (float)x, (float)y, (float)z };
    host_pose_to_transform(t, T, nullptr);
}

// odomDeskewInfo() (:411-491) over the samples in queue order
inline int host_odom_deskew_info(const s2m_odom_sample* q, size_t n, double timeScanCur, double timeScanEnd, float imuRate, s2m_odom_deskew* out)
{
    std::memset(out, 0, sizeof(*out));                                    // cloudInfo.odomAvailable = false (:413)
    const float sync_diff_time = (imuRate >= 300) ? 0.01 : 0.20;          // :414 (a float, as declared there)
    size_t front = 0;
    while (front < n) {                                                   // :415-421
        if (q[front].time < timeScanCur - sync_diff_time) ++front; else break;
    }
    out->n_popped = (int32_t)front;
    q += front; n -= front;
    if (n == 0) return S2M_OK;                                            // :423-424
    if (q[0].time > timeScanCur) return S2M_OK;                           // :426-427
    const s2m_odom_sample* startOdomMsg = &q[0];                          // :432-440
    for (size_t i = 0; i < n; ++i) {
        startOdomMsg = &q[i];
        if (startOdomMsg->time < timeScanCur) continue; else break;
    }
    double roll, pitch, yaw;                                              // :442-446
    quat_to_rpy(Quat{ startOdomMsg->qx, startOdomMsg->qy, startOdomMsg->qz, startOdomMsg->qw }, roll, pitch, yaw);
    out->initial_guess[0] = (float)startOdomMsg->px;                      // :449-454
    out->initial_guess[1] = (float)startOdomMsg->py;
    out->initial_guess[2] = (float)startOdomMsg->pz;
    out->initial_guess[3] = (float)roll;
    out->initial_guess[4] = (float)pitch;
    out->initial_guess[5] = (float)yaw;
    out->odom_available = 1;                                              // :456
    out->odom_deskew_flag = 0;                                            // :459
    if (q[n - 1].time < timeScanEnd) return S2M_OK;                       // :461-462
    const s2m_odom_sample* endOdomMsg = &q[0];                            // :466-474
    for (size_t i = 0; i < n; ++i) {
        endOdomMsg = &q[i];
        if (endOdomMsg->time < timeScanEnd) continue; else break;
    }
    if (int(std::round(startOdomMsg->cov0)) != int(std::round(endOdomMsg->cov0))) return S2M_OK;    // :476-477
    float transBegin[12], transEnd[12], S[12];
    host_transformation_xyzrpy(startOdomMsg->px, startOdomMsg->py, startOdomMsg->pz, roll, pitch, yaw, transBegin);          // :479
    quat_to_rpy(Quat{ endOdomMsg->qx, endOdomMsg->qy, endOdomMsg->qz, endOdomMsg->qw }, roll, pitch, yaw);                   // :481-482
    host_transformation_xyzrpy(endOdomMsg->px, endOdomMsg->py, endOdomMsg->pz, roll, pitch, yaw, transEnd);                  // :483
    host_affine_inverse(transBegin, S);                                   // transBt = transBegin.inverse() * transEnd (:485): its
    for (int a = 0; a < 3; a++)                                           // translation column (:488), the 4x4 product's term order
        out->odom_incre[a] = ((S[a * 4 + 0] * transEnd[3] + S[a * 4 + 1] * transEnd[7]) + S[a * 4 + 2] * transEnd[11]) + S[a * 4 + 3] * 1.0f;
    out->odom_deskew_flag = 1;                                            // :490
    return S2M_OK;
}

inline bool proj_motion_ok(const s2m_motion_info* m)
{
    if (!m || !m->enabled) return true;
    return std::isfinite(m->time_scan_end) && std::isfinite(m->odom_incre[0]) && std::isfinite(m->odom_incre[1]) && std::isfinite(m->odom_incre[2]);
}

// updateInitialGuess() (src/mapOptmization.cpp:899-958)
inline void host_guess_step(float t[6], const float last[12], const float transBack[12])
{
    float inv[12], transIncre[12], transTobe[12], transFinal[12], o[6];
    host_affine_inverse(last, inv);
    host_affine_mul(inv, transBack, transIncre);                          // last.inverse() * transBack (:931, :948)
    host_pose_to_transform(t, transTobe, nullptr);                        // trans2Affine3f(transformTobeMapped) (:932, :950)
    host_affine_mul(transTobe, transIncre, transFinal);                   // :933, :951
    host_translation_and_euler(transFinal, 4, o);                         // :934-935, :952-953
    t[3] = o[0]; t[4] = o[1]; t[5] = o[2]; t[0] = o[3]; t[1] = o[4]; t[2] = o[5];
}
inline void host_update_initial_guess(s2m_guess_state* st, float t[6], int key_poses_empty, const s2m_guess_info& ci, int useImuHeadingInitialization,
                                      int imuType, float affine_front[12])
{
    host_pose_to_transform(t, affine_front, nullptr);                     // incrementalOdometryAffineFront (:902)
    const float imuT[6] = { ci.imuRollInit, ci.imuPitchInit, ci.imuYawInit, 0.0f, 0.0f, 0.0f };
    if (key_poses_empty) {                                                // :906-917
        t[0] = ci.imuRollInit; t[1] = ci.imuPitchInit; t[2] = ci.imuYawInit;
        if (!useImuHeadingInitialization) t[2] = 0;
        host_pose_to_transform(imuT, st->last_imu_transformation, nullptr);
        return;
    }
    if (ci.odomAvailable == 1) {                                          // :922
        const float g[6] = { ci.initialGuess[3], ci.initialGuess[4], ci.initialGuess[5], ci.initialGuess[0], ci.initialGuess[1], ci.initialGuess[2] };
        float transBack[12];
        host_pose_to_transform(g, transBack, nullptr);                    // :924-925
        if (!st->last_imu_pre_trans_available) {                          // :926-929, then on to the IMU branch
            std::memcpy(st->last_imu_pre_transformation, transBack, sizeof(transBack));
            st->last_imu_pre_trans_available = 1;
        } else {                                                          // :930-941
            host_guess_step(t, st->last_imu_pre_transformation, transBack);
            std::memcpy(st->last_imu_pre_transformation, transBack, sizeof(transBack));
            host_pose_to_transform(imuT, st->last_imu_transformation, nullptr);
            return;
        }
    }
    if (ci.imuAvailable == 1 && imuType) {                                // :945-957
        float transBack[12];
        host_pose_to_transform(imuT, transBack, nullptr);
        host_guess_step(t, st->last_imu_transformation, transBack);
        host_pose_to_transform(imuT, st->last_imu_transformation, nullptr);
    }
}

}  // namespace s2m
