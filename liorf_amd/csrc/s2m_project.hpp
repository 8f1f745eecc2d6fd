// s2m_project.hpp — imageProjection's point filter and IMU deskew on the device: projectPointCloud()
// (reference src/imageProjection.cpp:568-598) with deskewPoint() (:536-566) and findRotation() (:493-518) over the raw
// records of one lidar message, read in place through a layout. Implemented in s2m_project.hip (own translation unit).
// The host half, imuDeskewInfo() (:350-409), and the argument checks are plain inline C++ here: they need no device.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int    kProjTile = 1024;         // records per workgroup: 4 waves x 4 rounds of 64
constexpr int    kProjRounds = 4;
constexpr size_t kProjOutStride = 32;      // cloud_deskewed records are pcl::PointXYZI

// What the kernels leave for the host, in pinned memory.
struct ProjCount {
    int32_t n_out;                         // survivors
    int32_t first;                         // index of the first survivor, or -1
};

// Device scratch of one call; the caller (the handle) owns the memory and sizes it with these.
inline int    proj_blocks(size_t n) { return (int)((n + kProjTile - 1) / kProjTile); }
inline size_t proj_mask_bytes(size_t n) { return sizeof(unsigned long long) * 16 * (size_t)(proj_blocks(n) + 1); }   // one ballot per (workgroup, wave, round)
inline size_t proj_part_bytes(size_t n) { return sizeof(int32_t) * 2 * (size_t)(proj_blocks(n) + 1); }              // {survivors, lowest surviving index} per workgroup; later the exclusive prefix
constexpr size_t kProjTableBytes = sizeof(double) * 4 * S2M_IMU_QUEUE_LENGTH;                                       // imu_time | rot_x | rot_y | rot_z
constexpr size_t kProjStartBytes = 64;                                                                                // S = transStartInverse, row-major 3x4 floats

struct ProjArgs {
    const unsigned char* d_in;             // n raw records
    size_t               n;
    s2m_scan_layout      lay;
    s2m_project_params   prm;
    int                  deskew;
    int                  imu_pointer_cur;
    double               time_scan_cur;
    const double*        d_table;          // 4 x S2M_IMU_QUEUE_LENGTH doubles (read when deskew != 0)
    unsigned long long*  d_mask;
    int32_t*             d_part;
    float*               d_start;
    unsigned char*       d_out;            // room for ceil(n / point_filter_num) records of kProjOutStride bytes
    ProjCount*           h_count;          // pinned, written by the device
    int                  motion;           // findPosition() with its commented lines live (:526-533); acts only with deskew != 0
    double               time_scan_end;    // (read when motion != 0)
    float                odom_incre[3];
};

// Enqueues the three kernels on `stream` (n > 0); the count is in *h_count once the stream has drained.
hipError_t proj_launch(hipStream_t stream, const ProjArgs& a);

// ---- argument checks (host) ---------------------------------------------------------------------------
inline bool proj_layout_ok(const s2m_scan_layout& l)
{
    auto field = [&](uint32_t off, uint32_t size, uint32_t bytes) { return off % size == 0 && l.stride % size == 0 && (uint64_t)off + bytes <= l.stride; };
    if (l.stride == 0 || l.stride > 4096) return false;
    if (!field(l.off_x, 4, 12) || !field(l.off_intensity, 4, 4)) return false;
    switch (l.ring_type) {
        case S2M_RING_U8:  if (!field(l.off_ring, 1, 1)) return false; break;
        case S2M_RING_U16: if (!field(l.off_ring, 2, 2)) return false; break;
        case S2M_RING_I32: if (!field(l.off_ring, 4, 4)) return false; break;
        default: return false;
    }
    switch (l.time_type) {
        case S2M_TIME_F32: case S2M_TIME_U32_NS: case S2M_TIME_U32: return field(l.off_time, 4, 4);
        case S2M_TIME_F64_REL: return field(l.off_time, 8, 8);
        default: return false;
    }
}

inline bool proj_params_ok(const s2m_project_params& p)
{
    return p.n_scan >= 1 && p.downsample_rate >= 1 && p.point_filter_num >= 1 && std::isfinite(p.lidar_min_range) &&
           std::isfinite(p.lidar_max_range);
}

inline bool proj_deskew_ok(const s2m_deskew_info& d)
{
    if (!d.deskew) return true;
    if (d.imu_pointer_cur < 1 || d.imu_pointer_cur >= S2M_IMU_QUEUE_LENGTH) return false;
    if (!d.imu_time || !d.imu_rot_x || !d.imu_rot_y || !d.imu_rot_z) return false;
    for (int i = 1; i <= d.imu_pointer_cur; i++)
        if (!(d.imu_time[i] >= d.imu_time[i - 1])) return false;          // (a NaN time is not ordered)
    return d.imu_time[0] == d.imu_time[0];
}

// imuDeskewInfo() (:350-409): the loop over the queue (:367-401), --imuPointerCur (:403), imuAvailable (:405-408).
inline int proj_imu_deskew_info(const double* imu, size_t n, double time_scan_cur, double time_scan_end, double* imu_time,
                                double* rot_x, double* rot_y, double* rot_z, int32_t* pointer_cur, int32_t* available)
{
    (void)time_scan_cur;                    // (the queue is already popped to time_scan_cur - 0.01, :354-360)
    *available = 0;                         // :352
    *pointer_cur = 0;
    if (n == 0) return S2M_OK;              // :362-363
    int cur = 0;                            // :365
    for (size_t i = 0; i < n; i++) {
        const double t = imu[4 * i];        // :370
        if (t > time_scan_end + 0.01) break;                               // :378-379
        if (cur >= S2M_IMU_QUEUE_LENGTH) return S2M_ERR_CAPACITY;
        if (cur == 0) {                     // :381-388
            rot_x[0] = 0; rot_y[0] = 0; rot_z[0] = 0;
            imu_time[0] = t;
            ++cur;
            continue;
        }
        const double dt = t - imu_time[cur - 1];                           // :395
        rot_x[cur] = rot_x[cur - 1] + imu[4 * i + 1] * dt;                 // :396-398
        rot_y[cur] = rot_y[cur - 1] + imu[4 * i + 2] * dt;
        rot_z[cur] = rot_z[cur - 1] + imu[4 * i + 3] * dt;
        imu_time[cur] = t;                  // :399
        ++cur;
    }
    --cur;                                  // :403
    *pointer_cur = cur;
    if (cur <= 0) return S2M_OK;            // :405-406
    *available = 1;                         // :408
    return S2M_OK;
}

}  // namespace s2m
