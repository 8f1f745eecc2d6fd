// s2m_abi_front_end.hip — C ABI of the odometry front end: imageProjection's point filter and deskew (s2m_project.hip's stages),
// the host-only deskew tables and initial guess (s2m_front_end.hpp), and the ScanContext descriptor of the projected cloud.
#include <cmath>
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_front_end.hpp"

using namespace s2m;
using namespace s2m::host;

// ---- imageProjection's point filter and IMU deskew (reference src/imageProjection.cpp:350-409, :493-598) ---------------

int s2m_scan_layout_preset(int32_t sensor, s2m_scan_layout* out)
{
    if (!out) return S2M_ERR_INVALID_ARG;
    switch (sensor) {                                     // the reference's point structs (:4-57)
        case S2M_SENSOR_VELODYNE: case S2M_SENSOR_LIVOX: *out = s2m_scan_layout{ 32, 0, 16, 20, 24, S2M_RING_U16, S2M_TIME_F32 }; return S2M_OK;
        case S2M_SENSOR_OUSTER:    *out = s2m_scan_layout{ 48, 0, 16, 26, 20, S2M_RING_U8, S2M_TIME_U32_NS }; return S2M_OK;
        case S2M_SENSOR_MULRAN:    *out = s2m_scan_layout{ 32, 0, 16, 24, 20, S2M_RING_I32, S2M_TIME_U32 }; return S2M_OK;
        case S2M_SENSOR_ROBOSENSE: *out = s2m_scan_layout{ 32, 0, 16, 20, 24, S2M_RING_U16, S2M_TIME_F64_REL }; return S2M_OK;
        default: return S2M_ERR_INVALID_ARG;
    }
}

int s2m_project_default_params(s2m_project_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    p->n_scan = 16; p->downsample_rate = 1; p->point_filter_num = 3;         // include/utility.h:204-207
    p->lidar_min_range = 1.0f; p->lidar_max_range = 1000.0f;                 // include/utility.h:208-209
    return S2M_OK;
}

int s2m_imu_deskew_info(const double* imu, size_t n, double time_scan_cur, double time_scan_end, double* imu_time, double* imu_rot_x,
                        double* imu_rot_y, double* imu_rot_z, int32_t* imu_pointer_cur, int32_t* imu_available)
{
    if ((n > 0 && !imu) || !imu_time || !imu_rot_x || !imu_rot_y || !imu_rot_z || !imu_pointer_cur || !imu_available) return S2M_ERR_INVALID_ARG;
    return proj_imu_deskew_info(imu, n, time_scan_cur, time_scan_end, imu_time, imu_rot_x, imu_rot_y, imu_rot_z, imu_pointer_cur, imu_available);
}

int s2m_project_check_args(const s2m_scan_layout* layout, const s2m_project_params* params, const s2m_deskew_info* deskew)
{
    if (!layout || !proj_layout_ok(*layout)) return S2M_ERR_INVALID_ARG;
    if (params && !proj_params_ok(*params)) return S2M_ERR_INVALID_ARG;
    if (deskew && !proj_deskew_ok(*deskew)) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

int s2m_project_check_args_motion(const s2m_scan_layout* layout, const s2m_project_params* params, const s2m_deskew_info* deskew,
                                  const s2m_motion_info* motion)
{
    if (s2m_project_check_args(layout, params, deskew) != S2M_OK) return S2M_ERR_INVALID_ARG;
    return proj_motion_ok(motion) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

// s2m_project_scan (motion == nullptr) and s2m_project_scan_motion
static int project_scan_impl(s2m_handle h, const void* pts, size_t n, const s2m_scan_layout* layout, int on_device, const s2m_project_params* params,
                             const s2m_deskew_info* deskew, const s2m_motion_info* motion, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (s2m_project_check_args(layout, params, deskew) != S2M_OK)
        return fail(h, S2M_ERR_INVALID_ARG, "scan layout (fields inside the stride, naturally aligned), project params (n_scan, downsample_rate, "
                                            "point_filter_num >= 1, finite ranges) or deskew tables (1 <= imu_pointer_cur < 2000, non-decreasing times)");
    if (!proj_motion_ok(motion)) return fail(h, S2M_ERR_INVALID_ARG, "motion: time_scan_end and the three increments must be finite");
    s2m_project_params prm;
    if (params) prm = *params; else s2m_project_default_params(&prm);
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    if (!h) return S2M_ERR_INVALID_ARG;
    if (n > 0 && !pts) return fail(h, S2M_ERR_INVALID_ARG, "null record buffer");
    if (on_device && (reinterpret_cast<uintptr_t>(pts) & 7) != 0) return fail(h, S2M_ERR_INVALID_ARG, "device records must be 8-byte aligned");
    if (n > (size_t)0x3fffffff) return fail(h, S2M_ERR_CAPACITY, "too many records");
    S2M_HIP(h, hipSetDevice(h->device));
    if (!h->proj.h_count) S2M_HIP(h, hipHostMalloc((void**)&h->proj.h_count, 64));
    const int do_deskew = (deskew && deskew->deskew) ? 1 : 0;
    h->proj.have_deskewed = false;
    h->proj.deskewed_n = 0;
    int rc;
    if ((rc = ensure(h, h->proj.cloud_deskewed, kProjOutStride))) return rc;      // empty and valid
    if (n == 0) { h->proj.have_deskewed = true; return S2M_OK; }

    const size_t ub = (n + (size_t)prm.point_filter_num - 1) / (size_t)prm.point_filter_num;      // survivors pass i % point_filter_num == 0
    if ((rc = ensure(h, h->proj.cloud_deskewed, kProjOutStride * ub)) || (rc = ensure(h, h->proj.mask, proj_mask_bytes(n))) ||
        (rc = ensure(h, h->proj.part, proj_part_bytes(n))) || (rc = ensure(h, h->proj.table, kProjTableBytes)) ||
        (rc = ensure(h, h->proj.start, kProjStartBytes))) return rc;
    ProjArgs a{};
    a.d_in = static_cast<const unsigned char*>(pts);
    if (!on_device) {
        if ((rc = stage_host_records(h, h->proj.in, pts, n * (size_t)layout->stride))) return rc;
        a.d_in = h->proj.in.as<unsigned char>();
    }
    if (do_deskew) {
        const size_t m = sizeof(double) * (size_t)(deskew->imu_pointer_cur + 1);
        double* t = h->proj.table.as<double>();
        S2M_HIP(h, hipMemcpyAsync(t, deskew->imu_time, m, hipMemcpyHostToDevice, h->stream));
        S2M_HIP(h, hipMemcpyAsync(t + S2M_IMU_QUEUE_LENGTH, deskew->imu_rot_x, m, hipMemcpyHostToDevice, h->stream));
        S2M_HIP(h, hipMemcpyAsync(t + 2 * S2M_IMU_QUEUE_LENGTH, deskew->imu_rot_y, m, hipMemcpyHostToDevice, h->stream));
        S2M_HIP(h, hipMemcpyAsync(t + 3 * S2M_IMU_QUEUE_LENGTH, deskew->imu_rot_z, m, hipMemcpyHostToDevice, h->stream));
    }
    a.n = n; a.lay = *layout; a.prm = prm; a.deskew = do_deskew;
    a.imu_pointer_cur = do_deskew ? deskew->imu_pointer_cur : 0;
    a.time_scan_cur = deskew ? deskew->time_scan_cur : 0.0;
    if (motion && motion->enabled) {                                         // findPosition() live (:526-533)
        a.motion = 1;
        a.time_scan_end = motion->time_scan_end;
        for (int k = 0; k < 3; k++) a.odom_incre[k] = motion->odom_incre[k];
    }
    a.d_table = h->proj.table.as<double>();
    a.d_mask = h->proj.mask.as<unsigned long long>();
    a.d_part = h->proj.part.as<int32_t>();
    a.d_start = h->proj.start.as<float>();
    a.d_out = h->proj.cloud_deskewed.as<unsigned char>();
    a.h_count = h->proj.h_count;
    hipError_t e = proj_launch(h->stream, a);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "point filter and deskew", e);
    // the one wait: the count is in pinned memory and the kernels have left the caller's records (host or device)
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const size_t cnt = (size_t)h->proj.h_count->n_out;
    *n_out = cnt;
    h->proj.deskewed_n = cnt;
    h->proj.have_deskewed = true;
    return finish_cloud(h, h->proj.cloud_deskewed, VoxResult{ cnt, 0 }, out, out_stride_bytes, cap, "output buffer too small for the deskewed cloud");
}

int s2m_project_scan(s2m_handle h, const void* pts, size_t n, const s2m_scan_layout* layout, int on_device, const s2m_project_params* params,
                     const s2m_deskew_info* deskew, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    return project_scan_impl(h, pts, n, layout, on_device, params, deskew, nullptr, out, out_stride_bytes, cap, n_out);
}

int s2m_project_scan_motion(s2m_handle h, const void* pts, size_t n, const s2m_scan_layout* layout, int on_device, const s2m_project_params* params,
                            const s2m_deskew_info* deskew, const s2m_motion_info* motion, void* out, size_t out_stride_bytes, size_t cap,
                            size_t* n_out)
{
    return project_scan_impl(h, pts, n, layout, on_device, params, deskew, motion, out, out_stride_bytes, cap, n_out);
}

// ---- odomDeskewInfo() and updateInitialGuess(): host code, no handle ---------------------------------------------------
int s2m_odom_deskew_info(const s2m_odom_sample* odom, size_t n, double time_scan_cur, double time_scan_end, float imu_rate, s2m_odom_deskew* out)
{
    if ((n > 0 && !odom) || !out || !std::isfinite(time_scan_cur) || !std::isfinite(time_scan_end)) return S2M_ERR_INVALID_ARG;
    return host_odom_deskew_info(odom, n, time_scan_cur, time_scan_end, imu_rate, out);
}

int s2m_guess_state_init(s2m_guess_state* st)
{
    if (!st) return S2M_ERR_INVALID_ARG;
    std::memset(st, 0, sizeof(*st));
    return S2M_OK;
}

int s2m_update_initial_guess(s2m_guess_state* st, float pose[6], int key_poses_empty, const s2m_guess_info* info,
                             int use_imu_heading_initialization, int imu_type, float affine_front[12])
{
    if (!st || !pose || !info || !affine_front) return S2M_ERR_INVALID_ARG;
    host_update_initial_guess(st, pose, key_poses_empty, *info, use_imu_heading_initialization, imu_type, affine_front);
    return S2M_OK;
}

int s2m_sc_add_projected(s2m_handle h)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!h->proj.have_deskewed) return fail(h, S2M_ERR_NO_SCAN, "s2m_sc_add_projected before s2m_project_scan");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = sc_build_descriptor(h, h->proj.cloud_deskewed.p, h->proj.deskewed_n, kProjOutStride, true))) return rc;
    if ((rc = sc_append_from_out(h))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}
