// image_projection_s2m.hpp - C++ mirror of the cloud path of the reference's ImageProjection node (src/imageProjection.cpp)
// over the C ABI of include/liorf_s2m.h: member and method names are the reference's. imuDeskewInfo() and odomDeskewInfo() run on the host,
// projectPointCloud() on the device of the handle it is given (a MapOptimizationS2M's), where cloud_deskewed stays for
// MapOptimizationS2M::downsampleCurrentScanProjected() and SCManagerS2M::makeAndSaveScancontextAndKeysProjected().
#pragma once
#include <array>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "map_optimization_s2m.hpp"

namespace liorf_amd {

class ImageProjectionS2M {
public:
    explicit ImageProjectionS2M(s2m_handle h, int32_t sensor = S2M_SENSOR_VELODYNE) : h_(h)
    {
        if (s2m_scan_layout_preset(sensor, &layout) != S2M_OK) throw std::runtime_error("unknown sensor");
        s2m_project_default_params(&params);
        imuTime.resize(S2M_IMU_QUEUE_LENGTH); imuRotX.resize(S2M_IMU_QUEUE_LENGTH);
        imuRotY.resize(S2M_IMU_QUEUE_LENGTH); imuRotZ.resize(S2M_IMU_QUEUE_LENGTH);
    }

    // ParamServer members (include/utility.h:204-209) and the record layout of the sensor
    s2m_project_params params{};
    s2m_scan_layout layout{};
    int deskewFlag = 1;                                // (:310-323): 1 when the message has a time field, else -1
    // members of the reference (:83-99)
    double timeScanCur = 0, timeScanEnd = 0;
    std::vector<double> imuTime, imuRotX, imuRotY, imuRotZ;
    int imuPointerCur = 0;
    bool imuAvailable = false;                         // cloudInfo.imuAvailable
    std::vector<PointXYZI> fullCloud;                  // host copy of cloud_deskewed, filled on request
    size_t fullCloudNum = 0;
    float imuRate = 500.0f;                            // include/utility.h:212
    std::deque<s2m_odom_sample> odomQueue;             // stand-in for odomQueue (:77): the node pushes, odomDeskewInfo() pops
    bool odomAvailable = false;                        // cloudInfo.odomAvailable
    bool odomDeskewFlag = false;                       // (:102)
    float odomIncreX = 0, odomIncreY = 0, odomIncreZ = 0;      // (:103-105)
    float initialGuess[6] = { 0, 0, 0, 0, 0, 0 };      // cloudInfo.initialGuessX, Y, Z, Roll, Pitch, Yaw
    bool positionalDeskew = false;                     // findPosition() with its commented lines live (:526-533); off = the reference as shipped

    // the part of cachePointCloud() (:206-343) the cloud path needs: the raw bytes stay as they are; timeScanCur = header stamp,
    // timeScanEnd = timeScanCur + time of the last record (:282-283)
    void cachePointCloud(const void* data, size_t bytes, double stamp)
    {
        if (bytes % layout.stride) throw std::runtime_error("the buffer is not a whole number of records");
        raw_ = static_cast<const unsigned char*>(data);
        n_ = bytes / layout.stride;
        timeScanCur = stamp;
        timeScanEnd = timeScanCur + (n_ ? (double)recordTime(n_ - 1) : 0.0);
    }

    // laserCloudIn->points[i].time as the conversion loops leave it (:216-274)
    float recordTime(size_t i) const
    {
        const unsigned char* r = raw_ + i * layout.stride + layout.off_time;
        if (layout.time_type == S2M_TIME_F32) { float t; std::memcpy(&t, r, 4); return t; }
        if (layout.time_type == S2M_TIME_F64_REL) { double t, t0; std::memcpy(&t, r, 8); std::memcpy(&t0, raw_ + layout.off_time, 8); return (float)(t - t0); }
        uint32_t t; std::memcpy(&t, r, 4);
        return layout.time_type == S2M_TIME_U32_NS ? (float)t * 1e-9f : (float)t;
    }

    // void imuDeskewInfo() (:350-409) on samples {time, wx, wy, wz} already converted and popped to timeScanCur - 0.01
    void imuDeskewInfo(const std::vector<std::array<double, 4>>& imu)
    {
        int32_t cur = 0, avail = 0;
        const int rc = s2m_imu_deskew_info(imu.empty() ? nullptr : imu[0].data(), imu.size(), timeScanCur, timeScanEnd, imuTime.data(),
                                           imuRotX.data(), imuRotY.data(), imuRotZ.data(), &cur, &avail);
        if (rc != S2M_OK) throw std::runtime_error("s2m_imu_deskew_info: more samples than queueLength");
        imuPointerCur = cur;
        imuAvailable = avail != 0;
    }

    // void odomDeskewInfo() (:411-491) on odomQueue: pops its front as the reference does; like the reference's members,
    // initialGuess and odomIncre keep their previous values where the reference does not write them
    void odomDeskewInfo()
    {
        const std::vector<s2m_odom_sample> q(odomQueue.begin(), odomQueue.end());
        s2m_odom_deskew r{};
        if (s2m_odom_deskew_info(q.empty() ? nullptr : q.data(), q.size(), timeScanCur, timeScanEnd, imuRate, &r) != S2M_OK)
            throw std::runtime_error("s2m_odom_deskew_info: scan times are not finite");
        odomQueue.erase(odomQueue.begin(), odomQueue.begin() + r.n_popped);
        odomAvailable = r.odom_available != 0;
        if (r.odom_available) {
            std::memcpy(initialGuess, r.initial_guess, sizeof(initialGuess));
            odomDeskewFlag = r.odom_deskew_flag != 0;
        }
        if (r.odom_deskew_flag) { odomIncreX = r.odom_incre[0]; odomIncreY = r.odom_incre[1]; odomIncreZ = r.odom_incre[2]; }
    }

    // cloudInfo.odomAvailable and the six initialGuess fields, as publishClouds() sends them to mapOptimization (:602-604)
    void fillCloudInfo(CloudInfo& ci) const
    {
        ci.odomAvailable = odomAvailable ? 1 : 0;
        ci.initialGuessX = initialGuess[0]; ci.initialGuessY = initialGuess[1]; ci.initialGuessZ = initialGuess[2];
        ci.initialGuessRoll = initialGuess[3]; ci.initialGuessPitch = initialGuess[4]; ci.initialGuessYaw = initialGuess[5];
        ci.imuAvailable = imuAvailable ? 1 : 0;
    }

    // void projectPointCloud() (:568-598): cloud_deskewed stays on the device; fullCloud is filled when readback is set.
    // With positionalDeskew set, and odomAvailable and odomDeskewFlag (:526), findPosition()'s commented lines are live.
    void projectPointCloud(bool readback = true)
    {
        s2m_deskew_info d{};
        d.time_scan_cur = timeScanCur;
        d.deskew = (deskewFlag == 1 && imuAvailable) ? 1 : 0;
        d.imu_pointer_cur = d.deskew ? imuPointerCur : 0;
        d.imu_time = imuTime.data(); d.imu_rot_x = imuRotX.data(); d.imu_rot_y = imuRotY.data(); d.imu_rot_z = imuRotZ.data();
        const size_t cap = readback ? (n_ + (size_t)params.point_filter_num - 1) / (size_t)params.point_filter_num : 0;
        if (readback) fullCloud.resize(cap);
        size_t n_out = 0;
        s2m_motion_info mo{};
        mo.enabled = (positionalDeskew && odomAvailable && odomDeskewFlag) ? 1 : 0;
        mo.time_scan_end = timeScanEnd;
        mo.odom_incre[0] = odomIncreX; mo.odom_incre[1] = odomIncreY; mo.odom_incre[2] = odomIncreZ;
        const int rc = mo.enabled
            ? s2m_project_scan_motion(h_, raw_, n_, &layout, 0, &params, &d, &mo, readback ? fullCloud.data() : nullptr, sizeof(PointXYZI), cap, &n_out)
            : s2m_project_scan(h_, raw_, n_, &layout, 0, &params, &d, readback ? fullCloud.data() : nullptr, sizeof(PointXYZI), cap, &n_out);
        if (rc != S2M_OK) throw std::runtime_error(std::string("s2m_project_scan: ") + s2m_last_error(h_));
        if (readback) fullCloud.resize(n_out);
        fullCloudNum = n_out;
    }

private:
    s2m_handle h_;
    const unsigned char* raw_ = nullptr;
    size_t n_ = 0;
};

}  // namespace liorf_amd
