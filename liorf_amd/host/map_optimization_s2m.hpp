// map_optimization_s2m.hpp — C++ host-side mirror of the reference's mapOptimization members
// and methods that belong to the scan-to-map path, on top of the C ABI (include/liorf_s2m.h).
//
// The reference keeps this path's state as members of `class mapOptimization`
// (src/mapOptmization.cpp:87-233) and runs it from laserCloudInfoHandler() (:236-275, step :265).
// This class carries the same names with the same meaning so that the node's handler can keep
// its shape: fill laserCloudSurfFromMapDS / laserCloudSurfLastDS / transformTobeMapped / cloudInfo,
// call scan2MapOptimization(), read transformTobeMapped / isDegenerate /
// incrementalOdometryAffineBack.  All arithmetic runs in the HIP library; there is no CPU path here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/liorf_s2m.h"

namespace liorf_amd {

// pcl::PointXYZI layout (reference `typedef pcl::PointXYZI PointType`, include/utility.h:61):
// x,y,z,pad at 0..15, intensity at 16, padded to 32 bytes.
struct alignas(16) PointXYZI {
    float x, y, z, pad0;
    float intensity, pad1, pad2, pad3;
};
static_assert(sizeof(PointXYZI) == 32, "PointXYZI must match pcl::PointXYZI");

// PointTypePose (reference include/utility.h:66-83): key pose with the id in `intensity`.
struct PointTypePose {
    float x = 0, y = 0, z = 0, intensity = 0;
    float roll = 0, pitch = 0, yaw = 0;
    double time = 0;
};

// The fields of liorf::cloud_info this path reads (reference msg/cloud_info.msg:10-16).
struct CloudInfo {
    int64_t imuAvailable = 0;
    int64_t odomAvailable = 0;
    float imuRollInit = 0, imuPitchInit = 0, imuYawInit = 0;
    float initialGuessX = 0, initialGuessY = 0, initialGuessZ = 0;
    float initialGuessRoll = 0, initialGuessPitch = 0, initialGuessYaw = 0;
};

class SCManagerS2M;

class MapOptimizationS2M {
public:
    // reference members, same names -----------------------------------------------------------
    std::vector<PointXYZI> laserCloudSurfFromMapDS;   // local surf map, voxel-filtered (:124)
    std::vector<PointXYZI> laserCloudSurfLastDS;      // current scan, voxel-filtered (:108)
    int   laserCloudSurfLastDSNum = 0;                // (:131)
    int   laserCloudSurfFromMapDSNum = 0;             // (:130)
    std::vector<PointXYZI> laserCloudSurfLast;        // current scan before the filter (:107)
    std::vector<std::vector<PointXYZI>> surfCloudKeyFrames;   // key-frame clouds (:93)
    std::vector<PointTypePose> cloudKeyPoses6D;       // (:96)
    float mappingSurfLeafSize = 0.2f;                 // include/utility.h:227 (the shipped yaml files set 0.4)
    float surroundingKeyframeMapLeafSize = 0.2f;      // include/utility.h:228
    float surroundingKeyframeSearchRadius = 50.0f;    // include/utility.h:240
    float transformTobeMapped[6] = { 0, 0, 0, 0, 0, 0 };   // roll,pitch,yaw,x,y,z (:134)
    bool  isDegenerate = false;                       // (:139)
    float incrementalOdometryAffineBack[12] = { 0 };  // row-major 3x4 (:157)
    float incrementalOdometryAffineFront[12] = { 0 }; // row-major 3x4 (:156), set by updateInitialGuess()
    bool  useImuHeadingInitialization = false;        // include/utility.h:170
    CloudInfo cloudInfo;                              // (:99)
    bool  haveKeyPoses = false;                       // !cloudKeyPoses3D->points.empty() (:1297)
    // ParamServer values the path reads (include/utility.h:211-233)
    int   imuType = 0;
    float imuRPYWeight = 0.01f, z_tollerance = 3.4028235e38f, rotation_tollerance = 3.4028235e38f;
    // what the last call did
    s2m_result lastResult{};

    explicit MapOptimizationS2M(int device_id = 0, void* hip_stream = nullptr)
    {
        s2m_params p;
        s2m_default_params(&p);
        p.device_id = device_id;
        p.stream = hip_stream;
        s2m_guess_state_init(&guessState_);
        const int rc = s2m_create(&p, &h_);       // the ParamServer members below are pushed before every call (pushParams)
        if (rc != S2M_OK)
            throw std::runtime_error("s2m_create failed (" + std::to_string(rc) + "): no gfx950 device; there is no CPU fallback");
    }
    ~MapOptimizationS2M() { if (h_) s2m_destroy(h_); }
    MapOptimizationS2M(const MapOptimizationS2M&) = delete;
    MapOptimizationS2M& operator=(const MapOptimizationS2M&) = delete;

    // kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS) (:1302), hoisted so that a map
    // that did not change between scans is not rebuilt
    void setInputCloud()
    {
        check(s2m_set_map(h_, laserCloudSurfFromMapDS.data(), haveKeyPoses ? laserCloudSurfFromMapDS.size() : 0,
                          sizeof(PointXYZI)), "s2m_set_map");
    }

    // void downsampleCurrentScan() (:1061-1067): laserCloudSurfLast -> laserCloudSurfLastDS on the device;
    // the filtered scan stays resident for scan2MapOptimization() and is copied back for the key-frame store
    void downsampleCurrentScan()
    {
        laserCloudSurfLastDS.resize(laserCloudSurfLast.size());
        size_t n_out = 0;
        checkVoxel(s2m_downsample_scan(h_, laserCloudSurfLast.data(), laserCloudSurfLast.size(), sizeof(PointXYZI), 0,
                                       mappingSurfLeafSize, laserCloudSurfLastDS.data(), sizeof(PointXYZI),
                                       laserCloudSurfLastDS.size(), &n_out), "s2m_downsample_scan");
        laserCloudSurfLastDS.resize(n_out);
        laserCloudSurfLastDSNum = (int)n_out;
        scanResident_ = true;
    }

    // downsampleCurrentScan() on the cloud_deskewed an ImageProjectionS2M::projectPointCloud() left on this handle's device: no
    // deskewed cloud crosses the bus. cloudDeskewedNum is that projection's count (ImageProjectionS2M::fullCloudNum): the filter
    // never returns more points than it was given, so it sizes laserCloudSurfLastDS the way laserCloudSurfLast.size() does in
    // downsampleCurrentScan(). With readback off laserCloudSurfLastDS is left empty (the scan is resident; saveKeyFrame() would
    // store an empty host cloud) and only laserCloudSurfLastDSNum is set.
    void downsampleCurrentScanProjected(size_t cloudDeskewedNum, bool readback = true)
    {
        size_t n_out = 0;
        laserCloudSurfLastDS.resize(readback ? cloudDeskewedNum : 0);
        checkVoxel(s2m_downsample_projected(h_, mappingSurfLeafSize, readback ? laserCloudSurfLastDS.data() : nullptr, sizeof(PointXYZI),
                                            laserCloudSurfLastDS.size(), &n_out), "s2m_downsample_projected");
        if (readback) {
            if (n_out > laserCloudSurfLastDS.size()) throw std::runtime_error("s2m_downsample_projected: cloudDeskewedNum is not the projection's count");
            laserCloudSurfLastDS.resize(n_out);
        }
        laserCloudSurfLastDSNum = (int)n_out;
        scanResident_ = true;
    }

    // void extractCloud(cloudToExtract) (:1014-1039): `keyInds` are the key-frame ids the caller's radius
    // search and time filter chose (extractNearby, :973-1012). Frames farther than
    // surroundingKeyframeSearchRadius from the newest key pose are dropped (:1018), the rest are transformed
    // by their key pose, concatenated, voxel-filtered and indexed on the device; there is no
    // laserCloudMapContainer cache to maintain.
    void extractCloud(const std::vector<int>& keyInds)
    {
        std::vector<const void*> frames;
        std::vector<size_t> sizes;
        std::vector<float> poses;
        size_t total = 0;
        if (!cloudKeyPoses6D.empty()) {
            const PointTypePose& last = cloudKeyPoses6D.back();
            for (int k : keyInds) {
                const PointTypePose& p = cloudKeyPoses6D[(size_t)k];
                const float dx = p.x - last.x, dy = p.y - last.y, dz = p.z - last.z;
                if (std::sqrt(dx * dx + dy * dy + dz * dz) > surroundingKeyframeSearchRadius) continue;
                frames.push_back(surfCloudKeyFrames[(size_t)k].data());
                sizes.push_back(surfCloudKeyFrames[(size_t)k].size());
                const float v[6] = { p.x, p.y, p.z, p.roll, p.pitch, p.yaw };
                poses.insert(poses.end(), v, v + 6);
                total += sizes.back();
            }
        }
        laserCloudSurfFromMapDS.resize(total);
        size_t n_out = 0;
        checkVoxel(s2m_extract_cloud(h_, (int)frames.size(), frames.data(), sizes.data(), sizeof(PointXYZI), 0, poses.data(),
                                     surroundingKeyframeMapLeafSize, laserCloudSurfFromMapDS.data(), sizeof(PointXYZI),
                                     total, &n_out), "s2m_extract_cloud");
        laserCloudSurfFromMapDS.resize(n_out);
        laserCloudSurfFromMapDSNum = (int)n_out;
        haveKeyPoses = !cloudKeyPoses6D.empty();
    }

    // The resident key-frame store (s2m_kf_*): the device keeps every key frame's cloud and pose, so the handler's
    // extractSurroundingKeyFrames() needs no kd-tree over the key poses and uploads no key-frame cloud. The host copy of
    // cloudKeyPoses6D stays for the pose graph; surfCloudKeyFrames only for extractCloud() above (the global map and the saved
    // map come from the store: publishGlobalMap(), globalMapCloud()).
    float surroundingKeyframeDensity = 1.0f;          // include/utility.h:238 (the shipped yaml files set 2.0)
    double timeLaserInfoCur = 0;                      // (:255)
    std::vector<int> surroundingKeyInds;              // the key ids the last extractSurroundingKeyFrames() concatenated

    // void extractSurroundingKeyFrames() (:1046-1059): extractNearby + extractCloud against the store, map installed
    void extractSurroundingKeyFrames()
    {
        s2m_kf_params p;
        s2m_kf_default_params(&p);
        p.search_radius = surroundingKeyframeSearchRadius;
        p.density = surroundingKeyframeDensity;
        p.map_leaf = surroundingKeyframeMapLeafSize;
        surroundingKeyInds.resize(2 * cloudKeyPoses6D.size() + 1);
        size_t n_out = 0, n_keys = 0;
        checkVoxel(s2m_extract_surrounding(h_, timeLaserInfoCur, &p, nullptr, sizeof(PointXYZI), 0, &n_out,
                                           surroundingKeyInds.data(), surroundingKeyInds.size(), &n_keys),
                   "s2m_extract_surrounding");
        surroundingKeyInds.resize(n_keys);
        if (!cloudKeyPoses6D.empty()) {
            laserCloudSurfFromMapDSNum = (int)n_out;
            haveKeyPoses = true;
        }
    }

    // s2m_extract_surrounding_at: the same around centre_xyz instead of the newest key, without the recent keys - the local map of
    // a node that was localised in a stored map (relocalizeScan below) and is not at its newest key
    void extractSurroundingKeyFramesAt(const float centre_xyz[3])
    {
        s2m_kf_params p;
        s2m_kf_default_params(&p);
        p.search_radius = surroundingKeyframeSearchRadius;
        p.density = surroundingKeyframeDensity;
        p.map_leaf = surroundingKeyframeMapLeafSize;
        surroundingKeyInds.resize(2 * cloudKeyPoses6D.size() + 1);
        size_t n_out = 0, n_keys = 0;
        checkVoxel(s2m_extract_surrounding_at(h_, centre_xyz, &p, nullptr, sizeof(PointXYZI), 0, &n_out,
                                              surroundingKeyInds.data(), surroundingKeyInds.size(), &n_keys),
                   "s2m_extract_surrounding_at");
        surroundingKeyInds.resize(n_keys);
        if (!cloudKeyPoses6D.empty()) {
            laserCloudSurfFromMapDSNum = (int)n_out;
            haveKeyPoses = true;
        }
    }

    // the key-frame part of saveKeyFramesAndFactor() (:1549-1580): the pose after scan2MapOptimization() and
    // laserCloudSurfLastDS as downsampleCurrentScan() left it on the device (copied device to device)
    void saveKeyFrame()
    {
        PointTypePose p;
        p.x = transformTobeMapped[3]; p.y = transformTobeMapped[4]; p.z = transformTobeMapped[5];
        p.roll = transformTobeMapped[0]; p.pitch = transformTobeMapped[1]; p.yaw = transformTobeMapped[2];
        p.intensity = (float)cloudKeyPoses6D.size();
        p.time = timeLaserInfoCur;
        const float v[6] = { p.x, p.y, p.z, p.roll, p.pitch, p.yaw };
        check(s2m_kf_add(h_, v, timeLaserInfoCur, nullptr, 0, sizeof(PointXYZI), S2M_KF_FROM_LAST_DOWNSAMPLE), "s2m_kf_add");
        cloudKeyPoses6D.push_back(p);
        surfCloudKeyFrames.push_back(laserCloudSurfLastDS);
    }

    // correctPoses() (:1611-1640) after the pose graph moved the key poses: cloudKeyPoses6D holds the new values
    void correctPoses()
    {
        std::vector<float> v;
        v.reserve(6 * cloudKeyPoses6D.size());
        for (const PointTypePose& p : cloudKeyPoses6D) { const float q[6] = { p.x, p.y, p.z, p.roll, p.pitch, p.yaw }; v.insert(v.end(), q, q + 6); }
        check(s2m_kf_set_poses(h_, 0, (int)cloudKeyPoses6D.size(), v.data()), "s2m_kf_set_poses");
    }

    // One closure the loop thread queued (loopIndexQueue / loopPoseQueue / loopNoiseQueue, :1513-1534): rel is
    // poseFrom.between(poseTo) as {x, y, z, roll, pitch, yaw}; robust_k > 0 is the SC loop's Cauchy model.
    struct LoopFactor { int key_cur, key_pre; float rel[6]; double var[6]; double robust_k; };
    std::vector<LoopFactor> loopQueue;
    bool aLoopIsClosed = false;
    s2m_pg_result lastGraphResult{};

    // saveKeyFramesAndFactor() (:1536-1609) on the library's pose graph, without the saveFrame() gate and the GPS queue (the
    // caller's): odometry factor, the queued loop factors, the update - twice after a closure, as the reference repeats
    // isam->update() - then the key frame with the graph's latest estimate, which also becomes transformTobeMapped (:1583-1588).
    void saveKeyFramesAndFactor()
    {
        const float v[6] = { transformTobeMapped[3], transformTobeMapped[4], transformTobeMapped[5],
                             transformTobeMapped[0], transformTobeMapped[1], transformTobeMapped[2] };
        check(s2m_pg_add_odometry(h_, v), "s2m_pg_add_odometry");
        for (const LoopFactor& l : loopQueue) {
            check(s2m_pg_add_between(h_, l.key_cur, l.key_pre, l.rel, l.var, l.robust_k), "s2m_pg_add_between");
            aLoopIsClosed = true;
        }
        loopQueue.clear();
        check(s2m_pg_optimize(h_, nullptr, &lastGraphResult), "s2m_pg_optimize");
        if (aLoopIsClosed) check(s2m_pg_optimize(h_, nullptr, &lastGraphResult), "s2m_pg_optimize");
        float latest[6];
        check(s2m_pg_get_poses(h_, (int32_t)cloudKeyPoses6D.size(), 1, latest), "s2m_pg_get_poses");
        transformTobeMapped[3] = latest[0]; transformTobeMapped[4] = latest[1]; transformTobeMapped[5] = latest[2];
        transformTobeMapped[0] = latest[3]; transformTobeMapped[1] = latest[4]; transformTobeMapped[2] = latest[5];
        saveKeyFrame();
    }

    // The optimise beside the scan handler (s2m_pg_optimize_launch / _poll / _collect), for the update after a loop or GPS factor
    // went in: take the scan handler's lock, pgOptimizeLaunch(), release; key frames keep going into the graph meanwhile
    // (s2m_pg_add_odometry chains on the launch-time estimate); then lock, pgOptimizePoll(), release, sleep - until it returns
    // S2M_OK, and then correctPosesFromGraph(). Each returns the status: S2M_PG_PENDING, S2M_PG_IDLE (nothing pending) or
    // S2M_OK with lastGraphResult final (from the launch: an empty graph). Everything else throws.
    int pgOptimizeLaunch(const s2m_pg_params* p = nullptr) { return pgCode(s2m_pg_optimize_launch(h_, p, &lastGraphEarly), "s2m_pg_optimize_launch", &lastGraphEarly); }
    int pgOptimizePoll() { s2m_pg_result r{}; return pgCode(s2m_pg_optimize_poll(h_, &r), "s2m_pg_optimize_poll", &r); }       // never waits for the device
    int pgOptimizeCollect() { s2m_pg_result r{}; return pgCode(s2m_pg_optimize_collect(h_, &r), "s2m_pg_optimize_collect", &r); }
    s2m_pg_result lastGraphEarly{};

    // poseCovariance (:1565) for several keys in one block solve (s2m_pg_marginals): 36 doubles per key, row-major 6x6 in the
    // tangent order of rotation then translation; and the joint covariance of two keys (s2m_pg_joint_marginal), row-major 12x12
    std::vector<double> poseCovariances(const std::vector<int32_t>& keys)
    {
        std::vector<double> cov(36 * keys.size());
        check(s2m_pg_marginals(h_, keys.data(), (int32_t)keys.size(), cov.data()), "s2m_pg_marginals");
        return cov;
    }
    std::vector<double> jointPoseCovariance(int32_t key_a, int32_t key_b)
    {
        std::vector<double> cov(144);
        check(s2m_pg_joint_marginal(h_, key_a, key_b, cov.data()), "s2m_pg_joint_marginal");
        return cov;
    }

    // correctPoses() (:1611-1642) from the pose graph: the store is corrected in place on the device, cloudKeyPoses6D follows
    bool correctPosesFromGraph()
    {
        if (cloudKeyPoses6D.empty() || !aLoopIsClosed) return false;
        const int32_t n = (int32_t)cloudKeyPoses6D.size();
        check(s2m_pg_apply_to_store(h_, 0, n), "s2m_pg_apply_to_store");
        std::vector<float> v(6 * (size_t)n);
        check(s2m_pg_get_poses(h_, 0, n, v.data()), "s2m_pg_get_poses");
        for (int32_t k = 0; k < n; k++) {
            PointTypePose& q = cloudKeyPoses6D[(size_t)k];
            q.x = v[6 * k]; q.y = v[6 * k + 1]; q.z = v[6 * k + 2]; q.roll = v[6 * k + 3]; q.pitch = v[6 * k + 4]; q.yaw = v[6 * k + 5];
        }
        aLoopIsClosed = false;
        return true;
    }

    // The global map and the saved map from the store (s2m_global_map, s2m_kf_map_cloud): visualizeGlobalMapThread() and
    // saveMapService() need no host copy of surfCloudKeyFrames. Both run under the lock the scan handler holds, for the
    // whole call; the node still publishes the cloud and writes the PCD files (trajectory.pcd / transformations.pcd from
    // cloudKeyPoses3D / cloudKeyPoses6D, as before).
    float globalMapVisualizationSearchRadius = 1e3f;   // include/utility.h:250
    float globalMapVisualizationPoseDensity = 10.0f;   // include/utility.h:251 (M2DGR.yaml: 3.0)
    float globalMapVisualizationLeafSize = 1.0f;       // include/utility.h:252
    std::vector<PointXYZI> globalMapKeyFramesDS;       // what publishGlobalMap() publishes (:500)
    std::vector<int> globalMapKeyInds;                 // the key ids concatenated into it, in order

    // publishGlobalMap() (:453-502) without the subscriber test and the publish: fills globalMapKeyFramesDS
    void publishGlobalMap()
    {
        s2m_gmap_params p;
        s2m_gmap_default_params(&p);
        p.search_radius = globalMapVisualizationSearchRadius;
        p.pose_density = globalMapVisualizationPoseDensity;
        p.leaf = globalMapVisualizationLeafSize;
        globalMapKeyInds.resize(cloudKeyPoses6D.size() + 1);
        globalMapKeyFramesDS.resize(globalMapKeyFramesDS.capacity());      // the last call's size: one call in the steady state
        size_t n_out = 0, n_keys = 0;
        int rc = S2M_OK;
        for (int attempt = 0; attempt < 2; attempt++) {          // a cloud larger than the buffer: once more with room for it
            rc = s2m_global_map(h_, &p, globalMapKeyFramesDS.data(), sizeof(PointXYZI), globalMapKeyFramesDS.size(), &n_out,
                                globalMapKeyInds.data(), globalMapKeyInds.size(), &n_keys);
            if ((rc != S2M_OK && rc != S2M_ERR_CAPACITY && rc != S2M_WARN_LEAF_TOO_SMALL) || n_out <= globalMapKeyFramesDS.size()) break;
            globalMapKeyFramesDS.resize(n_out);
        }
        checkVoxel(rc, "s2m_global_map");
        globalMapKeyFramesDS.resize(n_out);
        globalMapKeyInds.resize(n_keys);
    }

    // saveMapService()'s clouds (:395-407): globalSurfCloud of keys first .. first+count-1 (resolution 0: GlobalMap.pcd, and
    // SurfMap.pcd at resolution 0) or its VoxelGrid at `resolution` (SurfMap.pcd)
    void globalMapCloud(std::vector<PointXYZI>& cloud, float resolution, int first = 0, int count = -1)
    {
        if (count < 0) count = (int)cloudKeyPoses6D.size() - first;
        size_t n = 0;
        check(s2m_kf_map_cloud(h_, first, count, 0.0f, nullptr, sizeof(PointXYZI), 0, &n), "s2m_kf_map_cloud");   // the size query
        cloud.resize(n);
        if (n > 0) checkVoxel(s2m_kf_map_cloud(h_, first, count, resolution, cloud.data(), sizeof(PointXYZI), n, &n), "s2m_kf_map_cloud");
        cloud.resize(n);
    }

    // The reference reads imuType / imuRPYWeight / z_tollerance / rotation_tollerance (ParamServer members, set from
    // the yaml after construction) whenever transformUpdate() runs (:1325-1350): the current member values are
    // handed to the library before every registration.
    void pushParams()
    {
        s2m_params p;
        check(s2m_get_params(h_, &p), "s2m_get_params");
        if (p.imu_type == imuType && p.imu_rpy_weight == imuRPYWeight && p.z_tol == z_tollerance && p.rot_tol == rotation_tollerance) return;
        p.imu_type = imuType; p.imu_rpy_weight = imuRPYWeight;
        p.z_tol = z_tollerance; p.rot_tol = rotation_tollerance;
        check(s2m_set_params(h_, &p), "s2m_set_params");
    }

    // void updateInitialGuess() (:899-958): transformTobeMapped becomes the pose scan2MapOptimization() starts from,
    // incrementalOdometryAffineFront the transform before the update; the three function statics live in guessState_.
    // haveKeyPoses is !cloudKeyPoses3D->points.empty() (:906).
    void updateInitialGuess()
    {
        s2m_guess_info ci{};
        ci.imuAvailable = cloudInfo.imuAvailable; ci.odomAvailable = cloudInfo.odomAvailable;
        ci.imuRollInit = cloudInfo.imuRollInit; ci.imuPitchInit = cloudInfo.imuPitchInit; ci.imuYawInit = cloudInfo.imuYawInit;
        ci.initialGuess[0] = cloudInfo.initialGuessX; ci.initialGuess[1] = cloudInfo.initialGuessY; ci.initialGuess[2] = cloudInfo.initialGuessZ;
        ci.initialGuess[3] = cloudInfo.initialGuessRoll; ci.initialGuess[4] = cloudInfo.initialGuessPitch; ci.initialGuess[5] = cloudInfo.initialGuessYaw;
        check(s2m_update_initial_guess(&guessState_, transformTobeMapped, haveKeyPoses ? 0 : 1, &ci, useImuHeadingInitialization ? 1 : 0, imuType,
                                       incrementalOdometryAffineFront), "s2m_update_initial_guess");
    }

    // void scan2MapOptimization() (:1295-1321)
    void scan2MapOptimization()
    {
        pushParams();
        s2m_imu_init imu;
        imu.imuAvailable = cloudInfo.imuAvailable;
        imu.imuRollInit = cloudInfo.imuRollInit; imu.imuPitchInit = cloudInfo.imuPitchInit; imu.imuYawInit = cloudInfo.imuYawInit;
        if (scanResident_) {        // downsampleCurrentScan() left the scan on the device
            scanResident_ = false;
            check(s2m_optimize_resident(h_, transformTobeMapped, &imu, &lastResult), "s2m_optimize_resident");
        } else {
            laserCloudSurfLastDSNum = (int)laserCloudSurfLastDS.size();
            check(s2m_optimize(h_, laserCloudSurfLastDS.data(), laserCloudSurfLastDS.size(), sizeof(PointXYZI),
                               transformTobeMapped, &imu, &lastResult), "s2m_optimize");
        }
        if (lastResult.skipped == 2) {
            // ROS_WARN("Not enough features! Only %d planar features available.", ...) (:1319)
            return;
        }
        if (lastResult.skipped == 0) {
            isDegenerate = lastResult.is_degenerate != 0;
            std::memcpy(incrementalOdometryAffineBack, lastResult.affine, sizeof(incrementalOdometryAffineBack));
        }
    }

    // No counterpart in the reference (it registers one scan at a time under `mtx`, :252): n scans against the resident map at
    // once - s2m_optimize_batch, the scans' LM loops in lockstep inside one graph.  `scans[b]` = laserCloudSurfLastDS of scan b,
    // `poses[6*b..]` in: initial guess, out: transformTobeMapped of scan b; results as lastResult would hold them.  Bitwise
    // what n calls of scan2MapOptimization() give.
    std::vector<s2m_result> scan2MapOptimizationBatch(const std::vector<const std::vector<PointXYZI>*>& scans, std::vector<float>& poses,
                                                      const std::vector<CloudInfo>* infos = nullptr)
    {
        pushParams();
        const int n = (int)scans.size();
        if ((int)poses.size() != 6 * n) throw std::runtime_error("scan2MapOptimizationBatch: poses must hold 6 floats per scan");
        std::vector<const void*> ptrs((size_t)n);
        std::vector<size_t> sizes((size_t)n);
        for (int b = 0; b < n; b++) { ptrs[(size_t)b] = scans[(size_t)b]->data(); sizes[(size_t)b] = scans[(size_t)b]->size(); }
        std::vector<s2m_imu_init> imu((size_t)n);
        for (int b = 0; b < n; b++) {
            const CloudInfo& ci = infos ? (*infos)[(size_t)b] : cloudInfo;
            imu[(size_t)b].imuAvailable = ci.imuAvailable;
            imu[(size_t)b].imuRollInit = ci.imuRollInit; imu[(size_t)b].imuPitchInit = ci.imuPitchInit; imu[(size_t)b].imuYawInit = ci.imuYawInit;
        }
        std::vector<s2m_result> res((size_t)n);
        check(s2m_optimize_batch(h_, n, ptrs.data(), sizes.data(), sizeof(PointXYZI), poses.data(), imu.data(), res.data()), "s2m_optimize_batch");
        return res;
    }

    // A stream of scans through two slots (s2m_slot_*): prepareNextScan(slot, cloud) orders the NEXT scan on that slot's stream
    // while the loop launched with launchSlot() on the other slot runs; collectSlot() is scan2MapOptimization()'s second half
    // (synchronise, transformUpdate(), members updated).  The reference does the steps strictly one after the other (:257-265).
    void prepareNextScan(int slot, const std::vector<PointXYZI>& cloud)
    {
        check(s2m_slot_set_scan(h_, slot, cloud.data(), cloud.size(), sizeof(PointXYZI), 0), "s2m_slot_set_scan");
    }
    void launchSlot(int slot)
    {
        pushParams();
        check(s2m_slot_optimize_launch(h_, slot, transformTobeMapped), "s2m_slot_optimize_launch");
    }
    void collectSlot(int slot)
    {
        s2m_imu_init imu;
        imu.imuAvailable = cloudInfo.imuAvailable;
        imu.imuRollInit = cloudInfo.imuRollInit; imu.imuPitchInit = cloudInfo.imuPitchInit; imu.imuYawInit = cloudInfo.imuYawInit;
        check(s2m_slot_optimize_collect(h_, slot, transformTobeMapped, &imu, &lastResult), "s2m_slot_optimize_collect");
        if (lastResult.skipped == 0) {
            isDegenerate = lastResult.is_degenerate != 0;
            std::memcpy(incrementalOdometryAffineBack, lastResult.affine, sizeof(incrementalOdometryAffineBack));
        }
    }

    // The ICP block of performRSLoopClosure / performSCLoopClosure (:571-586, :663-678): settings, align(),
    // hasConverged(), getFitnessScore(), getFinalTransformation().  Returns false where the reference returns early.
    float historyKeyframeSearchRadius = 10.0f;        // include/utility.h:245
    float historyKeyframeFitnessScore = 0.3f;         // include/utility.h:248
    bool icpAlign(const std::vector<PointXYZI>& cureKeyframeCloud, const std::vector<PointXYZI>& prevKeyframeCloud,
                  float finalTransformation[16])
    {
        if (cureKeyframeCloud.size() < 300 || prevKeyframeCloud.size() < 1000) return false;       // :565-566
        s2m_icp_params p;
        s2m_icp_default_params(&p);
        p.max_correspondence_distance = historyKeyframeSearchRadius * 2;                            // :573
        s2m_icp_result r;
        check(s2m_icp_align(h_, cureKeyframeCloud.data(), cureKeyframeCloud.size(), prevKeyframeCloud.data(),
                            prevKeyframeCloud.size(), sizeof(PointXYZI), &p, &r), "s2m_icp_align");
        if (!r.converged || r.fitness_score > historyKeyframeFitnessScore) return false;            // :585-586
        std::memcpy(finalTransformation, r.T, sizeof(r.T));
        return true;
    }

    // icp.align(output, guess): the same block started at `guess` (row-major 4x4, nullptr: the identity - icpAlign);
    // finalTransformation includes the guess
    bool icpAlignGuess(const std::vector<PointXYZI>& cureKeyframeCloud, const std::vector<PointXYZI>& prevKeyframeCloud,
                       const float guess[16], float finalTransformation[16])
    {
        if (cureKeyframeCloud.size() < 300 || prevKeyframeCloud.size() < 1000) return false;       // :565-566
        s2m_icp_params p;
        s2m_icp_default_params(&p);
        p.max_correspondence_distance = historyKeyframeSearchRadius * 2;                            // :573
        s2m_icp_result r;
        check(s2m_icp_align_guess(h_, cureKeyframeCloud.data(), cureKeyframeCloud.size(), prevKeyframeCloud.data(),
                                  prevKeyframeCloud.size(), sizeof(PointXYZI), guess, &p, &r), "s2m_icp_align_guess");
        if (!r.converged || r.fitness_score > historyKeyframeFitnessScore) return false;            // :585-586
        std::memcpy(finalTransformation, r.T, sizeof(r.T));
        return true;
    }

    // Loop closure against the resident key-frame store (:542-844): no host key-frame clouds and no kdtreeHistoryKeyPoses.
    // Every call runs under the lock the scan handler holds (one handle, calls not concurrent); the launched forms below hold it
    // up to the size gate only. GTSAM stays here: an
    // accepted result gives loopIndexQueue / loopPoseQueue / loopNoiseQueue as poseFrom.between(poseTo) of pose_from and
    // pose_to, with the noise from icp.fitness_score (RS) or the robust model (SC).
    float historyKeyframeSearchTimeDiff = 30.0f;      // include/utility.h:246
    int   historyKeyframeSearchNum = 25;              // include/utility.h:247
    float loopClosureICPSurfLeafSize = 0.3f;          // include/utility.h:239 (the shipped yaml files set 0.5)
    s2m_loop_result lastLoop{};                       // what the last loop call did
    std::vector<std::pair<int, int>> loopIndexContainer;   // accepted (key_cur, key_pre), in order (visualizeLoopClosure)

    s2m_loop_params loopParams() const
    {
        s2m_loop_params p;
        s2m_loop_default_params(&p);
        p.search_radius = historyKeyframeSearchRadius;
        p.time_diff_s = historyKeyframeSearchTimeDiff;
        p.search_num = historyKeyframeSearchNum;
        p.fitness_score = historyKeyframeFitnessScore;
        p.icp_leaf = loopClosureICPSurfLeafSize;
        return p;
    }

    // void performRSLoopClosure() (:542-622) with detectLoopClosureDistance() (:732-765) at timeLaserInfoCur
    bool performRSLoopClosure()
    {
        const s2m_loop_params p = loopParams();
        check(s2m_loop_closure_rs(h_, timeLaserInfoCur, &p, &lastLoop), "s2m_loop_closure_rs");
        return accepted();
    }

    // The launched forms (loopClosureThread, :506-622, beside laserCloudInfoHandler): the launch runs detection, submaps and the
    // size gate and queues the whole ICP on the handle's loop stream; the handle is free for the scan handler meanwhile. The
    // loop thread takes the scan handler's lock, launches, releases; then lock, loopPoll(), release, sleep - until loopPending()
    // is false. s2m_loop_align, s2m_loop_closure_rs, s2m_loop_near_keyframes and s2m_icp_align are S2M_ERR_BUSY in between.
    // Return value: a closure is pending (false: lastLoop is final - none, closed, too few points).
    bool performRSLoopClosureLaunch()
    {
        const s2m_loop_params p = loopParams();
        check(s2m_loop_closure_rs_launch(h_, timeLaserInfoCur, &p, &lastLoop), "s2m_loop_closure_rs_launch");
        return loopPending();
    }
    bool loopAlignLaunch(int key_cur, int key_pre, int base_key = -1)
    {
        const s2m_loop_params p = loopParams();
        check(s2m_loop_align_launch(h_, key_cur, key_pre, base_key, &p, &lastLoop), "s2m_loop_align_launch");
        return loopPending();
    }
    bool loopPending() const { return lastLoop.status == S2M_LOOP_PENDING; }
    // never waits for the device; true once the closure has ended and was accepted (lastLoop holds the result either way)
    bool loopPoll()
    {
        check(s2m_loop_poll(h_, &lastLoop), "s2m_loop_poll");
        return accepted();
    }
    // waits for the pending closure; true if it was accepted
    bool loopCollect()
    {
        check(s2m_loop_collect(h_, &lastLoop), "s2m_loop_collect");
        return accepted();
    }

    // -- verification: key_cur against up to S2M_LOOP_MAX_CANDIDATES stored keys, aligned in lockstep (s2m_loop_verify*) --
    // lastVerify[i] is what loopAlign(key_cur, key_pre[i], base_key) gives on a container without key_cur; lastBest the position
    // of the accepted record with the least (fitness, position) or -1. Only that pair goes into the container. A pending
    // verification is a pending closure: the same lock discipline and the same BUSY calls as performRSLoopClosureLaunch().
    std::vector<s2m_loop_result> lastVerify;
    int lastBest = -1;
    bool loopVerify(int key_cur, const std::vector<int32_t>& key_pre, int base_key = -1)
    {
        const s2m_loop_params p = loopParams();
        lastVerify.assign(S2M_LOOP_MAX_CANDIDATES, s2m_loop_result{});
        int32_t best = -1;
        check(s2m_loop_verify(h_, key_cur, key_pre.data(), (int32_t)key_pre.size(), base_key, &p, lastVerify.data(), &best), "s2m_loop_verify");
        lastVerify.resize(key_pre.size());
        lastBest = best;
        return verifyAccepted();
    }
    // -- relocalisation: where in the stored map is this scan (s2m_relocalize_scan) --
    // The top relocTopK hits of the place query, each aligned from T(pose[key]) * Rz(-yaw) in lockstep; lastReloc holds the
    // records in the query's order, lastRelocBest the accepted one with the least (fitness, position) or -1. true: a record was
    // accepted, and transformTobeMapped is its pose - extractSurroundingKeyFramesAt(&transformTobeMapped[3]) installs the map there.
    int relocTopK = 4;
    std::vector<s2m_reloc_candidate> lastReloc;
    int lastRelocBest = -1;
    bool relocalizeScan(const std::vector<PointXYZI>& scan)
    {
        s2m_reloc_params p;
        s2m_reloc_default_params(&p);
        p.query.top_k = relocTopK;
        p.loop = loopParams();
        lastReloc.assign(S2M_LOOP_MAX_CANDIDATES, s2m_reloc_candidate{});
        int32_t n = 0, best = -1;
        check(s2m_relocalize_scan(h_, scan.data(), scan.size(), sizeof(PointXYZI), 0, &p, lastReloc.data(), &n, &best), "s2m_relocalize_scan");
        lastReloc.resize((size_t)n);
        lastRelocBest = best;
        if (best < 0) return false;
        std::memcpy(transformTobeMapped, lastReloc[(size_t)best].pose_tobemapped, sizeof(float) * 6);
        return true;
    }

    // -- a session: the key-frame store, the ScanContext store, the loop container and the pose graph in one file
    // (s2m_session_save_file / s2m_session_load_file). A node that starts in yesterday's map: loadSession(path),
    // relocalizeScan(scan), extractSurroundingKeyFramesAt(&transformTobeMapped[3]), scan2MapOptimization().
    void saveSession(const std::string& path) { check(s2m_session_save_file(h_, path.c_str()), "s2m_session_save_file"); }
    // Into a node that has stored nothing yet (the library refuses anything else). The clouds stay in the library's store -
    // surfCloudKeyFrames is not filled - and cloudKeyPoses6D mirrors the loaded keys with the pose graph's estimates where the
    // graph holds them (after correctPoses() they are the store's poses), intensity = index; the keys' times stay with the library.
    s2m_session_info loadSession(const std::string& path)
    {
        s2m_session_info info{};
        check(s2m_session_load_file(h_, path.c_str(), &info), "s2m_session_load_file");
        cloudKeyPoses6D.assign((size_t)info.n_keys, PointTypePose{});
        const int32_t n = info.n_keys < info.n_variables ? info.n_keys : info.n_variables;
        std::vector<float> v(6 * (size_t)n);
        if (n > 0) check(s2m_pg_get_poses(h_, 0, n, v.data()), "s2m_pg_get_poses");
        for (int32_t k = 0; k < info.n_keys; k++) {
            PointTypePose& q = cloudKeyPoses6D[(size_t)k];
            q.intensity = (float)k;
            if (k < n) { q.x = v[6 * k]; q.y = v[6 * k + 1]; q.z = v[6 * k + 2]; q.roll = v[6 * k + 3]; q.pitch = v[6 * k + 4]; q.yaw = v[6 * k + 5]; }
        }
        surfCloudKeyFrames.clear();
        loopQueue.clear();
        aLoopIsClosed = false;
        return info;
    }

    // -- one map from two runs (s2m_session_append, s2m_relocalize_key, s2m_session_anchor_from_pairs, s2m_session_place) --
    // A saved session behind the keys the node holds, placed by `anchor` {x, y, z, roll, pitch, yaw} (nullptr: as stored).
    // cloudKeyPoses6D grows by the appended keys as loadSession fills it; surfCloudKeyFrames stays with the library.
    s2m_session_append_info sessionAppend(const std::string& path, const float* anchor = nullptr, const double* junction_var = nullptr)
    {
        s2m_session_append_info info{};
        check(s2m_session_append_file(h_, path.c_str(), anchor, junction_var, &info), "s2m_session_append_file");
        cloudKeyPoses6D.resize((size_t)info.first_key + (size_t)info.blob.n_keys, PointTypePose{});
        refreshAppendedPoses(info.first_key, info.blob.n_keys < info.blob.n_variables ? info.blob.n_keys : info.blob.n_variables);
        return info;
    }
    void sessionPlace(const float move[6])
    {
        check(s2m_session_place(h_, move), "s2m_session_place");
        int32_t first = -1, count = 0, nv = 0;
        check(s2m_session_appended(h_, &first, &count), "s2m_session_appended");
        check(s2m_pg_size(h_, &nv, nullptr), "s2m_pg_size");
        refreshAppendedPoses(first, nv - first < count ? nv - first : count);
    }
    // relocalizeScan for a stored key, against keys [first, first + count) only; does not touch transformTobeMapped
    bool relocalizeKey(int key, int first, int count)
    {
        s2m_reloc_params p;
        s2m_reloc_default_params(&p);
        p.query.top_k = relocTopK;
        p.query.first = first; p.query.count = count;
        p.loop = loopParams();
        lastReloc.assign(S2M_LOOP_MAX_CANDIDATES, s2m_reloc_candidate{});
        int32_t n = 0, best = -1;
        check(s2m_relocalize_key(h_, key, &p, lastReloc.data(), &n, &best), "s2m_relocalize_key");
        lastReloc.resize((size_t)n);
        lastRelocBest = best;
        return best >= 0;
    }
    // the anchor most of the pairs (a pose in the session's frame, the same pose in the map's frame) agree on; returns its supporters
    static int anchorFromPairs(const std::vector<float>& pose_in_session, const std::vector<float>& pose_in_map, float anchor[6],
                               double tol_m = 1.0, double tol_rad = 0.1)
    {
        int32_t n = 0;
        if (s2m_session_anchor_from_pairs(pose_in_session.data(), pose_in_map.data(), (int32_t)(pose_in_session.size() / 6), tol_m, tol_rad, anchor,
                                          &n, nullptr) != S2M_OK) return 0;
        return n;
    }
    // The first half of the merge workflow: append unplaced, relocalise the probe keys of the appended
    // session against the keys held before, take the anchor most accepted probes agree on and place the session by it. Returns
    // the supporters (0: no probe was accepted, the session stays as stored). The probes need pose-graph variables in the file.
    int mergeSession(const std::string& path, const std::vector<int>& probe_keys, double tol_m = 1.0, double tol_rad = 0.1)
    {
        const s2m_session_append_info info = sessionAppend(path);
        std::vector<float> in_session, in_map;
        for (int k : probe_keys) {
            if (k < 0 || k >= info.blob.n_variables || !relocalizeKey(info.first_key + k, 0, info.first_key)) continue;
            float v[6];
            check(s2m_pg_get_poses(h_, info.first_key + k, 1, v), "s2m_pg_get_poses");
            in_session.insert(in_session.end(), v, v + 6);
            const float* q = lastReloc[(size_t)lastRelocBest].pose_xyzrpy;
            in_map.insert(in_map.end(), q, q + 6);
        }
        if (in_session.empty()) return 0;
        float anchor[6];
        const int n = anchorFromPairs(in_session, in_map, anchor, tol_m, tol_rad);
        if (n > 0) sessionPlace(anchor);
        return n;
    }

    // true: a verification is pending (false: lastVerify is final)
    bool loopVerifyLaunch(int key_cur, const std::vector<int32_t>& key_pre, int base_key = -1)
    {
        const s2m_loop_params p = loopParams();
        lastVerify.assign(S2M_LOOP_MAX_CANDIDATES, s2m_loop_result{});
        int32_t best = -1;
        check(s2m_loop_verify_launch(h_, key_cur, key_pre.data(), (int32_t)key_pre.size(), base_key, &p, lastVerify.data(), &best),
              "s2m_loop_verify_launch");
        lastVerify.resize(key_pre.size());
        lastBest = best;
        return verifyPending();
    }
    bool verifyPending() const
    {
        for (const s2m_loop_result& r : lastVerify) if (r.status == S2M_LOOP_PENDING) return true;
        return false;
    }
    // never waits for the device; true once the verification has ended with an accepted candidate
    bool loopVerifyPoll() { return verifyFetch(false); }
    // waits for the pending verification; true if a candidate was accepted
    bool loopVerifyCollect() { return verifyFetch(true); }

    // performSCLoopClosure() on the place query: the top_k hits of s2m_sc_query_key for the newest key (ordered by descriptor
    // distance) verified in lockstep, SC form; the verification re-ranks them by fitness. true: lastVerify[lastBest] is the closure.
    bool performSCLoopClosureVerified(int top_k)
    {
        lastVerify.clear();
        lastBest = -1;
        if (cloudKeyPoses6D.empty()) return false;
        const int key_cur = (int)cloudKeyPoses6D.size() - 1;
        s2m_sc_query_params q;
        s2m_sc_query_default_params(&q);
        q.top_k = top_k;
        s2m_sc_hit hits[S2M_SC_QUERY_MAX_K];
        int32_t n_hits = 0;
        check(s2m_sc_query_key(h_, key_cur, &q, hits, &n_hits), "s2m_sc_query_key");
        std::vector<int32_t> cand;
        for (int32_t i = 0; i < n_hits && (int)cand.size() < S2M_LOOP_MAX_CANDIDATES; i++)
            if (hits[i].key != key_cur) cand.push_back(hits[i].key);
        if (cand.empty()) return false;
        return loopVerify(key_cur, cand, 0);
    }

    // The place query for many queries at once (s2m_sc_query_keys / _descriptors): row i holds the hits of query i, each row what
    // s2m_sc_query_key / _descriptor returns for the same searched set. p.rel_lo / rel_hi leave out a window around each key.
    std::vector<std::vector<s2m_sc_hit>> scQueryKeys(const std::vector<int32_t>& keys, const s2m_sc_query_many_params& p)
    {
        std::vector<s2m_sc_hit> hits(keys.size() * (size_t)(p.q.top_k > 0 ? p.q.top_k : 0));
        std::vector<int32_t> n(keys.size(), 0);
        check(s2m_sc_query_keys(h_, keys.data(), (int32_t)keys.size(), &p, hits.data(), n.data()), "s2m_sc_query_keys");
        return split_rows(hits, n, p.q.top_k);
    }
    // descs: m x 1200 doubles, row-major as s2m_sc_add_descriptor takes them
    std::vector<std::vector<s2m_sc_hit>> scQueryDescriptors(const std::vector<double>& descs, const s2m_sc_query_many_params& p)
    {
        const size_t m = descs.size() / (S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR);
        std::vector<s2m_sc_hit> hits(m * (size_t)(p.q.top_k > 0 ? p.q.top_k : 0));
        std::vector<int32_t> n(m, 0);
        check(s2m_sc_query_descriptors(h_, descs.data(), (int32_t)m, &p, hits.data(), n.data()), "s2m_sc_query_descriptors");
        return split_rows(hits, n, p.q.top_k);
    }
    // The place query behind a ring-key prefilter (s2m_sc_query_keys_ring / s2m_sc_ring_neighbours_keys):
    // scQueryKeys with every query's searched set cut to its p.n_candidates ring-key neighbours; and those neighbours themselves.
    std::vector<std::vector<s2m_sc_hit>> scQueryKeysRing(const std::vector<int32_t>& keys, const s2m_sc_ring_params& p)
    {
        std::vector<s2m_sc_hit> hits(keys.size() * (size_t)(p.m.q.top_k > 0 ? p.m.q.top_k : 0));
        std::vector<int32_t> n(keys.size(), 0);
        check(s2m_sc_query_keys_ring(h_, keys.data(), (int32_t)keys.size(), &p, hits.data(), n.data()), "s2m_sc_query_keys_ring");
        return split_rows(hits, n, p.m.q.top_k);
    }
    std::vector<std::vector<s2m_sc_hit>> scQueryDescriptorsRing(const std::vector<double>& descs, const s2m_sc_ring_params& p)
    {
        const size_t m = descs.size() / (S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR);
        std::vector<s2m_sc_hit> hits(m * (size_t)(p.m.q.top_k > 0 ? p.m.q.top_k : 0));
        std::vector<int32_t> n(m, 0);
        check(s2m_sc_query_descriptors_ring(h_, descs.data(), (int32_t)m, &p, hits.data(), n.data()), "s2m_sc_query_descriptors_ring");
        return split_rows(hits, n, p.m.q.top_k);
    }
    std::vector<std::vector<s2m_sc_ring_neighbour>> scRingNeighboursKeys(const std::vector<int32_t>& keys, const s2m_sc_ring_params& p)
    {
        const size_t c = (size_t)(p.n_candidates > 0 ? p.n_candidates : 0);
        std::vector<s2m_sc_ring_neighbour> nb(keys.size() * c);
        std::vector<int32_t> n(keys.size(), 0);
        check(s2m_sc_ring_neighbours_keys(h_, keys.data(), (int32_t)keys.size(), &p, nb.data(), n.data()), "s2m_sc_ring_neighbours_keys");
        return split_rows(nb, n, c);
    }
    // the stored descriptors first .. first+count-1, bit for bit what was added
    std::vector<double> scGetDescriptors(int32_t first, int32_t count)
    {
        std::vector<double> descs((size_t)(count > 0 ? count : 0) * S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR);
        check(s2m_sc_get_descriptors(h_, first, count, descs.data()), "s2m_sc_get_descriptors");
        return descs;
    }
    // Loop discovery over a whole session (after a load, say): every stored key against the keys at least `gap` before it. The
    // candidates come in key_cur order, per key by (dist, key_pre); a node hands each key_cur's to loopVerify.
    struct SessionLoop { int32_t key_cur, key_pre; double dist; float yaw; };
    // ring_candidates > 0: every key against its ring_candidates ring-key neighbours among them only (scQueryKeysRing).
    std::vector<SessionLoop> findSessionLoops(int gap, double max_dist, int top_k, int align, int ring_candidates = 0)
    {
        s2m_sc_ring_params rp;
        s2m_sc_ring_default_params(&rp);
        s2m_sc_query_many_params& p = rp.m;
        p.q.top_k = top_k; p.q.align = align; p.q.max_dist = max_dist;
        p.rel_lo = 1 - gap; p.rel_hi = INT32_MAX;
        rp.n_candidates = ring_candidates;
        const int n_keys = s2m_sc_size(h_);
        std::vector<int32_t> keys((size_t)(n_keys > 0 ? n_keys : 0));
        for (size_t k = 0; k < keys.size(); k++) keys[k] = (int32_t)k;
        std::vector<SessionLoop> out;
        const std::vector<std::vector<s2m_sc_hit>> rows = ring_candidates > 0 ? scQueryKeysRing(keys, rp) : scQueryKeys(keys, p);
        for (size_t k = 0; k < rows.size(); k++)
            for (const s2m_sc_hit& hit : rows[k]) out.push_back(SessionLoop{ (int32_t)k, hit.key, hit.dist, hit.yaw_diff_rad });
        return out;
    }

    // s2m_loop_verify_many: the candidate rows of many keys verified in one call, row r what loopVerify(rows[r].key_cur,
    // rows[r].key_pre, base_key) gives in turn (records, best, the container). A row without candidates gives no records and -1.
    struct VerifyRow { int32_t key_cur; std::vector<int32_t> key_pre; };
    struct VerifiedRow { std::vector<s2m_loop_result> records; int32_t best; };
    std::vector<VerifiedRow> loopVerifyMany(const std::vector<VerifyRow>& rows, int base_key = -1)
    {
        const s2m_loop_params p = loopParams();
        size_t stride = 1;
        for (const VerifyRow& r : rows) stride = std::max(stride, r.key_pre.size());
        std::vector<int32_t> key_cur(rows.size()), n_cand(rows.size()), best(rows.size(), -1), key_pre(rows.size() * stride, 0);
        for (size_t r = 0; r < rows.size(); r++) {
            key_cur[r] = rows[r].key_cur;
            n_cand[r] = (int32_t)rows[r].key_pre.size();
            std::copy(rows[r].key_pre.begin(), rows[r].key_pre.end(), key_pre.begin() + r * stride);
        }
        std::vector<s2m_loop_result> recs(rows.size() * stride, s2m_loop_result{});
        check(s2m_loop_verify_many(h_, key_cur.data(), key_pre.data(), n_cand.data(), (int32_t)rows.size(), (int32_t)stride, base_key, &p,
                                   recs.data(), best.data()), "s2m_loop_verify_many");
        std::vector<VerifiedRow> out(rows.size());
        for (size_t r = 0; r < rows.size(); r++) {
            out[r].records.assign(recs.begin() + r * stride, recs.begin() + r * stride + n_cand[r]);
            out[r].best = best[r];
        }
        return out;
    }
    // findSessionLoops' query followed by loopVerifyMany in chunks of rows_per_call rows: the winning records, one per key that has
    // an accepted candidate, in key_cur order. between_chunks (may be empty) is called after every chunk: a node releases the scan
    // handler's lock there and takes it again, so the lock is held for rows_per_call rows at a time.
    std::vector<s2m_loop_result> verifySessionLoops(int gap, double max_dist, int top_k, int align, int base_key, int rows_per_call,
                                                    const std::function<void()>& between_chunks = {}, int ring_candidates = 0)
    {
        std::vector<VerifyRow> rows;
        for (const SessionLoop& c : findSessionLoops(gap, max_dist, std::min(top_k, (int)S2M_LOOP_MAX_CANDIDATES), align, ring_candidates)) {
            if (rows.empty() || rows.back().key_cur != c.key_cur) rows.push_back(VerifyRow{ c.key_cur, {} });
            rows.back().key_pre.push_back(c.key_pre);
        }
        std::vector<s2m_loop_result> won;
        const size_t step = (size_t)std::max(rows_per_call, 1);
        for (size_t i = 0; i < rows.size(); i += step) {
            const std::vector<VerifyRow> chunk(rows.begin() + i, rows.begin() + std::min(rows.size(), i + step));
            for (const VerifiedRow& v : loopVerifyMany(chunk, base_key))
                if (v.best >= 0) won.push_back(v.records[(size_t)v.best]);
            if (between_chunks) between_chunks();
        }
        return won;
    }

    // Loop candidates by position for many keys (s2m_loop_detect_keys): detectLoopClosureDistance() for
    // every key of `keys` against the searched set of p, row i as a VerifyRow - what loopVerifyMany(rows, -1) takes - with the
    // fp32 squared distances alike in d2 (may be null). time_cur: empty (a query's time is its key's) or one time per key.
    std::vector<VerifyRow> loopDetectKeys(const std::vector<int32_t>& keys, const std::vector<double>& time_cur, const s2m_loop_detect_params& p,
                                          std::vector<std::vector<float>>* d2 = nullptr)
    {
        if (!time_cur.empty() && time_cur.size() != keys.size()) throw std::invalid_argument("loopDetectKeys: one time per key");
        const size_t K = (size_t)(p.top_k > 0 ? p.top_k : 0);
        std::vector<int32_t> key_pre(keys.size() * K, -1), n(keys.size(), 0);
        std::vector<float> dist(keys.size() * K, 0.0f);
        check(s2m_loop_detect_keys(h_, keys.data(), time_cur.empty() ? nullptr : time_cur.data(), (int32_t)keys.size(), &p, key_pre.data(),
                                   dist.data(), n.data()), "s2m_loop_detect_keys");
        std::vector<VerifyRow> rows(keys.size());
        if (d2) d2->assign(keys.size(), {});
        for (size_t i = 0; i < keys.size(); i++) {
            rows[i].key_cur = keys[i];
            rows[i].key_pre.assign(key_pre.begin() + i * K, key_pre.begin() + i * K + n[i]);
            if (d2) (*d2)[i].assign(dist.begin() + i * K, dist.begin() + i * K + n[i]);
        }
        return rows;
    }
    // Every stored key, or `keys`, against the whole store by position: the candidates a node hands to loopVerifyMany(rows, -1),
    // in the order of the keys and per key by (d2, key_pre). Take them after a place or an optimise has made the poses
    // consistent; before the two trajectories agree, take findSessionLoops' descriptor candidates.
    struct DistanceLoop { int32_t key_cur, key_pre; float d2; };
    std::vector<int32_t> allKeys() const
    {
        const int n_keys = s2m_kf_size(h_);
        std::vector<int32_t> keys((size_t)(n_keys > 0 ? n_keys : 0));
        for (size_t k = 0; k < keys.size(); k++) keys[k] = (int32_t)k;
        return keys;
    }
    s2m_loop_detect_params loopDetectParams(float radius, float time_diff, int top_k) const
    {
        s2m_loop_detect_params p;
        s2m_loop_detect_default_params(&p);
        p.search_radius = radius; p.time_diff_s = time_diff; p.top_k = top_k;
        return p;
    }
    std::vector<DistanceLoop> findSessionLoopsByDistance(float radius, float time_diff, int top_k, const std::vector<int32_t>* keys = nullptr)
    {
        std::vector<std::vector<float>> d2;
        const std::vector<VerifyRow> rows = loopDetectKeys(keys ? *keys : allKeys(), {}, loopDetectParams(radius, time_diff, top_k), &d2);
        std::vector<DistanceLoop> out;
        for (size_t r = 0; r < rows.size(); r++)
            for (size_t i = 0; i < rows[r].key_pre.size(); i++) out.push_back(DistanceLoop{ rows[r].key_cur, rows[r].key_pre[i], d2[r][i] });
        return out;
    }
    // findSessionLoopsByDistance's query followed by loopVerifyMany in chunks of rows_per_call rows, as verifySessionLoops: the
    // winning records, one per key that has an accepted candidate. `keys` must be distinct.
    std::vector<s2m_loop_result> verifySessionLoopsByDistance(float radius, float time_diff, int top_k, const std::vector<int32_t>* keys,
                                                              int base_key, int rows_per_call, const std::function<void()>& between_chunks = {})
    {
        std::vector<VerifyRow> rows;
        for (VerifyRow& r : loopDetectKeys(keys ? *keys : allKeys(), {}, loopDetectParams(radius, time_diff, std::min(top_k, (int)S2M_LOOP_MAX_CANDIDATES))))
            if (!r.key_pre.empty()) rows.push_back(std::move(r));
        std::vector<s2m_loop_result> won;
        const size_t step = (size_t)std::max(rows_per_call, 1);
        for (size_t i = 0; i < rows.size(); i += step) {
            const std::vector<VerifyRow> chunk(rows.begin() + i, rows.begin() + std::min(rows.size(), i + step));
            for (const VerifiedRow& v : loopVerifyMany(chunk, base_key))
                if (v.best >= 0) won.push_back(v.records[(size_t)v.best]);
            if (between_chunks) between_chunks();
        }
        return won;
    }

    // The mutually consistent loops among many candidates (s2m_pg_consistent_loops), between the
    // verification and the graph: candidates as s2m_pg_add_between would take them against the graph's current estimates;
    // keep[i] != 0 for the ones kept. The set is the library's stated greedy rule, not the maximum clique; the default
    // tolerances have not been measured on real data. Nothing is added to the graph. lastConsistency holds the counts.
    s2m_pg_consistency_result lastConsistency{};
    std::vector<uint8_t> pgConsistentLoops(const std::vector<int32_t>& key_from, const std::vector<int32_t>& key_to, const std::vector<float>& rel_xyzrpy,
                                           const s2m_pg_consistency_params* params = nullptr, std::vector<int32_t>* degree = nullptr)
    {
        const size_t m = key_from.size();
        if (key_to.size() != m || rel_xyzrpy.size() != 6 * m) throw std::runtime_error("pgConsistentLoops: one key pair and six floats per candidate");
        std::vector<uint8_t> keep(m, 0);
        if (degree) degree->assign(m, 0);
        check(s2m_pg_consistent_loops(h_, key_from.data(), key_to.data(), rel_xyzrpy.data(), (int32_t)m, params, keep.data(),
                                      degree ? degree->data() : nullptr, nullptr, &lastConsistency), "s2m_pg_consistent_loops");
        return keep;
    }
    // poseFrom.between(poseTo) of two {x, y, z, roll, pitch, yaw} poses (Rot3::RzRyRx) in fp64, as a float pose vector: what
    // addLoopFactor hands to s2m_pg_add_between for an accepted s2m_loop_result
    static void betweenXyzrpy(const float from[6], const float to[6], float rel[6])
    {
        auto mat = [](const float p[6], double R[9]) {
            const double cr = std::cos((double)p[3]), sr = std::sin((double)p[3]), cp = std::cos((double)p[4]), sp = std::sin((double)p[4]);
            const double cy = std::cos((double)p[5]), sy = std::sin((double)p[5]);
            R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = sy * sr + cy * sp * cr;
            R[3] = sy * cp; R[4] = cy * cr + sy * sp * sr; R[5] = sy * sp * cr - cy * sr;
            R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
        };
        double A[9], B[9], R[9], t[3];
        mat(from, A);
        mat(to, B);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) R[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
            t[i] = A[i] * ((double)to[0] - from[0]) + A[3 + i] * ((double)to[1] - from[1]) + A[6 + i] * ((double)to[2] - from[2]);
        }
        rel[0] = (float)t[0]; rel[1] = (float)t[1]; rel[2] = (float)t[2];
        rel[3] = (float)std::atan2(R[7], R[8]);
        rel[4] = (float)std::asin(std::min(1.0, std::max(-1.0, -R[6])));
        rel[5] = (float)std::atan2(R[3], R[0]);
    }
    // The records of verifySessionLoops / verifySessionLoopsByDistance that pgConsistentLoops keeps, in their order: record r is
    // the candidate (key_cur, key_pre, pose_from.between(pose_to)). Pass the kept ones on to the graph.
    std::vector<s2m_loop_result> selectConsistentLoops(const std::vector<s2m_loop_result>& records, const s2m_pg_consistency_params* params = nullptr)
    {
        std::vector<int32_t> from, to;
        std::vector<float> rel(6 * records.size());
        for (size_t r = 0; r < records.size(); r++) {
            from.push_back(records[r].key_cur);
            to.push_back(records[r].key_pre);
            betweenXyzrpy(records[r].pose_from, records[r].pose_to, rel.data() + 6 * r);
        }
        std::vector<s2m_loop_result> kept;
        if (records.empty()) return kept;
        const std::vector<uint8_t> keep = pgConsistentLoops(from, to, rel, params);
        for (size_t r = 0; r < records.size(); r++)
            if (keep[r]) kept.push_back(records[r]);
        return kept;
    }

    // void performSCLoopClosure() (:624-730): the ScanContext detector on this handle, then the store's extraction and ICP
    inline bool performSCLoopClosure(SCManagerS2M& scManager);

    // loopFindNearKeyframes(nearKeyframes, key, searchNum, loop_index) (:821-844), filtered with downSizeFilterICP
    void loopFindNearKeyframes(std::vector<PointXYZI>& nearKeyframes, int key, int searchNum, int loop_index)
    {
        size_t n = 0;
        int rc = s2m_loop_near_keyframes(h_, key, searchNum, loop_index, loopClosureICPSurfLeafSize, nullptr, sizeof(PointXYZI), 0, &n);
        if (rc != S2M_ERR_CAPACITY) checkVoxel(rc, "s2m_loop_near_keyframes");
        nearKeyframes.resize(n);
        if (n > 0)
            checkVoxel(s2m_loop_near_keyframes(h_, key, searchNum, loop_index, loopClosureICPSurfLeafSize, nearKeyframes.data(),
                                               sizeof(PointXYZI), n, &n), "s2m_loop_near_keyframes");
    }

    s2m_handle handle() const { return h_; }

private:
    // row i: the first counts[i] of the `width` records the flat block holds for it
    template <typename T>
    static std::vector<std::vector<T>> split_rows(const std::vector<T>& flat, const std::vector<int32_t>& counts, size_t width)
    {
        std::vector<std::vector<T>> rows(counts.size());
        for (size_t i = 0; i < counts.size(); i++) rows[i].assign(flat.begin() + i * width, flat.begin() + i * width + counts[i]);
        return rows;
    }
    bool accepted()
    {
        if (lastLoop.status != S2M_LOOP_ACCEPTED) return false;
        loopIndexContainer.emplace_back(lastLoop.key_cur, lastLoop.key_pre);
        return true;
    }
    bool verifyAccepted()
    {
        if (lastBest < 0) return false;
        loopIndexContainer.emplace_back(lastVerify[(size_t)lastBest].key_cur, lastVerify[(size_t)lastBest].key_pre);
        return true;
    }
    bool verifyFetch(bool wait)
    {
        lastVerify.assign(S2M_LOOP_MAX_CANDIDATES, s2m_loop_result{});
        int32_t n = 0, best = -1;
        check(wait ? s2m_loop_verify_collect(h_, lastVerify.data(), S2M_LOOP_MAX_CANDIDATES, &n, &best)
                   : s2m_loop_verify_poll(h_, lastVerify.data(), S2M_LOOP_MAX_CANDIDATES, &n, &best),
              wait ? "s2m_loop_verify_collect" : "s2m_loop_verify_poll");
        lastVerify.resize((size_t)n);
        lastBest = best;
        return verifyAccepted();
    }

    void check(int rc, const char* what)
    {
        if (rc != S2M_OK) throw std::runtime_error(std::string(what) + ": " + s2m_last_error(h_));
    }
    int pgCode(int rc, const char* what, const s2m_pg_result* r)
    {
        if (rc != S2M_PG_PENDING && rc != S2M_PG_IDLE) check(rc, what);
        if (rc == S2M_OK) lastGraphResult = *r;
        return rc;
    }
    // cloudKeyPoses6D[first .. first+n) from the pose graph's estimates (an appended session's keys, after an append or a place)
    void refreshAppendedPoses(int32_t first, int32_t n)
    {
        if (first < 0 || n <= 0) return;
        std::vector<float> v(6 * (size_t)n);
        check(s2m_pg_get_poses(h_, first, n, v.data()), "s2m_pg_get_poses");
        for (int32_t k = 0; k < n; k++) {
            PointTypePose& q = cloudKeyPoses6D[(size_t)(first + k)];
            q.intensity = (float)(first + k);
            q.x = v[6 * k]; q.y = v[6 * k + 1]; q.z = v[6 * k + 2]; q.roll = v[6 * k + 3]; q.pitch = v[6 * k + 4]; q.yaw = v[6 * k + 5];
        }
    }
    // S2M_WARN_LEAF_TOO_SMALL is PCL's PCL_WARN case (output = input): not an error
    void checkVoxel(int rc, const char* what) { if (rc != S2M_WARN_LEAF_TOO_SMALL) check(rc, what); }
    s2m_handle h_ = nullptr;
    bool scanResident_ = false;
    s2m_guess_state guessState_{};                    // lastImuTransformation, lastImuPreTransformation, lastImuPreTransAvailable (:904, :920-921)
};

// SCManager (reference include/Scancontext.h:56-113) on top of the same handle: the descriptor store and the
// loop detector live on the device; method names and return values are the reference's.
class SCManagerS2M {
public:
    explicit SCManagerS2M(s2m_handle h) : h_(h) {}
    // void makeAndSaveScancontextAndKeys(pcl::PointCloud<SCPointType>& _scan_down) (Scancontext.cpp:236-250)
    void makeAndSaveScancontextAndKeys(const std::vector<PointXYZI>& scan_down)
    {
        check(s2m_sc_add_scan(h_, scan_down.data(), scan_down.size(), sizeof(PointXYZI)), "s2m_sc_add_scan");
    }
    // makeAndSaveScancontextAndKeys(cloud_deskewed) at key-frame save (src/mapOptmization.cpp:1591-1594) from the resident cloud
    void makeAndSaveScancontextAndKeysProjected() { check(s2m_sc_add_projected(h_), "s2m_sc_add_projected"); }
    // std::pair<int, float> detectLoopClosureID(void) (Scancontext.cpp:253-344): {loop_id or -1, yaw_diff_rad}
    std::pair<int, float> detectLoopClosureID()
    {
        int32_t id = -1; float yaw = 0.0f;
        check(s2m_sc_detect_loop(h_, &id, &yaw, &lastMatch), "s2m_sc_detect_loop");
        return { (int)id, yaw };
    }
    int size() const { return s2m_sc_size(h_); }
    s2m_sc_match lastMatch{};

private:
    void check(int rc, const char* what)
    {
        if (rc != S2M_OK) throw std::runtime_error(std::string(what) + ": " + s2m_last_error(h_));
    }
    s2m_handle h_;
};

inline bool MapOptimizationS2M::performSCLoopClosure(SCManagerS2M& scManager)
{
    lastLoop = s2m_loop_result{};
    lastLoop.key_cur = lastLoop.key_pre = -1;
    if (cloudKeyPoses6D.empty()) return false;                       // (:626-627)
    const int loopKeyPre = scManager.detectLoopClosureID().first;    // (:636-639)
    if (loopKeyPre == -1) return false;
    const s2m_loop_params p = loopParams();
    check(s2m_loop_align(h_, (int)cloudKeyPoses6D.size() - 1, loopKeyPre, 0, &p, &lastLoop), "s2m_loop_align");
    return accepted();
}

}  // namespace liorf_amd
