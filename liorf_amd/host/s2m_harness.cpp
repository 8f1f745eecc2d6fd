// s2m_harness.cpp — ROS-free C++ harness of the drop-in boundary: reads a map and a scan as raw
// PointXYZI records (32-byte stride, the reference's wire layout) and an initial guess, runs
// scan2MapOptimization() through the host mirror, prints the result.  Fails loudly without a GPU.
//
//   s2m_harness map.bin scan.bin roll pitch yaw x y z [imuType imuRPYWeight z_tollerance rotation_tollerance imuAvailable imuRollInit imuPitchInit]
//       the optional tail sets the ParamServer members AFTER the node is constructed (as the reference's yaml
//       loading does) and the cloud_info IMU fields transformUpdate() reads (:1325-1350)
//   s2m_harness --chain frames.bin frames.txt raw_scan.bin map_leaf scan_leaf roll pitch yaw x y z
//       the handler's three steps in order: extractCloud() over the key frames listed in frames.txt (one line
//       "n_points x y z roll pitch yaw" per frame, clouds back to back in frames.bin), downsampleCurrentScan(),
//       scan2MapOptimization().
//   s2m_harness --keyframes scans.bin scans.txt map_leaf scan_leaf density
//       a scripted trajectory through extractSurroundingKeyFrames() -> downsampleCurrentScan() ->
//       scan2MapOptimization() -> saveKeyFrame() on the resident key-frame store; prints every pose.
//   s2m_harness --loop keys.bin keys.txt scan_leaf search_radius search_num icp_leaf fitness_score [--async]
//       a scripted revisit through downsampleCurrentScan() -> saveKeyFrame() -> makeAndSaveScancontextAndKeys() ->
//       performRSLoopClosure() -> performSCLoopClosure() on the resident key-frame store; prints every loop result.
//   s2m_harness --global-map keys.bin keys.txt scan_leaf search_radius pose_density leaf out.bin
//       the key frames through downsampleCurrentScan() -> saveKeyFrame(), then publishGlobalMap() (globalMapKeyFramesDS written
//       to out.bin) and saveMapService()'s unfiltered cloud; prints the key list and both sizes.
//   s2m_harness --pose-graph keys.bin keys.txt scan_leaf loops.txt out.bin [--async]
//       the pose graph beside the store: every key through downsampleCurrentScan() -> saveKeyFramesAndFactor() (with the loop
//       factors loops.txt queues for it) -> correctPosesFromGraph(); prints every update, the graph's estimates and the
//       size of the unfiltered map cloud, which goes to out.bin.
//   s2m_harness --project raw.bin sensor stamp imu.bin n_scan downsample_rate point_filter_num scan_leaf out.bin ds.bin
//       the front end: cachePointCloud() of the raw records (sensor 0..4), imuDeskewInfo() over the samples of imu.bin
//       ({time, wx, wy, wz} doubles), projectPointCloud(), downsampleCurrentScanProjected(), the ScanContext add from the
//       resident cloud; fullCloud goes to out.bin, laserCloudSurfLastDS to ds.bin; prints the counts.
//   s2m_harness --front-end raw.bin sensor stamp imu.bin odom.bin n_scan downsample_rate point_filter_num scan_leaf positional imu_rate out.bin
//       the whole front end of one scan: cachePointCloud(), imuDeskewInfo(), odomDeskewInfo() over the samples of odom.bin ({time, px, py, pz, qx,
//       qy, qz, qw, cov0} doubles), projectPointCloud() with positional deskew when `positional` is 1,
//       downsampleCurrentScanProjected(), updateInitialGuess() three times (no key poses; first odometry sample; odometry
//       increment of a queue shifted by its own increment); fullCloud goes to out.bin; prints the guess, the counts and a checksum.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "map_optimization_s2m.hpp"
#include "image_projection_s2m.hpp"

static std::vector<liorf_amd::PointXYZI> read_cloud(const char* path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const std::streamsize n = f.tellg();
    f.seekg(0);
    std::vector<liorf_amd::PointXYZI> pts((size_t)n / sizeof(liorf_amd::PointXYZI));
    f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * sizeof(liorf_amd::PointXYZI)));
    return pts;
}

static void print_result(const liorf_amd::MapOptimizationS2M& node)
{
    const s2m_result& r = node.lastResult;
    std::printf("skipped %d iters %d converged %d degenerate %d n_sel %d\n", r.skipped, r.iters_run, r.converged, r.is_degenerate, r.n_sel_last);
    std::printf("transformTobeMapped %.9g %.9g %.9g %.9g %.9g %.9g\n", node.transformTobeMapped[0], node.transformTobeMapped[1],
                node.transformTobeMapped[2], node.transformTobeMapped[3], node.transformTobeMapped[4], node.transformTobeMapped[5]);
    std::printf("incrementalOdometryAffineBack");
    for (int k = 0; k < 12; k++) std::printf(" %.9g", node.incrementalOdometryAffineBack[k]);
    std::printf("\n");
}

static int run_chain(char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    const std::vector<liorf_amd::PointXYZI> all = read_cloud(argv[2]);
    std::ifstream tab(argv[3]);
    if (!tab) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    size_t n, at = 0;
    liorf_amd::PointTypePose p;
    std::vector<int> keyInds;
    while (tab >> n >> p.x >> p.y >> p.z >> p.roll >> p.pitch >> p.yaw) {
        if (at + n > all.size()) throw std::runtime_error("frames.txt asks for more points than frames.bin holds");
        p.intensity = (float)node.cloudKeyPoses6D.size();
        keyInds.push_back((int)node.cloudKeyPoses6D.size());
        node.cloudKeyPoses6D.push_back(p);
        node.surfCloudKeyFrames.emplace_back(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
    }
    node.laserCloudSurfLast = read_cloud(argv[4]);
    node.surroundingKeyframeMapLeafSize = (float)std::atof(argv[5]);
    node.mappingSurfLeafSize = (float)std::atof(argv[6]);
    for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = (float)std::atof(argv[7 + k]);
    node.extractCloud(keyInds);
    node.downsampleCurrentScan();
    node.scan2MapOptimization();
    std::printf("laserCloudSurfFromMapDSNum %d laserCloudSurfLastDSNum %d\n", node.laserCloudSurfFromMapDSNum, node.laserCloudSurfLastDSNum);
    print_result(node);
    return 0;
}

// --keyframes scans.bin scans.txt map_leaf scan_leaf density: a scripted trajectory through the handler with the resident
// key-frame store. scans.txt holds one line "n_points time roll pitch yaw x y z" per scan (the guess), the raw scans back to back
// in scans.bin; every scan runs extractSurroundingKeyFrames() -> downsampleCurrentScan() -> scan2MapOptimization() ->
// saveKeyFrame() and prints "pose <i> roll pitch yaw x y z".
static int run_keyframes(char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    const std::vector<liorf_amd::PointXYZI> all = read_cloud(argv[2]);
    std::ifstream tab(argv[3]);
    if (!tab) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    node.surroundingKeyframeMapLeafSize = (float)std::atof(argv[4]);
    node.mappingSurfLeafSize = (float)std::atof(argv[5]);
    node.surroundingKeyframeDensity = (float)std::atof(argv[6]);
    size_t n, at = 0;
    double t;
    float g[6];
    for (int i = 0; tab >> n >> t >> g[0] >> g[1] >> g[2] >> g[3] >> g[4] >> g[5]; i++) {
        if (at + n > all.size()) throw std::runtime_error("scans.txt asks for more points than scans.bin holds");
        node.timeLaserInfoCur = t;
        node.extractSurroundingKeyFrames();
        node.laserCloudSurfLast.assign(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
        node.downsampleCurrentScan();
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = g[k];
        node.scan2MapOptimization();
        node.saveKeyFrame();
        const float* p = node.transformTobeMapped;
        std::printf("pose %d %.9g %.9g %.9g %.9g %.9g %.9g\n", i, p[0], p[1], p[2], p[3], p[4], p[5]);
    }
    return 0;
}

static void print_loop(const char* what, int i, const s2m_loop_result& r)
{
    std::printf("%s %d status %d keys %d %d n %d %d iters %d converged %d fitness %.17g pose_from", what, i, r.status, r.key_cur,
                r.key_pre, r.n_cur, r.n_prev, r.icp.iterations, r.icp.converged, r.icp.fitness_score);
    for (int k = 0; k < 6; k++) std::printf(" %.9g", r.pose_from[k]);
    std::printf(" pose_to");
    for (int k = 0; k < 6; k++) std::printf(" %.9g", r.pose_to[k]);
    std::printf("\n");
}

// --loop keys.bin keys.txt scan_leaf search_radius search_num icp_leaf fitness_score: keys.txt holds one line
// "n_points time x y z roll pitch yaw" per key frame, the raw clouds back to back in keys.bin. Every key runs
// downsampleCurrentScan() -> saveKeyFrame() -> makeAndSaveScancontextAndKeys() at its pose, then performRSLoopClosure() at its
// time and performSCLoopClosure(); prints "rs <i> ..." and "sc <i> ..." for every key, then "near <n>" for
// loopFindNearKeyframes(last key, search_num, -1). --async: the RS closure is launched (performRSLoopClosureLaunch) and polled,
// the scan downsampled again between two polls as the scan handler would go on working; the lines printed are the same.
static int run_loop(char** argv, bool async)
{
    liorf_amd::MapOptimizationS2M node;
    liorf_amd::SCManagerS2M sc(node.handle());
    const std::vector<liorf_amd::PointXYZI> all = read_cloud(argv[2]);
    std::ifstream tab(argv[3]);
    if (!tab) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    node.mappingSurfLeafSize = (float)std::atof(argv[4]);
    node.historyKeyframeSearchRadius = (float)std::atof(argv[5]);
    node.historyKeyframeSearchNum = std::atoi(argv[6]);
    node.loopClosureICPSurfLeafSize = (float)std::atof(argv[7]);
    node.historyKeyframeFitnessScore = (float)std::atof(argv[8]);
    size_t n, at = 0;
    double t;
    float p[6];
    int i = 0;
    for (; tab >> n >> t >> p[0] >> p[1] >> p[2] >> p[3] >> p[4] >> p[5]; i++) {
        if (at + n > all.size()) throw std::runtime_error("keys.txt asks for more points than keys.bin holds");
        node.timeLaserInfoCur = t;
        node.laserCloudSurfLast.assign(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
        node.downsampleCurrentScan();
        const float rpyxyz[6] = { p[3], p[4], p[5], p[0], p[1], p[2] };
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = rpyxyz[k];
        node.saveKeyFrame();
        sc.makeAndSaveScancontextAndKeys(node.laserCloudSurfLastDS);
        if (async) {
            long polls = 0;
            for (bool pending = node.performRSLoopClosureLaunch(); pending; pending = node.loopPending(), polls++) {
                node.downsampleCurrentScan();
                node.loopPoll();
            }
            std::fprintf(stderr, "rs %d polls %ld\n", i, polls);
        } else {
            node.performRSLoopClosure();
        }
        print_loop("rs", i, node.lastLoop);
        node.performSCLoopClosure(sc);
        print_loop("sc", i, node.lastLoop);
    }
    std::vector<liorf_amd::PointXYZI> near;
    if (i > 0) node.loopFindNearKeyframes(near, i - 1, node.historyKeyframeSearchNum, -1);
    std::printf("near %zu\n", near.size());
    if (i > 0) {
        // the position candidates of the last key and their verification (loopDetectKeys behind both); stderr: the lines above
        // are the record a caller compares
        const std::vector<int32_t> last{ (int32_t)(i - 1) };
        const size_t n_cand = node.findSessionLoopsByDistance(node.historyKeyframeSearchRadius, node.historyKeyframeSearchTimeDiff, 2, &last).size();
        const size_t n_won = node.verifySessionLoopsByDistance(node.historyKeyframeSearchRadius, node.historyKeyframeSearchTimeDiff, 2, &last, -1, 64).size();
        std::fprintf(stderr, "by distance: key %d, %zu candidates, %zu verified\n", i - 1, n_cand, n_won);
    }
    return 0;
}

// --global-map keys.bin keys.txt scan_leaf search_radius pose_density leaf out.bin: keys.txt as for --loop. Prints
// "keys <n> k0 k1 ...", "global_map <n>" (the records go to out.bin) and "map_cloud <n>" (globalSurfCloud of all keys).
static int run_global_map(char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    const std::vector<liorf_amd::PointXYZI> all = read_cloud(argv[2]);
    std::ifstream tab(argv[3]);
    if (!tab) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    node.mappingSurfLeafSize = (float)std::atof(argv[4]);
    node.globalMapVisualizationSearchRadius = (float)std::atof(argv[5]);
    node.globalMapVisualizationPoseDensity = (float)std::atof(argv[6]);
    node.globalMapVisualizationLeafSize = (float)std::atof(argv[7]);
    size_t n, at = 0;
    double t;
    float p[6];
    while (tab >> n >> t >> p[0] >> p[1] >> p[2] >> p[3] >> p[4] >> p[5]) {
        if (at + n > all.size()) throw std::runtime_error("keys.txt asks for more points than keys.bin holds");
        node.timeLaserInfoCur = t;
        node.laserCloudSurfLast.assign(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
        node.downsampleCurrentScan();
        const float rpyxyz[6] = { p[3], p[4], p[5], p[0], p[1], p[2] };
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = rpyxyz[k];
        node.saveKeyFrame();
    }
    node.publishGlobalMap();
    std::printf("keys %zu", node.globalMapKeyInds.size());
    for (int k : node.globalMapKeyInds) std::printf(" %d", k);
    std::printf("\nglobal_map %zu\n", node.globalMapKeyFramesDS.size());
    std::ofstream o(argv[8], std::ios::binary);
    o.write(reinterpret_cast<const char*>(node.globalMapKeyFramesDS.data()),
            (std::streamsize)(node.globalMapKeyFramesDS.size() * sizeof(liorf_amd::PointXYZI)));
    if (!o) throw std::runtime_error(std::string("cannot write ") + argv[8]);
    std::vector<liorf_amd::PointXYZI> cloud;
    node.globalMapCloud(cloud, 0.0f);
    std::printf("map_cloud %zu\n", cloud.size());
    return 0;
}

static int run_project(char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    liorf_amd::SCManagerS2M sc(node.handle());
    liorf_amd::ImageProjectionS2M proj(node.handle(), std::atoi(argv[3]));
    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[2]);
    std::vector<unsigned char> raw((size_t)f.tellg());
    f.seekg(0);
    f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)raw.size());
    std::ifstream fi(argv[5], std::ios::binary | std::ios::ate);
    if (!fi) throw std::runtime_error(std::string("cannot open ") + argv[5]);
    std::vector<std::array<double, 4>> imu((size_t)fi.tellg() / 32);
    fi.seekg(0);
    fi.read(reinterpret_cast<char*>(imu.data()), (std::streamsize)(imu.size() * 32));
    proj.params.n_scan = std::atoi(argv[6]);
    proj.params.downsample_rate = std::atoi(argv[7]);
    proj.params.point_filter_num = std::atoi(argv[8]);
    node.mappingSurfLeafSize = (float)std::atof(argv[9]);
    proj.cachePointCloud(raw.data(), raw.size(), std::atof(argv[4]));
    proj.imuDeskewInfo(imu);
    proj.projectPointCloud();
    node.downsampleCurrentScanProjected(proj.fullCloudNum);
    sc.makeAndSaveScancontextAndKeysProjected();
    std::ofstream o(argv[10], std::ios::binary);
    o.write(reinterpret_cast<const char*>(proj.fullCloud.data()), (std::streamsize)(proj.fullCloud.size() * sizeof(liorf_amd::PointXYZI)));
    if (!o) throw std::runtime_error(std::string("cannot write ") + argv[10]);
    std::ofstream od(argv[11], std::ios::binary);
    od.write(reinterpret_cast<const char*>(node.laserCloudSurfLastDS.data()),
             (std::streamsize)(node.laserCloudSurfLastDS.size() * sizeof(liorf_amd::PointXYZI)));
    if (!od) throw std::runtime_error(std::string("cannot write ") + argv[11]);
    std::printf("timeScanEnd %.17g imuPointerCur %d imuAvailable %d\n", proj.timeScanEnd, proj.imuPointerCur, proj.imuAvailable ? 1 : 0);
    std::printf("fullCloud %zu laserCloudSurfLastDSNum %d sc_size %d\n", proj.fullCloud.size(), node.laserCloudSurfLastDSNum, sc.size());
    return 0;
}

template <typename T>
static std::vector<T> read_records(const char* path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

static int run_front_end(char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    liorf_amd::ImageProjectionS2M proj(node.handle(), std::atoi(argv[3]));
    const std::vector<unsigned char> raw = read_records<unsigned char>(argv[2]);
    const std::vector<std::array<double, 4>> imu = read_records<std::array<double, 4>>(argv[5]);
    const std::vector<s2m_odom_sample> odom = read_records<s2m_odom_sample>(argv[6]);
    proj.params.n_scan = std::atoi(argv[7]);
    proj.params.downsample_rate = std::atoi(argv[8]);
    proj.params.point_filter_num = std::atoi(argv[9]);
    node.mappingSurfLeafSize = (float)std::atof(argv[10]);
    proj.positionalDeskew = std::atoi(argv[11]) != 0;
    proj.imuRate = (float)std::atof(argv[12]);
    proj.odomQueue.assign(odom.begin(), odom.end());
    proj.cachePointCloud(raw.data(), raw.size(), std::atof(argv[4]));
    proj.imuDeskewInfo(imu);
    proj.odomDeskewInfo();
    proj.projectPointCloud();
    node.downsampleCurrentScanProjected(proj.fullCloudNum);
    std::ofstream o(argv[13], std::ios::binary);
    o.write(reinterpret_cast<const char*>(proj.fullCloud.data()), (std::streamsize)(proj.fullCloud.size() * sizeof(liorf_amd::PointXYZI)));
    if (!o) throw std::runtime_error(std::string("cannot write ") + argv[13]);
    uint64_t sum = 0;                                   // checksum of fullCloud: the 32-bit words added up
    const uint32_t* w = reinterpret_cast<const uint32_t*>(proj.fullCloud.data());
    for (size_t k = 0; k < proj.fullCloud.size() * (sizeof(liorf_amd::PointXYZI) / 4); k++) sum += w[k];
    std::printf("timeScanEnd %.17g imuPointerCur %d imuAvailable %d\n", proj.timeScanEnd, proj.imuPointerCur, proj.imuAvailable ? 1 : 0);
    std::printf("odomAvailable %d odomDeskewFlag %d queue %zu\n", proj.odomAvailable ? 1 : 0, proj.odomDeskewFlag ? 1 : 0, proj.odomQueue.size());
    std::printf("odomIncre %.9g %.9g %.9g\n", proj.odomIncreX, proj.odomIncreY, proj.odomIncreZ);
    std::printf("initialGuess %.9g %.9g %.9g %.9g %.9g %.9g\n", proj.initialGuess[0], proj.initialGuess[1], proj.initialGuess[2], proj.initialGuess[3],
                proj.initialGuess[4], proj.initialGuess[5]);
    std::printf("fullCloud %zu laserCloudSurfLastDSNum %d checksum %llu\n", proj.fullCloud.size(), node.laserCloudSurfLastDSNum, (unsigned long long)sum);
    // updateInitialGuess(): no key poses; then with key poses the first odometry sample (falls through to the IMU branch);
    // then the same guess moved by odomIncre, as the next scan's odometry would be
    node.imuType = 1;
    node.useImuHeadingInitialization = true;
    proj.fillCloudInfo(node.cloudInfo);
    node.cloudInfo.imuRollInit = 0.01f; node.cloudInfo.imuPitchInit = -0.02f; node.cloudInfo.imuYawInit = proj.initialGuess[5];
    for (int step = 0; step < 3; step++) {
        node.haveKeyPoses = step > 0;
        if (step == 2) {
            node.cloudInfo.initialGuessX += proj.odomIncreX; node.cloudInfo.initialGuessY += proj.odomIncreY; node.cloudInfo.initialGuessZ += proj.odomIncreZ;
            node.cloudInfo.imuYawInit += 0.005f;
        }
        node.updateInitialGuess();
        std::printf("guess%d %.9g %.9g %.9g %.9g %.9g %.9g\n", step, node.transformTobeMapped[0], node.transformTobeMapped[1], node.transformTobeMapped[2],
                    node.transformTobeMapped[3], node.transformTobeMapped[4], node.transformTobeMapped[5]);
        std::printf("front%d", step);
        for (int k = 0; k < 12; k++) std::printf(" %.9g", node.incrementalOdometryAffineFront[k]);
        std::printf("\n");
    }
    return 0;
}

// --many map.bin roll pitch yaw x y z scan0.bin scan1.bin ...: the same initial guess for every scan; the scans once as a batch
// (scan2MapOptimizationBatch), once as a stream through two slots (prepareNextScan / launchSlot / collectSlot), once one by one
// (scan2MapOptimization): prints "batch|stream|single <i> iters <n> pose ..." - the three must agree bit for bit.
static int run_many(int argc, char** argv)
{
    liorf_amd::MapOptimizationS2M node;
    node.laserCloudSurfFromMapDS = read_cloud(argv[2]);
    node.haveKeyPoses = !node.laserCloudSurfFromMapDS.empty();
    float guess[6];
    for (int k = 0; k < 6; k++) guess[k] = (float)std::atof(argv[3 + k]);
    std::vector<std::vector<liorf_amd::PointXYZI>> scans;
    for (int a = 9; a < argc; a++) scans.push_back(read_cloud(argv[a]));
    const int n = (int)scans.size();
    node.setInputCloud();
    auto show = [](const char* tag, int i, int iters, const float* p) {
        std::printf("%s %d iters %d pose %.9g %.9g %.9g %.9g %.9g %.9g\n", tag, i, iters, p[0], p[1], p[2], p[3], p[4], p[5]);
    };
    {
        std::vector<const std::vector<liorf_amd::PointXYZI>*> ptrs;
        std::vector<float> poses;
        for (int b = 0; b < n; b++) { ptrs.push_back(&scans[(size_t)b]); for (int k = 0; k < 6; k++) poses.push_back(guess[k]); }
        const std::vector<s2m_result> res = node.scan2MapOptimizationBatch(ptrs, poses);
        for (int b = 0; b < n; b++) show("batch", b, res[(size_t)b].iters_run, &poses[(size_t)6 * (size_t)b]);
    }
    node.prepareNextScan(0, scans[0]);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = guess[k];
        node.launchSlot(i & 1);
        if (i + 1 < n) node.prepareNextScan((i + 1) & 1, scans[(size_t)i + 1]);
        node.collectSlot(i & 1);
        show("stream", i, node.lastResult.iters_run, node.transformTobeMapped);
    }
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = guess[k];
        node.laserCloudSurfLastDS = scans[(size_t)i];
        node.scan2MapOptimization();
        show("single", i, node.lastResult.iters_run, node.transformTobeMapped);
    }
    return 0;
}

// --pose-graph keys.bin keys.txt scan_leaf loops.txt out.bin: keys.txt as for --loop (the pose is the front end's); loops.txt holds
// one line "at key_cur key_pre x y z roll pitch yaw variance robust_k" per closure, queued before key `at` is processed. Prints
// "key <i> iterations inner converged factors error pose(6) corrected" per key, then "kp <i> pose(6)" per key (the graph's
// estimates) and "map_cloud <n>".  The last key's covariance goes to the standard error stream, so that the standard output stays
// the record the Python mirror is compared with: "marginal_old 36 values" from s2m_pg_marginal, "marginal_new 36 values" from
// poseCovariances() (%.17g: equal lines are equal bits).  With --async two more lines follow "map_cloud": the final estimates as
// an odometry chain with every closure of loops.txt, on two fresh nodes, optimised once by s2m_pg_optimize ("optimize_sync") and
// once by launch and polls ("optimize_launched": "iterations inner converged variables factors error_before error_after
// robust_weight_min"; equal lines are equal bits), and the number of polls on the standard error stream.
static void print_pg_result(const char* name, const s2m_pg_result& r)
{
    std::printf("%s %d %d %d %d %d %.17g %.17g %.17g\n", name, r.iterations, r.inner_iterations, r.converged, r.n_variables, r.n_factors,
                r.error_before, r.error_after, r.robust_weight_min);
}

static int run_pose_graph(char** argv, bool launched)
{
    liorf_amd::MapOptimizationS2M node;
    const std::vector<liorf_amd::PointXYZI> all = read_cloud(argv[2]);
    std::ifstream tab(argv[3]);
    if (!tab) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    node.mappingSurfLeafSize = (float)std::atof(argv[4]);
    std::ifstream lf(argv[5]);
    if (!lf) throw std::runtime_error(std::string("cannot open ") + argv[5]);
    std::vector<std::pair<int, liorf_amd::MapOptimizationS2M::LoopFactor>> loops;
    {
        int at;
        liorf_amd::MapOptimizationS2M::LoopFactor l;
        double var;
        while (lf >> at >> l.key_cur >> l.key_pre >> l.rel[0] >> l.rel[1] >> l.rel[2] >> l.rel[3] >> l.rel[4] >> l.rel[5] >> var >> l.robust_k) {
            for (int k = 0; k < 6; k++) l.var[k] = var;
            loops.push_back({ at, l });
        }
    }
    size_t n, at = 0;
    double t;
    float p[6];
    for (int i = 0; tab >> n >> t >> p[0] >> p[1] >> p[2] >> p[3] >> p[4] >> p[5]; i++) {
        if (at + n > all.size()) throw std::runtime_error("keys.txt asks for more points than keys.bin holds");
        node.timeLaserInfoCur = t;
        node.laserCloudSurfLast.assign(all.begin() + (std::ptrdiff_t)at, all.begin() + (std::ptrdiff_t)(at + n));
        at += n;
        node.downsampleCurrentScan();
        const float rpyxyz[6] = { p[3], p[4], p[5], p[0], p[1], p[2] };
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = rpyxyz[k];
        for (const auto& l : loops) if (l.first == i) node.loopQueue.push_back(l.second);
        node.saveKeyFramesAndFactor();
        const bool corrected = node.correctPosesFromGraph();
        const s2m_pg_result& r = node.lastGraphResult;
        const float* q = node.transformTobeMapped;
        std::printf("key %d %d %d %d %d %.17g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", i, r.iterations, r.inner_iterations, r.converged, r.n_factors,
                    r.error_after, q[3], q[4], q[5], q[0], q[1], q[2], corrected ? 1 : 0);
    }
    const size_t N = node.cloudKeyPoses6D.size();
    std::vector<float> est(6 * N);
    if (N > 0 && s2m_pg_get_poses(node.handle(), 0, (int32_t)N, est.data()) != S2M_OK) throw std::runtime_error("s2m_pg_get_poses");
    for (size_t k = 0; k < N; k++)
        std::printf("kp %zu %.9g %.9g %.9g %.9g %.9g %.9g\n", k, est[6 * k], est[6 * k + 1], est[6 * k + 2], est[6 * k + 3], est[6 * k + 4], est[6 * k + 5]);
    std::vector<liorf_amd::PointXYZI> cloud;
    node.globalMapCloud(cloud, 0.0f);
    std::printf("map_cloud %zu\n", cloud.size());
    if (launched) {
        for (int which = 0; which < 2; which++) {
            liorf_amd::MapOptimizationS2M twin;
            for (size_t k = 0; k < N; k++)
                if (s2m_pg_add_odometry(twin.handle(), est.data() + 6 * k) != S2M_OK) throw std::runtime_error("s2m_pg_add_odometry");
            for (const auto& l : loops)
                if ((size_t)l.second.key_cur < N && (size_t)l.second.key_pre < N &&
                    s2m_pg_add_between(twin.handle(), l.second.key_cur, l.second.key_pre, l.second.rel, l.second.var, l.second.robust_k) != S2M_OK)
                    throw std::runtime_error("s2m_pg_add_between");
            if (which == 0) {
                if (s2m_pg_optimize(twin.handle(), nullptr, &twin.lastGraphResult) != S2M_OK) throw std::runtime_error("s2m_pg_optimize");
                print_pg_result("optimize_sync", twin.lastGraphResult);
            } else {
                long polls = 0;
                int rc = twin.pgOptimizeLaunch();
                while (rc == S2M_PG_PENDING) { rc = twin.pgOptimizePoll(); polls++; }
                print_pg_result("optimize_launched", twin.lastGraphResult);
                std::fprintf(stderr, "polls %ld\n", polls);
            }
        }
    }
    if (N > 0) {
        double old_cov[36];
        if (s2m_pg_marginal(node.handle(), (int32_t)N - 1, old_cov) != S2M_OK) throw std::runtime_error("s2m_pg_marginal");
        const std::vector<double> new_cov = node.poseCovariances({ (int32_t)N - 1 });
        for (int which = 0; which < 2; which++) {
            std::fprintf(stderr, which ? "marginal_new" : "marginal_old");
            for (int k = 0; k < 36; k++) std::fprintf(stderr, " %.17g", which ? new_cov[(size_t)k] : old_cov[k]);
            std::fprintf(stderr, "\n");
        }
    }
    std::ofstream out(argv[6], std::ios::binary);
    out.write(reinterpret_cast<const char*>(cloud.data()), (std::streamsize)(cloud.size() * sizeof(liorf_amd::PointXYZI)));
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "--version") { std::puts(s2m_version()); return 0; }
        if (argc == 13 && std::string(argv[1]) == "--chain") return run_chain(argv);
        if (argc >= 10 && std::string(argv[1]) == "--many") return run_many(argc, argv);
        if (argc == 7 && std::string(argv[1]) == "--keyframes") return run_keyframes(argv);
        if (argc == 9 && std::string(argv[1]) == "--loop") return run_loop(argv, false);
        if (argc == 10 && std::string(argv[1]) == "--loop" && std::string(argv[9]) == "--async") return run_loop(argv, true);
        if (argc == 9 && std::string(argv[1]) == "--global-map") return run_global_map(argv);
        if (argc == 7 && std::string(argv[1]) == "--pose-graph") return run_pose_graph(argv, false);
        if (argc == 8 && std::string(argv[1]) == "--pose-graph" && std::string(argv[7]) == "--async") return run_pose_graph(argv, true);
        if (argc == 12 && std::string(argv[1]) == "--project") return run_project(argv);
        if (argc == 14 && std::string(argv[1]) == "--front-end") return run_front_end(argv);
        if (argc != 9 && argc != 16) {
            std::fprintf(stderr, "usage: %s map.bin scan.bin roll pitch yaw x y z [imuType imuRPYWeight z_tol rot_tol imuAvailable imuRoll imuPitch]\n", argv[0]);
            return 2;
        }
        liorf_amd::MapOptimizationS2M node;                 // throws without a gfx950 device
        node.laserCloudSurfFromMapDS = read_cloud(argv[1]);
        node.laserCloudSurfLastDS = read_cloud(argv[2]);
        node.haveKeyPoses = !node.laserCloudSurfFromMapDS.empty();
        for (int k = 0; k < 6; k++) node.transformTobeMapped[k] = (float)std::atof(argv[3 + k]);
        if (argc == 16) {       // members set after construction, like ParamServer's yaml values
            node.imuType = std::atoi(argv[9]);
            node.imuRPYWeight = (float)std::atof(argv[10]);
            node.z_tollerance = (float)std::atof(argv[11]);
            node.rotation_tollerance = (float)std::atof(argv[12]);
            node.cloudInfo.imuAvailable = std::atoll(argv[13]);
            node.cloudInfo.imuRollInit = (float)std::atof(argv[14]);
            node.cloudInfo.imuPitchInit = (float)std::atof(argv[15]);
        }
        node.setInputCloud();
        node.scan2MapOptimization();
        print_result(node);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "s2m_harness: %s\n", e.what());
        return 1;
    }
}
