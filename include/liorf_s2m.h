/*
 * liorf_s2m.h — C ABI of the MI355X (gfx950) scan-to-map registration path.
 *
 * This is the drop-in boundary for ONE path of jimmyshe/liorf's mapOptimization
 * node: scan2MapOptimization() -> surfOptimization() + combineOptimizationCoeffs()
 * + LMOptimization() + transformUpdate()   (reference src/mapOptmization.cpp:1295-1363).
 * Everything behind these entry points runs as hand-written HIP kernels; there is
 * no CPU fallback (calls fail with S2M_ERR_NO_DEVICE when no gfx950 device is usable).
 *
 * Conventions
 *   - plain C types only: pointers, sizes, fixed-width ints, float/double.
 *   - every function returns an int status: 0 = S2M_OK, < 0 = error. The reference's
 *     three soft conditions (no map :1297, <= 30 features :1300, < 50 correspondences
 *     :1178) are NOT errors: status 0, pose unchanged, counters set in s2m_result.
 *   - point clouds are handed over as arrays of records of `stride_bytes` bytes whose
 *     first 12 bytes are float x,y,z. pcl::PointXYZI (the reference's PointType,
 *     include/utility.h:61) is stride 32; tightly packed xyz is stride 12.
 *   - pose vectors are float[6] = {roll, pitch, yaw, x, y, z}: the layout of the
 *     reference's transformTobeMapped[6] (src/mapOptmization.cpp:134, :337-351).
 *   - a handle is single-caller (the reference serialises this path under `mtx`,
 *     :252); separate handles are independent (one per GPU / per stream).
 *   - no C++ exception crosses this boundary.
 */
#ifndef LIORF_S2M_H
#define LIORF_S2M_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2M_ABI_VERSION 1

/* status codes */
#define S2M_OK                 0
#define S2M_ERR_INVALID_ARG   -1
#define S2M_ERR_NO_DEVICE     -2   /* no usable HIP device / kernel image for it   */
#define S2M_ERR_HIP           -3   /* a HIP runtime call failed (see s2m_last_error) */
#define S2M_ERR_NO_SCAN       -4   /* *_resident call without s2m_set_scan          */
#define S2M_ERR_CAPACITY      -5   /* grid / buffer limit exceeded                   */
#define S2M_ERR_BUSY          -6   /* a launched loop closure is pending and this call needs its buffers, or a launched
                                      pose-graph optimise is pending and this call needs the estimates it is working on */
#define S2M_WARN_LEAF_TOO_SMALL 1   /* voxel filter: PCL's "leaf size is too small" case, output = input */

/* ScanContext descriptor shape (reference include/Scancontext.h:82-84) */
#define S2M_SC_NUM_RING    20
#define S2M_SC_NUM_SECTOR  60

typedef struct s2m_context* s2m_handle;

/*
 * Parameters. s2m_default_params() fills in the reference's constants; the
 * comments give the reference line each one restates (src/mapOptmization.cpp
 * unless another file is named).
 */
typedef struct s2m_params {
    uint32_t struct_size;     /* sizeof(s2m_params), set by s2m_default_params          */
    int32_t  device_id;       /* HIP device ordinal (default 0)                          */
    void*    stream;          /* optional caller-owned hipStream_t; NULL = library makes one */
    int32_t  k_neighbors;     /* 5: nearestKSearch(pointSel, 5, ...)              :1087  */
    double   gate_sq;         /* 1.0: pointSearchSqDis[4] < 1.0                   :1097  */
    double   plane_tol;       /* 0.2: |n.p_j + d| > 0.2 rejects the plane         :1118  */
    double   weight_scale;    /* 0.9: s = 1 - 0.9*|pd2|/sqrt(range)               :1127  */
    double   weight_min;      /* 0.1: keep iff s > 0.1                            :1135  */
    int32_t  min_corr;        /* 50: laserCloudSelNum < 50 -> return false        :1178  */
    int32_t  min_feats;       /* 30: laserCloudSurfLastDSNum > 30                 :1300  */
    int32_t  max_iter;        /* 30: iterCount < 30                               :1304  */
    float    eig_thresh;      /* 100: eignThre[6]                                 :1252  */
    double   conv_deg;        /* 0.05: deltaR < 0.05 (degrees)                    :1289  */
    double   conv_cm;         /* 0.05: deltaT < 0.05 (centimetres)                :1289  */
    float    z_tol;           /* z_tollerance, FLT_MAX default  include/utility.h:230     */
    float    rot_tol;         /* rotation_tollerance, FLT_MAX   include/utility.h:231     */
    int32_t  imu_type;        /* imuType (0: 6-axis, 1: 9-axis) include/utility.h:211     */
    float    imu_rpy_weight;  /* imuRPYWeight 0.01              include/utility.h:218     */
    int32_t  early_exit;      /* 1 = break when LMOptimization() returns true (:1313);
                                 0 = always run max_iter iterations (benchmark mode)      */
} s2m_params;

/*
 * The cloud_info fields the hot path reads (reference msg/cloud_info.msg:10-16;
 * read at src/mapOptmization.cpp:1325-1342 by transformUpdate()). NULL is
 * accepted wherever this struct is taken and means imuAvailable = 0.
 */
typedef struct s2m_imu_init {
    int64_t imuAvailable;     /* cloud_info.imuAvailable; the path tests `imuAvailable == true` (:1325), i.e. == 1 */
    float   imuRollInit;      /* cloud_info.imuRollInit  */
    float   imuPitchInit;     /* cloud_info.imuPitchInit */
    float   imuYawInit;       /* cloud_info.imuYawInit (not read on this path) */
} s2m_imu_init;

/* What scan2MapOptimization() leaves behind in the node's members. */
typedef struct s2m_result {
    int32_t iters_run;        /* LM iterations executed (1..max_iter), 0 if skipped       */
    int32_t converged;        /* 1 if LMOptimization() returned true                      */
    int32_t is_degenerate;    /* isDegenerate (:139) -> pose.covariance[0] (:1724-1727)   */
    int32_t n_sel_last;       /* laserCloudSelNum of the last executed iteration          */
    int32_t skipped;          /* 0 ran; 1 no map (:1297); 2 not enough features (:1300)   */
    float   pose[6];          /* transformTobeMapped after transformUpdate()              */
    float   affine[12];       /* incrementalOdometryAffineBack, row-major 3x4 (:1352)     */
} s2m_result;

/* One record per executed LM iteration (s2m_get_trace). */
typedef struct s2m_iter_trace {
    int32_t n_sel;            /* correspondences kept by surfOptimization()               */
    int32_t stepped;          /* 0 if n_sel < min_corr (pose unchanged), else 1           */
    float   delta[6];         /* matX after the degeneracy projection (:1266-1278)        */
    float   pose[6];          /* transformTobeMapped after this iteration                 */
    float   deltaR, deltaT;   /* :1280-1287                                               */
} s2m_iter_trace;

/* ---- lifecycle ---------------------------------------------------------- */
const char* s2m_version(void);
int  s2m_default_params(s2m_params* p);
int  s2m_create(const s2m_params* p, s2m_handle* out);
int  s2m_destroy(s2m_handle h);
const char* s2m_last_error(s2m_handle h);       /* valid until the next call on h */
/* The reference reads its ParamServer members (z_tollerance, rotation_tollerance, imuType, imuRPYWeight,
 * include/utility.h:211-233) every time the path runs; a caller that changes them after s2m_create applies the new
 * values here. Everything except device_id, stream, k_neighbors and gate_sq (fixed at creation: the search grid is
 * built for the gate) may change between scans; takes effect with the next s2m_optimize* call. */
int  s2m_set_params(s2m_handle h, const s2m_params* p);
int  s2m_get_params(s2m_handle h, s2m_params* out);

/* ---- inputs ------------------------------------------------------------- */
/* Replaces kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS) (:1302):
 * uploads the local surf map and builds the device neighbour-search index.
 * n == 0 is allowed and models "cloudKeyPoses3D->points.empty()" (:1297).
 * A map whose extent no search grid can cover (e.g. a finite point at 1e30) returns S2M_ERR_CAPACITY and leaves the
 * handle with no map: s2m_optimize* then report skipped == 1 until a map is set that succeeds. */
int  s2m_set_map(s2m_handle h, const void* pts, size_t n, size_t stride_bytes);
/* Same, for a map that already lives in device memory (hipMalloc'd). */
int  s2m_set_map_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes);
/* Uploads laserCloudSurfLastDS (lidar-frame points) for the *_resident calls. */
int  s2m_set_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes);
int  s2m_set_scan_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes);

/* ---- the path ----------------------------------------------------------- */
/* scan2MapOptimization() (:1295-1321) on host buffers: s2m_set_scan() followed
 * by s2m_optimize_resident(). pose is in/out (= transformTobeMapped). */
int  s2m_optimize(s2m_handle h, const void* scan, size_t n, size_t stride_bytes,
                  float pose[6], const s2m_imu_init* imu, s2m_result* out);
/* The <= max_iter x {surfOptimization, combineOptimizationCoeffs, LMOptimization}
 * loop (:1304-1315) plus transformUpdate() (:1317) on the resident scan + map.
 * Runs entirely on the device; one synchronisation at the end. */
int  s2m_optimize_resident(s2m_handle h, float pose[6], const s2m_imu_init* imu,
                           s2m_result* out);
/* Asynchronous form for throughput measurement: enqueue the same device work on
 * the handle's stream and return without synchronising; s2m_optimize_collect()
 * synchronises and fills the outputs of the most recent launch. */
int  s2m_optimize_launch(s2m_handle h, const float pose[6]);
int  s2m_optimize_collect(s2m_handle h, float pose[6], const s2m_imu_init* imu,
                          s2m_result* out);
/* ---- a batch of scans against one resident map (BASELINE config 4 on one GPU; the multi-GPU form shards scans over
 * ranks, liorf_amd/host/s2m_multi_gpu.cpp) --------------------------------------------------------------------------
 * The reference registers one scan at a time (laserCloudInfoHandler holds `mtx`, :252); scans of a batch share nothing but the
 * read-only local map, so n_scans scan2MapOptimization() calls can be in flight at once: every scan
 * slot has its own buffers, loop state and trace, all slots search the map installed with s2m_set_map / s2m_extract_cloud on
 * `h`, and the n_scans LM loops advance in lockstep inside ONE captured graph (one launch, one synchronisation): every kernel
 * launch of the loop carries one grid row per scan, so that while one scan's workgroups wait on a dependent load the others'
 * points are processed.
 * Results are those of n_scans separate s2m_optimize calls, bit for bit.
 * In every function of this group n_scans is 1 to 64 and slot is 0 to 63: anything else is S2M_ERR_INVALID_ARG with nothing changed.
 *   scans[b], sizes[b]   laserCloudSurfLastDS of scan b (host records, stride_bytes as everywhere)
 *   poses[6*b .. 6*b+5]   in: initial guess of scan b, out: its transformTobeMapped
 *   imu                   NULL, or n_scans entries;  out: NULL, or n_scans entries */
int  s2m_optimize_batch(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes,
                        float* poses, const s2m_imu_init* imu, s2m_result* out);
/* The same in steps: install scan b in slot b (host or device records; a device source must stay valid until the collect),
 * enqueue the batch without synchronising, synchronise and fetch.
 * One batch is in flight at a time: s2m_optimize_batch_launch is refused (S2M_ERR_INVALID_ARG, nothing changed) while a batch
 * is pending or while one of its slots runs a loop of its own (s2m_slot_optimize_launch).
 * A launch that is refused or fails leaves nothing pending: no slot of it can be collected.
 * s2m_optimize_batch_collect takes the n_scans of the pending launch and is refused with any other, or with no batch pending.
 * A collect ends the batch whatever it returns: after an error the results are lost and the slots are free again.
 * s2m_set_params on `h` is refused while a batch or a slot is pending. */
int  s2m_batch_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device);
/* All slots 0 .. n_scans-1 at once: the ordering kernels of the n_scans scans share their launches (six launches for the batch
 * instead of six per scan; the host side of a batch of eight scans is otherwise a quarter of its wall time). */
int  s2m_batch_set_scans(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes, int on_device);
int  s2m_optimize_batch_launch(s2m_handle h, int n_scans, const float* poses);
int  s2m_optimize_batch_collect(s2m_handle h, int n_scans, float* poses, const s2m_imu_init* imu, s2m_result* out);
int  s2m_batch_get_trace(s2m_handle h, int slot, s2m_iter_trace* out, int cap);
/* A stream of scans against the resident map, one in flight per slot: slot k's preparation (scan ordering, wave table) and its
 * loop run on slot k's own stream, so the preparation of scan i+1 in one slot overlaps the LM loop of scan i in the other - the
 * reference does downsampleCurrentScan() and scan2MapOptimization() strictly one after the other (:257-265).  Typical use:
 *     s2m_slot_set_scan(h, 0, scan0 ..);
 *     for i:  s2m_slot_optimize_launch(h, i & 1, guess_i);  s2m_slot_set_scan(h, (i + 1) & 1, scan_{i+1} ..);  s2m_slot_optimize_collect(h, i & 1, ..)
 * Every result is bitwise that of s2m_optimize on the same scan.  The map must not be replaced while a slot is in flight.
 * Slots and batches do not cross: s2m_slot_optimize_launch is refused (S2M_ERR_INVALID_ARG, nothing changed) while a batch is
 * pending, and a batch launch while a slot is in flight.
 * s2m_slot_optimize_collect is refused on a slot that has no launch of its own pending; it ends that launch whatever it returns. */
int  s2m_slot_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device);
int  s2m_slot_optimize_launch(s2m_handle h, int slot, const float pose[6]);
int  s2m_slot_optimize_collect(s2m_handle h, int slot, float pose[6], const s2m_imu_init* imu, s2m_result* out);

/* Per-iteration records of the last optimize call; returns the count (<= cap). */
int  s2m_get_trace(s2m_handle h, s2m_iter_trace* out, int cap);

/* ---- observation hooks (used by the parity tests) ----------------------- */
/* One surfOptimization() pass (:1074-1143) at `pose` on the resident scan + map.
 * Outputs are in the scan's ORIGINAL point order; any may be NULL.
 *   idx5   [n*5]  neighbour indices into the map as given to s2m_set_map, ascending d2
 *   d2_5   [n*5]  squared distances (fp32, ((dx^2+dy^2)+dz^2))
 *   flag   [n]    laserCloudOriSurfFlag (:1138)
 *   coeff4 [n*4]  coeffSelSurfVec: s*pa, s*pb, s*pc, s*pd2 (:1130-1133); 0 if !flag
 * idx5/d2_5 are defined for queries whose 5th neighbour passes the gate
 * (d2 < gate_sq); for the others idx5 = -1 (the reference never reads them). */
int  s2m_surf_optimization(s2m_handle h, const float pose[6],
                           int32_t* idx5, float* d2_5, uint8_t* flag, float* coeff4);
/* matAtA / matAtB / laserCloudSelNum of one iteration at `pose` (:1182-1239). */
int  s2m_normal_eq(s2m_handle h, const float pose[6], float AtA[36], float AtB[6],
                   int32_t* n_sel);
/* Raw device time (ms) of the last s2m_optimize* call and of the last s2m_set_map / s2m_set_scan index build.
 * For a single scan both intervals come from the device's constant-frequency wall clock, stamped by the kernels
 * that bracket them: set_scan_ms runs from the start of the first ordering kernel to the end of the last,
 * optimize_ms from the end of the state upload of s2m_optimize_launch to the end of the last close of the loop
 * (no longer from event to event: the idle time around an event record is not part of it, and no event record
 * costs GPU time in a step).  A batch and s2m_set_map are timed with HIP events on the handle's stream.
 * Synchronises the handle's stream when a scan preparation is still to be timed. */
int  s2m_last_timing(s2m_handle h, float* optimize_ms, float* set_map_ms, float* set_scan_ms);
/* Diagnostic and benchmark entry points (per-launch timing, per-wave profiles, the device's trig arithmetic, experiment
 * switches read from the environment) are declared in liorf_s2m_debug.h: they are exported by the same library but are not part
 * of the boundary a node binds. */

/* ---- The voxel-grid stages either side of the path ----------
 * pcl::VoxelGrid<pcl::PointXYZI>::applyFilter with the reference's settings (all fields averaged,
 * no minimum point count): one output record {centroid x, y, z, 1.0f, mean intensity, 0...} per occupied
 * voxel, in ascending voxel-index order like PCL. Input records carry intensity at byte 16 when
 * stride_bytes >= 20 (pcl::PointXYZI). Points with a non-finite coordinate are skipped. Within a voxel the
 * points are summed in ascending input order (PCL's unstable std::sort leaves that order unspecified).
 * `cap` is the capacity of `out` in records; *n_out is always the number of voxels, and a result that does
 * not fit returns S2M_ERR_CAPACITY after writing the first `cap` records. S2M_WARN_LEAF_TOO_SMALL (> 0)
 * reports PCL's index-overflow case, where the output is the unfiltered input. */

/* downSizeFilter*.setInputCloud(cloud); .filter(out) for a host cloud (reference :1064-1065, :1037-1038). */
int  s2m_voxel_downsample(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, float leaf,
                          void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* Same with both clouds in device memory (no host copies; returns after the handle's stream has drained). */
int  s2m_voxel_downsample_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes, float leaf,
                                 void* d_out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* downsampleCurrentScan() (reference :1061-1067) fused with s2m_set_scan: filters laserCloudSurfLast
 * (host records, or device records when on_device != 0) with leaf mappingSurfLeafSize and installs the result
 * as the scan of the next s2m_optimize_resident / s2m_optimize_launch. If cap > 0 the filtered cloud
 * (laserCloudSurfLastDS, which the node later stores as the key frame's cloud) is also copied to host `out`. */
int  s2m_downsample_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, int on_device, float leaf,
                         void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* extractCloud() (reference :1014-1039) after the key-frame selection, fused with s2m_set_map: for the
 * chosen key frames f = 0..n_frames-1, transformPointCloud(frames[f], pose f) (:310-329; poses_xyzrpy holds
 * {x, y, z, roll, pitch, yaw} of each PointTypePose), concatenated in that order, filtered with leaf
 * surroundingKeyframeMapLeafSize, and installed as the local surf map (the reference's kd-tree build,
 * :1302). frames[] are host buffers, or device buffers when on_device != 0 (a device-resident key-frame
 * store replaces the reference's laserCloudMapContainer cache: re-transforming is cheaper than caching).
 * If cap > 0 the filtered map (laserCloudSurfFromMapDS) is also copied to host `out`. */
int  s2m_extract_cloud(s2m_handle h, int n_frames, const void* const* frames, const size_t* frame_sizes,
                       size_t stride_bytes, int on_device, const float* poses_xyzrpy, float leaf,
                       void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* transformPointCloud(cloudIn, transformIn) (reference :310-329) for one host cloud; out holds n records. */
int  s2m_transform_cloud(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, const float pose_xyzrpy[6],
                         void* out, size_t out_stride_bytes);

/* ---- The resident key-frame store and extractSurroundingKeyFrames() -------------------------------------
 * The key-frame containers of mapOptimization (cloudKeyPoses3D / cloudKeyPoses6D / surfCloudKeyFrames, :93-100)
 * kept on the device, and extractSurroundingKeyFrames() (:1046-1059 -> extractNearby :975-1010 -> extractCloud
 * :1012-1044) run against them. Key frames are numbered 0.. in the order they are added (at most 2^24: the
 * reference carries key ids in a float intensity). With P[i] the position of key i, N the store size and R, D, L, W
 * the four parameters below, the selection is:
 *   (b) every key with d2(P[i], P[N-1]) < (float)(R*R), in ascending (d2, i); d2 = fp32 ((dx*dx + dy*dy) + dz*dz).
 *       [ext] FLANN 1.9's radius search: L2_Simple accumulation, strict '<', ties in index order.
 *   (c) those positions as records {P[i], 1, intensity i} through the VoxelGrid above with leaf D.
 *   (d) for every centroid, in voxel order, its nearest key among all N (same d2; equal distances: lower index).
 *   (e) then keys N-1, N-2, ... while time_cur - time[i] < W (double), stopping at the first that fails (duplicates
 *       of (d) are kept, and concatenated twice, as in the reference).
 *   (f) an entry is dropped when sqrtf(|x - P[N-1]|^2) > R, x being the CENTROID for entries of (d) (the reference
 *       tests the down-sampled key pose, :1018) and the key's own position for entries of (e).
 *   (g) the surviving keys' clouds, each transformed by its current pose, concatenated in that order, filtered with
 *       leaf L and installed as the local map: bit for bit s2m_extract_cloud on those frames and poses.
 * Each key's transform is computed once, when its pose is set (the reference's laserCloudMapContainer cache).
 * (b)-(d) and (f) run on the device; the count of recent keys in (e) is taken on the host, from the key times it
 * keeps, and handed to the kernels (a double comparison over the newest keys, no data leaves the device for it). */
typedef struct s2m_kf_params {
    float  search_radius;    /* surroundingKeyframeSearchRadius 50.0   include/utility.h:240 */
    float  density;          /* surroundingKeyframeDensity 1.0         include/utility.h:238 (configs: 2.0) */
    float  map_leaf;         /* surroundingKeyframeMapLeafSize 0.2     include/utility.h:228 (configs: 0.5) */
    double recent_window_s;  /* 10.0, the literal at :1003 */
} s2m_kf_params;
#define S2M_KF_FROM_HOST            0   /* pts: host records of stride_bytes */
#define S2M_KF_FROM_DEVICE          1   /* pts: device records of stride_bytes */
#define S2M_KF_FROM_LAST_DOWNSAMPLE 2   /* laserCloudSurfLastDS as the last s2m_downsample_scan left it (:1577); pts, n and
                                           stride_bytes are ignored; S2M_ERR_NO_SCAN before any s2m_downsample_scan */
int  s2m_kf_default_params(s2m_kf_params* p);
int  s2m_kf_reset(s2m_handle h);
int  s2m_kf_size(s2m_handle h);                                   /* key frames stored, or a negative status */
/* saveKeyFramesAndFactor() (:1549-1580): append key frame N with pose {x, y, z, roll, pitch, yaw} and time. The
 * cloud is copied into the store as 32-byte records. A failed add leaves the store as it was. */
int  s2m_kf_add(s2m_handle h, const float pose_xyzrpy[6], double time,
                const void* pts, size_t n, size_t stride_bytes, int source);
/* correctPoses() (:1611-1640): replace the poses of key frames first .. first+count-1 (a range inside [0, N)). */
int  s2m_kf_set_poses(s2m_handle h, int first, int count, const float* poses_xyzrpy);
/* extractSurroundingKeyFrames() at timeLaserInfoCur = time_cur, fused with s2m_set_map like s2m_extract_cloud: an
 * empty store returns S2M_OK with *n_out = *n_keys = 0 and leaves the installed map alone (:1048-1049). If cap > 0
 * the filtered map is copied to host `out`; keys (optional) receives the key id of every frame concatenated into the
 * map, in concatenation order. *n_out and *n_keys (optional) always hold the full counts; an output that does not
 * fit gets its first cap / keys_cap entries and the call returns S2M_ERR_CAPACITY (the map is installed). */
int  s2m_extract_surrounding(s2m_handle h, double time_cur, const s2m_kf_params* p /* NULL = defaults */,
                             void* out, size_t out_stride_bytes, size_t cap, size_t* n_out,
                             int32_t* keys, size_t keys_cap, size_t* n_keys);
/* ---- The local map around a given position ------------------------------------------------------------------
 * A node that starts, or recovers, inside a map it already holds is not at the newest key: it is wherever
 * s2m_relocalize_scan (below) found it. This call is s2m_extract_surrounding with centre_xyz in place of P[N-1]:
 *   (b) every key with d2(P[i], centre) < (float)(R*R), (c) the key-pose VoxelGrid, (d) the nearest key of every
 *   centroid, (f) an entry dropped when sqrtf(|centroid - centre|^2) > R, (g) the transformed clouds concatenated,
 *   filtered with leaf L and installed as the local map with its index - the same kernels; the centre reaches them
 *   by value, and s2m_extract_surrounding / s2m_global_map hand them P[N-1]'s own bits.
 *   There are no recent keys (e): recent_window_s is ignored, the times of a stored map belong to another session.
 * With centre_xyz = P[N-1] the result is what s2m_extract_surrounding gives with recent_window_s = 0 and
 * time_cur = t[N-1]. Capacity, counts, S2M_ERR_CAPACITY, the empty store and S2M_WARN_LEAF_TOO_SMALL behave as there.
 * A null or non-finite centre is S2M_ERR_INVALID_ARG. */
int  s2m_extract_surrounding_at(s2m_handle h, const float centre_xyz[3], const s2m_kf_params* p /* NULL = defaults */,
                                void* out, size_t out_stride_bytes, size_t cap, size_t* n_out,
                                int32_t* keys, size_t keys_cap, size_t* n_keys);

/* ---- The global map and the saved map from the key-frame store -------------------------------------------
 * publishGlobalMap() (reference src/mapOptmization.cpp:453-502) and saveMapService() (:375-432) against the resident store,
 * so that the node keeps no host copy of surfCloudKeyFrames. N, P[i] and pose[i] as above.
 * s2m_global_map: (b), (c), (d) and (f) of the selection above around key N-1 with R = search_radius and D = pose_density,
 *   and no recent keys (e); the surviving keys' clouds transformed by their current poses, concatenated in selection order
 *   and filtered with leaf `leaf` (globalMapKeyFramesDS). Capacity, *n_out, keys, *n_keys and S2M_ERR_CAPACITY behave as in
 *   s2m_extract_surrounding; an empty store gives S2M_OK with zero counts; S2M_WARN_LEAF_TOO_SMALL returns the unfiltered
 *   concatenation. At most 2^31 - 2^21 concatenated points (S2M_ERR_CAPACITY beyond, before anything is transformed).
 * s2m_kf_map_cloud: keys first .. first+count-1 (a range inside [0, N)) transformed by their current poses and concatenated in
 *   key order (globalSurfCloud, :395-398); with leaf > 0 also filtered with that leaf (SurfMap.pcd at req.resolution, :400-407).
 *   leaf == 0 is the unfiltered cloud (GlobalMap.pcd, and SurfMap.pcd at resolution 0): it is produced in bounded chunks of
 *   frames and never held whole on the device; cap == 0 is the size query (*n_out set, nothing written). With leaf > 0 the
 *   whole concatenation is filtered on the device: more than 2^31 - 2^21 points give S2M_ERR_CAPACITY before any launch.
 *   *n_out always holds the full count; a short `out` gets its first cap records and S2M_ERR_CAPACITY.
 * Neither call touches the installed local map and its index, the scan, the pose, the batch and stream slots, the key store
 * or the loop-index container: the next registration is bit for bit the one without them. The handle is held for the whole
 * call, the copy to `out` included. */
typedef struct s2m_gmap_params {
    float search_radius;     /* globalMapVisualizationSearchRadius 1e3  include/utility.h:250 */
    float pose_density;      /* globalMapVisualizationPoseDensity  10.0 include/utility.h:251 (M2DGR.yaml: 3.0) */
    float leaf;              /* globalMapVisualizationLeafSize     1.0  include/utility.h:252 */
} s2m_gmap_params;
int  s2m_gmap_default_params(s2m_gmap_params* p);
int  s2m_global_map(s2m_handle h, const s2m_gmap_params* p /* NULL = defaults */,
                    void* out, size_t out_stride_bytes, size_t cap, size_t* n_out,
                    int32_t* keys, size_t keys_cap, size_t* n_keys);
int  s2m_kf_map_cloud(s2m_handle h, int first, int count, float leaf /* 0 = no filter */,
                      void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);

/* ---- imageProjection's point filter and IMU deskew (reference src/imageProjection.cpp) ---------------------
 * projectPointCloud() (:568-598) with deskewPoint() (:536-566) and findRotation() (:493-518) on the raw records of one
 * lidar message, and the host half that prepares it, imuDeskewInfo() (:350-409). The raw bytes of a
 * sensor_msgs::PointCloud2 (or of the reference's PCL structs, :4-57) are read in place through an s2m_scan_layout, so the
 * per-sensor conversion loops (:216-274) have no counterpart. Citations below are into src/imageProjection.cpp.
 *
 * A record i survives when, in this order and with these types,
 *   range = sqrtf((x*x + y*y) + z*z) is not < lidar_min_range and not > lidar_max_range (a NaN range survives, :581),
 *   0 <= ring < n_scan (:585; ring as int: an i32 ring is taken as it is, the reference narrows it to uint16_t first),
 *   ring % downsample_rate == 0 (:588), i % point_filter_num == 0 (:591).
 * Survivors keep index order. With deskew == 0 a survivor is copied (:538-539). Otherwise, per survivor:
 *   pointTime = time_scan_cur + (double)time (:541), time being the record's time field converted as time_type says;
 *   findRotation() as written: front = the first table index in [0, imu_pointer_cur) with pointTime < imu_time[front], else
 *     imu_pointer_cur; pointTime > imu_time[front] or front == 0 copies entry front; otherwise the two ratios and the
 *     two-term sums in double, narrowed to float (a point time equal to the last table time therefore interpolates with
 *     ratio 1, and front == 0 copies entry 0);
 *   R = pcl::getTransformation(0, 0, 0, rotX, rotY, rotZ) in float with the host libm's sinf / cosf;
 *   S = inverse(R of the first survivor) (transStartInverse, :551); B = S * R; the output is
 *     ((B00*x + B01*y) + B02*z) + B03 and so on (:560-562), intensity copied, the record's other 4-byte slots zero.
 *   [ext] Eigen 3.3 Transform<float,3,Affine>::inverse() is the general 3x3 inverse: Linv(r, c) = cofactor(c, r) * (1 / det)
 *     with cofactor(i, j) = m(i+1, j+1) * m(i+2, j+2) - m(i+1, j+2) * m(i+2, j+1) (indices mod 3) and
 *     det = (cof(0,0)*m00 + cof(1,0)*m10) + cof(2,0)*m20, translation -(Linv * t) - not the transpose.
 *   [ext] the 4x4 product accumulates ((a0*b0 + a1*b1) + a2*b2) + a3*b3 without contraction (the reference builds with -O3
 *     only). The translation column is kept and added although findPosition() returns zeros: it decides the sign of a zero.
 *     The particular doubt: Eigen 3.3's transform_transform_product_impl for two Affine (non-projective) transforms may
 *     instead form linear = L * L (three terms per entry) and translation = L * t + t. With R's zero translation and
 *     (0, 0, 0, 1) bottom row the extra terms are signed zeros, so the two forms can differ only in the sign of a zero
 *     entry of B. Eigen is not available to this repository; this stays unpinned.
 * Output records are 32 bytes on the device (pcl::PointXYZI): the handle's cloud_deskewed, which stays resident with its
 * count for s2m_downsample_projected / s2m_sc_add_projected.
 * odomDeskewInfo() and findPosition() with its commented lines live: s2m_odom_deskew_info / s2m_project_scan_motion below. */
#define S2M_RING_U8        0
#define S2M_RING_U16       1
#define S2M_RING_I32       2
#define S2M_TIME_F32       0   /* float, as stored (Velodyne, Livox :216-219)                                   */
#define S2M_TIME_U32_NS    1   /* uint32 t: (float)t * 1e-9f, the product in float (Ouster :235)               */
#define S2M_TIME_U32       2   /* uint32 t: (float)t (MulRan :253)                                              */
#define S2M_TIME_F64_REL   3   /* double timestamp: (float)(timestamp - timestamp of record 0) (Robosense :263, :272) */
#define S2M_SENSOR_VELODYNE  0
#define S2M_SENSOR_LIVOX     1
#define S2M_SENSOR_OUSTER    2
#define S2M_SENSOR_MULRAN    3
#define S2M_SENSOR_ROBOSENSE 4
#define S2M_IMU_QUEUE_LENGTH 2000   /* queueLength (:62): entries of the four deskew tables */
typedef struct s2m_scan_layout {
    uint32_t stride;          /* bytes per record (PointCloud2.point_step)                                      */
    uint32_t off_x;           /* byte offset of float x; y and z follow                                         */
    uint32_t off_intensity;   /* float intensity                                                                */
    uint32_t off_ring;
    uint32_t off_time;
    int32_t  ring_type;       /* S2M_RING_*                                                                     */
    int32_t  time_type;       /* S2M_TIME_*                                                                     */
} s2m_scan_layout;
/* The reference's own structs (:4-57): Velodyne / Livox 32 bytes (intensity 16, ring u16 20, time f32 24), Ouster 48
 * (intensity 16, t u32 20, ring u8 26), MulRan 32 (t u32 20, ring i32 24), Robosense 32 (ring u16 20, timestamp f64 24).
 * A layout is valid when every field lies inside the stride and is naturally aligned (offset and stride multiples of
 * the field's size); everything else is S2M_ERR_INVALID_ARG, from every call that takes a layout. */
int  s2m_scan_layout_preset(int32_t sensor, s2m_scan_layout* out);
typedef struct s2m_project_params {
    int32_t n_scan;            /* N_SCAN 16              include/utility.h:204 */
    int32_t downsample_rate;   /* downsampleRate 1       include/utility.h:206 */
    int32_t point_filter_num;  /* point_filter_num 3     include/utility.h:207 */
    float   lidar_min_range;   /* lidarMinRange 1.0      include/utility.h:208 */
    float   lidar_max_range;   /* lidarMaxRange 1000.0   include/utility.h:209 */
} s2m_project_params;
int  s2m_project_default_params(s2m_project_params* p);
/* imuDeskewInfo() (:350-409) without the queue and without the imuType RPY lines: imu holds n samples {time, wx, wy, wz}
 * (doubles; already through imuConverter, already popped to time_scan_cur - 0.01). Fills the four tables (room for
 * S2M_IMU_QUEUE_LENGTH entries each) with the reference's double arithmetic, its break at > time_scan_end + 0.01 and its
 * final --imuPointerCur; *imu_available = imuPointerCur > 0. n == 0 gives pointer 0, not available. More than
 * S2M_IMU_QUEUE_LENGTH used samples: S2M_ERR_CAPACITY (the reference would write past its arrays). Host code: no handle,
 * no GPU. */
int  s2m_imu_deskew_info(const double* imu, size_t n, double time_scan_cur, double time_scan_end,
                         double* imu_time, double* imu_rot_x, double* imu_rot_y, double* imu_rot_z,
                         int32_t* imu_pointer_cur, int32_t* imu_available);
typedef struct s2m_deskew_info {
    double  time_scan_cur;     /* timeScanCur (:282)                                                            */
    int32_t deskew;            /* deskewFlag == 1 && cloudInfo.imuAvailable; 0 copies the survivors             */
    int32_t imu_pointer_cur;   /* imuPointerCur after imuDeskewInfo(): the tables hold imu_pointer_cur + 1 entries */
    const double* imu_time;
    const double* imu_rot_x;
    const double* imu_rot_y;
    const double* imu_rot_z;
} s2m_deskew_info;
/* The argument checks of s2m_project_scan on their own (host code, no handle, no GPU): S2M_OK or S2M_ERR_INVALID_ARG.
 * params and deskew may be NULL (defaults, no deskew). Why it is part of the boundary: s2m_project_scan answers a null
 * handle with the same S2M_ERR_INVALID_ARG, so on a machine without a GPU (no handle can be created there) a caller - a
 * node validating its yaml and message fields at start-up, or a test - could not tell a refused layout from a refused
 * handle through s2m_project_scan alone. */
int  s2m_project_check_args(const s2m_scan_layout* layout, const s2m_project_params* params, const s2m_deskew_info* deskew);
/* projectPointCloud() on records `pts` (host bytes, or device bytes when on_device != 0; 8-byte aligned). With
 * deskew->deskew != 0 the table times must be non-decreasing and 1 <= imu_pointer_cur < S2M_IMU_QUEUE_LENGTH, else
 * S2M_ERR_INVALID_ARG (for non-decreasing times the reference's linear walk and the device's bisection find the same
 * index; nothing else is promised). params: downsample_rate < 1, point_filter_num < 1, n_scan < 1 or a non-finite range
 * are S2M_ERR_INVALID_ARG (the reference would divide by zero); NULL = defaults. deskew NULL = no deskew.
 * The result stays on the device as cloud_deskewed; cap > 0 also copies it to host `out` (out_stride >= 12, a multiple
 * of 4); *n_out is always the full count; a short `out` gets cap records and S2M_ERR_CAPACITY. n == 0 or no survivor:
 * S2M_OK, count 0, cloud_deskewed empty and valid. Three launches; the host waits once, for the count (and for the kernels
 * to have left `pts`), and with cap > 0 a second time for the copy. The call does not touch the map and its index, the
 * scan, scan_ds, the pose, the slots, the key store, the ScanContext store or the loop container. */
int  s2m_project_scan(s2m_handle h, const void* pts, size_t n, const s2m_scan_layout* layout, int on_device,
                      const s2m_project_params* params, const s2m_deskew_info* deskew,
                      void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* downsampleCurrentScan() on the resident cloud_deskewed: exactly s2m_downsample_scan(on_device = 1) on that buffer (same
 * scan_ds, same installed scan, same warnings). S2M_ERR_NO_SCAN before the first s2m_project_scan. */
int  s2m_downsample_projected(s2m_handle h, float leaf, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* makeAndSaveScancontextAndKeys(cloud_deskewed) (src/mapOptmization.cpp:1591-1594) from the resident buffer: the stored
 * descriptor and keys are those of s2m_sc_add_scan on the downloaded cloud. S2M_ERR_NO_SCAN before the first
 * s2m_project_scan. */
int  s2m_sc_add_projected(s2m_handle h);

/* ---- odomDeskewInfo(), positional deskew and the initial pose guess ---------------------------------------
 * The rest of the chain from a raw lidar message to a registered pose: odomDeskewInfo() (src/imageProjection.cpp:411-491),
 * findPosition() with its commented lines live (:520-534) inside deskewPoint(), and updateInitialGuess()
 * (src/mapOptmization.cpp:899-958). The ROS queues, imuConverter, imuPreintegration and publishOdometry()'s IMU slerp
 * stay with the node. */

/* One nav_msgs::Odometry of odomQueue as odomDeskewInfo() reads it. */
typedef struct s2m_odom_sample {
    double time;               /* header.stamp.toSec()                                */
    double px, py, pz;         /* pose.pose.position                                  */
    double qx, qy, qz, qw;     /* pose.pose.orientation                               */
    double cov0;               /* pose.covariance[0] (imuPreintegration's reset mark) */
} s2m_odom_sample;
typedef struct s2m_odom_deskew {
    int32_t odom_available;    /* cloudInfo.odomAvailable (:413, :456)                                            */
    int32_t odom_deskew_flag;  /* odomDeskewFlag (:459, :490)                                                     */
    float   initial_guess[6];  /* cloudInfo.initialGuessX, Y, Z, Roll, Pitch, Yaw: the message's float32 fields (:449-454) */
    float   odom_incre[3];     /* odomIncreX, Y, Z (:488)                                                          */
    int32_t n_popped;          /* front samples the reference pops (:415-421): the caller pops as many             */
} s2m_odom_deskew;
/* odomDeskewInfo() (src/imageProjection.cpp:411-491) over odom[0 .. n) in queue order. Host code: no handle, no GPU.
 *   - the front pop (:415-421): samples with time < time_scan_cur - sync_diff_time, sync_diff_time being the reference's
 *     `static float` (imuRate >= 300) ? 0.01 : 0.20, i.e. 0.01f or 0.20f widened to double in the subtraction; *out reports
 *     how many were popped. The reference evaluates the static once; a caller keeps imu_rate constant.
 *   - the remaining queue empty, or its front later than time_scan_cur: not available (:423-427). The fields of *out other
 *     than odom_available and n_popped are then zero - the reference leaves its members as the previous scan set them;
 *     a node that wants that keeps its own copy, as the mirrors do.
 *   - start sample: the first with time >= time_scan_cur, else the last (:432-440); end sample likewise at time_scan_end
 *     (:466-474), after the `back().time < time_scan_end` return (:461-462: available, flag off, odom_incre zero).
 *   - int(round(cov0)) of the two samples differing: available, flag off (:476-477).
 *   - roll, pitch, yaw in double. [ext] tf::Matrix3x3(q).getRPY: Matrix3x3::setRotation with s = 2 / length2(q) (a
 *     quaternion that is not unit length is scaled, not refused), entries 1 - (yy + zz), xy - wz, ...; getEulerYPR
 *     solution 1: |m20| >= 1 gives yaw = 0, pitch = +-pi/2, roll = atan2(m01, m02) or atan2(-m01, -m02); otherwise
 *     pitch = -asin(m20), roll = atan2(m21 / cos(pitch), m22 / cos(pitch)), yaw = atan2(m10 / cos(pitch), m00 / cos(pitch)).
 *   - transBegin, transEnd = pcl::getTransformation of the six values narrowed to float (its parameters are float), term
 *     order as everywhere in this library; transBegin.inverse() * transEnd with the Affine3f conventions stated for
 *     s2m_project_scan above ([ext] general 3x3 inverse by cofactors, translation -(Linv * t); 4x4 product accumulating
 *     ((a0*b0 + a1*b1) + a2*b2) + a3*b3); odom_incre = its translation column (pcl::getTranslationAndEulerAngles).
 *   tf and PCL are not available to this repository: parity unpinned, like the float chain above.
 * odom NULL with n > 0, out NULL or a non-finite time_scan_cur / time_scan_end: S2M_ERR_INVALID_ARG. */
int  s2m_odom_deskew_info(const s2m_odom_sample* odom, size_t n, double time_scan_cur, double time_scan_end, float imu_rate,
                          s2m_odom_deskew* out);

/* Positional deskew: what findPosition() (:520-534) adds when its commented lines are live. The reference ships them
 * commented out ("if the sensor moves relatively slow, like walking speed ..."); a vehicle at 10-30 m/s smears a 0.1 s
 * sweep by 1-3 m. Opt-in: */
typedef struct s2m_motion_info {
    int32_t enabled;           /* cloudInfo.odomAvailable && odomDeskewFlag (the test of :526); 0 = s2m_project_scan */
    double  time_scan_end;     /* timeScanEnd (:283)                                                              */
    float   odom_incre[3];     /* odomIncreX, Y, Z (s2m_odom_deskew.odom_incre)                                   */
} s2m_motion_info;
/* s2m_project_check_args plus the motion argument: with motion != NULL and motion->enabled != 0 a non-finite
 * time_scan_end or increment is S2M_ERR_INVALID_ARG (a disabled motion's other fields are not read). */
int  s2m_project_check_args_motion(const s2m_scan_layout* layout, const s2m_project_params* params, const s2m_deskew_info* deskew,
                                   const s2m_motion_info* motion);
/* s2m_project_scan with findPosition() live. motion == NULL or motion->enabled == 0: s2m_project_scan bit for bit (the
 * same kernels), the resident cloud_deskewed and its count included. deskew->deskew == 0 copies the survivors whatever
 * motion says (:538-539). Otherwise, per survivor, after findRotation():
 *   float ratio = relTime / (timeScanEnd - timeScanCur) (:529): relTime is the record's float time widened to double
 *     (:594 -> :536), the subtraction and the division are in double, the quotient is narrowed once to float;
 *   posX, Y, Z = ratio * odom_incre[0..2], in float (:531-533);
 *   pcl::getTransformation(posX, posY, posZ, rotX, rotY, rotZ) replaces the pure rotation in both places: the first
 *     survivor's transform, whose own position is in general not zero, inverted into transStartInverse (:551; the
 *     translation of the inverse is -((Linv0*t0 + Linv1*t1) + Linv2*t2) per row), and every survivor's transFinal (:556);
 *   B = S * T as the 4x4 product above - the translation column is ((S0*pos0 + S1*pos1) + S2*pos2) + S3*1.0f - and the
 *     output expression are unchanged.
 * time_scan_end == time_scan_cur is not refused: the ratio is infinite or NaN as the reference's arithmetic makes it.
 * Zero increments with enabled != 0 may differ from s2m_project_scan in the sign of a zero.
 * Arguments, outputs, waits (three launches, one wait, a second with cap > 0), errors and the "does not touch" promise
 * are those of s2m_project_scan. */
int  s2m_project_scan_motion(s2m_handle h, const void* pts, size_t n, const s2m_scan_layout* layout, int on_device,
                             const s2m_project_params* params, const s2m_deskew_info* deskew, const s2m_motion_info* motion,
                             void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);

/* updateInitialGuess() (src/mapOptmization.cpp:899-958). The caller owns the three function statics of the reference: */
typedef struct s2m_guess_state {
    float   last_imu_transformation[12];      /* lastImuTransformation (:904), row-major 3x4                       */
    float   last_imu_pre_transformation[12];  /* lastImuPreTransformation (:921)                                   */
    int32_t last_imu_pre_trans_available;     /* lastImuPreTransAvailable (:920)                                   */
} s2m_guess_state;
/* The cloud_info fields updateInitialGuess() reads (msg/cloud_info.msg:10-24). */
typedef struct s2m_guess_info {
    int64_t imuAvailable;      /* tested `== true` (:945), i.e. == 1, as s2m_imu_init.imuAvailable */
    int64_t odomAvailable;     /* tested `== true` (:922), i.e. == 1                                */
    float   imuRollInit, imuPitchInit, imuYawInit;
    float   initialGuess[6];   /* X, Y, Z, Roll, Pitch, Yaw (s2m_odom_deskew.initial_guess)        */
} s2m_guess_info;
/* The state before the first scan: lastImuPreTransAvailable = false; the two transforms all zero ([ext] a function-static
 * Eigen::Affine3f is zero-initialised storage; the reference writes lastImuTransformation on the first scan, before any
 * read). */
int  s2m_guess_state_init(s2m_guess_state* st);
/* One call of updateInitialGuess(). Host code: no handle, no GPU. pose is transformTobeMapped {roll, pitch, yaw, x, y, z},
 * in and out: the result is what s2m_optimize* takes as pose. affine_front receives incrementalOdometryAffineFront =
 * trans2Affine3f(pose on entry) (:902), row-major 3x4 like s2m_result.affine (incrementalOdometryAffineBack).
 * The reference's control flow exactly:
 *   key_poses_empty (:906-917): pose[0..2] = the three imu*Init, pose[2] = 0 unless use_imu_heading_initialization;
 *     lastImuTransformation = getTransformation(0, 0, 0, imu*Init); return.
 *   odomAvailable == 1 (:922-942): transBack = getTransformation(initialGuess). First time: it becomes
 *     lastImuPreTransformation, the flag is set, and control FALLS THROUGH to the IMU branch. Later:
 *     pose = getTranslationAndEulerAngles(trans2Affine3f(pose) * (lastImuPreTransformation.inverse() * transBack)),
 *     lastImuPreTransformation = transBack, lastImuTransformation refreshed; return.
 *   imuAvailable == 1 && imu_type (:945-957): the same with transBack = getTransformation(0, 0, 0, imu*Init) against
 *     lastImuTransformation, which is refreshed; return. Otherwise nothing changes (lastImuTransformation is NOT refreshed).
 * All in float: getTransformation in host term order with libm sinf / cosf; [ext] the Affine3f product as for the
 * loop-closure pose result (linear = ((a0 b0 + a1 b1) + a2 b2), translation = ((a0 t0 + a1 t1) + a2 t2) + a3);
 * [ext] inverse() as stated for s2m_project_scan; [ext] pcl::getTranslationAndEulerAngles: roll = atan2f(T21, T22),
 * pitch = asinf(-T20), yaw = atan2f(T10, T00). Parity unpinned. */
int  s2m_update_initial_guess(s2m_guess_state* st, float pose[6], int key_poses_empty, const s2m_guess_info* info,
                              int use_imu_heading_initialization, int imu_type, float affine_front[12]);

/* ---- ScanContext descriptor (BASELINE config 5) ------------------------- */
/* SCManager::makeScancontext + makeRingkeyFromScancontext
 * (reference include/Scancontext.cpp:151-211): desc is 20x60 row-major doubles,
 * ringkey 20 doubles. Points are host records as above. */
int  s2m_make_scancontext(s2m_handle h, const void* pts, size_t n, size_t stride_bytes,
                          double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR],
                          double ringkey[S2M_SC_NUM_RING]);

/* ---- ScanContext matching ----------------------------------------------
 * The SCManager's containers (reference include/Scancontext.h:102-113) kept on the device, and
 * SCManager::detectLoopClosureID (include/Scancontext.cpp:253-344) with distanceBtnScanContext /
 * fastAlignUsingVkey / distDirectSC (:69-148) as one kernel. Key frames are numbered in the order they are
 * added. The reference rebuilds its ring-key kd-tree every 10th detection (TREE_MAKING_PERIOD_); the same
 * staleness is kept: between rebuilds the search sees the key frames that existed at the last rebuild,
 * minus the 30 most recent (NUM_EXCLUDE_RECENT). The 3 ring-key neighbours (NUM_CANDIDATES_FROM_TREE) are an
 * exact fp32 3-NN in nanoflann's accumulation order; equal distances go to the lower index. */
typedef struct s2m_sc_match {
    double  min_dist;        /* best distanceBtnScanContext over the candidates (10000000 if none)  */
    int32_t nn_idx;          /* its key frame                                                        */
    int32_t nn_align;        /* its column shift (yaw difference in units of 6 degrees)             */
    int32_t cand_idx[3];     /* ring-key neighbours, ascending distance                              */
    float   cand_d2[3];      /* their squared ring-key distances                                     */
} s2m_sc_match;
int  s2m_sc_reset(s2m_handle h);
int  s2m_sc_size(s2m_handle h);                                   /* key frames stored, or a negative status */
/* makeAndSaveScancontextAndKeys(scan) (:236-250): descriptor, ring key and sector key of a host cloud, appended. */
int  s2m_sc_add_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes);
/* The same for a descriptor computed elsewhere (20x60 row-major doubles). */
int  s2m_sc_add_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR]);
/* detectLoopClosureID() for the newest key frame: *loop_id = matching key frame or -1, *yaw_diff_rad as the
 * reference returns it (also when there is no loop); `detail` (optional) receives the intermediate values. */
int  s2m_sc_detect_loop(s2m_handle h, int32_t* loop_id, float* yaw_diff_rad, s2m_sc_match* detail);
/* distanceBtnScanContext(query, candidate k) for m stored candidates at once (one workgroup each): the
 * batched form in which this row is worth running on a GPU. */
int  s2m_sc_distance(s2m_handle h, int32_t query_idx, const int32_t* cand_idx, int32_t m, double* dist, int32_t* shift);

/* ---- ScanContext place query -------------------------------------------------------
 * "Where in the stored map is this scan?": a query descriptor against EVERY stored descriptor of a range, on the
 * device, and the K nearest keys under a threshold, each with its shift and yaw. Not a function of the reference:
 * detectLoopClosureID compares the newest key with 3 ring-key neighbours at 7 of the 60 column shifts; this
 * compares any descriptor with all keys, at 7 shifts or at all 60. Read-only; no existing call changes.
 *
 * Searched set. S is the keys of [first, first+count) outside [exclude_lo, exclude_hi). A stored-key query does
 * not exclude itself; the caller does that with the window (exclude_lo = N-30, exclude_hi = N is the reference's
 * NUM_EXCLUDE_RECENT).
 * Distance, sector-key alignment (S2M_SC_ALIGN_SECTOR_KEY). d(q, c) and shift are distanceBtnScanContext(q, c)
 * (:116-148). For a stored query they are bit for bit what s2m_sc_distance returns.
 * Distance, full alignment (S2M_SC_ALIGN_FULL). Start from 10000000 and shift 0. For s = 0 .. 59 ascending, take
 * distDirectSC(q, circshift(c, s)) (:69-91) whenever it is strictly smaller. Every sum runs left to right in fp64,
 * like the oracle's restatement of distDirectSC. A NaN never wins: a candidate with no comparable sector keeps
 * 10000000, as in the reference. The full distance is never above the sector-key one.
 * Hits. A hit is a key of S with d < max_dist. The hits are ordered by ascending (d, key) and the first top_k are
 * written; *n_hits is how many were written. `hits` has room for top_k records.
 * Yaw. yaw_diff_rad is formed from shift exactly as s2m_sc_detect_loop forms it (:339).
 * Query sources. _key queries with a stored key; _descriptor takes its sector key as an appended descriptor gets
 * it (makeSectorkeyFromScancontext, :214-227); _scan builds the descriptor as s2m_sc_add_scan does; _projected
 * builds it as s2m_sc_add_projected does, S2M_ERR_NO_SCAN before any s2m_project_scan. None of the four appends
 * anything.
 * Read-only. The calls leave the store, s2m_sc_size, the detector's rebuild counter and its searched set as they
 * were: the next s2m_sc_detect_loop is bit for bit the one without the query. Like the other s2m_sc_* calls they
 * work beside a pending loop closure or a pending pose-graph optimise; they run on the handle's main stream and
 * touch only ScanContext buffers. One synchronisation per query; the ranking happens on the device.
 * Errors and empty cases. S2M_ERR_INVALID_ARG: a null handle or null outputs; top_k outside 1..32; an unknown
 * align; max_dist not in (0, 10000000], NaN included; first < 0, count < -1 or a range past the store; a _key
 * query outside [0, N). S2M_OK with *n_hits = 0: an empty store; an empty S. p == NULL means the defaults. */
#define S2M_SC_QUERY_MAX_K       32
#define S2M_SC_ALIGN_SECTOR_KEY  0   /* distanceBtnScanContext as the reference: 7 shifts around fastAlignUsingVkey */
#define S2M_SC_ALIGN_FULL        1   /* all 60 shifts */
typedef struct s2m_sc_query_params {
    int32_t first, count;            /* searched keys [first, first+count); count = -1: to the end of the store */
    int32_t exclude_lo, exclude_hi;  /* keys in [exclude_lo, exclude_hi) are left out; lo >= hi: none */
    int32_t top_k;                   /* 1 .. S2M_SC_QUERY_MAX_K */
    int32_t align;                   /* S2M_SC_ALIGN_* */
    double  max_dist;                /* a hit needs dist < max_dist; default SC_DIST_THRES 0.3 (Scancontext.h:95) */
} s2m_sc_query_params;
typedef struct s2m_sc_hit { double dist; int32_t key; int32_t shift; float yaw_diff_rad; int32_t reserved; } s2m_sc_hit;

int  s2m_sc_query_default_params(s2m_sc_query_params* p);   /* 0, -1, 0, 0, 1, SECTOR_KEY, 0.3 */
/* The argument table above for a store of n_stored keys: S2M_OK or S2M_ERR_INVALID_ARG. Host only, no handle. */
int  s2m_sc_query_check_args(int32_t n_stored, const s2m_sc_query_params* p);
int  s2m_sc_query_key       (s2m_handle h, int32_t key, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits);
int  s2m_sc_query_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR], const s2m_sc_query_params* p,
                             s2m_sc_hit* hits, int32_t* n_hits);
int  s2m_sc_query_scan      (s2m_handle h, const void* pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p,
                             s2m_sc_hit* hits, int32_t* n_hits);
int  s2m_sc_query_projected (s2m_handle h, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits);

/* ---- The place query for many queries at once ----------------------------------------
 * "Which pairs of keys of this session are the same place?" and "which keys of this session are places of that
 * other session?": m queries - stored keys, or descriptors from elsewhere - against the store in one call, as a
 * tiled all-pairs problem on the device instead of m single queries.
 *
 * Rows. Row i is hits[i * top_k ..]; its first n_hits[i] records are valid, the records behind them are left as
 * the caller had them. Row i is bit for bit what s2m_sc_query_key(keys[i]) or s2m_sc_query_descriptor(descs +
 * 1200 * i) returns for the same searched set: dist, key, shift, yaw_diff_rad, reserved = 0, in the same
 * (dist, key) order, with the same 10000000 / NaN rule. keys may repeat and come in any order.
 * Searched set. Per query exactly the single query's set (q: range, fixed window), and for a stored-key query
 * ALSO without the keys c with keys[i] + rel_lo <= c < keys[i] + rel_hi (sums in 64 bits; rel_lo >= rel_hi:
 * no relative window). The detector's exclusion, "nothing from the 30 most recent keys on", is rel_lo = -29,
 * rel_hi = INT32_MAX: key i is compared with the keys 0 .. i-30. A descriptor has no key to be relative to: a
 * non-empty relative window on s2m_sc_query_descriptors is an error.
 * Read-only, exactly as the single query: the store, s2m_sc_size, the detector's counter and its searched set
 * are untouched; the calls work beside a pending closure, verification or optimise and run on the handle's main
 * stream. The queries go through in passes whose lists, staged queries and rows take at most 64 MiB of device
 * memory whatever m and N are; a call synchronises once per pass, never once per query.
 * s2m_sc_get_descriptors copies the stored descriptors first .. first+count-1 out, bit for bit what was added
 * (20x60 row-major doubles each): what a node needs to carry one session's descriptors to another handle.
 * Errors. S2M_ERR_INVALID_ARG: what the single query rejects; m < 0; null keys / descs / outputs with m > 0; a
 * key outside [0, N); a non-empty relative window on a descriptor query; a range of s2m_sc_get_descriptors
 * outside the store. S2M_OK: m == 0 writes nothing; an empty store or an empty set gives n_hits[i] = 0.
 * p == NULL means the defaults. */
typedef struct s2m_sc_query_many_params {
    s2m_sc_query_params q;   /* range, fixed window, top_k, align, max_dist: per query exactly as in the single query */
    int32_t rel_lo, rel_hi;  /* stored-key queries: ALSO leave out c with key + rel_lo <= c < key + rel_hi
                                (sums in 64 bits); rel_lo >= rel_hi: none */
} s2m_sc_query_many_params;

int  s2m_sc_query_many_default_params(s2m_sc_query_many_params* p);   /* single-query defaults, rel 0, 0 */
/* The argument table above for a store of n_stored keys and m queries: S2M_OK or S2M_ERR_INVALID_ARG. Host only. */
int  s2m_sc_query_many_check_args(int32_t n_stored, int32_t m, const s2m_sc_query_many_params* p, int32_t descriptor_query);
int  s2m_sc_query_keys(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_query_many_params* p,
                       s2m_sc_hit* hits /* m * top_k */, int32_t* n_hits /* m */);
int  s2m_sc_query_descriptors(s2m_handle h, const double* descs /* m * 1200, row-major as s2m_sc_add_descriptor */, int32_t m,
                              const s2m_sc_query_many_params* p, s2m_sc_hit* hits, int32_t* n_hits);
int  s2m_sc_get_descriptors(s2m_handle h, int32_t first, int32_t count, double* descs /* count * 1200 */);

/* ---- The place query behind a ring-key prefilter --------------------------------------
 * The two-stage search of detectLoopClosureID (:253-344) for any query: the rotation-invariant 20-float ring key
 * names n_candidates keys of the searched set, and only those are compared column by column. The exhaustive
 * queries above cost (queries x searched keys) descriptor pairs; these cost (queries x n_candidates). The caller
 * chooses n_candidates and with it recall against time: 3 is the detector's choice; an n_candidates of at least
 * the size of the searched set gives the exhaustive query's row bit for bit. A single query is m = 1.
 *
 * Ring-key distance. d2(q, c) is the squared L2 distance of two fp32 ring keys in the order of nanoflann's
 * L2_Adaptor - five groups of four, result += d0*d0 + d1*d1 + d2*d2 + d3*d3, fp32, uncontracted - the statement
 * s2m_sc_detect_loop's three-neighbour search uses. A stored key's ring key is the stored fp32 row; an external
 * descriptor's is (float) of its row means, exactly what s2m_sc_add_descriptor would store for it: a descriptor
 * query equals the key query of the same descriptor once added.
 * Neighbour set. S_i is query i's searched set exactly as s2m_sc_query_keys / _descriptors define it (range,
 * fixed window and, for a stored-key query, the relative window, sums in 64 bits); a stored-key query does not
 * exclude itself unless a window does. R_i is the first n_candidates keys of { c in S_i : d2(q_i, c) < +inf } in
 * ascending (d2, key) order. A NaN or infinite d2 is never a neighbour, so |R_i| may be below n_candidates.
 * s2m_sc_ring_neighbours_*: row i is out[i * n_candidates ..], R_i in that order; n_out[i] = |R_i|.
 * Hits. s2m_sc_query_*_ring: row i is hits[i * top_k ..], the ranking the single query would give were its
 * searched set R_i: the keys of R_i with dist < max_dist in ascending (dist, key) order, the first top_k; dist,
 * shift and yaw_diff_rad as every other place query forms them (both alignments), reserved = 0, the same
 * 10000000 / NaN rule. Records behind n_out[i] / n_hits[i] are left as the caller had them.
 * Read-only, exactly as the many-query: the store, s2m_sc_size, the detector's counter and its searched set are
 * untouched; the calls work beside a pending closure, verification or optimise, run on the handle's main stream,
 * touch only ScanContext buffers, go through in passes of at most 64 MiB of device memory and synchronise once
 * per pass, never once per query.
 * Errors. S2M_ERR_INVALID_ARG: a null handle; everything s2m_sc_query_many_check_args rejects (the neighbour
 * calls check top_k, align and max_dist too and do not use them); n_candidates outside 1 ..
 * S2M_SC_RING_MAX_CAND; reserved != 0; null queries or outputs with m > 0; a key outside [0, N). The outputs are
 * then untouched. S2M_OK: m == 0 writes nothing; an empty store or an empty S_i gives 0 for that row.
 * p == NULL means the defaults. */
#define S2M_SC_RING_MAX_CAND 256
typedef struct s2m_sc_ring_params {
    s2m_sc_query_many_params m;   /* searched set, top_k, align, max_dist: exactly as in the many-query */
    int32_t n_candidates;         /* 1 .. S2M_SC_RING_MAX_CAND; default 3 = NUM_CANDIDATES_FROM_TREE */
    int32_t reserved;             /* 0 */
} s2m_sc_ring_params;
typedef struct s2m_sc_ring_neighbour { float d2; int32_t key; } s2m_sc_ring_neighbour;

int  s2m_sc_ring_default_params(s2m_sc_ring_params* p);   /* the many-query's defaults, n_candidates 3, reserved 0 */
/* The argument table above for a store of n_stored keys and m queries: S2M_OK or S2M_ERR_INVALID_ARG. Host only, no handle. */
int  s2m_sc_ring_check_args(int32_t n_stored, int32_t m, const s2m_sc_ring_params* p, int32_t descriptor_query);
/* stage one alone */
int  s2m_sc_ring_neighbours_keys(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_ring_params* p,
                                 s2m_sc_ring_neighbour* out /* m * n_candidates */, int32_t* n_out /* m */);
int  s2m_sc_ring_neighbours_descriptors(s2m_handle h, const double* descs /* m * 1200 */, int32_t m, const s2m_sc_ring_params* p,
                                        s2m_sc_ring_neighbour* out, int32_t* n_out);
/* both stages */
int  s2m_sc_query_keys_ring(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_ring_params* p,
                            s2m_sc_hit* hits /* m * top_k */, int32_t* n_hits /* m */);
int  s2m_sc_query_descriptors_ring(s2m_handle h, const double* descs /* m * 1200 */, int32_t m, const s2m_sc_ring_params* p,
                                   s2m_sc_hit* hits, int32_t* n_hits);

/* ---- ICP loop-closure alignment ------------------------------------------
 * pcl::IterativeClosestPoint<PointType, PointType> as performRSLoopClosure / performSCLoopClosure configure
 * and run it (reference src/mapOptmization.cpp:571-586, :663-678): setMaxCorrespondenceDistance,
 * setMaximumIterations, setTransformationEpsilon, setEuclideanFitnessEpsilon, RANSAC off, identity guess
 * (s2m_icp_align_guess below takes one),
 * align(); then hasConverged(), getFitnessScore(), getFinalTransformation(). src = cureKeyframeCloud, tgt =
 * prevKeyframeCloud (host records). T is the row-major 4x4 final transformation (source -> target). As in
 * PCL, reaching max_iterations counts as converged; fewer than 3 correspondences does not. */
typedef struct s2m_icp_params {
    double  max_correspondence_distance;   /* historyKeyframeSearchRadius * 2 (:573)  */
    int32_t max_iterations;                /* 100 (:574)                              */
    double  transformation_epsilon;        /* 1e-6 (:575)                             */
    double  euclidean_fitness_epsilon;     /* 1e-6 (:576)                             */
} s2m_icp_params;
typedef struct s2m_icp_result {
    float   T[16];
    int32_t converged;
    int32_t iterations;
    double  fitness_score;                 /* getFitnessScore(): mean squared nearest-neighbour distance after alignment */
} s2m_icp_result;
int  s2m_icp_default_params(s2m_icp_params* p);
int  s2m_icp_align(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                   const s2m_icp_params* p /* NULL = defaults */, s2m_icp_result* out);
/* ---- ICP with an initial guess --------------------------------------------------------------------------------
 * pcl::IterativeClosestPoint::align(output, guess): final_transformation_ starts as `guess` (row-major 4x4), the
 * source is moved by it before the first correspondence search, and everything after that is the loop of
 * s2m_icp_align - so out->T includes the guess (source frame -> target frame) and the fitness pass, which applies the
 * final T to the source as it was given, is the same pass.
 * [ext] PCL's own point-transform arithmetic is not pinned here: the source is moved in fp32 as
 *       m0*x + m1*y + m2*z + m3 per row, evaluated left to right without contraction - the arithmetic that moves the
 *       source between iterations.
 * guess == NULL, or a matrix equal to the identity (PCL tests `guess != Identity` the same way), is byte for byte
 * s2m_icp_align. A guess with an entry that is not finite, or a last row other than 0 0 0 1, is S2M_ERR_INVALID_ARG.
 * Busy rules as s2m_icp_align. */
int  s2m_icp_align_guess(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                         const float guess[16] /* row-major 4x4, NULL = identity */,
                         const s2m_icp_params* p /* NULL = defaults */, s2m_icp_result* out);

/* ---- Loop closure against the key-frame store (SURVEY.md section 8(f), row F4 with its inputs) -------------------
 * performRSLoopClosure() (reference src/mapOptmization.cpp:542-622) and the extraction / ICP / gate half of
 * performSCLoopClosure() (:624-730) run against the resident key-frame store above, so that the loop thread keeps no
 * host key-frame clouds and no kd-tree over the key poses. N is the store size; P[i], t[i], pose[i] the position, time
 * and {x, y, z, roll, pitch, yaw} of key i as s2m_kf_add / s2m_kf_set_poses left them.
 *   Detection, detectLoopClosureDistance() (:732-765): the candidates are keys with d2(P[i], P[N-1]) < (float)(R*R),
 *       d2 and order as (b) of s2m_extract_surrounding (ascending d2, equal distances: lower index). key_pre is the
 *       first candidate with fabs(t[i] - time_cur) > (double)time_diff_s; time_cur is timeLaserInfoCur, the current
 *       scan's time, not t[N-1]. No such key, or key_pre == N-1: S2M_LOOP_NONE.
 *       [ext] `abs` of a double at :755 is std::abs(double) (libstdc++ with <cmath>), not the int overload.
 *   Loop-index container (loopIndexContainer, :146): the handle keeps key_cur -> key_pre of every accepted closure. A
 *       key_cur already in it gives S2M_LOOP_ALREADY_CLOSED before any extraction (:737-739, :641-643). s2m_kf_reset
 *       clears it.
 *   Submaps, loopFindNearKeyframes(key, search_num, loop_index) (:821-844): for i = -search_num .. search_num the cloud
 *       of key + i (skipped outside [0, N)), transformed by pose[loop_index != -1 ? loop_index : key + i], concatenated
 *       in i order and filtered with leaf icp_leaf (downSizeFilterICP). An empty concatenation stays empty.
 *       cur = (key_cur, 0, base_key), prev = (key_pre, search_num, base_key).
 *   Gates and ICP (:565-586): n_cur < 300 or n_prev < 1000 gives S2M_LOOP_TOO_FEW_POINTS. Otherwise s2m_icp_align's
 *       ICP (source cur, target prev, max correspondence distance (double)(search_radius * 2.0f), 100 iterations,
 *       1e-6 / 1e-6) on the device submaps; !converged or fitness_score > (double)fitness_score gives
 *       S2M_LOOP_REJECTED, anything else S2M_LOOP_ACCEPTED, recorded in the container.
 *   Pose result (accepted closures): with C = icp.T,
 *       base_key == -1 (RS): pose_from = getTranslationAndEulerAngles(C * getTransformation(pose[key_cur])) (:597-604),
 *                            pose_to = pose[key_pre] (:606);
 *       base_key >= 0  (SC): pose_from = getTranslationAndEulerAngles(C) (:707), pose_to = zeros (:709).
 *       [ext] pcl::getTranslationAndEulerAngles (PCL 1.10 common/impl/eigen.hpp) in float: x, y, z = T(0..2, 3),
 *       roll = atan2(T21, T22), pitch = asin(-T20), yaw = atan2(T10, T00); the Affine3f product in float, each entry
 *       ((a0 b0 + a1 b1) + a2 b2). GTSAM stays with the caller: poseFrom.between(poseTo) and the noise model
 *       (fitness_score for RS, the robust Cauchy model for SC) are formed from pose_from, pose_to and icp.
 * None of these calls touches the installed local map and its index, the scan (scan_ds included, which
 * S2M_KF_FROM_LAST_DOWNSAMPLE reads), the pose, the batch and stream slots, or the key store: the next registration is
 * bit for bit the one without the loop call. Calls on a handle are not concurrent: the node's loop thread takes the same
 * lock as the scan handler around them. s2m_loop_align and s2m_loop_closure_rs hold the handle for the whole call, ICP included;
 * the launched forms below hold it up to the size gate only.
 * Errors: a null handle, params outside their range or keys outside [0, N) give S2M_ERR_INVALID_ARG; an empty store gives
 * S2M_OK with S2M_LOOP_NONE (or no records); a short output buffer gives S2M_ERR_CAPACITY after writing cap records. */
typedef struct s2m_loop_params {
    float   search_radius;   /* historyKeyframeSearchRadius   10.0  include/utility.h:245 (configs: 15.0) */
    float   time_diff_s;     /* historyKeyframeSearchTimeDiff 30.0  include/utility.h:246 */
    int32_t search_num;      /* historyKeyframeSearchNum      25    include/utility.h:247 */
    float   fitness_score;   /* historyKeyframeFitnessScore   0.3   include/utility.h:248 */
    float   icp_leaf;        /* loopClosureICPSurfLeafSize    0.3   include/utility.h:239 (configs: 0.5), downSizeFilterICP :196 */
} s2m_loop_params;
#define S2M_LOOP_NONE            0  /* no candidate, or the candidate is the current key (:761) */
#define S2M_LOOP_ALREADY_CLOSED  1  /* the container already holds key_cur (:737-739, :641-643) */
#define S2M_LOOP_TOO_FEW_POINTS  2  /* cureKeyframeCloud < 300 or prevKeyframeCloud < 1000 points (:565-566) */
#define S2M_LOOP_REJECTED        3  /* !hasConverged() or getFitnessScore() > fitness_score (:585) */
#define S2M_LOOP_ACCEPTED        4
typedef struct s2m_loop_result {
    int32_t status;                 /* S2M_LOOP_* */
    int32_t key_cur, key_pre;       /* both -1 with S2M_LOOP_NONE; key_pre -1 when RS finds key_cur already closed */
    int32_t n_cur, n_prev;          /* sizes of the two filtered submaps (0 when not built) */
    s2m_icp_result icp;             /* valid when ICP ran (S2M_LOOP_REJECTED, S2M_LOOP_ACCEPTED) */
    float pose_from[6];             /* x y z roll pitch yaw, accepted closures: see above */
    float pose_to[6];
} s2m_loop_result;
int  s2m_loop_default_params(s2m_loop_params* p);
/* loopFindNearKeyframes(key, search_num, loop_index) (:821-844) with leaf `leaf`, to host records (pubHistoryKeyFrames,
 * MULTI_SCAN_FEAT). loop_index is -1 or a key. *n_out holds the full count; S2M_WARN_LEAF_TOO_SMALL as the voxel calls. */
int  s2m_loop_near_keyframes(s2m_handle h, int32_t key, int32_t search_num, int32_t loop_index, float leaf,
                             void* out, size_t out_stride_bytes, size_t cap, size_t* n_out);
/* Extraction, gates, ICP and pose result for a given pair (the container test first). base_key = -1 is the RS / external
 * form; base_key >= 0 is the SC form (performSCLoopClosure passes 0). */
int  s2m_loop_align(s2m_handle h, int32_t key_cur, int32_t key_pre, int32_t base_key,
                    const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* out);
/* performRSLoopClosure() without the external detection: the container test for key N-1, the device detection at
 * timeLaserInfoCur = time_cur, then s2m_loop_align(N-1, key_pre, -1, p). */
int  s2m_loop_closure_rs(s2m_handle h, double time_cur, const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* out);

/* ---- Loop closure beside the scan handler: launch, poll, collect ------------------------------------------------
 * The reference runs loop closure in a thread of its own (loopClosureThread, :506-622): ICP takes as long as it takes while
 * laserCloudInfoHandler keeps registering scans. The launched forms give the handle the same property. A launch does what
 * s2m_loop_align / s2m_loop_closure_rs do up to and including the size gate (argument checks, the container test, the
 * detection of the RS form, both submaps, n_cur < 300 || n_prev < 1000) and waits for the device only where they do (the
 * detection result, the voxel counts). A call decided there returns in `early` exactly what the synchronous call returns
 * (S2M_LOOP_NONE, S2M_LOOP_ALREADY_CLOSED, S2M_LOOP_TOO_FEW_POINTS, the errors) and nothing is pending. Otherwise
 * early->status = S2M_LOOP_PENDING with key_cur, key_pre, n_cur, n_prev filled, and the whole ICP - the search structure over
 * the target submap, every iteration with its close and convergence test, the fitness pass - is queued on a stream of the
 * handle's own, of the lowest priority the device offers, behind the submap writes; the call returns without waiting for it.
 * The launch keeps what the pose result needs, transCur of key_cur and pose[key_pre], as they are at that moment (the
 * reference copies copy_cloudKeyPoses6D the same way): a later s2m_kf_set_poses or s2m_pg_apply_to_store does not change
 * the result.
 *   s2m_loop_poll never waits for the device: it tests an event. While the queued iterations run it returns S2M_OK with
 *       S2M_LOOP_PENDING (keys and sizes filled). Iterations are queued a range at a time; a poll that finds a range ended
 *       and the alignment not, queues the next range; one that finds the alignment ended queues the fitness pass; one that
 *       finds the fitness pass ended applies the fitness gate, forms the pose result from the launch-time poses, records an
 *       accepted closure in the container and returns S2M_LOOP_REJECTED / S2M_LOOP_ACCEPTED - the bytes s2m_loop_align
 *       returns for the same store. With nothing pending: S2M_LOOP_NONE, keys -1.
 *   s2m_loop_collect is the same with waits: it returns the final result.
 *   The container is written when the result is collected, not at launch. One closure is in flight per handle.
 *   While a closure is pending, every call that does not use the loop's buffers works as before and returns what it
 *       would without it (s2m_set_*, s2m_optimize*, batches, slots, s2m_extract_surrounding, s2m_kf_add, s2m_kf_set_poses,
 *       s2m_pg_*, s2m_project_*, the voxel calls, s2m_sc_*); s2m_loop_align, s2m_loop_closure_rs, s2m_loop_near_keyframes,
 *       s2m_icp_align and a second launch return S2M_ERR_BUSY and touch nothing; s2m_kf_reset and s2m_destroy first wait for
 *       the loop stream and drop the pending closure. A call that has to grow a device buffer may wait for the closure (the
 *       runtime frees memory only on an idle device).
 *   The node's loop thread: take the scan handler's lock, launch, release; then lock, s2m_loop_poll, release, sleep, until
 *       the status is not S2M_LOOP_PENDING. */
#define S2M_LOOP_PENDING         5
int  s2m_loop_align_launch(s2m_handle h, int32_t key_cur, int32_t key_pre, int32_t base_key,
                           const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* early);
int  s2m_loop_closure_rs_launch(s2m_handle h, double time_cur, const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* early);
int  s2m_loop_poll(s2m_handle h, s2m_loop_result* out);      /* never waits for the device */
int  s2m_loop_collect(s2m_handle h, s2m_loop_result* out);   /* waits; poll until not pending */

/* ---- Verification: one key against several candidates, aligned in lockstep ---------------------------------------
 * s2m_sc_query_* answers "which stored keys look like this one?" with a ranked list; descriptor distances rank places, they
 * do not verify them. A verification aligns key_cur against n_cand <= S2M_LOOP_MAX_CANDIDATES stored keys at once: the n_cand
 * alignments are independent and advance through the same kernel launches (the candidate is a grid dimension of every kernel
 * of the device loop), so the whole costs about what its slowest alignment costs alone.
 *   Records: record i is byte for byte what s2m_loop_align(h, key_cur, key_pre[i], base_key, p) returns on a handle whose
 *       container does not hold key_cur - status, keys, sizes, icp, pose_from, pose_to - in the caller's order. The source
 *       submap (key_cur, 0, base_key) is built once, the target submap (key_pre[i], search_num, base_key) of every candidate
 *       into a buffer of its own. The container test comes first: a key_cur it holds gives S2M_LOOP_ALREADY_CLOSED in every
 *       record. The size gates hold per candidate: n_prev < 1000 gives that candidate S2M_LOOP_TOO_FEW_POINTS at launch,
 *       n_cur < 300 gives it to all of them.
 *   s2m_loop_verify_launch returns without waiting for the alignments. If no candidate is left after the gates, `early`
 *       holds the final records and nothing is pending; otherwise the candidates that are left carry S2M_LOOP_PENDING,
 *       filled as s2m_loop_align_launch fills them, and their poses are kept as they are at launch. *best is -1.
 *   s2m_loop_verify_poll never waits for the device; it moves the queued work on as s2m_loop_poll does (ranges until every
 *       candidate's alignment has ended, then one fitness pass for all) and returns the records as they stand.
 *       s2m_loop_verify_collect is the same with waits. s2m_loop_verify is launch plus collect; `out` takes n_cand records.
 *   *best: the position of the accepted candidate with the least (icp.fitness_score, position), -1 if none is accepted
 *       or while pending. Only key_cur -> key_pre[*best] goes into the container, when the result is collected; the other
 *       records keep the status the single call would give, S2M_LOOP_ACCEPTED there meaning "passed the gate". So hits
 *       that s2m_sc_query_* orders by descriptor distance are re-ranked by fitness.
 *   A pending verification is a pending closure: every rule above about a pending closure holds for it. s2m_loop_poll and
 *       s2m_loop_collect with a verification pending, and s2m_loop_verify_poll / _collect with a single closure pending,
 *       return S2M_ERR_BUSY and touch nothing. With nothing pending the verify forms return S2M_OK, *n_out = 0, *best = -1.
 *   Errors: n_cand outside [1, S2M_LOOP_MAX_CANDIDATES], a key outside the store, a candidate listed twice or equal to
 *       key_cur give S2M_ERR_INVALID_ARG; s2m_loop_verify_check_args gives the same verdict from the store's size alone
 *       (host code, no handle, no GPU). An empty store gives S2M_OK with S2M_LOOP_NONE records. *n_out holds the number
 *       of records; cap below it gives S2M_ERR_CAPACITY after writing cap records. */
#define S2M_LOOP_MAX_CANDIDATES  8
int  s2m_loop_verify_check_args(int32_t n_stored, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key,
                                const s2m_loop_params* p /* NULL = defaults */);
int  s2m_loop_verify_launch(s2m_handle h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key,
                            const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* early /* n_cand records */, int32_t* best);
int  s2m_loop_verify_poll(s2m_handle h, s2m_loop_result* out, int32_t cap, int32_t* n_out, int32_t* best);      /* never waits */
int  s2m_loop_verify_collect(s2m_handle h, s2m_loop_result* out, int32_t cap, int32_t* n_out, int32_t* best);   /* waits */
int  s2m_loop_verify(s2m_handle h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key,
                     const s2m_loop_params* p /* NULL = defaults */, s2m_loop_result* out /* n_cand records */, int32_t* best);

/* ---- Verification of many keys: the candidate rows of s2m_sc_query_keys in one call -------------------------------------
 * s2m_sc_query_keys names the loop candidates of a whole session; s2m_loop_verify_many verifies them. Row r is key_cur[r]
 * against key_pre[r * row_stride .. + n_cand[r]), 1 <= row_stride <= S2M_LOOP_MAX_CANDIDATES, 0 <= n_cand[r] <= row_stride:
 * the shape of that call's hits / n_hits. out (m * row_stride records) and best (m) are laid out alike.
 *   Contract: records, best[] and the container afterwards are byte for byte what this loop leaves on the same handle:
 *       for r: if n_cand[r]: s2m_loop_verify(h, key_cur[r], key_pre + r * row_stride, n_cand[r], base_key, p,
 *                                            out + r * row_stride, &best[r])
 *       - S2M_LOOP_ALREADY_CLOSED for a key_cur the container held before the call, S2M_LOOP_TOO_FEW_POINTS per candidate
 *       or per row, the pose result from the store's poses; only each row's winner enters the container. A row with
 *       n_cand[r] == 0 writes no record and gives best[r] = -1; records behind n_cand[r] are left as the caller had them.
 *   Passes: consecutive rows are taken while the sum of their n_cand stays within S2M_LOOP_MANY_MAX_PAIRS; a row is never
 *       split, and the plan depends on the arguments alone. Within a pass the submaps of every row are built by the single
 *       call's path (one wait each) into buffers that hold them all, then every pair the gates left open is aligned in
 *       lockstep by the device loop (the pairs' descriptions in a table in device memory, one wait per range of
 *       iterations), then the rows are judged. The call is synchronous; a caller bounds the time it holds the handle by
 *       the rows it passes per call. There is no launched form.
 *   key_cur must be distinct over the rows that have candidates (the rows must not depend on one another's results): a
 *       repeat is S2M_ERR_INVALID_ARG, and so are m < 0, null arrays with m > 0, row_stride or n_cand[r] out of range and
 *       everything s2m_loop_verify rejects in a row - all before any device work, with out, best and the container
 *       untouched. s2m_loop_verify_many_check_args gives the same verdict from the store's size alone (host code).
 *       m == 0 is S2M_OK and writes nothing; an empty store gives S2M_LOOP_NONE records and best -1.
 *   S2M_ERR_BUSY, nothing touched, while a launched closure or verification is pending.
 *   A HIP error in pass k fails the call as s2m_loop_verify fails: the rows of the passes before keep their records and
 *       their winners stay in the container; the records of pass k and of later rows are S2M_LOOP_NONE with key_cur -1. */
#define S2M_LOOP_MANY_MAX_PAIRS  64
int  s2m_loop_verify_many_check_args(int32_t n_stored, const int32_t* key_cur, const int32_t* key_pre, const int32_t* n_cand,
                                     int32_t m, int32_t row_stride, int32_t base_key, const s2m_loop_params* p);   /* host only */
int  s2m_loop_verify_many(s2m_handle h, const int32_t* key_cur /* m */, const int32_t* key_pre /* m * row_stride */,
                          const int32_t* n_cand /* m */, int32_t m, int32_t row_stride, int32_t base_key,
                          const s2m_loop_params* p /* NULL = defaults */,
                          s2m_loop_result* out /* m * row_stride */, int32_t* best /* m */);

/* ---- Loop candidates by position, for many keys: detectLoopClosureDistance (:732-765) for any stored keys ---------------
 * s2m_loop_closure_rs detects for key N-1 alone, its first candidate only, and aligns at once. s2m_loop_detect_keys is that
 * detection on its own for m stored keys against the store, top_k candidates per key, in the row shape
 * s2m_loop_verify_many takes with base_key = -1 (key_cur = keys, row_stride = top_k, key_pre, n_cand). After a
 * s2m_session_load, a s2m_session_place or a s2m_pg_optimize the poses have just been made consistent: the keys that now
 * lie within the radius of older keys are the loops that densify the graph.
 *   Distance: d2(c, q) of the stored positions of keys c and q, ((dx*dx + dy*dy) + dz*dz) in fp32 without contraction - the
 *       statement of s2m_loop_closure_rs and s2m_extract_surrounding.
 *   Candidate: key c is a candidate of query i when c is in the searched set, d2(c, keys[i]) < (float)(R*R) with R*R formed
 *       in float as s2m_loop_closure_rs forms it, and fabs(t[c] - T_i) > (double)time_diff_s, where T_i = time_cur[i] if
 *       time_cur is given and t[keys[i]] otherwise. A NaN on either side of a comparison fails it.
 *   Searched set of query i: c in [first, first + count) (count = -1: to the end of the store), outside
 *       [exclude_lo, exclude_hi) and outside [keys[i] + rel_lo, keys[i] + rel_hi), the sums in 64 bits; a window with
 *       lo >= hi leaves nothing out.
 *   The query key itself is not left out by name. With the stored times the time gate leaves it out for every
 *       time_diff_s >= 0 (|0| > W is false); with an external time_cur it can appear in its own row, as it can in the
 *       reference's radius result.
 *   Row i: the first top_k candidates in ascending (bits of d2, key) order in key_pre[i * top_k ..] and d2[i * top_k ..]
 *       (d2 may be NULL), their number in n_cand[i]; the entries behind n_cand[i] stay as the caller had them. keys may
 *       repeat and come in any order; a row depends on its own query alone, and is bit for bit the same however the work is
 *       cut into tiles, store splits and passes.
 *   The detector: keys = {N-1}, time_cur = {timeLaserInfoCur}, top_k = 1 and the whole store give the row of the detection
 *       inside s2m_loop_closure_rs: that call reports S2M_LOOP_NONE exactly when the row is empty or holds N-1, and otherwise
 *       its key_pre is key_pre[0].
 *   Read-only, with buffers of its own: nothing of the key store, the loop container, the voxel workspace, the scan or the
 *       map is touched. It runs on the handle's stream and works beside a pending launched closure, a pending verification
 *       and a pending optimise: it never returns S2M_ERR_BUSY.
 *   Passes: the queries go through in passes of at most 64 MiB of device memory, whatever m and N are, with one wait per
 *       pass; the plan depends on the arguments alone.
 *   S2M_ERR_INVALID_ARG, outputs untouched: a null handle; m < 0; null keys, key_pre or n_cand with m > 0; a key outside
 *       [0, N); a time_cur[i] that is not finite; top_k outside 1 .. S2M_LOOP_MAX_CANDIDATES; reserved != 0; first < 0,
 *       count < -1 or a range past the store; a radius or time difference that s2m_loop_params would reject.
 *       s2m_loop_detect_keys_check_args gives the same verdict from the store's size alone (host code, no handle; the values
 *       of time_cur and the outputs are the call's own checks).
 *   S2M_OK without work: m == 0 writes nothing; an empty searched range gives n_cand[i] = 0, and so does an empty store,
 *       which holds no key for a query to be outside of (its keys are not looked at). */
typedef struct s2m_loop_detect_params {
    float   search_radius;           /* historyKeyframeSearchRadius   10.0  include/utility.h:245; range as s2m_loop_params */
    float   time_diff_s;             /* historyKeyframeSearchTimeDiff 30.0  include/utility.h:246; range as s2m_loop_params */
    int32_t first, count;            /* searched keys [first, first+count); count = -1: to the end of the store */
    int32_t exclude_lo, exclude_hi;  /* fixed window left out; lo >= hi: none */
    int32_t rel_lo, rel_hi;          /* ALSO leave out c with key + rel_lo <= c < key + rel_hi (sums in 64 bits); lo >= hi: none */
    int32_t top_k;                   /* 1 .. S2M_LOOP_MAX_CANDIDATES; default 1 */
    int32_t reserved;                /* 0 */
} s2m_loop_detect_params;
int  s2m_loop_detect_default_params(s2m_loop_detect_params* p);
int  s2m_loop_detect_keys_check_args(int32_t n_stored, const int32_t* keys, int32_t m, int has_time_cur,
                                     const s2m_loop_detect_params* p /* NULL = defaults */);   /* host only, no handle */
int  s2m_loop_detect_keys(s2m_handle h, const int32_t* keys /* m */, const double* time_cur /* m, or NULL */, int32_t m,
                          const s2m_loop_detect_params* p /* NULL = defaults */,
                          int32_t* key_pre /* m * top_k */, float* d2 /* m * top_k, may be NULL */, int32_t* n_cand /* m */);

/* ---- Relocalisation: where in the stored map is this scan, as a pose ------------------------------------------------
 * From a fresh scan (not a key) to a pose in the map frame, so that s2m_extract_surrounding_at and s2m_optimize* can start
 * or recover inside a map the handle already holds. ScanContext key i must be key-frame i (both stores filled in step).
 *   1. Query: the scan's descriptor against the descriptor store exactly as s2m_sc_query_scan(p->query) - the hits are
 *      bit for bit that call's. No hits: S2M_OK, *n_out = 0, *best = -1. A hit key >= s2m_kf_size: S2M_ERR_INVALID_ARG.
 *   2. Source: the scan in its own frame through the VoxelGrid at loop.icp_leaf, once, into the loop's source buffer
 *      (scan_ds, which S2M_KF_FROM_LAST_DOWNSAMPLE reads, is not touched). n_src < 300: every record
 *      S2M_LOOP_TOO_FEW_POINTS.
 *   3. Target per hit: loopFindNearKeyframes(hit.key, search_num, -1) at icp_leaf, in the map frame. n_tgt < 1000: that
 *      record is S2M_LOOP_TOO_FEW_POINTS and takes no slot.
 *   4. Guess per hit: G = T(pose[key]) * Rz(-yaw_diff_rad) (use_yaw = 0: G = T(pose[key])), T the key's stored 3x4, the
 *      product in float, each entry ((a0 b0 + a1 b1) + a2 b2). The sign: the descriptor's sector index grows with
 *      atan2(y, x), and a query that is the candidate's cloud turned by +12 degrees about z matches at shift 2, so a
 *      query point is about Rz(+yaw) * candidate point and the way back into the key's frame is Rz(-yaw).
 *   5. Alignment: the remaining hits through the slotted device loop in lockstep - one source, one target and one guess
 *      per slot - with the loop's ICP settings (max correspondence distance (double)(search_radius * 2.0f), 100
 *      iterations, 1e-6 / 1e-6). Record i's icp is byte for byte s2m_icp_align_guess(source, target i, guess i).
 *      The call waits for the result.
 *   6. Judgement: !converged or fitness_score > (double)loop.fitness_score gives S2M_LOOP_REJECTED, otherwise
 *      S2M_LOOP_ACCEPTED with both pose forms. *best: the accepted record with the least (fitness_score, position), or
 *      -1, as s2m_loop_verify chooses. Records are in the query's order: descriptor distance ranks places, it does not
 *      verify them (a mirror place of a symmetric scene can rank first and still pass the gate), so the top hits are
 *      aligned and the fitness decides.
 * Read-only: the loop-index container, both stores, the detector's state, the installed map and its index, the scan
 * (scan_ds included), the pose, the batch and stream slots stay as they were; the next registration and the next
 * s2m_sc_detect_loop are bit for bit what they would be without the call. It uses the loop's buffers: with a launched
 * closure or verification pending it returns S2M_ERR_BUSY and touches nothing.
 * Errors (S2M_ERR_INVALID_ARG): a null handle or null outputs; top_k outside 1 .. S2M_LOOP_MAX_CANDIDATES; a query the
 * s2m_sc_query_* argument table rejects; loop parameters s2m_loop_* reject. n == 0: S2M_OK with no records.
 * s2m_relocalize_check_args gives the same verdict from the two store sizes alone (host code, no handle). */
typedef struct s2m_reloc_params {
    s2m_sc_query_params query;   /* top_k 1 .. S2M_LOOP_MAX_CANDIDATES; defaults as s2m_sc_query_default_params but top_k 4, S2M_SC_ALIGN_FULL */
    s2m_loop_params     loop;    /* search_radius (max correspondence distance = 2x, as the loop), search_num, fitness_score, icp_leaf; time_diff_s unused */
    int32_t             use_yaw; /* 1 (default): guess = T(pose[key]) * Rz(-yaw_diff_rad);  0: guess = T(pose[key]) */
    int32_t             reserved;
} s2m_reloc_params;
typedef struct s2m_reloc_candidate {
    s2m_sc_hit     hit;          /* as s2m_sc_query_scan returns it */
    int32_t        status;       /* S2M_LOOP_TOO_FEW_POINTS / REJECTED / ACCEPTED */
    int32_t        n_src, n_tgt;
    float          guess[16];    /* the guess the alignment started from */
    s2m_icp_result icp;          /* T maps the scan's frame into the map frame (guess included); valid when ICP ran */
    float          pose_xyzrpy[6];       /* getTranslationAndEulerAngles(icp.T), accepted records */
    float          pose_tobemapped[6];   /* the same as {roll, pitch, yaw, x, y, z}: what s2m_optimize* takes */
} s2m_reloc_candidate;
int  s2m_reloc_default_params(s2m_reloc_params* p);
int  s2m_relocalize_check_args(int32_t n_sc, int32_t n_kf, const s2m_reloc_params* p);   /* host only, no handle */
int  s2m_relocalize_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, int on_device,
                         const s2m_reloc_params* p /* NULL = defaults */,
                         s2m_reloc_candidate* out /* top_k records */, int32_t* n_out, int32_t* best);
/* s2m_relocalize_scan for a key the store already holds: "where is key k of an appended, still unplaced session in the
 * rest of the map". The query is the key's stored descriptor, as s2m_sc_query_key(p->query); the source is the key's own
 * records in its own frame, read straight from the store on the device through the VoxelGrid at loop.icp_leaf. The target
 * submap of a hit is loopFindNearKeyframes(hit.key, search_num, -1) with its neighbours CLAMPED to the searched range
 * [query.first, query.first + query.count) of the query: a submap at the boundary never takes keys of the other session.
 * Guess, lockstep alignment, gates, records and *best are steps 4 to 6 above; with descriptors that were made from the stored
 * clouds and a range that holds every hit's neighbours the records are byte for byte s2m_relocalize_scan of the key's cloud.
 * Read-only; S2M_ERR_BUSY as there. A key outside the key-frame store, or without a descriptor: S2M_ERR_INVALID_ARG. A key
 * without records: S2M_OK with no records. */
int  s2m_relocalize_key(s2m_handle h, int32_t key, const s2m_reloc_params* p /* NULL = defaults */,
                        s2m_reloc_candidate* out /* top_k records */, int32_t* n_out, int32_t* best);

/* ---- Pose graph: factors, optimise, correct the key-frame store --------------------------------------------------
 * saveKeyFramesAndFactor() with addOdomFactor / addGPSFactor / addLoopFactor (reference src/mapOptmization.cpp:1386-1534)
 * and correctPoses() (:1611-1642) as a batch solve on the device. The graph lives in the handle beside the key-frame
 * store; variable i of the graph is key i of the store. Variables are dense: with N variables a call may name keys
 * 0..N, and key N creates variable N. Every variable needs an initial value before s2m_pg_optimize.
 *   State: (R_i, t_i) in fp64 on the device. Pose vectors {x, y, z, roll, pitch, yaw} convert as
 *       Rot3::RzRyRx(roll, pitch, yaw); read-out is roll = atan2(R21, R22), pitch = asin(-R20), yaw = atan2(R10, R00) in
 *       fp64, then rounded to float.
 *   Tangent and retraction: d = [w, v], rotation first (GTSAM's Pose3 order); R <- R Exp(w), t <- t + R v.
 *   Residuals [ext]: between, with E = Z^-1 X_i^-1 X_j: r = [Log_SO3(R_E), t_E]; prior, the same with E = P^-1 X;
 *       GPS: t_i - z. This is the first-order chart of a default GTSAM 4.0 build; a GTSAM built with POSE3_EXPMAP uses
 *       the full SE(3) logarithm and differs at second order in the residual.
 *   Weights: rows are whitened by 1 / sqrt(var) (var in tangent order: three rotation, three translation variances).
 *       robust_k > 0 makes the factor Cauchy: w = k^2 / (k^2 + |whitened r|^2), recomputed at every linearisation
 *       [ext]; its error term is k^2 / 2 log(1 + |whitened r|^2 / k^2), a plain factor's |whitened r|^2 / 2.
 *   Iteration: Gauss-Newton; a step is kept only if it lowers the error. The loop ends after max_iterations steps, at
 *       a step that does not lower the error (converged), or when a kept step lowered it by less than
 *       absolute_error_tol or by less than relative_error_tol times the error (converged).
 *   Linear solve: the chain prior(0), between(0,1), between(1,2), ... - the first prior on key 0 and, per i, the first
 *       between factor i -> i+1 with robust_k == 0 - is solved exactly in square-root form (its whitened Jacobian is
 *       never squared), every other factor enters through conjugate gradients preconditioned by that chain, with a
 *       device-side stop flag. A graph without such a chain over all its variables is S2M_ERR_INVALID_ARG from
 *       s2m_pg_optimize / s2m_pg_marginal (a disconnected variable, a missing prior on key 0), as is a variable
 *       without an initial value; the graph stays as it was.
 *   An empty graph optimises to S2M_OK with zero counts. A failed add leaves the graph as it was. Results are
 *   reproducible run to run: every sum is taken in a fixed order. Calls on a handle are not concurrent. */
typedef struct s2m_pg_params {
    double  prior_var[6];          /* {1e-2, 1e-2, pi*pi, 1e8, 1e8, 1e8}  :1390 (rad^2 x3, m^2 x3) */
    double  odom_var[6];           /* {1e-6 x3, 1e-4 x3}                  :1394 */
    double  sc_loop_var[6];        /* 0.5 x6                              :712-713 */
    double  sc_loop_robust_k;      /* Cauchy k = 1                        :716-719 */
    double  relative_error_tol;    /* 1e-5 */
    double  absolute_error_tol;    /* 1e-5 */
    double  cg_rel_tol;            /* 1e-13: the inner solve ends at |residual| <= cg_rel_tol |right-hand side| */
    int32_t max_iterations;        /* 100 */
    int32_t cg_max_iterations;     /* 0: six per factor off the chain, plus 20 */
} s2m_pg_params;
typedef struct s2m_pg_result {
    int32_t iterations;            /* Gauss-Newton steps kept */
    int32_t inner_iterations;      /* CG iterations over all steps */
    int32_t converged;
    int32_t n_variables, n_factors;
    int32_t reserved;
    double  error_before, error_after;
    double  robust_weight_min;     /* smallest Cauchy weight at the final estimate (1 without robust factors) */
} s2m_pg_result;
#define S2M_PG_PRIOR    0
#define S2M_PG_BETWEEN  1
#define S2M_PG_GPS      2
#define S2M_PG_INITIAL  3
int  s2m_pg_default_params(s2m_pg_params* p);
/* The argument checks of the add calls on their own (host code, no handle, no GPU): S2M_OK or S2M_ERR_INVALID_ARG.
 * kind is S2M_PG_*; n_variables the graph's current variable count; key_b is read for S2M_PG_BETWEEN only; values are
 * 6 floats (3 for S2M_PG_GPS), var 6 doubles (3 for S2M_PG_GPS, not read for S2M_PG_INITIAL). Rejected: null pointers,
 * non-finite values, variances that are not positive and finite, a negative or non-finite robust_k, negative keys, a
 * key above n_variables or two new keys at once (a gap), key_a == key_b (a self loop). */
int  s2m_pg_check_args(int32_t kind, int32_t n_variables, int32_t key_a, int32_t key_b, const float* values, const double* var,
                       double robust_k);
int  s2m_pg_reset(s2m_handle h);
int  s2m_pg_size(s2m_handle h, int32_t* n_variables, int32_t* n_factors);
int  s2m_pg_add_prior(s2m_handle h, int32_t key, const float pose_xyzrpy[6], const double var[6]);
int  s2m_pg_add_between(s2m_handle h, int32_t key_from, int32_t key_to, const float rel_xyzrpy[6], const double var[6], double robust_k);
int  s2m_pg_add_gps(s2m_handle h, int32_t key, const float xyz[3], const double var[3]);
int  s2m_pg_set_initial(s2m_handle h, int32_t key, const float pose_xyzrpy[6]);
/* addOdomFactor() (:1386-1400): on an empty graph the prior (prior_var) and initial value of key 0; otherwise the
 * between factor (odom_var) from the last variable's current estimate, in fp64, to `pose`, and the new variable's
 * initial value. The variances are those of s2m_pg_default_params. */
int  s2m_pg_add_odometry(s2m_handle h, const float pose_xyzrpy[6]);
int  s2m_pg_optimize(s2m_handle h, const s2m_pg_params* p /* NULL = defaults */, s2m_pg_result* out /* may be NULL */);
/* The optimise beside the scan handler: launch, poll, collect. s2m_pg_optimize stays as it is and is the yardstick.
 *   s2m_pg_optimize_launch does everything s2m_pg_optimize does before its first kernel (parameter, chain and initial-value
 *       checks, uploads, device tables); every error is the synchronous call's, with nothing pending and the graph as it was.
 *       An empty graph returns S2M_OK with the synchronous result in `early` and nothing pending. Otherwise the solve is
 *       queued on a stream of the handle's own - the lowest priority the device offers, never the priority of the handle's
 *       stream; it may share a hardware queue with the loop-closure stream - behind the launch's uploads, and the call returns
 *       S2M_PG_PENDING without waiting: `early` holds n_variables, n_factors, robust_weight_min = 1 and zeros elsewhere. The
 *       pending solve is over the N_l variables and F_l factors of that moment. The launch brings the library's host mirror of
 *       the estimates up to date first; no later call reads the device's estimates while the solve runs.
 *   s2m_pg_optimize_poll never waits for the device: it tests an event. While the queued work runs it returns S2M_PG_PENDING
 *       and does not write *out. The Gauss-Newton loop's decisions (keep or reject a step, the two convergence tests, the
 *       counts) are taken on the device and the solve is queued a range at a time; a poll that finds a range ended and the
 *       solve not, queues the next range and returns S2M_PG_PENDING. The poll that finds the solve ended delivers the result
 *       once: S2M_OK with *out bytewise what s2m_pg_optimize returns for the same graph, estimates and params, and the device
 *       estimates of variables 0..N_l-1 bit for bit what it leaves. After that, and whenever nothing is pending: S2M_PG_IDLE,
 *       *out not written.
 *   s2m_pg_optimize_collect is the same with waits: S2M_OK with the final result, or S2M_PG_IDLE.
 *   While an optimise is pending: s2m_pg_size, s2m_pg_add_odometry (it chains on the launch-time estimate of the last
 *       variable), s2m_pg_add_prior / _between / _gps on any keys (the new factors are not part of the pending solve) and
 *       s2m_pg_set_initial for keys >= N_l work on host state and do not wait. s2m_pg_optimize, a second launch,
 *       s2m_pg_get_poses, s2m_pg_marginal, s2m_pg_marginals, s2m_pg_joint_marginal, s2m_pg_apply_to_store and
 *       s2m_pg_set_initial for a key < N_l return S2M_ERR_BUSY and touch nothing. s2m_pg_reset and s2m_destroy wait for the
 *       stream and drop the pending solve. Every call outside s2m_pg_* works as before and returns the bits it returns
 *       without a pending optimise (a launched loop closure may be pending at the same time); a call that has to grow a
 *       device buffer may wait for the solve.
 *   The tail: when the result is delivered with iterations > 0 (and only then), every variable k >= N_l that has a value is
 *       re-based on the host in fp64 by the correction of variable a = N_l - 1: with A its launch-time state and A' its
 *       state after the solve, D_R = A'_R A_R^T, D_t = A'_t - D_R A_t, X_R <- D_R X_R, X_t <- D_R X_t + D_t
 *       (s2m_debug_pg_rebase in liorf_s2m_debug.h is this rule). With only odometry factors added meanwhile that is the exact
 *       optimum of the grown graph; with loops or GPS added meanwhile it is the next optimise's initial value. */
#define S2M_PG_PENDING 2   /* positive, like S2M_WARN_LEAF_TOO_SMALL: an optimise is queued or running */
#define S2M_PG_IDLE    3   /* poll / collect with nothing pending; *out is not written */
int  s2m_pg_optimize_launch(s2m_handle h, const s2m_pg_params* p /* NULL = defaults */, s2m_pg_result* early /* may be NULL */);
int  s2m_pg_optimize_poll(s2m_handle h, s2m_pg_result* out);      /* never waits for the device */
int  s2m_pg_optimize_collect(s2m_handle h, s2m_pg_result* out);   /* waits */
/* The current estimates of variables first .. first+count-1 as floats; S2M_ERR_INVALID_ARG outside the graph or for a
 * variable of that range without a value. */
int  s2m_pg_get_poses(s2m_handle h, int32_t first, int32_t count, float* xyzrpy);
/* poseCovariance (:1565): the marginal covariance of `key` at the current estimates, row-major 6x6 in the tangent
 * order of rotation then translation, with the robust weights of those estimates. */
int  s2m_pg_marginal(s2m_handle h, int32_t key, double cov[36]);
/* Marginals of many keys, and the joint marginal of two, by a block solve: the six columns of every key's block are
 * right-hand sides that advance in lockstep through shared launches, S2M_PG_BLOCK_COLUMNS of them per pass, each bit for
 * bit what s2m_pg_marginal computes for it. One linearisation per call; per pass one copy of the wanted rows back.
 * Errors and chain requirements are those of s2m_pg_marginal; the graph is not changed.
 *   s2m_pg_marginals_check_args: the key list's checks on their own (host code, no handle, no GPU): S2M_OK, or
 *       S2M_ERR_INVALID_ARG for null keys with n_keys > 0, n_keys < 0, or a key outside 0..n_variables-1.
 *   s2m_pg_marginals: cov is n_keys x 36, block k the marginal of keys[k] in s2m_pg_marginal's layout and order. Keys may
 *       repeat; n_keys == 0 is S2M_OK.
 *   s2m_pg_joint_marginal: row-major 12x12 over [key_a's tangent, key_b's tangent]; block (r, c) holds the rows of key r in
 *       the columns solved for key c, so the diagonal blocks are s2m_pg_marginal's. Not symmetrised: cov[:6, 6:] and the
 *       transpose of cov[6:, :6] agree to the solve's accuracy. key_a == key_b is S2M_ERR_INVALID_ARG. */
#define S2M_PG_BLOCK_COLUMNS 24
int  s2m_pg_marginals_check_args(int32_t n_variables, const int32_t* keys, int32_t n_keys);
int  s2m_pg_marginals(s2m_handle h, const int32_t* keys, int32_t n_keys, double* cov);
int  s2m_pg_joint_marginal(s2m_handle h, int32_t key_a, int32_t key_b, double cov[144]);
/* correctPoses() (:1611-1642): the estimates of variables first .. first+count-1 become the poses of the same keys of
 * the key-frame store, computed and written on the device: the float pose vector of s2m_pg_get_poses, the position, and
 * each key's cached transform with the host libm's sinf / cosf restated on the device, so that the store ends up bit for
 * bit what s2m_kf_set_poses makes of s2m_pg_get_poses' floats. One copy brings the new poses and transforms back to the
 * library's host mirror of the store; nothing is uploaded. The range must lie inside both the graph and the store and
 * every variable in it needs a value (S2M_ERR_INVALID_ARG); an estimate that is not finite is S2M_ERR_INVALID_ARG and
 * leaves the store as it was. */
int  s2m_pg_apply_to_store(s2m_handle h, int32_t first, int32_t count);
/* The mutually consistent loops among many candidates, before any of them enters the graph.
 * key_from, key_to and rel_xyzrpy are what the caller would give s2m_pg_add_between: candidate p claims
 * Z_p = X_from^-1 X_to. Two candidates are consistent if the cycle they close through the current estimates returns to
 * the identity within a tolerance that grows with the length of chain the cycle runs over; the call returns a large set
 * of candidates that are consistent pair by pair. It is a heuristic with a fixed rule, stated below - NOT the maximum
 * clique, which it can miss. The four default tolerances are a starting point that has not been measured on real data.
 *   State read: the graph's current estimates (R row-major then t, fp64). Nothing is added to the graph, no estimate
 *       changes, and the call writes only device buffers of its own.
 *   Measurements: every rel_xyzrpy becomes (R, t) in fp64 on the host exactly as s2m_pg_add_between converts it.
 *   Chain length, in integers: step[0] = 0, step[k] = llrint(1e6 * sqrt(((dx*dx + dy*dy) + dz*dz))) of the translation
 *       difference of estimates k-1 and k (micrometres; a step of 2.5e11 or more, or one that is not finite, counts as
 *       2.5e11, so that the sum over 2^24 keys fits); s[k] their inclusive prefix sum in int64, recomputed in every
 *       call. For a pair (p, q): L = (double)(|s[from_p] - s[from_q]| + |s[to_p] - s[to_q]|) * 1e-6 metres.
 *   Pair measure, for a < b in the caller's order, SE(3) products in fp64 without fused multiply-add: O_t = X_to_a^-1 X_to_b,
 *       O_f = X_from_a^-1 X_from_b, M1 = Z_a O_t, M2 = O_f Z_b, D = M1^-1 M2. Every 3x3 entry is ((a0*b0 + a1*b1) + a2*b2),
 *       every inverse (R^T, -(R^T t)), every translation of a product (R t') + t in that association.
 *       rho2 = ((3 - R_D00) - R_D11) - R_D22 (the squared chord 4 sin^2(angle / 2)), d2 = (tx*tx + ty*ty) + tz*tz of D.
 *       The pair is consistent iff rho2 <= (tol_chord + rate_chord*L)^2 and d2 <= (tol_m + rate_m*L)^2.
 *   Matrix: bit q % 64 of word p * ((m + 63) / 64) + q / 64 is the pair (p, q). (q, p) is the pair (p, q), evaluated with the
 *       operands in candidate order, so the matrix is symmetric; the diagonal is 0; a measure that is not finite is not
 *       consistent; the bits of a row's last word behind m are 0. degree[p] is the number of set bits of row p.
 *   Selection: rank the candidates by (degree descending, index ascending). From every start v grow S = {v}, C = row(v);
 *       while C is not empty take its best-ranked member u, add it to S and set C &= row(u). The result is the largest S,
 *       equal sizes going to the best-ranked start: selected[p] = 1 for its members, n_selected, and start = v. With m == 1
 *       the one candidate is selected. The result is a fixed function of the inputs, bit for bit, run to run.
 *   S2M_ERR_BUSY, nothing touched, while a launched optimise is pending (it writes the estimates); a pending loop closure
 *       or verification does not matter.
 *   S2M_ERR_INVALID_ARG, outputs untouched: a null handle; m < 0 or m > S2M_PG_CONSISTENCY_MAX; null key_from, key_to,
 *       rel_xyzrpy or selected with m > 0; a key outside [0, n_variables) or key_from == key_to; a rel_xyzrpy that is not
 *       finite; a tolerance or rate that is negative or not finite; nonzero reserved; a variable of the graph without an
 *       initial value. m == 0 is S2M_OK with zero counts (start = -1).
 *   s2m_pg_consistency_check_args: the checks of the arrays and params on their own (host code, no handle, no GPU). */
#define S2M_PG_CONSISTENCY_MAX 4096          /* candidates per call; 64 words of 64 bits per row */
typedef struct s2m_pg_consistency_params {
    double  tol_m;       /* translation tolerance at zero chain length, metres              0.3    */
    double  tol_chord;   /* rotation tolerance at zero chain length, as a chord 2 sin(a/2)  0.03   */
    double  rate_m;      /* metres of tolerance per metre of chain travelled                0.02   */
    double  rate_chord;  /* chord per metre of chain travelled                              0.0005 */
    int32_t reserved[4]; /* 0 */
} s2m_pg_consistency_params;
typedef struct s2m_pg_consistency_result {
    int32_t n_candidates, n_selected;
    int32_t start;          /* the candidate the winning set was grown from */
    int32_t reserved;
    int64_t n_consistent_pairs;   /* set bits of the matrix / 2 */
} s2m_pg_consistency_result;
int  s2m_pg_consistency_default_params(s2m_pg_consistency_params* p);
int  s2m_pg_consistency_check_args(int32_t n_variables, const int32_t* key_from, const int32_t* key_to, const float* rel_xyzrpy,
                                   int32_t m, const s2m_pg_consistency_params* p /* NULL = defaults */);
int  s2m_pg_consistent_loops(s2m_handle h, const int32_t* key_from, const int32_t* key_to, const float* rel_xyzrpy /* m * 6 */,
                             int32_t m, const s2m_pg_consistency_params* p /* NULL = defaults */,
                             uint8_t* selected /* m: 1 = in the set */, int32_t* degree /* m, may be NULL */,
                             uint64_t* matrix /* m * ((m + 63) / 64) words, may be NULL */, s2m_pg_consistency_result* out /* may be NULL */);

/* ---- Saving and loading a session ---------------------------------------------------------------------------
 * One little-endian byte stream (format version 1) holds the primary state of a handle: the key-frame
 * store (pose, time, point count and the 32-byte records of every key, all eight words as they are stored), the ScanContext
 * store (the fp64 descriptors, n_search and the detector's call counter), the loop container's (key_cur, key_pre) pairs and the
 * pose graph (the factors in the order they were added, the fp64 estimates, which variables have a value). Not in it:
 * parameters, the installed map, the scan, scan_ds and cloud_deskewed, anything pending, caller-owned state such as
 * s2m_guess_state, and everything derived - key transforms, device positions, ring and sector keys, the pose graph's device
 * tables - which a load rebuilds by the paths the per-key calls use, so that after a successful load the handle answers every
 * call of this ABI bit for bit as the handle that saved did at that moment, and s2m_kf_add / s2m_sc_add_* / s2m_pg_add_*
 * continue from there.
 * The stream is a fixed header (magic, version, all counts, every section's byte size), six sections and a footer with a
 * checksum per section and one over header and footer. The checksum - two 64-bit sums over 32-bit words, computed on the
 * device while it moves the bytes - is an integrity check against truncation and corruption, NOT a security measure: do not
 * load a file from a source you do not trust on the strength of it.
 * The bulk (records, descriptors) never passes through host code: device -> pinned chunk -> callback, and back; the device packs
 * chunk k+1 while the callback has chunk k.
 *   s2m_session_write_fn / s2m_session_read_fn: called in stream order with chunks of any size; 0 = ok. A write callback's
 *       `data`, and a read callback's, are valid during the call only. Any other return ends the call with S2M_ERR_IO, except
 *       that a read callback may return S2M_ERR_FORMAT for "the stream has ended", which is passed on.
 *   s2m_session_info_of: what a save would write now (host only; fields of a pending launch are not waited for).
 *   s2m_session_save reads only. It first brings the library's host mirror of the estimates up to date where the device's
 *       are newer, as s2m_pg_get_poses does. S2M_ERR_BUSY while a launched loop closure or verification or a launched
 *       pose-graph optimise is pending. The bytes do not depend on the chunk size or on how the callback is called.
 *   s2m_session_load needs the key-frame store, the ScanContext store, the loop container and the pose graph EMPTY:
 *       otherwise S2M_ERR_INVALID_ARG, nothing touched - s2m_kf_reset, s2m_sc_reset and s2m_pg_reset first. S2M_ERR_BUSY as
 *       for a save. A load that fails at ANY point - a callback, a checksum, the content, a HIP error - leaves all four
 *       empty again, never half filled. It reports the first failure in stream order: content it cannot use as it arrives
 *       (S2M_ERR_FORMAT), then the checksums at the footer (S2M_ERR_CHECKSUM).
 *   s2m_session_save_file / s2m_session_load_file: the two above on a file (a file that ends early is S2M_ERR_FORMAT).
 *   s2m_session_check: a whole blob in memory, without a handle or a device: the structure (magic, version, the byte count;
 *       S2M_ERR_FORMAT), then every checksum, the header's first (S2M_ERR_CHECKSUM), then the content (S2M_ERR_FORMAT):
 *       section sizes that follow from the counts; at most 2^24 keys, descriptors and variables; point counts >= 0 that sum
 *       to the record section; finite poses and times; 0 <= n_search <= n, counter >= 0; loop pairs ascending in key_cur,
 *       both keys stored; every factor what s2m_pg_check_args accepts for a graph that holds its keys, with the rows of its
 *       type; and variables and values that the add calls can have produced in that factor order (a key is new only as the
 *       next variable, or it already holds a value). s2m_session_load checks the same. */
#define S2M_ERR_FORMAT        -7   /* session: bad magic, unknown version, truncated stream or inconsistent content */
#define S2M_ERR_CHECKSUM      -8   /* session: a section's or the header's checksum does not match                   */
#define S2M_ERR_IO            -9   /* session: a callback or a file call failed                                      */
#define S2M_SESSION_VERSION    1
typedef int (*s2m_session_write_fn)(void* user, const void* data, size_t bytes);   /* 0 = ok */
typedef int (*s2m_session_read_fn)(void* user, void* data, size_t bytes);          /* 0 = ok, fills exactly `bytes` */
typedef struct s2m_session_info {
    uint32_t version;
    int32_t  n_keys, n_descriptors, n_loop_pairs, n_variables, n_factors;
    uint64_t n_points, bytes;
} s2m_session_info;
int  s2m_session_info_of(s2m_handle h, s2m_session_info* out);
int  s2m_session_save(s2m_handle h, s2m_session_write_fn w, void* user);
int  s2m_session_load(s2m_handle h, s2m_session_read_fn r, void* user, s2m_session_info* out /* may be NULL */);
int  s2m_session_save_file(s2m_handle h, const char* path);
int  s2m_session_load_file(s2m_handle h, const char* path, s2m_session_info* out /* may be NULL */);
int  s2m_session_check(const void* blob, size_t bytes, s2m_session_info* out /* may be NULL */);

/* ---- Appending a saved session behind the stored keys, and placing it -----------------
 * With N0 keys in the handle (session A), a blob of session B (format version 1, unchanged) becomes keys N0 .. N0+nK-1.
 * A "state" is 12 doubles {R row-major, t}; the state of a float pose is Rot3::RzRyRx of it in fp64 with libm, as
 * s2m_pg_set_initial makes it; A o X is R' = A_R R, t' = A_R t + A_t, every entry ((a0 b0 + a1 b1) + a2 b2) in fp64 without
 * contraction, the translation that sum plus A_t.
 *   s2m_session_append: anchor_xyzrpy NULL = "as stored": nothing is composed, every pose and estimate keeps its bits (an
 *       identity anchor is not the same: it would turn -0.0 into +0.0). Otherwise A = the state of the anchor, and
 *         - a key's store pose becomes the float read-out (s2m_pg_get_poses' rule) of A o state(stored pose), its position
 *           record and cached transform follow from those floats as s2m_pg_apply_to_store makes them;
 *         - an estimate X becomes A o X; a prior's state P becomes A o P; a GPS factor's z becomes A_R z + A_t with its
 *           variances as stored - the diagonal covariance is NOT rotated; a between factor is unchanged.
 *       Times, point counts and records are kept as stored, byte for byte, in arena space behind A's keys, so the next
 *       s2m_kf_add continues as after nK adds. Descriptors go behind the store's own; n_search and the detector's counter
 *       stay the handle's. A stored loop pair (cur, pre) becomes (cur + N0, pre + N0). Factors keep their order with keys
 *       + N0, behind one new factor, the junction: between(N0-1 -> N0), robust_k 0, variances junction_var (NULL: 1.0 for
 *       all six - loose beside an odometry or loop factor), measured X[N0-1]^-1 o X'[N0] at the appended estimates, so its
 *       residual there is rounding-sized. It gives the merged graph the odometry chain s2m_pg_optimize needs.
 *       Preconditions, judged from the blob's header alone (S2M_ERR_INVALID_ARG, nothing touched): N0 >= 1 (an empty handle
 *       is s2m_session_load's); N0 + nK <= 2^24; with descriptors in the blob s2m_sc_size == N0 and nD <= nK; with variables
 *       in the blob the graph holds exactly N0 variables and nV <= nK; a finite anchor; positive finite variances.
 *       s2m_session_append_check_args gives that verdict from two s2m_session_info on the host, without a handle.
 *       S2M_ERR_BUSY exactly when save and load return it. B's variable 0 or A's variable N0-1 without a value is
 *       S2M_ERR_INVALID_ARG, found when the variables have arrived; a placed result that is not finite likewise.
 *       A failure at ANY point - a callback, an early end, a checksum, the content, a HIP error, the two late checks - leaves
 *       all four containers exactly as they were before the call (not emptied), arena blocks taken by the call released.
 *       Status codes and their order are s2m_session_load's. info_out (may be NULL): what the blob holds, the first new key
 *       and the junction's index in the factor list (-1: the blob has no variables).
 *   s2m_session_place: moves the session appended last by D = the state of move_xyzrpy: X <- D o X for its variables, its
 *       store poses likewise, priors and GPS factors of its keys as above, the junction measured again at the new estimates.
 *       Keys added after the append are not moved. One kernel launch (k_session_place) and one wait. Append with anchor A is,
 *       byte for byte, append with NULL followed by s2m_session_place(A). No appended session: S2M_ERR_INVALID_ARG; anything
 *       pending: S2M_ERR_BUSY; a result that is not finite: S2M_ERR_INVALID_ARG, handle as before.
 *   s2m_session_appended: the key range [first, first + count) of the session appended last, -1 and 0 when there is none:
 *       s2m_kf_reset, s2m_pg_reset and s2m_session_load forget it.
 *   s2m_session_anchor_from_pairs: host only, fp64, libm, no handle. Pair i (a pose of session B in B's frame, the same
 *       pose in the map's frame, both {x, y, z, roll, pitch, yaw}) gives A_i = state(map_i) o state(session_i)^-1. j supports
 *       i when |A_i.t - A_j.t| <= tol_m and acos(clamp((trace(A_i.R^T A_j.R) - 1) / 2)) <= tol_rad. anchor_out is the A_i
 *       with the most supporters (itself included; ties: the least summed translation distance to its supporters, then the
 *       lower index) read out as floats by s2m_pg_get_poses' rule. No averaging: one wrong pair must not bend the anchor.
 *       *n_inliers, *chosen (either may be NULL): its supporters and i. m <= 0, null arrays, tolerances that are negative
 *       or not finite, or inputs that are not finite: S2M_ERR_INVALID_ARG.
 * A merged handle keeps B's key times as they are (the recent-keys rule of s2m_extract_surrounding reads them so), and
 * index neighbourhoods cross the boundary: loop submaps around N0-1 / N0 take keys of the other session. */
typedef struct s2m_session_append_info {
    s2m_session_info blob;
    int32_t first_key, junction_factor;
} s2m_session_append_info;
int  s2m_session_append_check_args(const s2m_session_info* have, const s2m_session_info* blob_info, const float* anchor_xyzrpy /* NULL: as stored */,
                                   const double* junction_var /* NULL: 1.0 x 6 */);
int  s2m_session_append(s2m_handle h, s2m_session_read_fn r, void* user, const float* anchor_xyzrpy, const double* junction_var,
                        s2m_session_append_info* info_out /* may be NULL */);
int  s2m_session_append_file(s2m_handle h, const char* path, const float* anchor_xyzrpy, const double* junction_var,
                             s2m_session_append_info* info_out /* may be NULL */);
int  s2m_session_place(s2m_handle h, const float move_xyzrpy[6]);
int  s2m_session_appended(s2m_handle h, int32_t* first, int32_t* count);
int  s2m_session_anchor_from_pairs(const float* pose_in_session, const float* pose_in_map, int32_t m, double tol_m, double tol_rad,
                                   float anchor_out[6], int32_t* n_inliers, int32_t* chosen);

#ifdef __cplusplus
}
#endif
#endif /* LIORF_S2M_H */
