// s2m_voxel.hpp — device voxel-grid filter and cloud transform: the two stages that produce the
// inputs of the scan-to-map path.
//   downsampleCurrentScan()  reference src/mapOptmization.cpp:1061-1067   (VoxelGrid, leaf 0.4)
//   extractCloud()           reference src/mapOptmization.cpp:1014-1039   (transformPointCloud of
//                            the chosen key frames :310-329, concatenation, VoxelGrid, leaf 0.4-0.5)
// Implemented in s2m_voxel.hip (own translation unit; the stable radix sort of the (voxel, point) pairs is hand-written there).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace s2m {

struct VoxWorkspace;                       // grow-only device scratch of the filter

VoxWorkspace* vox_create();
void          vox_destroy(VoxWorkspace* w);

struct VoxResult {
    size_t n_out = 0;                      // voxels (records needed in `out`)
    int    leaf_too_small = 0;             // PCL's "Leaf size is too small" case: output = input
};

// pcl::VoxelGrid<PointXYZI>::applyFilter on device records (x, y, z at byte 0/4/8, intensity at
// byte 16 when stride >= 20). Writes min(n_out, cap) records {centroid xyz, 1.0f, mean intensity, 0...}
// in ascending voxel-index order and synchronises `stream` to return the count.
hipError_t vox_downsample(VoxWorkspace* w, hipStream_t stream, const unsigned char* d_in, size_t n, size_t stride,
                          float leaf, unsigned char* d_out, size_t out_stride, size_t cap, VoxResult* res);

// transformPointCloud (:310-329) of `n_frames` key-frame clouds: frame f is the device buffer h_src[f] holding
// h_offsets[f+1] - h_offsets[f] records and uses the row-major 3x4 transform h_T[12*f ..]; the transformed
// records are written back to back (the reference's `*laserCloudSurfFromMap += ...`) into d_out.
hipError_t vox_transform_frames(VoxWorkspace* w, hipStream_t stream, const unsigned char* const* h_src, size_t stride,
                                const int32_t* h_offsets, const float* h_T, int n_frames,
                                unsigned char* d_out, size_t out_stride);

// The same with the frame table already in device memory (src[f], offsets[0 .. n_frames], T[12 f ..]): n_points = offsets[n_frames]
// sizes the launch.
hipError_t vox_transform_frames_device(hipStream_t stream, const unsigned char* const* d_src, size_t stride, const int32_t* d_offsets,
                                       const float* d_T, int n_frames, size_t n_points, unsigned char* d_out, size_t out_stride);

// n records of `stride` bytes -> records of out_stride bytes (words past the input's are 0), all on the device.
hipError_t vox_copy_records(hipStream_t stream, const unsigned char* d_in, size_t stride, size_t n, unsigned char* d_out, size_t out_stride);

// ---- extractSurroundingKeyFrames() on the resident key-frame store (extractNearby :975-1010 + the selection of extractCloud
// :1012-1044). The store's per-key data the selection reads:
struct KfFrame {                           // what the frame table takes from key k (64 bytes)
    float                T[12];            // row-major 3x4 transform of the key pose (pcl::getTransformation, :317)
    const unsigned char* src;              // the key's 32-byte records
    int32_t              n;                // their count
    int32_t              pad;
};
struct KfSelect {                          // written by the device (pinned host memory)
    int32_t   n_frames;                    // entries of the frame table (= key ids reported)
    int32_t   n_cent;                      // centroids of the key-pose filter
    int32_t   n_cand;                      // radius candidates
    int32_t   pad;
    long long n_points;                    // records of the concatenated cloud
};
struct KfTable {                           // the frame table, device memory, valid until the next kf_select on the workspace
    const unsigned char* const* src;
    const int32_t* offsets;
    const float* T;
    const int32_t* keys;
};
// pos[k] = {x, y, z, 0} of key k, k = 0 .. n-1. centre: the point the radius search (b) and the distance filter (f) measure from, handed
// to the kernels by value - extractSurroundingKeyFrames and the global map pass P[n-1]'s own bits, s2m_extract_surrounding_at any
// finite point. n_recent: the newest keys whose time passes the recent-key test (:1000-1007, counted by
// the caller in double). Chooses the frames (radius search, key-pose voxel filter with leaf `density`, nearest key of every
// centroid, recent keys, distance filter), writes the table and synchronises `stream` once for the counts. Stores of more than
// 4 096 keys run the radius search over the whole grid; more than 4 096 candidates are sorted and filtered by device-wide radix
// passes after a first wait for their number (a second wait). Either way the result is that of the single-workgroup kernel.
hipError_t kf_select(VoxWorkspace* w, hipStream_t stream, const float4* d_pos, const KfFrame* d_frames, int n, const float centre[3],
                     int n_recent, float radius, float density, KfSelect* out, KfTable* tab);

// What the most recent kf_select on the workspace left resident, for the observation hook s2m_debug_kf_select_last: the path it took
// (a host-side note: 0 the single-workgroup kernel on a store of up to 4 096 keys, 1 the radius search over the whole grid with up
// to 4 096 candidates, 2 the device-wide sorts), its counts, the centroids of (c) as {x, y, z, 0} and the nearest key of each (d),
// and the frame table. The device pointers are valid until the next kf_select on the workspace. false: no selection has ended yet.
struct KfLast {
    int           path;
    KfSelect      sel;
    const float4* cent;                    // sel.n_cent entries
    const int32_t* nn;                     // sel.n_cent entries
    KfTable       tab;                     // sel.n_frames entries, sel.n_frames + 1 offsets
};
bool kf_select_last(const VoxWorkspace* w, KfLast* out);

// ---- detectLoopClosureDistance() (:732-765) on the same store: pos[k] and time[k] of key k = 0 .. n-1. *key_pre = the key with the
// least (d2, k) among those with d2(P[k], P[n-1]) < radius * radius (fp32, as kf_select) and |time[k] - time_cur| > time_diff
// (double), or -1. Two launches over all keys and one wait on `stream` for the result.
hipError_t loop_detect(VoxWorkspace* w, hipStream_t stream, const float4* d_pos, const double* d_time, int n, float radius,
                       double time_cur, double time_diff, int* key_pre);

}  // namespace s2m
