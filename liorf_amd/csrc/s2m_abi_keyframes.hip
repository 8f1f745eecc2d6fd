// s2m_abi_keyframes.hip — C ABI of the resident key-frame store and of what is built from it: extractSurroundingKeyFrames,
// the global map and the saved map.  Host orchestration of s2m_voxel.hip's stages only.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

// ---- the resident key-frame store and extractSurroundingKeyFrames() (:1046-1059) ----------------------

constexpr size_t kKfMaxKeys = (size_t)1 << 24;          // key ids travel in a float intensity in the reference (:991-997)
constexpr size_t kKfBlockBytes = (size_t)64 << 20;      // arena block: ~2 000 key frames of 1 000 points

int s2m_kf_default_params(s2m_kf_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    p->search_radius = 50.0f;       // surroundingKeyframeSearchRadius  include/utility.h:240
    p->density = 1.0f;              // surroundingKeyframeDensity       include/utility.h:238
    p->map_leaf = 0.2f;             // surroundingKeyframeMapLeafSize   include/utility.h:228
    p->recent_window_s = 10.0;      // :1003
    return S2M_OK;
}

int s2m_kf_reset(s2m_handle h)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    loop_drop_pending(h, false);                           // a launched closure reads the store's clouds: it ends first and is dropped
    // the store is emptied whatever happens: a block whose hipFree fails is dropped, never freed twice
    hipError_t e = hipSuccess;
    for (void* b : h->kf.blocks) { const hipError_t eb = hipFree(b); if (eb != hipSuccess && e == hipSuccess) e = eb; }
    h->kf.blocks.clear();
    h->kf.block_used = h->kf.block_cap = 0;
    h->kf.pose.clear(); h->kf.time.clear(); h->kf.frame.clear();
    h->loop.index.clear();
    h->sess.forget_appended();
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "hipFree of a key-frame block", e);
    return S2M_OK;
}

int s2m_kf_size(s2m_handle h) { return h ? (int)h->kf.time.size() : S2M_ERR_INVALID_ARG; }

namespace {

bool finite_pose(const float* p)
{
    for (int k = 0; k < 6; k++) if (!std::isfinite(p[k])) return false;
    return true;
}

KfFrame kf_frame_of(const float pose_xyzrpy[6], const unsigned char* src, int32_t n)
{
    KfFrame f{};
    xyzrpy_to_transform(pose_xyzrpy, f.T);                 // transCur of :317, once per pose (laserCloudMapContainer, :1025-1035)
    f.src = src; f.n = n;
    return f;
}

// the device arrays hold `want` keys (grow-with-copy: ensure() alone would drop them)
int kf_reserve(s2m_context* h, size_t want)
{
    if (want <= h->kf.cap) return S2M_OK;
    size_t cap = h->kf.cap ? h->kf.cap : 256;
    while (cap < want) cap *= 2;
    const size_t n = h->kf.time.size();
    constexpr int kParts = 3;
    struct Part { DevBuf* b; size_t elem; } parts[kParts] = { { &h->kf.pos, sizeof(float4) }, { &h->kf.frames, sizeof(KfFrame) },
                                                              { &h->kf.tdev, sizeof(double) } };
    void* np[kParts] = { nullptr, nullptr, nullptr };
    for (int k = 0; k < kParts; k++) {
        hipError_t e = hipMalloc(&np[k], parts[k].elem * cap);
        if (e != hipSuccess) { for (int j = 0; j < k; j++) (void)hipFree(np[j]); return fail(h, S2M_ERR_HIP, "key-frame store", e); }
    }
    hipError_t e = hipSuccess;
    for (int k = 0; k < kParts && e == hipSuccess; k++)
        if (n) e = hipMemcpyAsync(np[k], parts[k].b->p, parts[k].elem * n, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {                                 // the old arrays stay in place; the new ones go
        for (int k = 0; k < kParts; k++) (void)hipFree(np[k]);
        return fail(h, S2M_ERR_HIP, "key-frame store copy", e);
    }
    for (int k = 0; k < kParts; k++) {                          // (the copies are complete: the new arrays are installed in any case)
        (void)parts[k].b->reset(np[k], parts[k].elem * cap);
    }
    h->kf.cap = cap;
    return S2M_OK;
}

// The end of a selection from the store (s2m_extract_surrounding, s2m_global_map): the filtered cloud and the chosen keys to the
// host, as far as they are asked for and fit, then the capacity errors - the cloud's first - and the leaf warning.
int finish_cloud_and_keys(s2m_context* h, const DevBuf& src, const VoxResult& res, void* out, size_t out_stride, size_t cap, const char* too_small,
                          const KfSelect& sel, const KfTable& tab, int32_t* keys, size_t keys_cap)
{
    int rc;
    if (cap > 0 && (rc = download_records(h, src, res.n_out, out, out_stride, cap))) return rc;
    const size_t nk = (size_t)sel.n_frames < keys_cap ? (size_t)sel.n_frames : keys_cap;
    if (nk > 0) {
        S2M_HIP(h, hipMemcpyAsync(keys, tab.keys, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (cap > 0 && res.n_out > cap) return fail(h, S2M_ERR_CAPACITY, too_small);
    if (keys_cap > 0 && (size_t)sel.n_frames > keys_cap) return fail(h, S2M_ERR_CAPACITY, "key buffer too small for the frame list");
    return res.leaf_too_small ? S2M_WARN_LEAF_TOO_SMALL : S2M_OK;
}

// room for `bytes` of records in the arena (a new block when the current one is full; blocks never move)
int kf_arena_take(s2m_context* h, size_t bytes, unsigned char** dst)
{
    *dst = nullptr;
    if (bytes == 0) return S2M_OK;
    if (h->kf.blocks.empty() || h->kf.block_used + bytes > h->kf.block_cap) {
        const size_t cap = bytes > kKfBlockBytes ? bytes : kKfBlockBytes;
        void* b = nullptr;
        S2M_HIP(h, hipMalloc(&b, cap));
        h->kf.blocks.push_back(b);
        h->kf.block_cap = cap; h->kf.block_used = 0;
    }
    *dst = static_cast<unsigned char*>(h->kf.blocks.back()) + h->kf.block_used;
    return S2M_OK;
}

}  // namespace

int s2m_kf_add(s2m_handle h, const float pose_xyzrpy[6], double time, const void* pts, size_t n, size_t stride_bytes, int source)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!pose_xyzrpy || !finite_pose(pose_xyzrpy) || !std::isfinite(time))
        return fail(h, S2M_ERR_INVALID_ARG, "key pose and time must be finite");
    if (source != S2M_KF_FROM_HOST && source != S2M_KF_FROM_DEVICE && source != S2M_KF_FROM_LAST_DOWNSAMPLE)
        return fail(h, S2M_ERR_INVALID_ARG, "unknown key-frame source");
    int rc;
    if (source == S2M_KF_FROM_LAST_DOWNSAMPLE) {
        if (!h->voxel.have_scan_ds) return fail(h, S2M_ERR_NO_SCAN, "no s2m_downsample_scan before S2M_KF_FROM_LAST_DOWNSAMPLE");
        n = h->voxel.scan_ds_n;
    } else if ((rc = check_records(h, pts, n, stride_bytes))) return rc;
    const size_t N = h->kf.time.size();
    if (N >= kKfMaxKeys) return fail(h, S2M_ERR_CAPACITY, "key-frame store full (2^24 keys)");
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = kf_reserve(h, N + 1))) return rc;
    unsigned char* dst = nullptr;
    if ((rc = kf_arena_take(h, kDsStride * n, &dst))) return rc;
    if (n > 0) {
        hipError_t e = hipSuccess;
        if (source == S2M_KF_FROM_LAST_DOWNSAMPLE)
            e = hipMemcpyAsync(dst, h->voxel.scan_ds.p, kDsStride * n, hipMemcpyDeviceToDevice, h->stream);
        else if (source == S2M_KF_FROM_DEVICE)
            e = vox_copy_records(h->stream, static_cast<const unsigned char*>(pts), stride_bytes, n, dst, kDsStride);
        else {
            if ((rc = stage_host_records(h, h->voxel.in, pts, n * stride_bytes))) return rc;
            e = vox_copy_records(h->stream, h->voxel.in.as<unsigned char>(), stride_bytes, n, dst, kDsStride);
        }
        if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "key-frame copy", e);
    }
    const KfFrame f = kf_frame_of(pose_xyzrpy, dst, (int32_t)n);
    const float4 p = make_float4(pose_xyzrpy[0], pose_xyzrpy[1], pose_xyzrpy[2], 0.0f);
    S2M_HIP(h, hipMemcpyAsync(h->kf.pos.as<float4>() + N, &p, sizeof(p), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(h->kf.frames.as<KfFrame>() + N, &f, sizeof(f), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(h->kf.tdev.as<double>() + N, &time, sizeof(time), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // the caller's cloud and the staged entries are free again
    // committed only now: a failure above leaves the store as it was
    h->kf.block_used += kDsStride * n;
    h->kf.pose.insert(h->kf.pose.end(), pose_xyzrpy, pose_xyzrpy + 6);
    h->kf.time.push_back(time);
    h->kf.frame.push_back(f);
    return S2M_OK;
}

int s2m::host::copy_pipeline(s2m_context* h)
{
    if (!h->gmap.copy_stream) S2M_HIP(h, hipStreamCreateWithFlags(&h->gmap.copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        if (!h->gmap.ev_xf[k]) S2M_HIP(h, hipEventCreateWithFlags(&h->gmap.ev_xf[k], hipEventDisableTiming));
        if (!h->gmap.ev_cp[k]) S2M_HIP(h, hipEventCreateWithFlags(&h->gmap.ev_cp[k], hipEventDisableTiming));
    }
    return S2M_OK;
}

int s2m::host::kf_install_keys(s2m_context* h, size_t n, const float* pose_xyzrpy, const double* time, const int32_t* counts)
{
    const size_t N0 = h->kf.time.size();
    if (n == 0) return S2M_OK;
    if (N0 + n > kKfMaxKeys) return fail(h, S2M_ERR_CAPACITY, "key-frame store full (2^24 keys)");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = kf_reserve(h, N0 + n);
    if (rc) return rc;
    std::vector<float4> pos(n);
    std::vector<KfFrame> fr(n);
    for (size_t k = 0; k < n; k++) {
        const size_t bytes = kDsStride * (size_t)counts[k];
        unsigned char* dst = nullptr;
        if ((rc = kf_arena_take(h, bytes, &dst))) return rc;
        h->kf.block_used += bytes;
        const float* q = pose_xyzrpy + 6 * k;
        fr[k] = kf_frame_of(q, dst, counts[k]);
        pos[k] = make_float4(q[0], q[1], q[2], 0.0f);
    }
    S2M_HIP(h, hipMemcpyAsync(h->kf.pos.as<float4>() + N0, pos.data(), sizeof(float4) * n, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(h->kf.frames.as<KfFrame>() + N0, fr.data(), sizeof(KfFrame) * n, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(h->kf.tdev.as<double>() + N0, time, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // (the host vectors above are read by the copies until here)
    h->kf.pose.insert(h->kf.pose.end(), pose_xyzrpy, pose_xyzrpy + 6 * n);
    h->kf.time.insert(h->kf.time.end(), time, time + n);
    h->kf.frame.insert(h->kf.frame.end(), fr.begin(), fr.end());
    return S2M_OK;
}

void s2m::host::kf_truncate(s2m_context* h, const KfMark& m)
{
    while (h->kf.blocks.size() > m.n_blocks) { (void)hipFree(h->kf.blocks.back()); h->kf.blocks.pop_back(); }
    h->kf.block_used = m.block_used; h->kf.block_cap = m.block_cap;
    h->kf.pose.resize(6 * m.n_keys); h->kf.time.resize(m.n_keys); h->kf.frame.resize(m.n_keys);
}

int s2m_kf_set_poses(s2m_handle h, int first, int count, const float* poses_xyzrpy)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const size_t N = h->kf.time.size();
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > N || (count > 0 && !poses_xyzrpy))
        return fail(h, S2M_ERR_INVALID_ARG, "pose range outside the key-frame store");
    for (int k = 0; k < count; k++)
        if (!finite_pose(poses_xyzrpy + 6 * (size_t)k)) return fail(h, S2M_ERR_INVALID_ARG, "key poses must be finite");
    if (count == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    std::vector<float4> pos((size_t)count);
    std::vector<KfFrame> fr((size_t)count);
    for (int k = 0; k < count; k++) {
        const float* q = poses_xyzrpy + 6 * (size_t)k;
        pos[k] = make_float4(q[0], q[1], q[2], 0.0f);
        fr[k] = kf_frame_of(q, h->kf.frame[first + k].src, h->kf.frame[first + k].n);
    }
    S2M_HIP(h, hipMemcpyAsync(h->kf.pos.as<float4>() + first, pos.data(), sizeof(float4) * count, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(h->kf.frames.as<KfFrame>() + first, fr.data(), sizeof(KfFrame) * count, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    std::copy(poses_xyzrpy, poses_xyzrpy + 6 * (size_t)count, h->kf.pose.begin() + 6 * (size_t)first);
    for (int k = 0; k < count; k++) h->kf.frame[first + k] = fr[k];
    return S2M_OK;
}

namespace {

// extractSurroundingKeyFrames around `centre` (null: P[N-1], the newest key's position as the store holds it) with the n_recent newest
// keys as (e): the selection, the transform of the chosen frames, the VoxelGrid, the result installed as the local map with its index
int extract_around(s2m_context* h, const float* centre, int n_recent, const s2m_kf_params& prm, void* out, size_t out_stride_bytes,
                   size_t cap, size_t* n_out, int32_t* keys, size_t keys_cap, size_t* n_keys)
{
    const size_t N = h->kf.time.size();
    S2M_HIP(h, hipSetDevice(h->device));
    KfSelect sel;
    KfTable tab;
    hipError_t e = kf_select(h->voxel.ws, h->stream, h->kf.pos.as<float4>(), h->kf.frames.as<KfFrame>(), (int)N,
                             centre ? centre : &h->kf.pose[6 * (N - 1)], n_recent, prm.search_radius, prm.density, &sel, &tab);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "key-frame selection", e);
    if (n_keys) *n_keys = (size_t)sel.n_frames;
    if (sel.n_points > 0x3fffffffLL) return fail(h, S2M_ERR_CAPACITY, "too many points");
    VoxResult res;
    int rc;
    if (sel.n_points > 0) {
        const size_t total = (size_t)sel.n_points;
        if ((rc = ensure(h, h->voxel.frames_xf, kDsStride * total))) return rc;
        e = vox_transform_frames_device(h->stream, tab.src, kDsStride, tab.offsets, tab.T, sel.n_frames, total,
                                        h->voxel.frames_xf.as<unsigned char>(), kDsStride);
        if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "key-frame transform", e);
        if ((rc = voxel_into(h, h->voxel.frames_xf.as<unsigned char>(), total, kDsStride, prm.map_leaf, h->voxel.map_ds, &res))) return rc;
    }
    *n_out = res.n_out;
    // laserCloudSurfFromMapDS becomes the search index (:1302), as in s2m_extract_cloud
    if ((rc = set_map_impl(h, h->voxel.map_ds.p, res.n_out, kDsStride, true))) return rc;
    return finish_cloud_and_keys(h, h->voxel.map_ds, res, out, out_stride_bytes, cap, "output buffer too small for the local map",
                                 sel, tab, keys, keys_cap);
}

// the parameter and buffer checks the two extractions share; *prm: the caller's parameters or the defaults
int extract_args(s2m_context* h, const s2m_kf_params* p, s2m_kf_params* prm, const void* out, size_t out_stride_bytes, size_t cap,
                 size_t* n_out, const int32_t* keys, size_t keys_cap, size_t* n_keys)
{
    if (p) *prm = *p; else s2m_kf_default_params(prm);
    if (!(prm->search_radius > 0.0f) || !std::isfinite(prm->search_radius) || !(prm->density > 0.0f) || !std::isfinite(prm->density))
        return fail(h, S2M_ERR_INVALID_ARG, "search radius and density must be positive, window and time finite");
    const int rc = check_leaf(h, prm->map_leaf);
    if (rc) return rc;
    if (!n_out || bad_out(out, out_stride_bytes, cap) || (keys_cap > 0 && !keys)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    if (n_keys) *n_keys = 0;
    return S2M_OK;
}

}  // namespace

int s2m_extract_surrounding(s2m_handle h, double time_cur, const s2m_kf_params* p, void* out, size_t out_stride_bytes, size_t cap,
                            size_t* n_out, int32_t* keys, size_t keys_cap, size_t* n_keys)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if ((p && !std::isfinite(p->recent_window_s)) || !std::isfinite(time_cur))
        return fail(h, S2M_ERR_INVALID_ARG, "search radius and density must be positive, window and time finite");
    s2m_kf_params prm;
    const int rc = extract_args(h, p, &prm, out, out_stride_bytes, cap, n_out, keys, keys_cap, n_keys);
    if (rc) return rc;
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;                             // cloudKeyPoses3D->points.empty(): nothing changes (:1048-1049)
    // (e) the recent keys: i = N-1, N-2, ... while timeLaserInfoCur - time < 10.0 (:1000-1007)
    int n_recent = 0;
    for (size_t i = N; i-- > 0 && time_cur - h->kf.time[i] < prm.recent_window_s;) n_recent++;
    return extract_around(h, nullptr, n_recent, prm, out, out_stride_bytes, cap, n_out, keys, keys_cap, n_keys);
}

// the local map around a given position: (b), (c), (d), (f), (g) with centre_xyz in place of P[N-1], no recent keys
int s2m_extract_surrounding_at(s2m_handle h, const float centre_xyz[3], const s2m_kf_params* p, void* out, size_t out_stride_bytes, size_t cap,
                               size_t* n_out, int32_t* keys, size_t keys_cap, size_t* n_keys)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!centre_xyz || !std::isfinite(centre_xyz[0]) || !std::isfinite(centre_xyz[1]) || !std::isfinite(centre_xyz[2]))
        return fail(h, S2M_ERR_INVALID_ARG, "the centre of the local map must be finite");
    s2m_kf_params prm;
    const int rc = extract_args(h, p, &prm, out, out_stride_bytes, cap, n_out, keys, keys_cap, n_keys);
    if (rc) return rc;
    if (h->kf.time.empty()) return S2M_OK;
    return extract_around(h, centre_xyz, 0, prm, out, out_stride_bytes, cap, n_out, keys, keys_cap, n_keys);
}

// ---- the global map and the saved map from the key-frame store (publishGlobalMap :453-502, saveMapService :375-432) ---------

int s2m_gmap_default_params(s2m_gmap_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    p->search_radius = 1e3f;        // globalMapVisualizationSearchRadius  include/utility.h:250
    p->pose_density = 10.0f;        // globalMapVisualizationPoseDensity   include/utility.h:251
    p->leaf = 1.0f;                 // globalMapVisualizationLeafSize      include/utility.h:252
    return S2M_OK;
}

namespace {

// Concatenations that go through the VoxelGrid: the voxel stage counts and places points in int32 (k_transform_frames' and
// k_vox_centroid's one lane per point, the radix sort's positions, the run starts) and k_vox_bbox strides up to 2^20 past the
// last point, so the total stays 2^21 below INT32_MAX.
constexpr size_t kMapMaxPts = ((size_t)1 << 31) - ((size_t)1 << 21);
constexpr size_t kMapChunkPts = (size_t)1 << 22;           // unfiltered copy-out: points per chunk (128 MiB of records per staging buffer)

// frames first .. first+count-1 of the store, each transformed by its current pose, back to back into gmap.xf
int map_transform_range(s2m_context* h, int first, int count)
{
    FrameTable tab;
    for (int f = 0; f < count; f++) {
        const KfFrame& kf = h->kf.frame[(size_t)first + f];
        tab.push(kf.src, (size_t)kf.n, kf.T);
    }
    int rc = tab.transform_into(h, h->gmap.xf, kDsStride, "key-frame transform");
    if (rc) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));           // (the host table above is read by the copies until here)
    return S2M_OK;
}

// the unfiltered concatenation of frames first .. first+count-1 to host `out`, its first m records: chunks of whole frames are
// transformed into two staging buffers in turn, and each chunk's copy to the host (a stream of its own) runs while the next
// chunk is transformed
int map_copy_out_chunked(s2m_context* h, int first, int count, size_t m, void* out, size_t out_stride)
{
    struct Chunk { int f0, nf; size_t at, n; };
    std::vector<Chunk> chunks;
    size_t at = 0, biggest = 0;
    for (int f = 0; f < count && at < m;) {
        Chunk c{ f, 0, at, 0 };
        while (f < count && (c.nf == 0 || c.n + (size_t)h->kf.frame[(size_t)first + f].n <= kMapChunkPts)) {
            c.n += (size_t)h->kf.frame[(size_t)first + f].n;
            c.nf++; f++;
        }
        at += c.n;
        biggest = std::max(biggest, c.n);
        if (c.n) chunks.push_back(c);
    }
    if (chunks.empty()) return S2M_OK;
    // device table: source pointers | transforms | per chunk its frames' offsets from the chunk's start
    const size_t nf_all = (size_t)(chunks.back().f0 + chunks.back().nf);
    const size_t ptr_bytes = (sizeof(void*) * nf_all + 15) & ~(size_t)15, t_bytes = (sizeof(float) * 12 * nf_all + 15) & ~(size_t)15;
    std::vector<unsigned char> tab(ptr_bytes + t_bytes + sizeof(int32_t) * (nf_all + chunks.size()));
    std::vector<size_t> off_at(chunks.size());
    {
        const unsigned char** src = reinterpret_cast<const unsigned char**>(tab.data());
        float* T = reinterpret_cast<float*>(tab.data() + ptr_bytes);
        int32_t* off = reinterpret_cast<int32_t*>(tab.data() + ptr_bytes + t_bytes);
        size_t o = 0;
        for (size_t c = 0; c < chunks.size(); c++) {
            off_at[c] = o;
            int32_t run = 0;
            for (int f = chunks[c].f0; f < chunks[c].f0 + chunks[c].nf; f++) {
                const KfFrame& kf = h->kf.frame[(size_t)first + f];
                src[f] = kf.src;
                std::copy(kf.T, kf.T + 12, T + 12 * (size_t)f);
                off[o++] = run;
                run += kf.n;
            }
            off[o++] = run;
        }
    }
    int rc = ensure(h, h->gmap.tab, tab.size());
    if (rc) return rc;
    for (int k = 0; k < 2 && k < (int)chunks.size(); k++)
        if ((rc = ensure(h, h->gmap.stage[k], kDsStride * biggest))) return rc;
    if ((rc = copy_pipeline(h))) return rc;
    unsigned char* d_tab = h->gmap.tab.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, h->stream));
    const unsigned char* const* d_src = reinterpret_cast<const unsigned char* const*>(d_tab);
    const float* d_T = reinterpret_cast<const float*>(d_tab + ptr_bytes);
    const int32_t* d_off = reinterpret_cast<const int32_t*>(d_tab + ptr_bytes + t_bytes);
    auto transform = [&](size_t c) -> int {
        const int b = (int)(c & 1);
        if (c >= 2) S2M_HIP(h, hipStreamWaitEvent(h->stream, h->gmap.ev_cp[b], 0));     // chunk c-2's copy has left the buffer
        hipError_t e = vox_transform_frames_device(h->stream, d_src + chunks[c].f0, kDsStride, d_off + off_at[c], d_T + 12 * (size_t)chunks[c].f0,
                                                   chunks[c].nf, chunks[c].n, h->gmap.stage[b].as<unsigned char>(), kDsStride);
        if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "key-frame transform", e);
        S2M_HIP(h, hipEventRecord(h->gmap.ev_xf[b], h->stream));
        return S2M_OK;
    };
    const size_t width = out_stride < kDsStride ? out_stride : kDsStride;
    if ((rc = transform(0))) return rc;
    for (size_t c = 0; c < chunks.size(); c++) {
        if (c + 1 < chunks.size() && (rc = transform(c + 1))) return rc;        // the next chunk is on its way before this one is copied
        const int b = (int)(c & 1);
        const size_t rows = std::min(chunks[c].n, m - chunks[c].at);
        S2M_HIP(h, hipStreamWaitEvent(h->gmap.copy_stream, h->gmap.ev_xf[b], 0));
        S2M_HIP(h, hipMemcpy2DAsync(static_cast<unsigned char*>(out) + chunks[c].at * out_stride, out_stride, h->gmap.stage[b].p, kDsStride,
                                    width, rows, hipMemcpyDeviceToHost, h->gmap.copy_stream));
        S2M_HIP(h, hipEventRecord(h->gmap.ev_cp[b], h->gmap.copy_stream));
    }
    S2M_HIP(h, hipStreamSynchronize(h->gmap.copy_stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (out_stride > kDsStride)                // records wider than the device's: the fields past it are 0, as download_records leaves them
        for (size_t i = 0; i < m; i++) memset(static_cast<unsigned char*>(out) + i * out_stride + kDsStride, 0, out_stride - kDsStride);
    return S2M_OK;
}

}  // namespace

int s2m_global_map(s2m_handle h, const s2m_gmap_params* p, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out,
                   int32_t* keys, size_t keys_cap, size_t* n_keys)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    s2m_gmap_params prm;
    if (p) prm = *p; else s2m_gmap_default_params(&prm);
    if (!(prm.search_radius > 0.0f) || !std::isfinite(prm.search_radius) || !(prm.pose_density > 0.0f) || !std::isfinite(prm.pose_density))
        return fail(h, S2M_ERR_INVALID_ARG, "search radius and pose density must be positive and finite");
    int rc = check_leaf(h, prm.leaf);
    if (rc) return rc;
    if (!n_out || bad_out(out, out_stride_bytes, cap) || (keys_cap > 0 && !keys)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    if (n_keys) *n_keys = 0;
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;                             // cloudKeyPoses3D->points.empty() (:458-459)
    S2M_HIP(h, hipSetDevice(h->device));
    // (b) radiusSearch around cloudKeyPoses3D->back(), (c) the key-pose VoxelGrid, (d) nearest key per centroid, (f) the distance
    // test at the centroid (:466-491): kf_select with no recent keys
    KfSelect sel;
    KfTable tab;
    hipError_t e = kf_select(h->voxel.ws, h->stream, h->kf.pos.as<float4>(), h->kf.frames.as<KfFrame>(), (int)N, &h->kf.pose[6 * (N - 1)], 0,
                             prm.search_radius, prm.pose_density, &sel, &tab);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "global-map key selection", e);
    if (n_keys) *n_keys = (size_t)sel.n_frames;
    if ((unsigned long long)sel.n_points > kMapMaxPts) return fail(h, S2M_ERR_CAPACITY, "too many points in the global map");
    VoxResult res;
    if (sel.n_points > 0) {
        const size_t total = (size_t)sel.n_points;
        if ((rc = ensure(h, h->gmap.xf, kDsStride * total))) return rc;
        e = vox_transform_frames_device(h->stream, tab.src, kDsStride, tab.offsets, tab.T, sel.n_frames, total, h->gmap.xf.as<unsigned char>(), kDsStride);
        if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "key-frame transform", e);
        if ((rc = voxel_into(h, h->gmap.xf.as<unsigned char>(), total, kDsStride, prm.leaf, h->gmap.out, &res))) return rc;   // globalMapKeyFramesDS
    }
    *n_out = res.n_out;
    return finish_cloud_and_keys(h, h->gmap.out, res, out, out_stride_bytes, cap, "output buffer too small for the global map",
                                 sel, tab, keys, keys_cap);
}

int s2m_kf_map_cloud(s2m_handle h, int first, int count, float leaf, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    if (!(leaf >= 0.0f) || !std::isfinite(leaf)) return fail(h, S2M_ERR_INVALID_ARG, "leaf size must be 0 (no filter) or positive and finite");
    const size_t N = h->kf.time.size();
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > N) return fail(h, S2M_ERR_INVALID_ARG, "key range outside the key-frame store");
    unsigned long long total = 0;                          // 64 bits, from the host mirror of the per-key counts
    for (int f = 0; f < count; f++) total += (unsigned long long)h->kf.frame[(size_t)first + f].n;
    if (total == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if (leaf == 0.0f) {                                    // globalSurfCloud as it is (GlobalMap.pcd, :410-415)
        *n_out = (size_t)total;
        const size_t m = (size_t)total < cap ? (size_t)total : cap;
        int rc = m > 0 ? map_copy_out_chunked(h, first, count, m, out, out_stride_bytes) : S2M_OK;
        if (rc) return rc;
        if (cap > 0 && (size_t)total > cap) return fail(h, S2M_ERR_CAPACITY, "output buffer too small for the map cloud");
        return S2M_OK;
    }
    // downSizeFilterSurf at req.resolution (:400-407): the whole concatenation on the device
    if (total > kMapMaxPts) return fail(h, S2M_ERR_CAPACITY, "too many points to filter on the device");
    int rc = map_transform_range(h, first, count);
    if (rc) return rc;
    VoxResult res;
    if ((rc = voxel_into(h, h->gmap.xf.as<unsigned char>(), (size_t)total, kDsStride, leaf, h->gmap.out, &res))) return rc;
    *n_out = res.n_out;
    return finish_cloud(h, h->gmap.out, res, out, out_stride_bytes, cap, "output buffer too small for the map cloud");
}
