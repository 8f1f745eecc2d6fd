// s2m_abi_voxel.hip — C ABI of the voxel-grid stages either side of the path (section 8(f) rows F2 / F1): downsampleCurrentScan,
// extractCloud, transformPointCloud.  Host orchestration of s2m_voxel.hip's stages only; also home of the helpers the other
// stages share for filtered clouds (voxel_into, download_records, finish_cloud, FrameTable::transform_into).
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

int s2m::host::voxel_into(s2m_context* h, const unsigned char* d_in, size_t n, size_t stride, float leaf, DevBuf& dst, VoxResult* res)
{
    int rc = ensure(h, dst, kDsStride * (n ? n : 1));
    if (rc) return rc;
    hipError_t e = vox_downsample(h->voxel.ws, h->stream, d_in, n, stride, leaf, dst.as<unsigned char>(), kDsStride, n, res);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "voxel grid filter", e);
    return S2M_OK;
}

int s2m::host::download_records(s2m_context* h, const DevBuf& src, size_t n, void* out, size_t out_stride, size_t cap)
{
    const size_t m = n < cap ? n : cap;
    if (m == 0 || !out) return S2M_OK;
    S2M_HIP(h, hipMemcpy2DAsync(out, out_stride, src.p, kDsStride, out_stride < kDsStride ? out_stride : kDsStride, m,
                                hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (out_stride > kDsStride)                // records wider than the device's: the fields past it are 0, as on the device path
        for (size_t i = 0; i < m; i++) memset(static_cast<unsigned char*>(out) + i * out_stride + kDsStride, 0, out_stride - kDsStride);
    return S2M_OK;
}

int s2m::host::finish_cloud(s2m_context* h, const DevBuf& src, const VoxResult& res, void* out, size_t out_stride, size_t cap, const char* too_small)
{
    int rc;
    if (cap > 0 && (rc = download_records(h, src, res.n_out, out, out_stride, cap))) return rc;
    if (cap > 0 && res.n_out > cap) return fail(h, S2M_ERR_CAPACITY, too_small);
    return res.leaf_too_small ? S2M_WARN_LEAF_TOO_SMALL : S2M_OK;
}

int s2m::host::FrameTable::transform_into(s2m_context* h, DevBuf& dst, size_t stride, const char* what) const
{
    int rc = ensure(h, dst, kDsStride * total);
    if (rc) return rc;
    hipError_t e = vox_transform_frames(h->voxel.ws, h->stream, src.data(), stride, offsets.data(), T.data(), (int)src.size(),
                                        dst.as<unsigned char>(), kDsStride);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, what, e);
    return S2M_OK;
}

static int voxel_downsample_impl(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, float leaf,
                                 void* out, size_t out_stride_bytes, size_t cap, size_t* n_out, bool on_device)
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if ((rc = check_leaf(h, leaf))) return rc;
    // (unlike bad_out: the stride is checked with cap == 0 too, and below a filtered cloud that does not fit cap == 0 is an error)
    if (!n_out || (cap > 0 && !out) || out_stride_bytes < 12 || (out_stride_bytes & 3))
        return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    VoxResult res;
    if (on_device) {
        hipError_t e = vox_downsample(h->voxel.ws, h->stream, static_cast<const unsigned char*>(pts), n, stride_bytes, leaf,
                                      static_cast<unsigned char*>(out), out_stride_bytes, cap, &res);
        if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "voxel grid filter", e);
    } else {
        if ((rc = stage_host_records(h, h->voxel.in, pts, n * stride_bytes))) return rc;
        if ((rc = voxel_into(h, h->voxel.in.as<unsigned char>(), n, stride_bytes, leaf, h->voxel.out, &res))) return rc;
        if ((rc = download_records(h, h->voxel.out, res.n_out, out, out_stride_bytes, cap))) return rc;
    }
    *n_out = res.n_out;
    if (res.n_out > cap) return fail(h, S2M_ERR_CAPACITY, "output buffer too small for the filtered cloud");
    return res.leaf_too_small ? S2M_WARN_LEAF_TOO_SMALL : S2M_OK;
}

int s2m_voxel_downsample(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, float leaf,
                         void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{ return voxel_downsample_impl(h, pts, n, stride_bytes, leaf, out, out_stride_bytes, cap, n_out, false); }

int s2m_voxel_downsample_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes, float leaf,
                                void* d_out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{ return voxel_downsample_impl(h, d_pts, n, stride_bytes, leaf, d_out, out_stride_bytes, cap, n_out, true); }

int s2m_downsample_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, int on_device, float leaf,
                        void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if ((rc = check_leaf(h, leaf))) return rc;
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    S2M_HIP(h, hipSetDevice(h->device));
    VoxResult res;
    if (n > 0) {
        const unsigned char* d_in = static_cast<const unsigned char*>(pts);
        if (!on_device) {
            if ((rc = stage_host_records(h, h->voxel.in, pts, n * stride_bytes))) return rc;
            d_in = h->voxel.in.as<unsigned char>();
        }
        h->voxel.have_scan_ds = false;
        if ((rc = voxel_into(h, d_in, n, stride_bytes, leaf, h->voxel.scan_ds, &res))) return rc;
    }
    *n_out = res.n_out;
    h->voxel.scan_ds_n = res.n_out;
    h->voxel.have_scan_ds = true;
    // laserCloudSurfLastDS stays on the device as the registration's scan; the host copy is for the key-frame store
    if ((rc = set_scan_impl(h, h->voxel.scan_ds.p, res.n_out, kDsStride, true))) return rc;
    return finish_cloud(h, h->voxel.scan_ds, res, out, out_stride_bytes, cap, "output buffer too small for the filtered scan");
}

int s2m_extract_cloud(s2m_handle h, int n_frames, const void* const* frames, const size_t* frame_sizes,
                      size_t stride_bytes, int on_device, const float* poses_xyzrpy, float leaf,
                      void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && (!frames || !frame_sizes || !poses_xyzrpy)))
        return fail(h, S2M_ERR_INVALID_ARG, "null key-frame table");
    int rc = check_leaf(h, leaf);
    if (rc) return rc;
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    size_t total = 0;
    for (int f = 0; f < n_frames; f++) {
        if ((rc = check_records(h, frames[f], frame_sizes[f], stride_bytes))) return rc;
        total += frame_sizes[f];
        if (total > (size_t)0x3fffffff) return fail(h, S2M_ERR_CAPACITY, "too many points");
    }
    S2M_HIP(h, hipSetDevice(h->device));
    VoxResult res;
    if (total > 0) {
        if (!on_device && (rc = ensure(h, h->voxel.in, total * stride_bytes))) return rc;
        FrameTable tab;
        for (int f = 0; f < n_frames; f++) {
            const unsigned char* src = static_cast<const unsigned char*>(frames[f]);
            if (!on_device) {                              // the host frames back to back in the staging buffer
                unsigned char* dst = h->voxel.in.as<unsigned char>() + tab.total * stride_bytes;
                if (frame_sizes[f])
                    S2M_HIP(h, hipMemcpyAsync(dst, frames[f], frame_sizes[f] * stride_bytes, hipMemcpyHostToDevice, h->stream));
                src = dst;
            }
            float T[12];
            xyzrpy_to_transform(poses_xyzrpy + 6 * (size_t)f, T);
            tab.push(src, frame_sizes[f], T);
        }
        if ((rc = tab.transform_into(h, h->voxel.frames_xf, stride_bytes, "key-frame transform"))) return rc;
        if ((rc = voxel_into(h, h->voxel.frames_xf.as<unsigned char>(), total, kDsStride, leaf, h->voxel.map_ds, &res))) return rc;
    }
    *n_out = res.n_out;
    // laserCloudSurfFromMapDS becomes the search index (the reference's kdtree->setInputCloud, :1302)
    if ((rc = set_map_impl(h, h->voxel.map_ds.p, res.n_out, kDsStride, true))) return rc;
    return finish_cloud(h, h->voxel.map_ds, res, out, out_stride_bytes, cap, "output buffer too small for the local map");
}

int s2m_transform_cloud(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, const float pose_xyzrpy[6],
                        void* out, size_t out_stride_bytes)
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if (!pose_xyzrpy || (n > 0 && !out) || out_stride_bytes < 12 || (out_stride_bytes & 3))
        return fail(h, S2M_ERR_INVALID_ARG, "bad pose or output buffer");
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = stage_host_records(h, h->voxel.in, pts, n * stride_bytes))) return rc;
    float T[12];
    xyzrpy_to_transform(pose_xyzrpy, T);
    FrameTable tab;
    tab.push(h->voxel.in.as<unsigned char>(), n, T);
    if ((rc = tab.transform_into(h, h->voxel.frames_xf, stride_bytes, "cloud transform"))) return rc;
    return download_records(h, h->voxel.frames_xf, n, out, out_stride_bytes, n);
}

int s2m_downsample_projected(s2m_handle h, float leaf, void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!h->proj.have_deskewed) return fail(h, S2M_ERR_NO_SCAN, "s2m_downsample_projected before s2m_project_scan");
    return s2m_downsample_scan(h, h->proj.cloud_deskewed.p, h->proj.deskewed_n, kProjOutStride, 1, leaf, out, out_stride_bytes, cap, n_out);
}
