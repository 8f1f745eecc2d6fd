// s2m_abi_sc.hip — C ABI of ScanContext (s2m_sc.hip's kernels): the descriptor of a cloud, the store, SCManager's loop detector
// and the batched distance.  Host only.  The place query has a unit of its own (s2m_abi_sc_query.hip).
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_sc.hpp"
#include "s2m_sc_keys.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

constexpr size_t kScDesc = (size_t)S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR;

}  // namespace

extern "C" {

int s2m_make_scancontext(s2m_handle h, const void* pts, size_t n, size_t stride_bytes,
                         double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR], double ringkey[S2M_SC_NUM_RING])
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if (!desc || !ringkey) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = sc_build_descriptor(h, pts, n, stride_bytes))) return rc;
    S2M_HIP(h, hipMemcpyAsync(h->sc.h_stage, h->sc.out.p, sizeof(double) * 1220, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(desc, h->sc.h_stage, sizeof(double) * 1200);
    memcpy(ringkey, h->sc.h_stage + 1200, sizeof(double) * 20);
    return S2M_OK;
}

// ---- section 8(f) row F3: the SCManager loop detector ---------------------------------------------

int s2m_sc_reset(s2m_handle h)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    h->sc.n = 0; h->sc.n_search = 0; h->sc.counter = 0;
    return S2M_OK;
}

int s2m_sc_size(s2m_handle h) { return h ? (int)h->sc.n : S2M_ERR_INVALID_ARG; }

int s2m_sc_add_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = sc_build_descriptor(h, pts, n, stride_bytes))) return rc;
    if ((rc = sc_append_from_out(h))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // the caller's cloud is free again
    return S2M_OK;
}

int s2m_sc_add_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR])
{
    if (!h || !desc) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    // ring key = row means, as makeRingkeyFromScancontext (:198-211) / k_sc_finish compute them
    memcpy(h->sc.h_stage, desc, sizeof(double) * kScDesc);
    for (int r = 0; r < S2M_SC_NUM_RING; r++) h->sc.h_stage[kScDesc + r] = sc_ring_key([&](int k) { return desc[r * S2M_SC_NUM_SECTOR + k]; });
    S2M_HIP(h, hipMemcpyAsync(h->sc.out.p, h->sc.h_stage, sizeof(double) * 1220, hipMemcpyHostToDevice, h->stream));
    int rc = sc_append_from_out(h);
    if (rc) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // h_sc is reused by the next call
    return S2M_OK;
}

int s2m_sc_detect_loop(s2m_handle h, int32_t* loop_id, float* yaw_diff_rad, s2m_sc_match* detail)
{
    if (!h || !loop_id || !yaw_diff_rad) return S2M_ERR_INVALID_ARG;
    *loop_id = -1; *yaw_diff_rad = 0.0f;
    if (detail) { memset(detail, 0, sizeof(*detail)); detail->min_dist = 10000000; }
    constexpr int NUM_EXCLUDE_RECENT = 30, TREE_MAKING_PERIOD = 10;       // Scancontext.h:89, :99
    if ((int)h->sc.n < NUM_EXCLUDE_RECENT + 1) return S2M_OK;              // :263-267
    // the reference rebuilds its kd-tree every TREE_MAKING_PERIOD_ calls; between rebuilds the search sees the older set
    if (h->sc.counter % TREE_MAKING_PERIOD == 0) h->sc.n_search = h->sc.n - NUM_EXCLUDE_RECENT;
    h->sc.counter = h->sc.counter + 1;
    S2M_HIP(h, hipSetDevice(h->device));
    // the kernel writes its 48-byte result straight into the pinned staging block (host-coherent memory the device can address):
    // a copy behind the kernel would be a second trip through the queue, and one to pageable memory ~50 us more
    static_assert(sizeof(ScDetectOut) <= sizeof(double) * 1220, "the result fits the pinned ScanContext staging block");
    sc_launch_detect(h->stream, h->sc.store_desc.as<double>(), h->sc.store_ring.as<float>(), h->sc.store_sector.as<double>(),
                     (int)h->sc.n, (int)h->sc.n_search, reinterpret_cast<ScDetectOut*>(h->sc.h_stage));
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    ScDetectOut o;
    memcpy(&o, h->sc.h_stage, sizeof(o));
    *loop_id = o.loop_id; *yaw_diff_rad = o.yaw_diff_rad;
    if (detail) {
        detail->min_dist = o.min_dist; detail->nn_idx = o.nn_idx; detail->nn_align = o.nn_align;
        for (int k = 0; k < 3; k++) { detail->cand_idx[k] = o.cand_idx[k]; detail->cand_d2[k] = o.cand_d2[k]; }
    }
    return S2M_OK;
}

int s2m_sc_distance(s2m_handle h, int32_t query_idx, const int32_t* cand_idx, int32_t m, double* dist, int32_t* shift)
{
    if (!h || m < 0 || (m > 0 && (!cand_idx || !dist || !shift))) return S2M_ERR_INVALID_ARG;
    if (query_idx < 0 || (size_t)query_idx >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "query index outside the descriptor store");
    for (int32_t k = 0; k < m; k++)
        if (cand_idx[k] < 0 || (size_t)cand_idx[k] >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "candidate index outside the descriptor store");
    if (m == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t off_d = ((sizeof(int32_t) * (size_t)m + 15) & ~(size_t)15), off_s = off_d + sizeof(double) * (size_t)m;
    int rc = ensure(h, h->sc.cand, off_s + sizeof(int32_t) * (size_t)m);
    if (rc) return rc;
    unsigned char* base = h->sc.cand.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(base, cand_idx, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    sc_launch_distance_batch(h->stream, h->sc.store_desc.as<double>(), h->sc.store_sector.as<double>(), (int)query_idx, (const int32_t*)base,
                             (int)m, (double*)(base + off_d), (int32_t*)(base + off_s));
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(dist, base + off_d, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(shift, base + off_s, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

}  // extern "C"
