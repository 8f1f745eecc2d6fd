// s2m_abi_sc_query.hip — C ABI of the ScanContext place query (s2m_sc_query.hip's kernels): the argument
// table, the searched set, the four query sources.  Read-only on the store and the detector's counters.
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_sc_query.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

constexpr size_t kScDesc = (size_t)S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR;
static_assert(sizeof(s2m_sc_hit) == 24, "s2m_sc_hit is 24 bytes on both sides of the ABI");
static_assert(sizeof(ScQueryOut) <= sizeof(double) * 1220, "the hits fit the pinned ScanContext staging block");

const s2m_sc_query_params kScQueryDefaults = { 0, -1, 0, 0, 1, S2M_SC_ALIGN_SECTOR_KEY, 0.3 };   // SC_DIST_THRES (Scancontext.h:95)

// the searched set of a checked call: first + i for i < n_before, first + skip + i from there on, n_s keys in all
struct ScQueryPlan {
    s2m_sc_query_params p;
    int first, n_before, skip, n_s;
};

bool sc_query_args_ok(int64_t n, const s2m_sc_query_params& p)
{
    if (n < 0) return false;
    if (p.top_k < 1 || p.top_k > S2M_SC_QUERY_MAX_K) return false;
    if (p.align != S2M_SC_ALIGN_SECTOR_KEY && p.align != S2M_SC_ALIGN_FULL) return false;
    if (!(p.max_dist > 0.0 && p.max_dist <= 10000000.0)) return false;     // (a NaN fails both)
    if (p.first < 0 || p.count < -1 || p.first > n) return false;
    if (p.count >= 0 && (int64_t)p.first + p.count > n) return false;
    return true;
}

ScQueryPlan sc_query_plan(int64_t n, const s2m_sc_query_params& p)
{
    ScQueryPlan q{ p, p.first, 0, 0, 0 };
    const int64_t end = p.count < 0 ? n : (int64_t)p.first + p.count;
    int64_t lo = p.exclude_lo, hi = p.exclude_hi;                         // the window, cut to the range
    lo = lo < p.first ? p.first : (lo > end ? end : lo);
    hi = hi < p.first ? p.first : (hi > end ? end : hi);
    if (lo >= hi) lo = hi = end;
    q.n_before = (int)(lo - p.first);
    q.skip = (int)(hi - lo);
    q.n_s = (int)(end - p.first - (hi - lo));
    return q;
}

// null outputs and the argument table; *n_hits = 0 from here on
int sc_query_check(s2m_context* h, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits, ScQueryPlan* plan)
{
    if (!h || !hits || !n_hits) return S2M_ERR_INVALID_ARG;
    *n_hits = 0;
    const s2m_sc_query_params prm = p ? *p : kScQueryDefaults;
    if (!sc_query_args_ok((int64_t)h->sc.n, prm)) return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_query: top_k, align, max_dist or the range is invalid");
    *plan = sc_query_plan((int64_t)h->sc.n, prm);
    return S2M_OK;
}

// the query's descriptor is on the device at src_desc (its sector key at src_sector, or nullptr): the three kernels, one wait
int sc_query_run(s2m_context* h, const ScQueryPlan& q, const double* src_desc, const double* src_sector, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryArgs a{};
    a.store_desc = h->sc.store_desc.as<double>(); a.store_sector = h->sc.store_sector.as<double>();
    a.src_desc = src_desc; a.src_sector = src_sector;
    a.slot = h->sc.query.as<double>();
    a.first = q.first; a.n_before = q.n_before; a.skip = q.skip; a.n_s = q.n_s;
    a.top_k = q.p.top_k; a.align = q.p.align; a.max_dist = q.p.max_dist;
    int rc = ensure(h, h->sc.query_part, sc_query_part_bytes(q.n_s, q.p.top_k));
    if (rc) return rc;
    a.part = h->sc.query_part.as<unsigned char>();
    a.out = reinterpret_cast<ScQueryOut*>(h->sc.h_stage);
    S2M_HIP(h, sc_query_launch(h->stream, a));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const ScQueryOut* o = reinterpret_cast<const ScQueryOut*>(h->sc.h_stage);
    const int32_t n = o->n_hits;
    if (n < 0 || n > q.p.top_k) return fail(h, S2M_ERR_HIP, "s2m_sc_query: the device left no hit count");
    memcpy(hits, o->hits, sizeof(s2m_sc_hit) * (size_t)n);
    *n_hits = n;
    return S2M_OK;
}

}  // namespace

// s2m_sc_query_scan for a scan that is on the device already (the relocalisation's query): the same descriptor, the same hits
int s2m::host::sc_query_device_scan(s2m_context* h, const void* d_pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p,
                                    s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    int rc = sc_query_check(h, p, hits, n_hits, &q);
    if (rc) return rc;
    if (q.n_s == 0) return S2M_OK;
    if ((rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot))) return rc;
    if ((rc = sc_build_descriptor(h, d_pts, n, stride_bytes, true))) return rc;
    return sc_query_run(h, q, h->sc.out.as<double>(), nullptr, hits, n_hits);
}

extern "C" {

int s2m_sc_query_default_params(s2m_sc_query_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    *p = kScQueryDefaults;
    return S2M_OK;
}

int s2m_sc_query_check_args(int32_t n_stored, const s2m_sc_query_params* p)
{
    return sc_query_args_ok(n_stored, p ? *p : kScQueryDefaults) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

int s2m_sc_query_key(s2m_handle h, int32_t key, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    int rc = sc_query_check(h, p, hits, n_hits, &q);
    if (rc) return rc;
    if (key < 0 || (size_t)key >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "query key outside the descriptor store");
    if (q.n_s == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot))) return rc;
    return sc_query_run(h, q, h->sc.store_desc.as<double>() + (size_t)key * kScDesc, h->sc.store_sector.as<double>() + (size_t)key * S2M_SC_NUM_SECTOR,
                        hits, n_hits);
}

int s2m_sc_query_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR], const s2m_sc_query_params* p, s2m_sc_hit* hits,
                            int32_t* n_hits)
{
    ScQueryPlan q;
    int rc = sc_query_check(h, p, hits, n_hits, &q);
    if (rc) return rc;
    if (!desc) return S2M_ERR_INVALID_ARG;
    if (q.n_s == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot))) return rc;
    // through the pinned block into the slot; the hits come back through the same block, behind this copy on the stream
    memcpy(h->sc.h_stage, desc, sizeof(double) * kScDesc);
    S2M_HIP(h, hipMemcpyAsync(h->sc.query.p, h->sc.h_stage, sizeof(double) * kScDesc, hipMemcpyHostToDevice, h->stream));
    return sc_query_run(h, q, h->sc.query.as<double>(), nullptr, hits, n_hits);
}

int s2m_sc_query_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if ((rc = sc_query_check(h, p, hits, n_hits, &q))) return rc;
    if (q.n_s == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot))) return rc;
    if ((rc = sc_build_descriptor(h, pts, n, stride_bytes))) return rc;   // into sc.out, as s2m_sc_add_scan; nothing is appended
    return sc_query_run(h, q, h->sc.out.as<double>(), nullptr, hits, n_hits);
}

int s2m_sc_query_projected(s2m_handle h, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    int rc = sc_query_check(h, p, hits, n_hits, &q);
    if (rc) return rc;
    if (!h->proj.have_deskewed) return fail(h, S2M_ERR_NO_SCAN, "s2m_sc_query_projected before s2m_project_scan");
    if (q.n_s == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot))) return rc;
    if ((rc = sc_build_descriptor(h, h->proj.cloud_deskewed.p, h->proj.deskewed_n, kProjOutStride, true))) return rc;   // as s2m_sc_add_projected
    return sc_query_run(h, q, h->sc.out.as<double>(), nullptr, hits, n_hits);
}

}  // extern "C"
