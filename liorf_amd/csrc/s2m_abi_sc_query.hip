// s2m_abi_sc_query.hip — C ABI of the ScanContext place query (s2m_sc_query.hip's kernels): the argument
// table, the searched set, the four query sources; and of its many-query form (s2m_sc_many.hip's kernels; section 20): the
// passes, their staging and the rows.  Read-only on the store and the detector's counters.
#include <algorithm>
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_sc_many.hpp"
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


// ---- many queries at once ----------------------------------------------------------------

const s2m_sc_query_many_params kScManyDefaults = { { 0, -1, 0, 0, 1, S2M_SC_ALIGN_SECTOR_KEY, 0.3 }, 0, 0 };
constexpr size_t kScManyPinnedUp = (size_t)16 << 20;      // external descriptors of one pass go up through at most this much pinned memory

bool sc_many_args_ok(int64_t n, int64_t m, const s2m_sc_query_many_params& p, bool descriptor_query)
{
    if (!sc_query_args_ok(n, p.q) || m < 0) return false;
    if (descriptor_query && p.rel_lo < p.rel_hi) return false;            // a relative window needs a stored key to be relative to
    return true;
}

// a device buffer of exactly `bytes` (no slack: the pass's buffers together stay under kScManyScratchMax)
int sc_many_ensure(s2m_context* h, s2m_context::DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return S2M_OK;
    S2M_HIP(h, b.reset());
    S2M_HIP(h, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return S2M_OK;
}

// m queries - stored keys (by_key) or external descriptors - in passes of at most kScManyScratchMax of device memory;
// per pass one upload, the three kernels, one download, one wait
int sc_many_run(s2m_context* h, bool by_key, const int32_t* keys, const double* descs, int32_t m, const s2m_sc_query_many_params* pp,
                s2m_sc_hit* hits, int32_t* n_hits)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const s2m_sc_query_many_params p = pp ? *pp : kScManyDefaults;
    const int64_t n = (int64_t)h->sc.n;
    if (!sc_many_args_ok(n, m, p, !by_key))
        return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_query_many: top_k, align, max_dist, the range, m or a relative window on a descriptor query is invalid");
    if (m == 0) return S2M_OK;
    if (!hits || !n_hits || !(by_key ? (const void*)keys : (const void*)descs)) return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_query_many: null queries or outputs with m > 0");
    if (keys)
        for (int32_t i = 0; i < m; i++)
            if (keys[i] < 0 || (int64_t)keys[i] >= n) return fail(h, S2M_ERR_INVALID_ARG, "query key outside the descriptor store");
    ScManySet set{};
    set.first = p.q.first;
    set.end = (int32_t)(p.q.count < 0 ? n : (int64_t)p.q.first + p.q.count);
    set.ex_lo = p.q.exclude_lo; set.ex_hi = p.q.exclude_hi; set.rel_lo = p.rel_lo; set.rel_hi = p.rel_hi;
    h->sc.many_last_passes = 0; h->sc.many_last_scratch = 0;
    if (set.first >= set.end) { std::fill(n_hits, n_hits + m, 0); return S2M_OK; }   // an empty range: an empty set for every query
    S2M_HIP(h, hipSetDevice(h->device));
    const int K = p.q.top_k, groups = sc_many_groups(set.end - set.first);
    const size_t in_q = keys ? sizeof(int32_t) : kScManyExtBytes, up_q = keys ? sizeof(int32_t) : sizeof(double) * kScDesc;
    const size_t part_q = sc_many_part_bytes(groups, K), out_q = sc_many_out_bytes(K);
    const size_t per_q = in_q + kScManyNormBytes + part_q + out_q;
    size_t pass = std::max<size_t>(1, (kScManyScratchMax - 64) / per_q);  // (64: the rows' counts start on an 8-byte boundary)
    if (!keys) pass = std::min(pass, std::max<size_t>(1, kScManyPinnedUp / up_q));
    pass = std::min<size_t>(pass, (size_t)65535 * kScManyBlock);
    if (h->sc.many_pass > 0) pass = std::min<size_t>(pass, (size_t)h->sc.many_pass);
    pass = std::min<size_t>(pass, (size_t)m);
    int rc;
    if ((rc = sc_many_ensure(h, h->sc.many_in, in_q * pass)) || (rc = sc_many_ensure(h, h->sc.many_qnorm, kScManyNormBytes * pass)) ||
        (rc = sc_many_ensure(h, h->sc.many_part, part_q * pass)) || (rc = sc_many_ensure(h, h->sc.many_out, out_q * pass)))
        return rc;
    const size_t up_bytes = (up_q * pass + 15) & ~(size_t)15, pinned = up_bytes + out_q * pass;
    if (pinned > h->sc.h_many_cap) {
        if (h->sc.h_many) S2M_HIP(h, hipHostFree(h->sc.h_many));
        h->sc.h_many = nullptr; h->sc.h_many_cap = 0;
        S2M_HIP(h, hipHostMalloc((void**)&h->sc.h_many, pinned));
        h->sc.h_many_cap = pinned;
    }
    h->sc.many_last_scratch = per_q * pass;
    unsigned char* h_up = h->sc.h_many;
    unsigned char* h_down = h->sc.h_many + up_bytes;
    for (size_t i0 = 0; i0 < (size_t)m; i0 += pass) {
        const size_t mp = std::min(pass, (size_t)m - i0);
        ScManyArgs a{};
        a.store_desc = h->sc.store_desc.as<double>(); a.store_sector = h->sc.store_sector.as<double>();
        if (keys) {
            memcpy(h_up, keys + i0, sizeof(int32_t) * mp);
            a.keys = h->sc.many_in.as<int32_t>();
        } else {
            memcpy(h_up, descs + kScDesc * i0, sizeof(double) * kScDesc * mp);
            a.ext_desc = h->sc.many_in.as<double>();
            a.ext_sector = h->sc.many_in.as<double>() + kScDesc * mp;
        }
        S2M_HIP(h, hipMemcpyAsync(h->sc.many_in.p, h_up, up_q * mp, hipMemcpyHostToDevice, h->stream));
        a.qnorm = h->sc.many_qnorm.as<double>();
        a.m = (int)mp; a.set = set; a.top_k = K; a.align = p.q.align; a.max_dist = p.q.max_dist;
        a.part = h->sc.many_part.as<unsigned char>();
        a.out_hits = h->sc.many_out.as<s2m_sc_hit>();
        a.out_n = reinterpret_cast<int32_t*>(h->sc.many_out.as<unsigned char>() + sizeof(s2m_sc_hit) * (size_t)K * mp);
        S2M_HIP(h, sc_many_launch(h->stream, a));
        S2M_HIP(h, hipMemcpyAsync(h_down, h->sc.many_out.p, out_q * mp, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));      // the one wait of the pass: the pinned block is free again
        h->sc.many_last_passes++;
        const s2m_sc_hit* rows = reinterpret_cast<const s2m_sc_hit*>(h_down);
        const int32_t* counts = reinterpret_cast<const int32_t*>(h_down + sizeof(s2m_sc_hit) * (size_t)K * mp);
        for (size_t i = 0; i < mp; i++) {
            const int32_t c = counts[i];
            if (c < 0 || c > K) return fail(h, S2M_ERR_HIP, "s2m_sc_query_many: the device left no hit count");
            memcpy(hits + (i0 + i) * (size_t)K, rows + i * (size_t)K, sizeof(s2m_sc_hit) * (size_t)c);   // the records behind stay the caller's
            n_hits[i0 + i] = c;
        }
    }
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

int s2m_sc_query_many_default_params(s2m_sc_query_many_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    *p = kScManyDefaults;
    return S2M_OK;
}

int s2m_sc_query_many_check_args(int32_t n_stored, int32_t m, const s2m_sc_query_many_params* p, int32_t descriptor_query)
{
    return sc_many_args_ok(n_stored, m, p ? *p : kScManyDefaults, descriptor_query != 0) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

int s2m_sc_query_keys(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_query_many_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    return sc_many_run(h, true, keys, nullptr, m, p, hits, n_hits);
}

int s2m_sc_query_descriptors(s2m_handle h, const double* descs, int32_t m, const s2m_sc_query_many_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    return sc_many_run(h, false, nullptr, descs, m, p, hits, n_hits);
}

int s2m_sc_get_descriptors(s2m_handle h, int32_t first, int32_t count, double* descs)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_get_descriptors: range outside the descriptor store");
    if (count == 0) return S2M_OK;
    if (!descs) return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_get_descriptors: null output");
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipMemcpyAsync(descs, h->sc.store_desc.as<double>() + (size_t)first * kScDesc, sizeof(double) * kScDesc * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

// ---- test hooks (include/liorf_s2m_debug.h) ---------------------------------------------------------------------

int s2m_debug_sc_query_many_pass(s2m_handle h, int32_t queries_per_pass)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (queries_per_pass < 0) return fail(h, S2M_ERR_INVALID_ARG, "many-query pass: 0 (the default) or a positive number of queries");
    h->sc.many_pass = queries_per_pass;
    return S2M_OK;
}

int s2m_debug_sc_query_many_shape(int32_t* tile_cands, int32_t* block_queries)
{
    if (!tile_cands || !block_queries) return S2M_ERR_INVALID_ARG;
    *tile_cands = kScManyTile; *block_queries = kScManyBlock;
    return S2M_OK;
}

int s2m_debug_sc_query_many_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes)
{
    if (!h || !passes || !scratch_bytes) return S2M_ERR_INVALID_ARG;
    *passes = h->sc.many_last_passes; *scratch_bytes = h->sc.many_last_scratch;
    return S2M_OK;
}

}  // extern "C"
