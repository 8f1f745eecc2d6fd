// s2m_abi_sc_query.hip — C ABI of the ScanContext place query (s2m_sc_query.hip's kernels): the argument
// table, the searched set, the query sources behind sc_query_from; and of its many-query form (s2m_sc_many.hip's kernels; section
// 20) and the ring-key prefilter (s2m_sc_ring.hip's kernels; section 22): one pass driver, sc_pass_run, with the buffers and the
// launch of each.  Read-only on the store and the detector's counters.
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <utility>

#include "s2m_context.hpp"
#include "s2m_sc_many.hpp"
#include "s2m_sc_query.hpp"
#include "s2m_sc_ring.hpp"

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


// A checked query whose searched set is not empty: the slot, the query's descriptor on the device as `source` leaves it
// (src_desc and, where the store holds it, src_sector), the kernels.  What an entry point checks itself comes before this.
template <typename Source>
int sc_query_from(s2m_context* h, const ScQueryPlan& q, s2m_sc_hit* hits, int32_t* n_hits, Source source)
{
    if (q.n_s == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure(h, h->sc.query, sizeof(double) * kScQuerySlot);
    if (rc) return rc;
    const double* src_desc = nullptr;
    const double* src_sector = nullptr;
    if ((rc = source(src_desc, src_sector))) return rc;
    return sc_query_run(h, q, src_desc, src_sector, hits, n_hits);
}

// ... with the descriptor of a cloud, built into sc.out as s2m_sc_add_scan / s2m_sc_add_projected build it; nothing is appended
int sc_query_cloud(s2m_context* h, const ScQueryPlan& q, const void* pts, size_t n, size_t stride_bytes, bool on_device, s2m_sc_hit* hits, int32_t* n_hits)
{
    return sc_query_from(h, q, hits, n_hits, [&](const double*& desc, const double*&) {
        desc = h->sc.out.as<double>();
        return sc_build_descriptor(h, pts, n, stride_bytes, on_device);
    });
}


// ---- many queries at once (DESIGN.md sections 20 and 22): the passes ------------------------------------------------------

const s2m_sc_query_many_params kScManyDefaults = { { 0, -1, 0, 0, 1, S2M_SC_ALIGN_SECTOR_KEY, 0.3 }, 0, 0 };
constexpr size_t kScManyPinnedUp = (size_t)16 << 20;      // external descriptors of one pass go up through at most this much pinned memory

bool sc_many_args_ok(int64_t n, int64_t m, const s2m_sc_query_many_params& p, bool descriptor_query)
{
    if (!sc_query_args_ok(n, p.q) || m < 0) return false;
    if (descriptor_query && p.rel_lo < p.rel_hi) return false;            // a relative window needs a stored key to be relative to
    return true;
}

ScManySet sc_many_set(int64_t n, const s2m_sc_query_many_params& p)
{
    ScManySet set{};
    set.first = p.q.first;
    set.end = (int32_t)(p.q.count < 0 ? n : (int64_t)p.q.first + p.q.count);
    set.ex_lo = p.q.exclude_lo; set.ex_hi = p.q.exclude_hi; set.rel_lo = p.rel_lo; set.rel_hi = p.rel_hi;
    return set;
}

// device buffers of exactly their bytes (no slack: the pass's buffers together stay under kScManyScratchMax)
int sc_many_ensure(s2m_context* h, std::initializer_list<std::pair<s2m_context::DevBuf*, size_t>> bufs)
{
    for (const auto& [b, bytes] : bufs) {
        if (bytes <= b->cap) continue;
        S2M_HIP(h, b->reset());
        S2M_HIP(h, hipMalloc(&b->p, bytes));
        b->cap = bytes;
    }
    return S2M_OK;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

using ScPassState = s2m_context::ScanContext::ScPassState;

// A call of m queries - stored keys (by_key) or external descriptors - whose arguments its entry point has checked
struct ScPassCall {
    ScPassState* state;                             // the call's pass hook and what its last call did
    const char *null_msg, *count_msg;               // its error messages
    bool by_key; const int32_t* keys; const double* descs; int32_t m;
    ScManySet set;
    void* rows; int32_t* counts; size_t rec, width; // the caller's [m][width] records of `rec` bytes and [m] counts
    size_t per_q, slack;                            // device bytes of a query over the buffers of a pass; what the alignment of their parts adds
    size_t grid_max;                                // queries one grid takes
    s2m_context::DevBuf* in;                        // where the keys or descriptors of a pass go up
};
// what a pass leaves on the device; counts == nullptr: right behind the rows, brought back by the same copy
struct ScPassOut { const void* rows; const int32_t* counts; };

// The queries in passes of at most kScManyScratchMax of device memory: size(pass) makes the call's buffers for `pass` queries,
// launch(mp, &out) enqueues the kernels of mp queries (their keys or descriptors are at the head of c.in by then) and names the
// rows and counts.  Per pass one upload, the kernels, the download, one wait.
template <typename Size, typename Launch>
int sc_pass_run(s2m_context* h, const ScPassCall& c, Size size, Launch launch)
{
    const size_t m = (size_t)c.m;
    if (m == 0) return S2M_OK;
    if (!c.rows || !c.counts || !(c.by_key ? (const void*)c.keys : (const void*)c.descs)) return fail(h, S2M_ERR_INVALID_ARG, c.null_msg);
    if (c.by_key)
        for (size_t i = 0; i < m; i++)
            if (c.keys[i] < 0 || (int64_t)c.keys[i] >= (int64_t)h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "query key outside the descriptor store");
    c.state->last_passes = 0; c.state->last_scratch = 0;
    if (c.set.first >= c.set.end) { std::fill(c.counts, c.counts + m, 0); return S2M_OK; }   // an empty range: an empty set for every query
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t up_q = c.by_key ? sizeof(int32_t) : sizeof(double) * kScDesc, row = c.rec * c.width;
    size_t pass = std::max<size_t>(1, (kScManyScratchMax - c.slack) / c.per_q);
    if (!c.by_key) pass = std::min(pass, std::max<size_t>(1, kScManyPinnedUp / up_q));
    pass = std::min(pass, c.grid_max);
    if (c.state->pass > 0) pass = std::min(pass, (size_t)c.state->pass);
    pass = std::min(pass, m);
    int rc = size(pass);
    if (rc) return rc;
    const size_t up_bytes = up16(up_q * pass), pinned = up_bytes + (row + sizeof(int32_t)) * pass;   // the upload | rows, counts
    if (pinned > h->sc.h_many_cap) {
        if (h->sc.h_many) S2M_HIP(h, hipHostFree(h->sc.h_many));
        h->sc.h_many = nullptr; h->sc.h_many_cap = 0;
        S2M_HIP(h, hipHostMalloc((void**)&h->sc.h_many, pinned));
        h->sc.h_many_cap = pinned;
    }
    c.state->last_scratch = c.per_q * pass;
    unsigned char* h_up = h->sc.h_many;
    unsigned char* h_rows = h->sc.h_many + up_bytes;
    for (size_t i0 = 0; i0 < m; i0 += pass) {
        const size_t mp = std::min(pass, m - i0);
        if (c.by_key) memcpy(h_up, c.keys + i0, up_q * mp);
        else memcpy(h_up, c.descs + kScDesc * i0, up_q * mp);
        S2M_HIP(h, hipMemcpyAsync(c.in->p, h_up, up_q * mp, hipMemcpyHostToDevice, h->stream));
        ScPassOut out{};
        if ((rc = launch(mp, &out))) return rc;
        int32_t* h_counts = reinterpret_cast<int32_t*>(h_rows + row * mp);
        S2M_HIP(h, hipMemcpyAsync(h_rows, out.rows, (row + (out.counts ? 0 : sizeof(int32_t))) * mp, hipMemcpyDeviceToHost, h->stream));
        if (out.counts) S2M_HIP(h, hipMemcpyAsync(h_counts, out.counts, sizeof(int32_t) * mp, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));      // the one wait of the pass: the pinned block is free again
        c.state->last_passes++;
        for (size_t i = 0; i < mp; i++) {
            const int32_t n = h_counts[i];
            if (n < 0 || (size_t)n > c.width) return fail(h, S2M_ERR_HIP, c.count_msg);
            memcpy(static_cast<unsigned char*>(c.rows) + (i0 + i) * row, h_rows + i * row, c.rec * (size_t)n);   // the records behind stay the caller's
            c.counts[i0 + i] = n;
        }
    }
    return S2M_OK;
}

// the many-query: a pass is the queries' keys or descriptors + sector keys, their column norms, the (query, tile group) lists and
// the rows with their counts behind them - one download
int sc_many_run(s2m_context* h, bool by_key, const int32_t* keys, const double* descs, int32_t m, const s2m_sc_query_many_params* pp,
                s2m_sc_hit* hits, int32_t* n_hits)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const s2m_sc_query_many_params p = pp ? *pp : kScManyDefaults;
    if (!sc_many_args_ok((int64_t)h->sc.n, m, p, !by_key))
        return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_query_many: top_k, align, max_dist, the range, m or a relative window on a descriptor query is invalid");
    const ScManySet set = sc_many_set((int64_t)h->sc.n, p);
    const int K = p.q.top_k;
    const size_t in_q = by_key ? sizeof(int32_t) : kScManyExtBytes, part_q = sc_many_part_bytes(sc_many_groups(set.end - set.first), K), out_q = sc_many_out_bytes(K);
    s2m_context::ScanContext& sc = h->sc;
    const ScPassCall c{ &sc.many, "s2m_sc_query_many: null queries or outputs with m > 0", "s2m_sc_query_many: the device left no hit count",
                        by_key, keys, descs, m, set, hits, n_hits, sizeof(s2m_sc_hit), (size_t)K,
                        in_q + kScManyNormBytes + part_q + out_q, 64,                       // (64: the rows' counts start on an 8-byte boundary)
                        (size_t)65535 * kScManyBlock, &sc.many_in };
    return sc_pass_run(h, c,
        [&](size_t pass) {
            return sc_many_ensure(h, { { &sc.many_in, in_q * pass }, { &sc.many_qnorm, kScManyNormBytes * pass }, { &sc.many_part, part_q * pass },
                                       { &sc.many_out, out_q * pass } });
        },
        [&](size_t mp, ScPassOut* out) {
            ScManyArgs a{};
            a.store_desc = sc.store_desc.as<double>(); a.store_sector = sc.store_sector.as<double>();
            if (by_key) a.keys = sc.many_in.as<int32_t>();
            else { a.ext_desc = sc.many_in.as<double>(); a.ext_sector = sc.many_in.as<double>() + kScDesc * mp; }
            a.qnorm = sc.many_qnorm.as<double>();
            a.m = (int)mp; a.set = set; a.top_k = K; a.align = p.q.align; a.max_dist = p.q.max_dist;
            a.part = sc.many_part.as<unsigned char>();
            a.out_hits = sc.many_out.as<s2m_sc_hit>();
            a.out_n = reinterpret_cast<int32_t*>(sc.many_out.as<unsigned char>() + sizeof(s2m_sc_hit) * (size_t)K * mp);
            out->rows = a.out_hits;
            S2M_HIP(h, sc_many_launch(h->stream, a));
            return (int)S2M_OK;
        });
}


// ---- the ring-key prefilter ---------------------------------------------------------------

const s2m_sc_ring_params kScRingDefaults = { { { 0, -1, 0, 0, 1, S2M_SC_ALIGN_SECTOR_KEY, 0.3 }, 0, 0 }, 3, 0 };   // NUM_CANDIDATES_FROM_TREE (Scancontext.h:91)
static_assert(sizeof(s2m_sc_ring_params) == 48 && sizeof(s2m_sc_ring_neighbour) == 8, "the ring query's records on both sides of the ABI");

bool sc_ring_args_ok(int32_t n, int32_t m, const s2m_sc_ring_params& p, int32_t descriptor_query)
{
    if (s2m_sc_query_many_check_args(n, m, &p.m, descriptor_query) != S2M_OK) return false;
    return p.n_candidates >= 1 && p.n_candidates <= S2M_SC_RING_MAX_CAND && p.reserved == 0;
}

// the ring query: a pass is the queries' keys or descriptors + sector keys + fp32 ring keys, the neighbour lists and their sizes
// and, with `both`, the candidates' distances and shifts and the rows; every part starts on a 16-byte boundary, so rows and counts
// come back by a copy each.  both: stage two and the rows (hits, n_out = n_hits), else the neighbour lists (nb, n_out).
int sc_ring_run(s2m_context* h, bool by_key, bool both, const int32_t* keys, const double* descs, int32_t m, const s2m_sc_ring_params* pp,
                s2m_sc_ring_neighbour* nb, s2m_sc_hit* hits, int32_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const s2m_sc_ring_params p = pp ? *pp : kScRingDefaults;
    if (!sc_ring_args_ok((int32_t)h->sc.n, m, p, !by_key))
        return fail(h, S2M_ERR_INVALID_ARG, "s2m_sc_ring: what the many-query rejects, n_candidates outside 1..256 or reserved != 0");
    const ScManySet set = sc_many_set((int64_t)h->sc.n, p.m);
    const int K = p.m.q.top_k, C = p.n_candidates;
    const size_t in_q = by_key ? sizeof(int32_t) : kScRingExtBytes;
    const size_t cand_q = sc_ring_cand_bytes(C), dist_q = both ? sc_ring_dist_bytes(C) : 0, out_q = both ? sc_ring_out_bytes(K) : 0;
    s2m_context::ScanContext& sc = h->sc;
    const ScPassCall c{ &sc.ring, "s2m_sc_ring: null queries or outputs with m > 0", "s2m_sc_ring: the device left no count",
                        by_key, keys, descs, m, set, both ? (void*)hits : (void*)nb, n_out,
                        both ? sizeof(s2m_sc_hit) : sizeof(s2m_sc_ring_neighbour), both ? (size_t)K : (size_t)C,
                        in_q + cand_q + dist_q + out_q, 256,                                // (256: every part of a buffer starts on a 16-byte boundary)
                        65535, &sc.ring_in };                                               // k_sc_ring_dist: one grid row per query
    size_t ext_sector_off = 0, ext_ring_off = 0, cand_n_off = 0, shift_off = 0, out_n_off = 0;
    return sc_pass_run(h, c,
        [&](size_t pass) {
            ext_sector_off = up16(sizeof(double) * kScDesc * pass); ext_ring_off = ext_sector_off + up16(sizeof(double) * S2M_SC_NUM_SECTOR * pass);
            cand_n_off = up16(sizeof(s2m_sc_ring_neighbour) * (size_t)C * pass); shift_off = up16(sizeof(double) * (size_t)C * pass);
            out_n_off = up16(sizeof(s2m_sc_hit) * (size_t)K * pass);
            return sc_many_ensure(h, { { &sc.ring_in, by_key ? sizeof(int32_t) * pass : ext_ring_off + kScRingKeyBytes * pass },
                                       { &sc.ring_cand, cand_n_off + sizeof(int32_t) * pass },
                                       { &sc.ring_dist, both ? shift_off + sizeof(int32_t) * (size_t)C * pass : 0 },     // (stage one alone: none)
                                       { &sc.ring_out, both ? out_n_off + sizeof(int32_t) * pass : 0 } });
        },
        [&](size_t mp, ScPassOut* out) {
            ScRingArgs a{};
            a.store_desc = sc.store_desc.as<double>(); a.store_ring = sc.store_ring.as<float>(); a.store_sector = sc.store_sector.as<double>();
            if (by_key) a.keys = sc.ring_in.as<int32_t>();
            else {
                a.ext_desc = sc.ring_in.as<double>();
                a.ext_sector = reinterpret_cast<double*>(sc.ring_in.as<unsigned char>() + ext_sector_off);
                a.ext_ring = reinterpret_cast<float*>(sc.ring_in.as<unsigned char>() + ext_ring_off);
            }
            a.m = (int)mp; a.set = set; a.n_cand = C;
            a.cand = sc.ring_cand.as<s2m_sc_ring_neighbour>();
            a.n_out = reinterpret_cast<int32_t*>(sc.ring_cand.as<unsigned char>() + cand_n_off);
            a.top_k = K; a.align = p.m.q.align; a.max_dist = p.m.q.max_dist;
            *out = { a.cand, a.n_out };
            if (both) {
                a.dist = sc.ring_dist.as<double>();
                a.shift = reinterpret_cast<int32_t*>(sc.ring_dist.as<unsigned char>() + shift_off);
                a.out_hits = sc.ring_out.as<s2m_sc_hit>();
                a.out_n = reinterpret_cast<int32_t*>(sc.ring_out.as<unsigned char>() + out_n_off);
                *out = { a.out_hits, a.out_n };
            }
            S2M_HIP(h, sc_ring_launch(h->stream, a));
            return (int)S2M_OK;
        });
}

int sc_pass_set(s2m_context* h, ScPassState& s, int32_t queries_per_pass, const char* msg)
{
    if (queries_per_pass < 0) return fail(h, S2M_ERR_INVALID_ARG, msg);
    s.pass = queries_per_pass;
    return S2M_OK;
}

int sc_pass_last(const ScPassState& s, int32_t* passes, size_t* scratch_bytes)
{
    if (!passes || !scratch_bytes) return S2M_ERR_INVALID_ARG;
    *passes = s.last_passes; *scratch_bytes = s.last_scratch;
    return S2M_OK;
}

}  // namespace

// s2m_sc_query_scan for a scan that is on the device already (the relocalisation's query): the same descriptor, the same hits
int s2m::host::sc_query_device_scan(s2m_context* h, const void* d_pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p,
                                    s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    if (const int rc = sc_query_check(h, p, hits, n_hits, &q)) return rc;
    return sc_query_cloud(h, q, d_pts, n, stride_bytes, true, hits, n_hits);
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
    if (const int rc = sc_query_check(h, p, hits, n_hits, &q)) return rc;
    if (key < 0 || (size_t)key >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "query key outside the descriptor store");
    return sc_query_from(h, q, hits, n_hits, [&](const double*& desc, const double*& sector) {
        desc = h->sc.store_desc.as<double>() + (size_t)key * kScDesc;
        sector = h->sc.store_sector.as<double>() + (size_t)key * S2M_SC_NUM_SECTOR;
        return (int)S2M_OK;
    });
}

int s2m_sc_query_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR], const s2m_sc_query_params* p, s2m_sc_hit* hits,
                            int32_t* n_hits)
{
    ScQueryPlan q;
    if (const int rc = sc_query_check(h, p, hits, n_hits, &q)) return rc;
    if (!desc) return S2M_ERR_INVALID_ARG;
    return sc_query_from(h, q, hits, n_hits, [&](const double*& src, const double*&) {
        // through the pinned block into the slot; the hits come back through the same block, behind this copy on the stream
        memcpy(h->sc.h_stage, desc, sizeof(double) * kScDesc);
        S2M_HIP(h, hipMemcpyAsync(h->sc.query.p, h->sc.h_stage, sizeof(double) * kScDesc, hipMemcpyHostToDevice, h->stream));
        src = h->sc.query.as<double>();
        return (int)S2M_OK;
    });
}

int s2m_sc_query_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    if (const int rc = check_records(h, pts, n, stride_bytes)) return rc;
    if (const int rc = sc_query_check(h, p, hits, n_hits, &q)) return rc;
    return sc_query_cloud(h, q, pts, n, stride_bytes, false, hits, n_hits);
}

int s2m_sc_query_projected(s2m_handle h, const s2m_sc_query_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    ScQueryPlan q;
    if (const int rc = sc_query_check(h, p, hits, n_hits, &q)) return rc;
    if (!h->proj.have_deskewed) return fail(h, S2M_ERR_NO_SCAN, "s2m_sc_query_projected before s2m_project_scan");
    return sc_query_cloud(h, q, h->proj.cloud_deskewed.p, h->proj.deskewed_n, kProjOutStride, true, hits, n_hits);
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

int s2m_sc_ring_default_params(s2m_sc_ring_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    *p = kScRingDefaults;
    return S2M_OK;
}

int s2m_sc_ring_check_args(int32_t n_stored, int32_t m, const s2m_sc_ring_params* p, int32_t descriptor_query)
{
    return sc_ring_args_ok(n_stored, m, p ? *p : kScRingDefaults, descriptor_query) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

int s2m_sc_ring_neighbours_keys(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_ring_params* p, s2m_sc_ring_neighbour* out, int32_t* n_out)
{
    return sc_ring_run(h, true, false, keys, nullptr, m, p, out, nullptr, n_out);
}

int s2m_sc_ring_neighbours_descriptors(s2m_handle h, const double* descs, int32_t m, const s2m_sc_ring_params* p, s2m_sc_ring_neighbour* out,
                                       int32_t* n_out)
{
    return sc_ring_run(h, false, false, nullptr, descs, m, p, out, nullptr, n_out);
}

int s2m_sc_query_keys_ring(s2m_handle h, const int32_t* keys, int32_t m, const s2m_sc_ring_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    return sc_ring_run(h, true, true, keys, nullptr, m, p, nullptr, hits, n_hits);
}

int s2m_sc_query_descriptors_ring(s2m_handle h, const double* descs, int32_t m, const s2m_sc_ring_params* p, s2m_sc_hit* hits, int32_t* n_hits)
{
    return sc_ring_run(h, false, true, nullptr, descs, m, p, nullptr, hits, n_hits);
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
    return h ? sc_pass_set(h, h->sc.many, queries_per_pass, "many-query pass: 0 (the default) or a positive number of queries") : S2M_ERR_INVALID_ARG;
}

int s2m_debug_sc_query_many_shape(int32_t* tile_cands, int32_t* block_queries)
{
    if (!tile_cands || !block_queries) return S2M_ERR_INVALID_ARG;
    *tile_cands = kScManyTile; *block_queries = kScManyBlock;
    return S2M_OK;
}

int s2m_debug_sc_query_many_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes)
{
    return h ? sc_pass_last(h->sc.many, passes, scratch_bytes) : S2M_ERR_INVALID_ARG;
}

int s2m_debug_sc_ring_pass(s2m_handle h, int32_t queries_per_pass)
{
    return h ? sc_pass_set(h, h->sc.ring, queries_per_pass, "ring-query pass: 0 (the default) or a positive number of queries") : S2M_ERR_INVALID_ARG;
}

int s2m_debug_sc_ring_shape(int32_t* tile_keys, int32_t* block_queries, int32_t* buffer_words)
{
    if (!tile_keys || !block_queries || !buffer_words) return S2M_ERR_INVALID_ARG;
    *tile_keys = kScRingTile; *block_queries = kScRingBlock; *buffer_words = kScRingBuf;
    return S2M_OK;
}

int s2m_debug_sc_ring_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes)
{
    return h ? sc_pass_last(h->sc.ring, passes, scratch_bytes) : S2M_ERR_INVALID_ARG;
}

}  // extern "C"
