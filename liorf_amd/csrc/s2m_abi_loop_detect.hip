// s2m_abi_loop_detect.hip — C ABI of the loop detection by position for many keys (s2m_loop_detect.hip's kernels; DESIGN.md
// section 23): the argument table, the passes, the buffers.  Read-only on the key-frame store; it uses s2m_context::ldet alone -
// nothing of the loop container, the voxel workspace, the scan or the map - and never looks at what is pending.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_loop_detect.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

static_assert(sizeof(s2m_loop_detect_params) == 40, "s2m_loop_detect_params on both sides of the ABI");

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// device buffers of exactly their bytes (no slack: the pass's buffers together stay under kLdScratchMax)
int ld_ensure(s2m_context* h, s2m_context::DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return S2M_OK;
    S2M_HIP(h, b.reset());
    S2M_HIP(h, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return S2M_OK;
}

}  // namespace

extern "C" {

int s2m_loop_detect_default_params(s2m_loop_detect_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    *p = ld_defaults();
    return S2M_OK;
}

int s2m_loop_detect_keys_check_args(int32_t n_stored, const int32_t* keys, int32_t m, int /*has_time_cur*/, const s2m_loop_detect_params* p)
{
    return ld_args_ok(n_stored, keys, m, p ? *p : ld_defaults()) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

int s2m_loop_detect_keys(s2m_handle h, const int32_t* keys, const double* time_cur, int32_t m, const s2m_loop_detect_params* pp,
                         int32_t* key_pre, float* d2, int32_t* n_cand)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const s2m_loop_detect_params p = pp ? *pp : ld_defaults();
    const size_t N = h->kf.time.size();
    if (!ld_args_ok((int64_t)N, keys, m, p))
        return fail(h, S2M_ERR_INVALID_ARG, "s2m_loop_detect_keys: m, null keys, a key outside the store, the radius, the time difference, top_k, reserved or the range is invalid");
    if (m == 0) return S2M_OK;
    if (!key_pre || !n_cand) return fail(h, S2M_ERR_INVALID_ARG, "s2m_loop_detect_keys: null outputs with m > 0");
    if (time_cur)
        for (int32_t i = 0; i < m; i++)
            if (!std::isfinite(time_cur[i])) return fail(h, S2M_ERR_INVALID_ARG, "s2m_loop_detect_keys: time_cur must be finite");
    s2m_context::LoopDetect& ld = h->ldet;
    ld.last_passes = 0; ld.last_scratch = 0;
    const LdPlan pl = ld_plan((int64_t)N, m, time_cur != nullptr, p, ld.pass, ld.max_splits);
    if (pl.first >= pl.end) { std::fill(n_cand, n_cand + m, 0); return S2M_OK; }   // an empty store or range: an empty set for every query
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t K = (size_t)p.top_k, pass = pl.pass;
    // device: keys | times; the lists; key_pre | d2 | n_cand of the pass's queries back to back (one download)
    const size_t time_off = up16(sizeof(int32_t) * pass);
    int rc = ld_ensure(h, ld.in, time_off + (time_cur ? sizeof(double) * pass : 0));
    if (!rc) rc = ld_ensure(h, ld.part, ld_part_bytes(pl.splits, p.top_k) * pass);
    if (!rc) rc = ld_ensure(h, ld.out, ld_out_bytes(p.top_k) * pass);
    if (rc) return rc;
    const size_t up_bytes = time_off + up16(sizeof(double) * pass), pinned = up_bytes + ld_out_bytes(p.top_k) * pass;   // the upload | rows
    if (pinned > ld.h_pass_cap) {
        if (ld.h_pass) S2M_HIP(h, hipHostFree(ld.h_pass));
        ld.h_pass = nullptr; ld.h_pass_cap = 0;
        S2M_HIP(h, hipHostMalloc((void**)&ld.h_pass, pinned));
        ld.h_pass_cap = pinned;
    }
    ld.last_scratch = pl.per_q * pass;
    unsigned char* h_rows = ld.h_pass + up_bytes;
    for (size_t i0 = 0; i0 < (size_t)m; i0 += pass) {
        const size_t mp = std::min(pass, (size_t)m - i0);
        memcpy(ld.h_pass, keys + i0, sizeof(int32_t) * mp);
        if (time_cur) memcpy(ld.h_pass + time_off, time_cur + i0, sizeof(double) * mp);
        S2M_HIP(h, hipMemcpyAsync(ld.in.p, ld.h_pass, time_cur ? time_off + sizeof(double) * mp : sizeof(int32_t) * mp, hipMemcpyHostToDevice, h->stream));
        LdArgs a{};
        a.pos = h->kf.pos.as<float4>(); a.time = h->kf.tdev.as<double>();
        a.keys = ld.in.as<int32_t>();
        a.time_cur = time_cur ? reinterpret_cast<const double*>(ld.in.as<unsigned char>() + time_off) : nullptr;
        a.m = (int)mp;
        a.set = ScManySet{ pl.first, pl.end, p.exclude_lo, p.exclude_hi, p.rel_lo, p.rel_hi };
        a.r2 = p.search_radius * p.search_radius;         // (float)(R*R), as s2m_loop_closure_rs forms it
        a.time_diff = (double)p.time_diff_s;
        a.top_k = p.top_k; a.splits = pl.splits;
        a.part = ld.part.as<unsigned long long>();
        a.out_key = ld.out.as<int32_t>();
        a.out_d2 = reinterpret_cast<float*>(a.out_key + K * mp);
        a.out_n = reinterpret_cast<int32_t*>(a.out_d2 + K * mp);
        S2M_HIP(h, ld_launch(h->stream, a));
        S2M_HIP(h, hipMemcpyAsync(h_rows, ld.out.p, ld_out_bytes(p.top_k) * mp, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));      // the one wait of the pass: the pinned block is free again
        ld.last_passes++;
        const int32_t* r_key = reinterpret_cast<const int32_t*>(h_rows);
        const float* r_d2 = reinterpret_cast<const float*>(r_key + K * mp);
        const int32_t* r_n = reinterpret_cast<const int32_t*>(r_d2 + K * mp);
        for (size_t i = 0; i < mp; i++) {
            const int32_t n = r_n[i];
            if (n < 0 || (size_t)n > K) return fail(h, S2M_ERR_HIP, "s2m_loop_detect_keys: the device left no candidate count");
            memcpy(key_pre + (i0 + i) * K, r_key + i * K, sizeof(int32_t) * (size_t)n);   // the entries behind stay the caller's
            if (d2) memcpy(d2 + (i0 + i) * K, r_d2 + i * K, sizeof(float) * (size_t)n);
            n_cand[i0 + i] = n;
        }
    }
    return S2M_OK;
}

// ---- test hooks (include/liorf_s2m_debug.h) ---------------------------------------------------------------------

int s2m_debug_loop_detect_pass(s2m_handle h, int32_t queries_per_pass)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (queries_per_pass < 0) return fail(h, S2M_ERR_INVALID_ARG, "loop-detection pass: 0 (the default) or a positive number of queries");
    h->ldet.pass = queries_per_pass;
    return S2M_OK;
}

int s2m_debug_loop_detect_splits(s2m_handle h, int32_t max_splits)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (max_splits < 0) return fail(h, S2M_ERR_INVALID_ARG, "loop-detection splits: 0 (the default) or a positive number of store splits");
    h->ldet.max_splits = max_splits;
    return S2M_OK;
}

int s2m_debug_loop_detect_shape(int32_t* tile_keys, int32_t* block_queries, int32_t* max_splits)
{
    if (!tile_keys || !block_queries || !max_splits) return S2M_ERR_INVALID_ARG;
    *tile_keys = kLdTile; *block_queries = kLdBlock; *max_splits = kLdMaxSplits;
    return S2M_OK;
}

int s2m_debug_loop_detect_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes)
{
    if (!h || !passes || !scratch_bytes) return S2M_ERR_INVALID_ARG;
    *passes = h->ldet.last_passes; *scratch_bytes = h->ldet.last_scratch;
    return S2M_OK;
}

}  // extern "C"
