// s2m_abi_icp.hip — C ABI of the ICP alignment of host clouds (section 8(f) row F4), with or without an initial guess, and the
// diagnostics of the device loop (include/liorf_s2m_debug.h): everything that takes host clouds and no key-frame store.  Host
// orchestration of s2m_icp.hip's stages only; what it shares with the loop closure is declared in s2m_context.hpp.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

// ---- section 8(f) row F4: ICP loop-closure alignment -----------------------------------------------

int s2m_icp_default_params(s2m_icp_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    p->max_correspondence_distance = 20.0;      // historyKeyframeSearchRadius (10, include/utility.h:245) * 2 (:573)
    p->max_iterations = 100;                    // :574
    p->transformation_epsilon = 1e-6;           // :575
    p->euclidean_fitness_epsilon = 1e-6;        // :576
    return S2M_OK;
}

int s2m_icp_align(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                  const s2m_icp_params* p, s2m_icp_result* out)
{
    return s2m_icp_align_guess(h, src, n_src, tgt, n_tgt, stride_bytes, nullptr, p, out);
}

int s2m_icp_align_guess(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                        const float guess[16], const s2m_icp_params* p, s2m_icp_result* out)
{
    int rc = check_records(h, src, n_src, stride_bytes);
    if (rc) return rc;
    if ((rc = check_records(h, tgt, n_tgt, stride_bytes))) return rc;
    if (!out) return S2M_ERR_INVALID_ARG;
    if (guess && (rc = guess_ok(h, guess))) return rc;
    if ((rc = loop_busy(h))) return rc;
    IcpParams ip;
    if ((rc = icp_params_in(h, p, &ip))) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    if (n_src && (rc = stage_host_records(h, h->loop.icp_src, src, n_src * stride_bytes))) return rc;
    if (n_tgt && (rc = stage_host_records(h, h->loop.icp_tgt, tgt, n_tgt * stride_bytes))) return rc;
    IcpResult r;
    hipError_t e = icp_align(h->loop.icp, h->stream, h->loop.icp_src.as<unsigned char>(), n_src, h->loop.icp_tgt.as<unsigned char>(), n_tgt,
                             stride_bytes, ip, &r, guess);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "ICP alignment", e);
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    icp_result_out(r, out);
    return S2M_OK;
}

// ---- diagnostics of the device loop (include/liorf_s2m_debug.h) ---------------------------------------------------------

namespace {

// both host clouds into the ICP staging buffers, on the loop stream
int debug_stage(s2m_context* h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride)
{
    int rc = check_records(h, src, n_src, stride);
    if (rc) return rc;
    if ((rc = check_records(h, tgt, n_tgt, stride))) return rc;
    if ((rc = loop_busy(h))) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = loop_stream(h))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));            // (the staging buffers are the synchronous call's too)
    if ((rc = ensure(h, h->loop.icp_src, n_src * stride)) || (rc = ensure(h, h->loop.icp_tgt, n_tgt * stride))) return rc;
    if (n_src) S2M_HIP(h, hipMemcpyAsync(h->loop.icp_src.p, src, n_src * stride, hipMemcpyHostToDevice, h->loop.stream));
    if (n_tgt) S2M_HIP(h, hipMemcpyAsync(h->loop.icp_tgt.p, tgt, n_tgt * stride, hipMemcpyHostToDevice, h->loop.stream));
    return S2M_OK;
}

// the default icp_leaf: the leaf the hooks' grids are tuned at
float debug_leaf()
{
    s2m_loop_params lp;
    s2m_loop_default_params(&lp);
    return lp.icp_leaf;
}

// The list's alignments through the device loop on the loop stream, waited for; out: n results, those of the list's alignments at
// out[who], icp_result_none for an entry that took none (an empty cloud)
int debug_align_list(s2m_context* h, IcpList& al, const IcpParams& ip, const char* what, int32_t n, s2m_icp_result* out)
{
    const int rc = icp_list_align(h, h->loop.stream, al, ip, debug_leaf(), what);
    if (rc) return rc;
    for (int32_t i = 0; i < n; i++) icp_result_out(icp_result_none(), &out[i]);
    for (int k = 0; k < al.n; k++) icp_result_out(al.res[k], &out[al.who[k]]);
    return S2M_OK;
}

// one host source against n_cand host targets through the device loop, waited for: a slot per non-empty target, staged in the
// closure's target buffers; out: n_cand results
int debug_align_many(s2m_context* h, const void* src, size_t n_src, const void* const* tgts, const size_t* n_tgts, int32_t n_cand, size_t stride,
                     const IcpParams& ip, s2m_icp_result* out, const float* guesses = nullptr /* n_cand row-major 4x4, or none */)
{
    int rc = debug_stage(h, src, n_src, nullptr, 0, stride);
    if (rc) return rc;
    s2m_context::LoopClosure& L = h->loop;
    IcpList al(IcpForm::kSlots, stride);
    for (int32_t i = 0; i < n_cand; i++) {
        if ((rc = check_records(h, tgts[i], n_tgts[i], stride))) return rc;
        if (!n_src || !n_tgts[i]) continue;
        if ((rc = ensure(h, L.target(i), n_tgts[i] * stride))) return rc;
        S2M_HIP(h, hipMemcpyAsync(L.target(i).p, tgts[i], n_tgts[i] * stride, hipMemcpyHostToDevice, L.stream));
        al.add(L.icp_src.p, n_src, L.target(i).p, n_tgts[i], guesses ? guesses + 16 * (size_t)i : nullptr, (size_t)i);
    }
    return debug_align_list(h, al, ip, "ICP device loop", n_cand, out);
}

}  // namespace

int s2m_debug_icp_tuning(s2m_handle h, float cell_in_leaves, int32_t shell_cap, int32_t use_grid)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!(cell_in_leaves >= 0.0f) || !std::isfinite(cell_in_leaves) || shell_cap < 0)
        return fail(h, S2M_ERR_INVALID_ARG, "cell edge (in leaves) and shell cap must not be negative");
    const int rc = loop_busy(h);
    if (rc) return rc;
    h->loop.tune.cell = cell_in_leaves;                     // 0: the built-in edge
    h->loop.tune.shell_cap = shell_cap > 0 ? shell_cap : kIcpShellCap;
    h->loop.tune.use_grid = use_grid < 0 ? (kIcpUseGrid ? 1 : 0) : (use_grid != 0);
    return S2M_OK;
}

int s2m_debug_icp_nearest(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes, int32_t mode,
                          uint64_t* keys, int32_t* n_fallback)
{
    return s2m_debug_icp_time_nearest(h, src, n_src, tgt, n_tgt, stride_bytes, mode, 0, keys, n_fallback, nullptr, nullptr);
}

int s2m_debug_icp_time_nearest(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes, int32_t mode,
                               int32_t reps, uint64_t* keys, int32_t* n_fallback, float* us_build, float* us_search)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if ((mode != 0 && mode != 1) || reps < 0 || (n_src && !keys && reps == 0)) return fail(h, S2M_ERR_INVALID_ARG, "mode is 0 or 1, keys must not be null");
    int rc = debug_stage(h, src, n_src, tgt, n_tgt, stride_bytes);
    if (rc) return rc;
    if (n_fallback) *n_fallback = 0;
    if (us_build) *us_build = 0.0f;
    if (us_search) *us_search = 0.0f;
    if (n_src == 0) return S2M_OK;
    if (n_tgt == 0) {                                       // no target: no source has a match
        for (size_t i = 0; keys && i < n_src; i++) keys[i] = ~0ull;
        S2M_HIP(h, hipStreamSynchronize(h->loop.stream));
        return S2M_OK;
    }
    int nf = 0;
    const hipError_t e = icp_dev_nearest(h->loop.icp, h->loop.stream, h->loop.icp_src.as<unsigned char>(), n_src, h->loop.icp_tgt.as<unsigned char>(),
                                         n_tgt, stride_bytes, mode, loop_tuning(h, debug_leaf()), reinterpret_cast<unsigned long long*>(keys), &nf,
                                         reps, us_build, us_search);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "ICP nearest-neighbour search", e);
    if (n_fallback) *n_fallback = nf;
    return S2M_OK;
}

int s2m_debug_icp_align_device(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                               const s2m_icp_params* p, s2m_icp_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null ICP result");
    IcpParams ip;
    int rc = icp_params_in(h, p, &ip);
    if (rc || (rc = check_records(h, src, n_src, stride_bytes)) || (rc = check_records(h, tgt, n_tgt, stride_bytes))) return rc;   // (both before BUSY)
    return debug_align_many(h, src, n_src, &tgt, &n_tgt, 1, stride_bytes, ip, out);
}

int s2m_debug_icp_align_many_device(s2m_handle h, const void* src, size_t n_src, const void* const* tgts, const size_t* n_tgts, int32_t n_cand,
                                    size_t stride_bytes, const s2m_icp_params* p, s2m_icp_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out || !tgts || !n_tgts || n_cand < 1 || n_cand > S2M_LOOP_MAX_CANDIDATES)
        return fail(h, S2M_ERR_INVALID_ARG, "null ICP result or target list, or not 1 .. S2M_LOOP_MAX_CANDIDATES targets");
    IcpParams ip;
    const int rc = icp_params_in(h, p, &ip);
    return rc ? rc : debug_align_many(h, src, n_src, tgts, n_tgts, n_cand, stride_bytes, ip, out);
}

int s2m_debug_icp_align_guess_many_device(s2m_handle h, const void* src, size_t n_src, const void* const* tgts, const size_t* n_tgts,
                                          const float* guesses, int32_t n_cand, size_t stride_bytes, const s2m_icp_params* p, s2m_icp_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out || !tgts || !n_tgts || n_cand < 1 || n_cand > S2M_LOOP_MAX_CANDIDATES)
        return fail(h, S2M_ERR_INVALID_ARG, "null ICP result or target list, or not 1 .. S2M_LOOP_MAX_CANDIDATES targets");
    IcpParams ip;
    int rc = icp_params_in(h, p, &ip);
    for (int32_t i = 0; !rc && guesses && i < n_cand; i++) rc = guess_ok(h, guesses + 16 * (size_t)i);
    return rc ? rc : debug_align_many(h, src, n_src, tgts, n_tgts, n_cand, stride_bytes, ip, out, guesses);
}

// P host pairs through the table form of the device loop, waited for: the clouds staged in the arena of a many-keys pass
int s2m_debug_icp_align_pairs_device(s2m_handle h, const void* const* srcs, const size_t* n_srcs, const void* const* tgts, const size_t* n_tgts,
                                     int32_t n_pairs, size_t stride_bytes, const float* const* guesses, const s2m_icp_params* p, s2m_icp_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out || !srcs || !n_srcs || !tgts || !n_tgts || n_pairs < 1 || n_pairs > kIcpMaxPairs)
        return fail(h, S2M_ERR_INVALID_ARG, "null ICP results or cloud lists, or not 1 .. 64 pairs");
    IcpParams ip;
    int rc = icp_params_in(h, p, &ip);
    for (int32_t k = 0; !rc && k < n_pairs; k++) {
        if ((rc = check_records(h, srcs[k], n_srcs[k], stride_bytes)) || (rc = check_records(h, tgts[k], n_tgts[k], stride_bytes))) break;
        if (guesses && guesses[k]) rc = guess_ok(h, guesses[k]);
    }
    if (rc || (rc = debug_stage(h, nullptr, 0, nullptr, 0, stride_bytes))) return rc;             // (BUSY, the loop stream)
    s2m_context::LoopClosure& L = h->loop;
    IcpList al(IcpForm::kTable, stride_bytes, &L.many_arena);
    L.many_used = 0;
    for (int32_t k = 0; k < n_pairs; k++) {
        if (!n_srcs[k] || !n_tgts[k]) continue;
        size_t s = 0, t = 0;
        if ((rc = arena_put(h, L.stream, srcs[k], hipMemcpyHostToDevice, n_srcs[k] * stride_bytes, &s)) ||
            (rc = arena_put(h, L.stream, tgts[k], hipMemcpyHostToDevice, n_tgts[k] * stride_bytes, &t))) return rc;
        al.add_at(s, n_srcs[k], t, n_tgts[k], guesses ? guesses[k] : nullptr, (size_t)k);
    }
    return debug_align_list(h, al, ip, "ICP device loop over pairs", n_pairs, out);
}

int s2m_debug_icp_grid_check_args(const void* const* tgts, const size_t* n_tgts, int32_t n_cand, size_t stride_bytes, const s2m_debug_icp_grid_out* out)
{
    if (!out || !tgts || !n_tgts || n_cand < 1 || n_cand > S2M_LOOP_MAX_CANDIDATES) return S2M_ERR_INVALID_ARG;
    if (stride_bytes < 12 || (stride_bytes & 3)) return S2M_ERR_INVALID_ARG;
    for (int32_t i = 0; i < n_cand; i++) {
        if (!tgts[i] || n_tgts[i] == 0 || (reinterpret_cast<uintptr_t>(tgts[i]) & 3) != 0) return S2M_ERR_INVALID_ARG;
        if (n_tgts[i] > (size_t)0x3fffffff) return S2M_ERR_CAPACITY;
    }
    return S2M_OK;
}

int s2m_debug_icp_grid(s2m_handle h, const void* const* tgts, const size_t* n_tgts, int32_t n_cand, size_t stride_bytes,
                       s2m_debug_icp_grid_out* out, int32_t* const* cell_start, int32_t* const* cell_end, int32_t* const* order)
{
    static_assert(S2M_DEBUG_ICP_GRID_MAX_CELLS == kIcpGridMaxCells, "the header's array size is the grid's");
    static_assert(sizeof(s2m_debug_icp_grid_out) == sizeof(IcpGridInfo) && sizeof(int32_t) == sizeof(int), "filled in place");
    if (!h) return S2M_ERR_INVALID_ARG;
    int rc = s2m_debug_icp_grid_check_args(tgts, n_tgts, n_cand, stride_bytes, out);
    if (rc) return fail(h, rc, "grid: 1 .. S2M_LOOP_MAX_CANDIDATES non-empty targets of 4-byte aligned records (stride >= 12, a multiple of 4), an output array");
    if ((rc = debug_stage(h, nullptr, 0, nullptr, 0, stride_bytes))) return rc;                  // (BUSY, the loop stream)
    s2m_context::LoopClosure& L = h->loop;
    const unsigned char* d_tgt[S2M_LOOP_MAX_CANDIDATES];
    for (int32_t i = 0; i < n_cand; i++) {
        if ((rc = ensure(h, L.target(i), n_tgts[i] * stride_bytes))) return rc;
        S2M_HIP(h, hipMemcpyAsync(L.target(i).p, tgts[i], n_tgts[i] * stride_bytes, hipMemcpyHostToDevice, L.stream));
        d_tgt[i] = L.target(i).as<unsigned char>();
    }
    const hipError_t e = icp_dev_grid(L.icp, L.stream, d_tgt, n_tgts, n_cand, stride_bytes, loop_tuning(h, debug_leaf()),
                                      reinterpret_cast<IcpGridInfo*>(out), cell_start, cell_end, order);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(L.stream);
        return fail(h, S2M_ERR_HIP, "ICP grid", e);
    }
    return S2M_OK;
}

// ---- the close and the sums of an ICP iteration on their own (tests/test_icp_close_gpu.py) ------------------------------------

int s2m_debug_icp_close_check_args(int32_t n, const double* sums, const s2m_debug_icp_state* in, const s2m_icp_params* p, const s2m_debug_icp_state* out)
{
    if (n < 1 || n > S2M_LOOP_MANY_MAX_PAIRS || !sums || !in || !out) return S2M_ERR_INVALID_ARG;
    if (p && (!(p->max_correspondence_distance > 0.0) || p->max_iterations < 1)) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

int s2m_debug_icp_close(s2m_handle h, int32_t n, const double* sums, const s2m_debug_icp_state* in, const s2m_icp_params* p, s2m_debug_icp_state* out)
{
    static_assert(sizeof(s2m_debug_icp_state) == sizeof(IcpLoopState) && offsetof(s2m_debug_icp_state, prev_mse) == offsetof(IcpLoopState, prev_mse) &&
                  offsetof(s2m_debug_icp_state, done) == offsetof(IcpLoopState, done), "handed over in place");
    static_assert(S2M_LOOP_MANY_MAX_PAIRS == kIcpMaxPairs, "a block per pair of the table");
    if (!h) return S2M_ERR_INVALID_ARG;
    int rc = s2m_debug_icp_close_check_args(n, sums, in, p, out);
    if (rc) return fail(h, rc, "close: 1 .. S2M_LOOP_MANY_MAX_PAIRS rows of sums and states, valid ICP parameters");
    IcpParams ip;
    if ((rc = icp_params_in(h, p, &ip)) || (rc = debug_stage(h, nullptr, 0, nullptr, 0, 16))) return rc;     // (BUSY, the loop stream)
    const hipError_t e = icp_dev_close(h->loop.icp, h->loop.stream, n, sums, reinterpret_cast<const IcpLoopState*>(in), ip,
                                       reinterpret_cast<IcpLoopState*>(out));
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->loop.stream);
        return fail(h, S2M_ERR_HIP, "ICP close", e);
    }
    return S2M_OK;
}

int s2m_debug_icp_sums_check_args(const void* const* srcs, const size_t* n_srcs, const void* const* tgts, const size_t* n_tgts, int32_t n_pairs,
                                  size_t stride_bytes, int32_t form, const double* sums, const int32_t* n_rows)
{
    if (form != S2M_DEBUG_ICP_SUMS_SLOTS && form != S2M_DEBUG_ICP_SUMS_TABLE) return S2M_ERR_INVALID_ARG;
    if (!srcs || !n_srcs || !tgts || !n_tgts || !sums || !n_rows) return S2M_ERR_INVALID_ARG;
    if (n_pairs < 1 || n_pairs > (form == S2M_DEBUG_ICP_SUMS_TABLE ? S2M_LOOP_MANY_MAX_PAIRS : S2M_LOOP_MAX_CANDIDATES)) return S2M_ERR_INVALID_ARG;
    if (stride_bytes < 12 || (stride_bytes & 3)) return S2M_ERR_INVALID_ARG;
    for (int32_t k = 0; k < n_pairs; k++) {
        if (!srcs[k] || !tgts[k] || n_srcs[k] == 0 || n_tgts[k] == 0) return S2M_ERR_INVALID_ARG;
        if ((reinterpret_cast<uintptr_t>(srcs[k]) & 3) != 0 || (reinterpret_cast<uintptr_t>(tgts[k]) & 3) != 0) return S2M_ERR_INVALID_ARG;
        if (n_srcs[k] > (size_t)0x3fffffff || n_tgts[k] > (size_t)0x3fffffff) return S2M_ERR_CAPACITY;
        if (form == S2M_DEBUG_ICP_SUMS_SLOTS && (srcs[k] != srcs[0] || n_srcs[k] != n_srcs[0])) return S2M_ERR_INVALID_ARG;
    }
    return S2M_OK;
}

int s2m_debug_icp_sums(s2m_handle h, const void* const* srcs, const size_t* n_srcs, const void* const* tgts, const size_t* n_tgts, int32_t n_pairs,
                       size_t stride_bytes, int32_t form, double max_correspondence_distance, double* sums, int32_t* n_rows,
                       double* const* parts, uint64_t* const* keys)
{
    static_assert(S2M_LOOP_MAX_CANDIDATES == kIcpMaxSlots && sizeof(int32_t) == sizeof(int), "a slot per target; n_rows filled in place");
    if (!h) return S2M_ERR_INVALID_ARG;
    int rc = s2m_debug_icp_sums_check_args(srcs, n_srcs, tgts, n_tgts, n_pairs, stride_bytes, form, sums, n_rows);
    if (rc) return fail(h, rc, "sums: non-empty clouds of 4-byte aligned records, 1 .. 8 targets of one source (slots) or 1 .. 64 pairs (table)");
    if (!(max_correspondence_distance > 0.0)) return fail(h, S2M_ERR_INVALID_ARG, "ICP needs a positive correspondence distance");
    if ((rc = debug_stage(h, nullptr, 0, nullptr, 0, stride_bytes))) return rc;                  // (BUSY, the loop stream)
    const bool table = form == S2M_DEBUG_ICP_SUMS_TABLE;
    s2m_context::LoopClosure& L = h->loop;
    IcpList al(table ? IcpForm::kTable : IcpForm::kSlots, stride_bytes, &L.many_arena);
    L.many_used = 0;
    size_t s = 0, t = 0;
    for (int32_t k = 0; k < n_pairs; k++) {                 // (the slots: one source, staged once)
        if ((table || k == 0) && (rc = arena_put(h, L.stream, srcs[k], hipMemcpyHostToDevice, n_srcs[k] * stride_bytes, &s))) return rc;
        if ((rc = arena_put(h, L.stream, tgts[k], hipMemcpyHostToDevice, n_tgts[k] * stride_bytes, &t))) return rc;
        al.add_at(s, n_srcs[k], t, n_tgts[k], nullptr, (size_t)k);
    }
    const hipError_t e = icp_dev_sums(L.icp, L.stream, al.set(), max_correspondence_distance, loop_tuning(h, debug_leaf()), sums, n_rows, parts,
                                      reinterpret_cast<unsigned long long* const*>(keys));
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(L.stream);
        return fail(h, S2M_ERR_HIP, "ICP sums", e);
    }
    return S2M_OK;
}
