// s2m_abi_pg_consistency.hip — C ABI of the mutually consistent loops among many candidates (s2m_pg_consistency.hip's kernels;
// DESIGN.md section 24): the argument table, the candidate table, the buffers, the one download.  It reads the pose graph's
// estimates on the device (brought up to date as an optimise does, s2m::host::pg_device_current) and otherwise uses
// s2m_context::pgc alone: no factor, estimate, key frame or loop state changes.  S2M_ERR_BUSY only while a launched optimise is
// pending, which writes the estimates.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "s2m_context.hpp"
#include "s2m_pg_consistency.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

static_assert(sizeof(s2m_pg_consistency_params) == 48 && sizeof(s2m_pg_consistency_result) == 24, "the structures on both sides of the ABI");
static_assert(sizeof(PgcCand) == 104, "the candidate table's record");

s2m_pg_consistency_params pgc_defaults()
{
    s2m_pg_consistency_params p{};
    p.tol_m = 0.3; p.tol_chord = 0.03; p.rate_m = 0.02; p.rate_chord = 0.0005;     // a starting point, not measured on real data
    return p;
}

bool tol_ok(double v) { return v >= 0.0 && std::isfinite(v); }

bool pgc_args_ok(int64_t n, const int32_t* key_from, const int32_t* key_to, const float* rel, int32_t m, const s2m_pg_consistency_params& p)
{
    if (m < 0 || m > S2M_PG_CONSISTENCY_MAX || n < 0) return false;
    if (!tol_ok(p.tol_m) || !tol_ok(p.tol_chord) || !tol_ok(p.rate_m) || !tol_ok(p.rate_chord)) return false;
    for (int k = 0; k < 4; k++) if (p.reserved[k] != 0) return false;
    if (m > 0 && (!key_from || !key_to || !rel)) return false;
    for (int32_t i = 0; i < m; i++) {
        if (key_from[i] < 0 || key_from[i] >= n || key_to[i] < 0 || key_to[i] >= n || key_from[i] == key_to[i]) return false;
        for (int k = 0; k < 6; k++) if (!std::isfinite(rel[6 * (size_t)i + k])) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int s2m_pg_consistency_default_params(s2m_pg_consistency_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    *p = pgc_defaults();
    return S2M_OK;
}

int s2m_pg_consistency_check_args(int32_t n_variables, const int32_t* key_from, const int32_t* key_to, const float* rel_xyzrpy, int32_t m,
                                  const s2m_pg_consistency_params* p)
{
    return pgc_args_ok(n_variables, key_from, key_to, rel_xyzrpy, m, p ? *p : pgc_defaults()) ? S2M_OK : S2M_ERR_INVALID_ARG;
}

int s2m_pg_consistent_loops(s2m_handle h, const int32_t* key_from, const int32_t* key_to, const float* rel_xyzrpy, int32_t m,
                            const s2m_pg_consistency_params* pp, uint8_t* selected, int32_t* degree, uint64_t* matrix, s2m_pg_consistency_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending)
        return fail(h, S2M_ERR_BUSY, "a launched pose-graph optimise is pending and writes the estimates: s2m_pg_optimize_poll / s2m_pg_optimize_collect it first");
    const s2m_pg_consistency_params p = pp ? *pp : pgc_defaults();
    const size_t n = h->pg.has_init.size();
    if (!pgc_args_ok((int64_t)n, key_from, key_to, rel_xyzrpy, m, p) || (m > 0 && !selected))
        return fail(h, S2M_ERR_INVALID_ARG, "s2m_pg_consistent_loops: m, null arrays, a key outside the graph, key_from == key_to, a measurement, a tolerance or reserved is invalid");
    if (m == 0) {
        if (out) { *out = s2m_pg_consistency_result{}; out->start = -1; }
        return S2M_OK;
    }
    for (size_t k = 0; k < n; k++)
        if (!h->pg.has_init[k]) return fail(h, S2M_ERR_INVALID_ARG, "s2m_pg_consistent_loops: a pose-graph variable has no initial value");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = pg_device_current(h);
    if (rc) return rc;
    s2m_context::PgConsistency& c = h->pgc;
    const size_t M = (size_t)m, W = pgc_words(m);
    const size_t tab_bytes = sizeof(PgcCand) * M, out_off = (tab_bytes + 15) & ~(size_t)15, out_bytes = pgc_out_bytes(m);
    if ((rc = ensure(h, c.s, sizeof(long long) * n)) || (rc = ensure(h, c.blk, sizeof(long long) * pgc_scan_blocks((int)n))) ||
        (rc = ensure(h, c.cand, tab_bytes)) || (rc = ensure(h, c.mat, sizeof(uint64_t) * M * W)) ||
        (rc = ensure(h, c.mat_rank, sizeof(uint64_t) * M * W)) || (rc = ensure(h, c.rank, sizeof(int32_t) * 3 * M)) ||
        (rc = ensure(h, c.out, out_bytes))) return rc;
    if (out_off + out_bytes > c.h_io_cap) {
        if (c.h_io) S2M_HIP(h, hipHostFree(c.h_io));
        c.h_io = nullptr; c.h_io_cap = 0;
        const size_t want = 2 * (out_off + out_bytes);
        S2M_HIP(h, hipHostMalloc((void**)&c.h_io, want));
        c.h_io_cap = want;
    }
    PgcCand* tab = reinterpret_cast<PgcCand*>(c.h_io);
    for (size_t i = 0; i < M; i++) {
        tab[i].from = key_from[i]; tab[i].to = key_to[i];
        pg_pose_to_state(rel_xyzrpy + 6 * i, tab[i].Z);    // as s2m_pg_add_between converts it
    }
    S2M_HIP(h, hipMemcpyAsync(c.cand.p, tab, tab_bytes, hipMemcpyHostToDevice, h->stream));
    PgcArgs a{};
    a.X = h->pg.est.as<double>(); a.n = (int)n;
    a.s = c.s.as<long long>(); a.blk = c.blk.as<long long>();
    a.cand = c.cand.as<PgcCand>(); a.m = m;
    a.tol_m = p.tol_m; a.tol_chord = p.tol_chord; a.rate_m = p.rate_m; a.rate_chord = p.rate_chord;
    a.mat = c.mat.as<unsigned long long>(); a.mat_rank = c.mat_rank.as<unsigned long long>();
    a.rank = c.rank.as<int32_t>();
    a.out = c.out.as<unsigned char>();
    S2M_HIP(h, pgc_launch(h->stream, a));
    unsigned char* back = c.h_io + out_off;
    S2M_HIP(h, hipMemcpyAsync(back, c.out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));      // selected | degree | record
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    PgcOut rec;
    memcpy(&rec, back + pgc_rec_off(m), sizeof(rec));
    if (rec.n_candidates != m || rec.n_selected < 1 || rec.n_selected > m || rec.start < 0 || rec.start >= m)
        return fail(h, S2M_ERR_HIP, "s2m_pg_consistent_loops: the device left no result record");
    if (matrix) {                                                                                // only a caller that asks pays for it
        S2M_HIP(h, hipMemcpyAsync(matrix, c.mat.p, sizeof(uint64_t) * M * W, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    memcpy(selected, back, M);
    if (degree) memcpy(degree, back + pgc_deg_off(m), sizeof(int32_t) * M);
    if (out) memcpy(out, &rec, sizeof(rec));
    return S2M_OK;
}

}  // extern "C"
