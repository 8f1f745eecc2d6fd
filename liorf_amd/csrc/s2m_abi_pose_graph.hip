// s2m_abi_pose_graph.hip — C ABI of the pose graph: the factor list and the estimates' mirror on the host, the device tables,
// the Gauss-Newton loop around s2m_pose_graph.hip's kernels, the marginal, and correctPoses() into the key-frame store.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

int s2m_pg_default_params(s2m_pg_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    const double prior[6] = { 1e-2, 1e-2, M_PI * M_PI, 1e8, 1e8, 1e8 };     // :1390
    const double odom[6] = { 1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4 };           // :1394
    for (int k = 0; k < 6; k++) { p->prior_var[k] = prior[k]; p->odom_var[k] = odom[k]; p->sc_loop_var[k] = 0.5; }   // :712-713
    p->sc_loop_robust_k = 1.0;                                               // :716-719
    p->relative_error_tol = 1e-5;
    p->absolute_error_tol = 1e-5;
    p->cg_rel_tol = 1e-13;
    p->max_iterations = 100;
    p->cg_max_iterations = 0;
    return S2M_OK;
}

int s2m_pg_check_args(int32_t kind, int32_t n_variables, int32_t key_a, int32_t key_b, const float* values, const double* var, double robust_k)
{
    if (kind < S2M_PG_PRIOR || kind > S2M_PG_INITIAL || n_variables < 0 || !values) return S2M_ERR_INVALID_ARG;
    const int nv = kind == S2M_PG_GPS ? 3 : 6;
    for (int k = 0; k < nv; k++) if (!std::isfinite(values[k])) return S2M_ERR_INVALID_ARG;
    if (kind != S2M_PG_INITIAL) {
        if (!var) return S2M_ERR_INVALID_ARG;
        for (int k = 0; k < nv; k++) if (!(var[k] > 0.0) || !std::isfinite(var[k])) return S2M_ERR_INVALID_ARG;
    }
    if (!(robust_k >= 0.0) || !std::isfinite(robust_k)) return S2M_ERR_INVALID_ARG;
    if (key_a < 0 || key_a > n_variables) return S2M_ERR_INVALID_ARG;
    if (kind == S2M_PG_BETWEEN) {
        if (key_b < 0 || key_b > n_variables || key_a == key_b) return S2M_ERR_INVALID_ARG;
    }
    return S2M_OK;                  // (key_a != key_b and both <= n_variables: at most one of them is new)
}

// The tail rule of a launched optimise: X <- D X with D = a_now a_launch^-1, every three-term sum as ((a0 b0 + a1 b1) + a2 b2).
int s2m_debug_pg_rebase(const double a_launch[12], const double a_now[12], double X[12])
{
    if (!a_launch || !a_now || !X) return S2M_ERR_INVALID_ARG;
    double D[12], O[12];
    for (int i = 0; i < 3; i++)                             // D_R = A'_R A_R^T
        for (int j = 0; j < 3; j++)
            D[i * 3 + j] = (a_now[i * 3] * a_launch[j * 3] + a_now[i * 3 + 1] * a_launch[j * 3 + 1]) + a_now[i * 3 + 2] * a_launch[j * 3 + 2];
    for (int i = 0; i < 3; i++)                             // D_t = A'_t - D_R A_t
        D[9 + i] = a_now[9 + i] - ((D[i * 3] * a_launch[9] + D[i * 3 + 1] * a_launch[10]) + D[i * 3 + 2] * a_launch[11]);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) O[i * 3 + j] = (D[i * 3] * X[j] + D[i * 3 + 1] * X[3 + j]) + D[i * 3 + 2] * X[6 + j];
        O[9 + i] = ((D[i * 3] * X[9] + D[i * 3 + 1] * X[10]) + D[i * 3 + 2] * X[11]) + D[9 + i];
    }
    std::copy(O, O + 12, X);
    return S2M_OK;
}

void s2m::host::pg_drop_pending(s2m_context* h, bool destroy)
{
    auto& g = h->pg;
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    g.pending = false;
    if (!destroy) return;
    if (g.ev_ready) (void)hipEventDestroy(g.ev_ready);
    if (g.ev_range) (void)hipEventDestroy(g.ev_range);
    if (g.stream) (void)hipStreamDestroy(g.stream);
    if (g.h_rec) (void)hipHostFree(g.h_rec);
    g.ev_ready = g.ev_range = nullptr; g.stream = nullptr; g.h_rec = nullptr;
}

namespace {

constexpr size_t kPgMaxVars = (size_t)1 << 24;          // as the key-frame store
constexpr int kPgCgChunk = 24;          // CG iterations after which the host reads the stop flags; a launched optimise's segment holds as many

void pose_to_state(const float p[6], double X[12])     // Rot3::RzRyRx(roll, pitch, yaw), fp64
{
    const double cr = std::cos((double)p[3]), sr = std::sin((double)p[3]), cp = std::cos((double)p[4]), sp = std::sin((double)p[4]);
    const double cy = std::cos((double)p[5]), sy = std::sin((double)p[5]);
    X[0] = cy * cp; X[1] = cy * sp * sr - sy * cr; X[2] = sy * sr + cy * sp * cr;
    X[3] = sy * cp; X[4] = cy * cr + sy * sp * sr; X[5] = sy * sp * cr - cy * sr;
    X[6] = -sp;     X[7] = cp * sr;                X[8] = cp * cr;
    X[9] = p[0]; X[10] = p[1]; X[11] = p[2];
}

size_t pg_n(const s2m_context* h) { return h->pg.has_init.size(); }

void touch(s2m_context* h, int32_t key)
{
    if ((size_t)key == pg_n(h)) {
        h->pg.has_init.push_back(0);
        h->pg.dirty.push_back(0);
        h->pg.X.resize(h->pg.X.size() + 12, 0.0);
        h->pg.topo_dirty = true;
    }
}

// the host mirror holds the newest estimates (the device's, except where set_initial wrote since)
int host_current(s2m_context* h)
{
    auto& g = h->pg;
    if (!g.dev_newer) return S2M_OK;
    std::vector<double> tmp(12 * g.n_dev);
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipMemcpyAsync(tmp.data(), g.est.p, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < g.n_dev; k++)
        if (!g.dirty[k]) std::copy(tmp.begin() + 12 * k, tmp.begin() + 12 * (k + 1), g.X.begin() + 12 * k);
    g.dev_newer = false;
    return S2M_OK;
}

// the device holds every variable's newest estimate; variables first .. first+count-1 must have one
int upload_state(s2m_context* h, size_t first, size_t count)
{
    auto& g = h->pg;
    const size_t n = pg_n(h);
    for (size_t k = first; k < first + count; k++)
        if (!g.has_init[k]) return fail(h, S2M_ERR_INVALID_ARG, "a pose-graph variable has no initial value");
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    const size_t bytes = sizeof(double) * 12 * n;
    if (bytes > g.est.cap || bytes > g.trial.cap) {        // the arrays move: everything goes up again
        if ((rc = host_current(h))) return rc;
        std::fill(g.dirty.begin(), g.dirty.end(), 1);
        if ((rc = ensure(h, g.est, 2 * bytes)) || (rc = ensure(h, g.trial, 2 * bytes))) return rc;
        g.n_dev = 0;
    }
    for (size_t k = g.n_dev; k < n; k++) g.dirty[k] = 1;
    for (size_t k = 0; k < n;) {
        if (!g.dirty[k]) { k++; continue; }
        size_t e = k;
        while (e < n && g.dirty[e]) e++;
        S2M_HIP(h, hipMemcpyAsync(g.est.as<double>() + 12 * k, g.X.data() + 12 * k, sizeof(double) * 12 * (e - k), hipMemcpyHostToDevice, h->stream));
        k = e;
    }
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    std::fill(g.dirty.begin(), g.dirty.end(), 0);
    g.n_dev = n;
    return S2M_OK;
}

template <typename T>
int upload_vec(s2m_context* h, DevBuf& b, const std::vector<T>& v)
{
    int rc = ensure(h, b, sizeof(T) * std::max<size_t>(v.size(), 1));
    if (rc) return rc;
    if (!v.empty()) S2M_HIP(h, hipMemcpyAsync(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, h->stream));
    return S2M_OK;
}

int setup_scan(s2m_context* h, int which, int n, PgScan& sc)
{
    auto& g = h->pg;
    sc.rev = which;
    sc.levels = 0;
    size_t total = 0;
    for (int m = n;; m = (m + kPgGroup - 1) / kPgGroup) {
        if (sc.levels >= kPgMaxLevels) return fail(h, S2M_ERR_CAPACITY, "pose graph too large");
        sc.n[sc.levels++] = m;
        total += (size_t)m;
        if (m <= kPgGroup) break;
    }
    int rc;
    if ((rc = ensure(h, g.scan_M[which], sizeof(double) * 36 * total)) || (rc = ensure(h, g.scan_Pre[which], sizeof(double) * 36 * total)) ||
        (rc = ensure(h, g.scan_loc[which], sizeof(double) * 6 * total)) || (rc = ensure(h, g.scan_C0[which], sizeof(double) * 36 * (size_t)n))) return rc;
    size_t at = 0;
    for (int l = 0; l < sc.levels; l++) {
        sc.M[l] = g.scan_M[which].as<double>() + 36 * at;
        sc.Pre[l] = g.scan_Pre[which].as<double>() + 36 * at;
        sc.loc[l] = g.scan_loc[which].as<double>() + 6 * at;
        at += (size_t)sc.n[l];
    }
    sc.C0 = g.scan_C0[which].as<double>();
    return S2M_OK;
}

// estimates, factor tables and work arrays on the device, h->pg.dev filled in
int prepare(s2m_context* h)
{
    auto& g = h->pg;
    const size_t n = pg_n(h);
    int rc;
    // the chain: the first prior on key 0 and, per i, the first plain between factor i -> i+1
    std::vector<int> chain_of(n, -1);
    for (size_t f = 0; f < g.factors.size(); f++) {
        const PgFactor& fa = g.factors[f];
        if (fa.type == kPgPrior && fa.i == 0 && chain_of[0] < 0) chain_of[0] = (int)f;
        if (fa.type == kPgBetween && fa.j == fa.i + 1 && fa.k == 0.0 && chain_of[(size_t)fa.j] < 0) chain_of[(size_t)fa.j] = (int)f;
    }
    if (chain_of[0] < 0) return fail(h, S2M_ERR_INVALID_ARG, "pose graph: key 0 has no prior");
    for (size_t k = 1; k < n; k++)
        if (chain_of[k] < 0) return fail(h, S2M_ERR_INVALID_ARG, "pose graph: a variable is not on the odometry chain from key 0");
    if ((rc = upload_state(h, 0, n))) return rc;
    if (!g.h_sc) S2M_HIP(h, hipHostMalloc((void**)&g.h_sc, sizeof(PgScalars) * kPgBlockCols));   // one per column of a solve
    if (g.topo_dirty) {
        std::vector<char> on_chain(g.factors.size(), 0);
        std::vector<PgFactor> chain(n), extra;
        for (size_t k = 0; k < n; k++) { chain[k] = g.factors[(size_t)chain_of[k]]; on_chain[(size_t)chain_of[k]] = 1; }
        for (size_t f = 0; f < g.factors.size(); f++) if (!on_chain[f]) extra.push_back(g.factors[f]);
        std::vector<int32_t> start(n + 1, 0);
        for (const PgFactor& fa : extra) { start[(size_t)fa.i + 1]++; if (fa.type == kPgBetween) start[(size_t)fa.j + 1]++; }
        for (size_t k = 0; k < n; k++) start[k + 1] += start[k];
        std::vector<PgIncidence> inc((size_t)start[n]);
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (size_t x = 0; x < extra.size(); x++) {          // in factor order: each key's sum has a fixed order
            inc[(size_t)fill[(size_t)extra[x].i]++] = PgIncidence{ (int32_t)x, 0 };
            if (extra[x].type == kPgBetween) inc[(size_t)fill[(size_t)extra[x].j]++] = PgIncidence{ (int32_t)x, 1 };
        }
        if ((rc = upload_vec(h, g.chain, chain)) || (rc = upload_vec(h, g.extra, extra)) || (rc = upload_vec(h, g.inc_start, start)) ||
            (rc = upload_vec(h, g.inc, inc))) return rc;
        S2M_HIP(h, hipStreamSynchronize(h->stream));       // (the host vectors above are read by the copies until here)
        const size_t m = std::max<size_t>(extra.size(), 1);
        if ((rc = ensure(h, g.Binv, sizeof(double) * 36 * n)) || (rc = ensure(h, g.Aof, sizeof(double) * 36 * n)) ||
            (rc = ensure(h, g.rc, sizeof(double) * 6 * n)) || (rc = ensure(h, g.Ji, sizeof(double) * 36 * m)) ||
            (rc = ensure(h, g.Jj, sizeof(double) * 36 * m)) || (rc = ensure(h, g.rx, sizeof(double) * 6 * m)) ||
            (rc = ensure(h, g.ferr, sizeof(double) * (n + m))) || (rc = ensure(h, g.fw, sizeof(double) * (n + m))) ||
            (rc = ensure(h, g.vecs, sizeof(double) * 6 * (9 * n + m))) || (rc = ensure(h, g.partial, sizeof(double) * kPgDotBlocks)) ||
            (rc = ensure(h, g.sc, sizeof(PgScalars)))) return rc;
        PgDev& d = g.dev;
        d.n = (int32_t)n; d.n_extra = (int32_t)extra.size();
        if ((rc = setup_scan(h, 0, d.n, d.fwd)) || (rc = setup_scan(h, 1, d.n, d.bwd))) return rc;
        d.chain = g.chain.as<PgFactor>(); d.extra = g.extra.as<PgFactor>();
        d.inc_start = g.inc_start.as<int32_t>(); d.inc = g.inc.as<PgIncidence>();
        d.Binv = g.Binv.as<double>(); d.Aof = g.Aof.as<double>(); d.rc = g.rc.as<double>();
        d.Ji = g.Ji.as<double>(); d.Jj = g.Jj.as<double>(); d.rx = g.rx.as<double>();
        d.ferr = g.ferr.as<double>(); d.fw = g.fw.as<double>();
        double* v = g.vecs.as<double>();
        double** slots[9] = { &d.b, &d.y, &d.r, &d.p, &d.q, &d.t1, &d.t2, &d.g, &d.delta };
        for (int k = 0; k < 9; k++) *slots[k] = v + 6 * n * (size_t)k;
        d.u = v + 6 * n * 9;
        d.partial = g.partial.as<double>();
        d.sc = g.sc.as<PgScalars>();
        g.topo_dirty = false;
    }
    g.dev.X = g.est.as<double>();
    g.dev.Xtrial = g.trial.as<double>();
    return S2M_OK;
}

int read_scalars(s2m_context* h)
{
    S2M_HIP(h, hipMemcpyAsync(h->pg.h_sc, h->pg.dev.sc, sizeof(PgScalars), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int pg_max_cg(const PgDev& d, const s2m_pg_params& prm)
{
    if (d.n_extra == 0) return 1;                          // K = 0: the first step is exact
    return prm.cg_max_iterations > 0 ? prm.cg_max_iterations : 6 * d.n_extra + 20;
}

// CG on (I + K^T K) y_c = b_c for the columns of `c` with the b_c in place (kPgOne: the graph's own vectors); every column's
// scalars come back in one copy per chunk of iterations (h_sc[c]); ends when all have stopped
int run_cg(s2m_context* h, const PgDev& db, const PgCols& c, const s2m_pg_params& prm)
{
    const int max_cg = pg_max_cg(db, prm);
    S2M_HIP(h, pg_cg_begin(h->stream, db, c, prm.cg_rel_tol, max_cg));
    PgScalars* hs = h->pg.h_sc;
    for (int done = 0; done < max_cg;) {
        const int k = std::min(kPgCgChunk, max_cg - done);
        S2M_HIP(h, pg_cg_iterations(h->stream, db, c, k));
        S2M_HIP(h, hipMemcpyAsync(hs, db.sc, sizeof(PgScalars) * (size_t)c.cols, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        done += k;
        bool all = true;
        for (int q = 0; q < c.cols; q++) all = all && hs[q].stop;
        if (all) break;
    }
    return S2M_OK;
}

// ---- the block solve behind s2m_pg_marginals / s2m_pg_joint_marginal ----
static_assert(kPgBlockCols == S2M_PG_BLOCK_COLUMNS && kPgBlockCols >= 12 && kPgBlockCols % 6 == 0, "a pass holds whole keys, and a joint marginal");

// block storage for `cols` columns (grow-only) after prepare(): db is the graph's PgDev with its work arrays in that storage
int prepare_block(s2m_context* h, int cols, PgDev& db, PgCols& c)
{
    auto& g = h->pg;
    const PgDev& d = g.dev;
    const size_t n = (size_t)d.n, m = std::max<size_t>((size_t)d.n_extra, 1), C = (size_t)cols;
    size_t total = 0;
    for (int l = 0; l < d.fwd.levels; l++) total += (size_t)d.fwd.n[l];
    int rc;
    if ((rc = ensure(h, g.blk_vecs, sizeof(double) * 6 * (9 * n + m) * C)) || (rc = ensure(h, g.blk_loc[0], sizeof(double) * 6 * total * C)) ||
        (rc = ensure(h, g.blk_loc[1], sizeof(double) * 6 * total * C)) || (rc = ensure(h, g.blk_partial, sizeof(double) * kPgDotBlocks * C)) ||
        (rc = ensure(h, g.blk_sc, sizeof(PgScalars) * C)) || (rc = ensure(h, g.blk_rows, sizeof(double) * 12 * C))) return rc;
    db = d;
    double* v = g.blk_vecs.as<double>();
    double** slots[9] = { &db.b, &db.y, &db.r, &db.p, &db.q, &db.t1, &db.t2, &db.g, &db.delta };
    for (int k = 0; k < 9; k++) *slots[k] = v + 6 * n * C * (size_t)k;
    db.u = v + 6 * n * C * 9;
    db.partial = g.blk_partial.as<double>();
    db.sc = g.blk_sc.as<PgScalars>();
    for (int l = 0; l < d.fwd.levels; l++) {               // each column's levels lie as the single form's do
        db.fwd.loc[l] = g.blk_loc[0].as<double>() + (d.fwd.loc[l] - d.fwd.loc[0]);
        db.bwd.loc[l] = g.blk_loc[1].as<double>() + (d.bwd.loc[l] - d.bwd.loc[0]);
    }
    c = PgCols{ cols, 0, 6 * n, 6 * m, 6 * total, 6 * total };
    return S2M_OK;
}

// One pass: column k is e_(at[k]) through J_c^-T, CG and J_c^-1; rows[12 k ..] holds its delta at keys ka[k] and kb[k].
int solve_pass(s2m_context* h, const PgDev& db, const PgCols& c, const s2m_pg_params& prm, const PgColAt& at, const PgColAt& ka, const PgColAt& kb,
               double* rows)
{
    S2M_HIP(h, pg_bwd_unit(h->stream, db, c, at));
    int rc = run_cg(h, db, c, prm);
    if (rc) return rc;
    S2M_HIP(h, pg_fwd_y(h->stream, db, c));
    double* dev_rows = h->pg.blk_rows.as<double>();
    S2M_HIP(h, pg_rows(h->stream, db, c, ka, kb, dev_rows));
    S2M_HIP(h, hipMemcpyAsync(rows, dev_rows, sizeof(double) * 12 * (size_t)c.cols, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

bool params_ok(const s2m_pg_params& p)
{
    return p.max_iterations >= 0 && p.cg_max_iterations >= 0 && p.relative_error_tol >= 0.0 && std::isfinite(p.relative_error_tol) &&
           p.absolute_error_tol >= 0.0 && std::isfinite(p.absolute_error_tol) && p.cg_rel_tol >= 0.0 && std::isfinite(p.cg_rel_tol);
}

// The head of a call that takes parameters: the defaults for null, the check, and the result of an empty graph.
int pg_params(s2m_context* h, const s2m_pg_params* p, s2m_pg_params& prm, s2m_pg_result* res = nullptr)
{
    if (p) prm = *p; else s2m_pg_default_params(&prm);
    if (!params_ok(prm)) return fail(h, S2M_ERR_INVALID_ARG, "pose-graph params: iteration counts and tolerances must be >= 0 and finite");
    if (res) {
        *res = s2m_pg_result{};
        res->robust_weight_min = 1.0;
        res->n_variables = (int32_t)pg_n(h);
        res->n_factors = (int32_t)h->pg.factors.size();
    }
    return S2M_OK;
}

int add_factor(s2m_context* h, const PgFactor& f)
{
    if (pg_n(h) + 1 >= kPgMaxVars) return fail(h, S2M_ERR_CAPACITY, "pose graph full (2^24 variables)");
    touch(h, std::min(f.i, f.type == kPgBetween ? f.j : f.i));
    touch(h, std::max(f.i, f.type == kPgBetween ? f.j : f.i));
    h->pg.factors.push_back(f);
    h->pg.topo_dirty = true;
    return S2M_OK;
}

PgFactor make_factor(int type, int32_t i, int32_t j, const double X[12], const double* var, int rows, double k)
{
    PgFactor f{};
    f.type = type; f.i = i; f.j = j; f.rows = rows; f.k = k;
    for (int a = 0; a < 9; a++) f.R[a] = X[a];
    for (int a = 0; a < 3; a++) f.t[a] = X[9 + a];
    for (int a = 0; a < 6; a++) f.sw[a] = a < rows ? 1.0 / std::sqrt(var[a]) : 0.0;
    return f;
}

// ---- the launched optimise ----
constexpr int kPgRangeSegments = 2;     // segments queued at a time; between two ranges the host looks at the record once

int pg_busy(s2m_context* h)
{
    return h->pg.pending ? fail(h, S2M_ERR_BUSY, "a launched pose-graph optimise is pending: s2m_pg_optimize_poll / s2m_pg_optimize_collect it first") : S2M_OK;
}

// The pose-graph stream: the lowest priority the device offers (create_stream), as the loop stream, so that the solve yields to
// the registration kernels.
int pg_stream(s2m_context* h)
{
    auto& g = h->pg;
    int rc;
    if (!g.stream && (rc = create_stream(h, &g.stream, false, "the pose-graph stream"))) return rc;
    if (!g.ev_ready) S2M_HIP(h, hipEventCreateWithFlags(&g.ev_ready, hipEventDisableTiming));
    if (!g.ev_range) S2M_HIP(h, hipEventCreateWithFlags(&g.ev_range, hipEventDisableTiming));
    if (!g.h_rec) S2M_HIP(h, hipHostMalloc((void**)&g.h_rec, sizeof(PgRecord)));
    return S2M_OK;
}

// one range: segments, the record to pinned memory, the event a poll tests
int queue_range(s2m_context* h)
{
    auto& g = h->pg;
    PgRecord* rec = g.rec.as<PgRecord>();
    for (int k = 0; k < kPgRangeSegments; k++)
        S2M_HIP(h, pg_async_segment(g.stream, g.dev, rec, g.pend_prm.cg_rel_tol, g.pend_max_cg, std::min(kPgCgChunk, g.pend_max_cg)));
    S2M_HIP(h, hipMemcpyAsync(g.h_rec, rec, sizeof(PgRecord), hipMemcpyDeviceToHost, g.stream));
    S2M_HIP(h, hipEventRecord(g.ev_range, g.stream));
    return S2M_OK;
}

// The range in flight has ended: the next one, or the result and the tail rule. Host memory only.
int advance(s2m_context* h, s2m_pg_result* out)
{
    auto& g = h->pg;
    const PgRecord& r = *g.h_rec;
    if (!r.done) {
        const int rc = queue_range(h);
        if (rc) { pg_drop_pending(h, false); return rc; }
        return S2M_PG_PENDING;
    }
    g.pending = false;
    s2m_pg_result res{};
    res.iterations = r.iterations; res.inner_iterations = r.inner_iterations; res.converged = r.converged;
    res.n_variables = (int32_t)g.n_l; res.n_factors = (int32_t)g.f_l;
    res.error_before = r.error_before; res.error_after = r.error_after; res.robust_weight_min = r.wmin;
    if (r.iterations > 0) {
        g.dev_newer = true;
        for (size_t k = g.n_l; k < pg_n(h); k++) {          // variables added since the launch follow the last one of the solve
            if (!g.has_init[k]) continue;
            (void)s2m_debug_pg_rebase(g.a_launch, r.A, g.X.data() + 12 * k);
            g.dirty[k] = 1;
        }
    }
    if (out) *out = res;
    return S2M_OK;
}

}  // namespace

int s2m::host::pg_host_current(s2m_context* h) { return host_current(h); }
void s2m::host::pg_pose_to_state(const float pose_xyzrpy[6], double X[12]) { pose_to_state(pose_xyzrpy, X); }
int s2m::host::pg_device_current(s2m_context* h) { return upload_state(h, 0, pg_n(h)); }

int s2m_pg_reset(s2m_handle h)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    auto& g = h->pg;
    if (g.pending) { (void)hipSetDevice(h->device); pg_drop_pending(h, false); }
    g.factors.clear(); g.X.clear(); g.has_init.clear(); g.dirty.clear();
    g.dev_newer = false; g.topo_dirty = true; g.n_dev = 0;
    h->sess.forget_appended();
    return S2M_OK;
}

int s2m_pg_size(s2m_handle h, int32_t* n_variables, int32_t* n_factors)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (n_variables) *n_variables = (int32_t)pg_n(h);
    if (n_factors) *n_factors = (int32_t)h->pg.factors.size();
    return S2M_OK;
}

int s2m_pg_add_prior(s2m_handle h, int32_t key, const float pose_xyzrpy[6], const double var[6])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_pg_check_args(S2M_PG_PRIOR, (int32_t)pg_n(h), key, 0, pose_xyzrpy, var, 0.0))
        return fail(h, S2M_ERR_INVALID_ARG, "prior: finite pose, positive finite variances, key in 0..N");
    double X[12];
    pose_to_state(pose_xyzrpy, X);
    return add_factor(h, make_factor(kPgPrior, key, -1, X, var, 6, 0.0));
}

int s2m_pg_add_between(s2m_handle h, int32_t key_from, int32_t key_to, const float rel_xyzrpy[6], const double var[6], double robust_k)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_pg_check_args(S2M_PG_BETWEEN, (int32_t)pg_n(h), key_from, key_to, rel_xyzrpy, var, robust_k))
        return fail(h, S2M_ERR_INVALID_ARG, "between: finite pose, positive finite variances, robust_k >= 0, two different keys in 0..N");
    double X[12];
    pose_to_state(rel_xyzrpy, X);
    return add_factor(h, make_factor(kPgBetween, key_from, key_to, X, var, 6, robust_k));
}

int s2m_pg_add_gps(s2m_handle h, int32_t key, const float xyz[3], const double var[3])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_pg_check_args(S2M_PG_GPS, (int32_t)pg_n(h), key, 0, xyz, var, 0.0))
        return fail(h, S2M_ERR_INVALID_ARG, "gps: finite position, positive finite variances, key in 0..N");
    double X[12] = { 1, 0, 0, 0, 1, 0, 0, 0, 1, xyz[0], xyz[1], xyz[2] };
    return add_factor(h, make_factor(kPgGps, key, -1, X, var, 3, 0.0));
}

int s2m_pg_set_initial(s2m_handle h, int32_t key, const float pose_xyzrpy[6])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_pg_check_args(S2M_PG_INITIAL, (int32_t)pg_n(h), key, 0, pose_xyzrpy, nullptr, 0.0))
        return fail(h, S2M_ERR_INVALID_ARG, "initial value: finite pose, key in 0..N");
    if (h->pg.pending && (size_t)key < h->pg.n_l) return pg_busy(h);
    if (pg_n(h) + 1 >= kPgMaxVars) return fail(h, S2M_ERR_CAPACITY, "pose graph full (2^24 variables)");
    touch(h, key);
    pose_to_state(pose_xyzrpy, h->pg.X.data() + 12 * (size_t)key);
    h->pg.has_init[(size_t)key] = 1;
    h->pg.dirty[(size_t)key] = 1;
    return S2M_OK;
}

int s2m_pg_add_odometry(s2m_handle h, const float pose_xyzrpy[6])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    const int32_t n = (int32_t)pg_n(h);
    if (s2m_pg_check_args(S2M_PG_INITIAL, n, n, 0, pose_xyzrpy, nullptr, 0.0)) return fail(h, S2M_ERR_INVALID_ARG, "odometry: the pose must be finite");
    s2m_pg_params prm;
    s2m_pg_default_params(&prm);
    int rc;
    if (n == 0) {
        if ((rc = s2m_pg_add_prior(h, 0, pose_xyzrpy, prm.prior_var))) return rc;
        return s2m_pg_set_initial(h, 0, pose_xyzrpy);
    }
    if (!h->pg.has_init[(size_t)n - 1]) return fail(h, S2M_ERR_INVALID_ARG, "odometry: the last variable has no value");
    if (!h->pg.pending && (rc = host_current(h))) return rc;   // (pending: the mirror is current since the launch)
    const double* L = h->pg.X.data() + 12 * (size_t)(n - 1);
    double Xn[12], Z[12];
    pose_to_state(pose_xyzrpy, Xn);
    for (int a = 0; a < 3; a++) {                           // poseFrom.between(poseTo) = L^-1 Xn
        for (int b = 0; b < 3; b++) Z[a * 3 + b] = L[a] * Xn[b] + L[3 + a] * Xn[3 + b] + L[6 + a] * Xn[6 + b];
        Z[9 + a] = L[a] * (Xn[9] - L[9]) + L[3 + a] * (Xn[10] - L[10]) + L[6 + a] * (Xn[11] - L[11]);
    }
    if ((rc = add_factor(h, make_factor(kPgBetween, n - 1, n, Z, prm.odom_var, 6, 0.0)))) return rc;
    std::copy(Xn, Xn + 12, h->pg.X.begin() + 12 * (size_t)n);
    h->pg.has_init[(size_t)n] = 1;
    h->pg.dirty[(size_t)n] = 1;
    return S2M_OK;
}

int s2m_pg_optimize(s2m_handle h, const s2m_pg_params* p, s2m_pg_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    s2m_pg_params prm;
    s2m_pg_result res;
    int rc = pg_params(h, p, prm, &res);
    if (rc) return rc;
    if (out) *out = res;
    if (pg_n(h) == 0) return S2M_OK;
    if ((rc = prepare(h))) return rc;
    auto& g = h->pg;
    PgDev& d = g.dev;
    S2M_HIP(h, pg_linearize(h->stream, d, d.X));
    if ((rc = read_scalars(h))) return rc;
    double err = g.h_sc->err;
    res.error_before = res.error_after = err;
    res.robust_weight_min = g.h_sc->wmin;
    for (int it = 0; it < prm.max_iterations; it++) {
        S2M_HIP(h, pg_rhs(h->stream, d));
        if ((rc = run_cg(h, d, kPgOne, prm))) return rc;
        res.inner_iterations += g.h_sc->iters;
        S2M_HIP(h, pg_step(h->stream, d));
        S2M_HIP(h, pg_linearize(h->stream, d, d.Xtrial));  // the trial point's error, and the next step's linearisation if it is kept
        if ((rc = read_scalars(h))) return rc;
        const double err_n = g.h_sc->err;
        if (!(err_n < err)) { res.converged = 1; break; }
        std::swap(g.est.p, g.trial.p);
        std::swap(g.est.cap, g.trial.cap);
        d.X = g.est.as<double>(); d.Xtrial = g.trial.as<double>();
        g.dev_newer = true;
        const double dec = err - err_n, old = err;
        err = err_n;
        res.iterations++;
        res.error_after = err;
        res.robust_weight_min = g.h_sc->wmin;
        if (dec < prm.absolute_error_tol || dec < prm.relative_error_tol * old) { res.converged = 1; break; }
    }
    if (out) *out = res;
    return S2M_OK;
}

int s2m_pg_optimize_launch(s2m_handle h, const s2m_pg_params* p, s2m_pg_result* early)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    s2m_pg_params prm;
    s2m_pg_result res;
    int rc = pg_params(h, p, prm, &res);
    if (rc) return rc;
    if (pg_n(h) == 0) { if (early) *early = res; return S2M_OK; }
    auto& g = h->pg;
    if ((rc = host_current(h)) || (rc = prepare(h))) return rc;      // from here on the host needs nothing the device holds
    if ((rc = pg_stream(h)) || (rc = ensure(h, g.rec, sizeof(PgRecord)))) return rc;
    const PgDev& d = g.dev;
    g.n_l = pg_n(h); g.f_l = g.factors.size();
    g.pend_prm = prm;
    g.pend_max_cg = pg_max_cg(d, prm);
    std::copy(g.X.begin() + 12 * (g.n_l - 1), g.X.begin() + 12 * g.n_l, g.a_launch);
    S2M_HIP(h, hipEventRecord(g.ev_ready, h->stream));               // behind the uploads of prepare()
    S2M_HIP(h, hipStreamWaitEvent(g.stream, g.ev_ready, 0));
    hipError_t e = pg_async_open(g.stream, d, g.rec.as<PgRecord>(), prm.max_iterations, prm.absolute_error_tol, prm.relative_error_tol);
    if (e == hipSuccess && (rc = queue_range(h)) == S2M_OK) {
        g.pending = true;
        if (early) *early = res;
        return S2M_PG_PENDING;
    }
    pg_drop_pending(h, false);                                       // what was queued ends; nothing stays pending
    return e != hipSuccess ? fail(h, S2M_ERR_HIP, "pg_async_open", e) : rc;
}

int s2m_pg_optimize_poll(s2m_handle h, s2m_pg_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!h->pg.pending) return S2M_PG_IDLE;
    S2M_HIP(h, hipSetDevice(h->device));
    const hipError_t e = hipEventQuery(h->pg.ev_range);
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return S2M_PG_PENDING; }   // (not an error of the launches that follow)
    if (e != hipSuccess) { pg_drop_pending(h, false); return fail(h, S2M_ERR_HIP, "hipEventQuery(pose-graph range)", e); }
    return advance(h, out);
}

int s2m_pg_optimize_collect(s2m_handle h, s2m_pg_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!h->pg.pending) return S2M_PG_IDLE;
    S2M_HIP(h, hipSetDevice(h->device));
    for (;;) {
        const hipError_t e = hipEventSynchronize(h->pg.ev_range);
        if (e != hipSuccess) { pg_drop_pending(h, false); return fail(h, S2M_ERR_HIP, "hipEventSynchronize(pose-graph range)", e); }
        const int rc = advance(h, out);
        if (rc != S2M_PG_PENDING) return rc;
    }
}

// ---- observation hooks of the stages (include/liorf_s2m_debug.h): each prepares the device tables as an optimise does and
// queues the product's own launches on the work vectors, which every optimise and marginal rewrites before it reads them.
namespace {

int32_t pg_n_extra(const s2m_context* h) { return (int32_t)h->pg.factors.size() - (int32_t)pg_n(h); }   // (a solvable graph: the chain holds n factors)

int pg_hook_begin(s2m_context* h, bool linearize)
{
    if (pg_n(h) == 0) return fail(h, S2M_ERR_INVALID_ARG, "pose-graph hook: the graph is empty");
    const int rc = prepare(h);
    if (rc) return rc;
    if (linearize) S2M_HIP(h, pg_linearize(h->stream, h->pg.dev, h->pg.dev.X));
    return S2M_OK;
}

int pg_up(s2m_context* h, double* dst, const double* src, size_t count)
{
    if (count) S2M_HIP(h, hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
    return S2M_OK;
}

int pg_down(s2m_context* h, double* dst, const double* src, size_t count)
{
    if (dst && count) S2M_HIP(h, hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    return S2M_OK;
}

}  // namespace

int s2m_debug_pg_apply_check_args(int32_t n_variables, int32_t n_extra, int32_t op, int32_t cols, const double* in, const double* out)
{
    if (n_variables <= 0 || n_extra < 0 || op < S2M_DEBUG_PG_FWD || op > S2M_DEBUG_PG_KT || cols < 0 || cols > S2M_PG_BLOCK_COLUMNS) return S2M_ERR_INVALID_ARG;
    if (op >= S2M_DEBUG_PG_K && n_extra == 0) return S2M_ERR_INVALID_ARG;
    if (!in || !out) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

int s2m_debug_pg_set_estimate(s2m_handle h, int32_t key, const double X[12])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (!X || key < 0 || (size_t)key > pg_n(h)) return fail(h, S2M_ERR_INVALID_ARG, "estimate: 12 doubles, key in 0..N");
    if (pg_n(h) + 1 >= kPgMaxVars) return fail(h, S2M_ERR_CAPACITY, "pose graph full (2^24 variables)");
    touch(h, key);
    std::copy(X, X + 12, h->pg.X.begin() + 12 * (size_t)key);
    h->pg.has_init[(size_t)key] = 1;
    h->pg.dirty[(size_t)key] = 1;
    return S2M_OK;
}

int s2m_debug_pg_linearize(s2m_handle h, int32_t n_variables, int32_t n_extra, double* rc_, double* Binv, double* Aof, double* Ji, double* Jj,
                           double* rx, double* ferr, double* fw, double* err, double* wmin)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (n_variables <= 0 || (size_t)n_variables != pg_n(h) || n_extra != pg_n_extra(h))
        return fail(h, S2M_ERR_INVALID_ARG, "linearise: the array sizes must be the graph's variables and extra factors");
    int rc = pg_hook_begin(h, true);
    if (rc) return rc;
    const PgDev& d = h->pg.dev;
    const size_t n = (size_t)d.n, m = (size_t)d.n_extra;
    if ((rc = pg_down(h, rc_, d.rc, 6 * n)) || (rc = pg_down(h, Binv, d.Binv, 36 * n)) || (rc = pg_down(h, Aof, d.Aof, 36 * n)) ||
        (rc = pg_down(h, Ji, d.Ji, 36 * m)) || (rc = pg_down(h, Jj, d.Jj, 36 * m)) || (rc = pg_down(h, rx, d.rx, 6 * m)) ||
        (rc = pg_down(h, ferr, d.ferr, n + m)) || (rc = pg_down(h, fw, d.fw, n + m))) return rc;
    if ((rc = read_scalars(h))) return rc;
    if (err) *err = h->pg.h_sc->err;
    if (wmin) *wmin = h->pg.h_sc->wmin;
    return S2M_OK;
}

int s2m_debug_pg_apply(s2m_handle h, int32_t op, int32_t cols, const double* in, double* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (s2m_debug_pg_apply_check_args((int32_t)pg_n(h), std::max(pg_n_extra(h), 0), op, cols, in, out))
        return fail(h, S2M_ERR_INVALID_ARG, "apply: op 0..3 (2 and 3 need an extra factor), cols 0..S2M_PG_BLOCK_COLUMNS, two arrays, a graph");
    int rc = pg_hook_begin(h, true);
    if (rc) return rc;
    PgDev db = h->pg.dev;                                   // cols == 0: one column on the graph's own vectors
    PgCols c = kPgOne;
    if (cols > 0 && (rc = prepare_block(h, cols, db, c))) return rc;
    // with an extra factor a column's u is 6 n_extra doubles apart, so the host's side-by-side columns are the device's
    const size_t C = (size_t)c.cols, nv = 6 * (size_t)db.n, nu = 6 * (size_t)db.n_extra;
    double* src = op == S2M_DEBUG_PG_BWD ? db.g : op == S2M_DEBUG_PG_KT ? db.u : db.p;
    const double* dst = op == S2M_DEBUG_PG_FWD ? db.t1 : op == S2M_DEBUG_PG_K ? db.u : db.t2;
    if ((rc = pg_up(h, src, in, C * (op == S2M_DEBUG_PG_KT ? nu : nv)))) return rc;
    S2M_HIP(h, pg_apply(h->stream, db, c, op));
    if ((rc = pg_down(h, out, dst, C * (op == S2M_DEBUG_PG_K ? nu : nv)))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_pg_cg(s2m_handle h, const s2m_pg_params* p, int32_t cols, const double* b, double* y, s2m_debug_pg_cg_out* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    s2m_pg_params prm;
    int rc = pg_params(h, p, prm);
    if (rc) return rc;
    if (cols < 0 || cols > S2M_PG_BLOCK_COLUMNS || !b || !y || !out)
        return fail(h, S2M_ERR_INVALID_ARG, "cg: cols 0..S2M_PG_BLOCK_COLUMNS, three arrays");
    if ((rc = pg_hook_begin(h, true))) return rc;
    PgDev db = h->pg.dev;                                   // cols == 0: one column on the graph's own vectors
    PgCols c = kPgOne;
    if (cols > 0 && (rc = prepare_block(h, cols, db, c))) return rc;
    const size_t C = (size_t)c.cols, nv = 6 * (size_t)db.n;
    if ((rc = pg_up(h, db.b, b, C * nv))) return rc;
    if ((rc = run_cg(h, db, c, prm))) return rc;
    if ((rc = pg_down(h, y, db.y, C * nv))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const PgScalars* hs = h->pg.h_sc;
    for (size_t q = 0; q < C; q++) out[q] = s2m_debug_pg_cg_out{ hs[q].rr, hs[q].bb, hs[q].iters, hs[q].stop };
    return S2M_OK;
}

int s2m_debug_pg_retract(s2m_handle h, int32_t n_variables, const double* delta, double* X)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (n_variables <= 0 || (size_t)n_variables != pg_n(h) || !delta || !X)
        return fail(h, S2M_ERR_INVALID_ARG, "retract: 6 doubles in and 12 out for every variable of the graph");
    int rc = pg_hook_begin(h, false);
    if (rc) return rc;
    const PgDev& d = h->pg.dev;
    if ((rc = pg_up(h, d.delta, delta, 6 * (size_t)d.n))) return rc;
    S2M_HIP(h, pg_retract(h->stream, d));
    if ((rc = pg_down(h, X, d.Xtrial, 12 * (size_t)d.n))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_pg_get_poses(s2m_handle h, int32_t first, int32_t count, float* xyzrpy)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > pg_n(h) || (count > 0 && !xyzrpy))
        return fail(h, S2M_ERR_INVALID_ARG, "pose range outside the pose graph");
    if (count == 0) return S2M_OK;
    int rc = upload_state(h, (size_t)first, (size_t)count);
    if (rc) return rc;
    if ((rc = ensure(h, h->pg.poses, sizeof(float) * 6 * (size_t)count))) return rc;
    S2M_HIP(h, pg_poses(h->stream, h->pg.est.as<double>(), first, count, h->pg.poses.as<float>(), nullptr));
    S2M_HIP(h, hipMemcpyAsync(xyzrpy, h->pg.poses.p, sizeof(float) * 6 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_pg_marginal(s2m_handle h, int32_t key, double cov[36])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (key < 0 || (size_t)key >= pg_n(h) || !cov) return fail(h, S2M_ERR_INVALID_ARG, "marginal: key outside the pose graph");
    int rc = prepare(h);
    if (rc) return rc;
    s2m_pg_params prm;
    s2m_pg_default_params(&prm);
    const PgDev& d = h->pg.dev;
    S2M_HIP(h, pg_linearize(h->stream, d, d.X));
    // column a of (J^T J)^-1 = J_c^-1 (I + K^T K)^-1 J_c^-T e_a
    for (int a = 0; a < 6; a++) {                           // six one-column solves on the graph's own vectors, one after the other
        PgColAt at{};
        at.v[0] = 6 * key + a;
        S2M_HIP(h, pg_bwd_unit(h->stream, d, kPgOne, at));
        if ((rc = run_cg(h, d, kPgOne, prm))) return rc;
        S2M_HIP(h, pg_fwd_y(h->stream, d, kPgOne));
        double col[6];
        S2M_HIP(h, hipMemcpyAsync(col, d.delta + 6 * (size_t)key, sizeof(col), hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (int b = 0; b < 6; b++) cov[b * 6 + a] = col[b];
    }
    return S2M_OK;
}

int s2m_pg_marginals_check_args(int32_t n_variables, const int32_t* keys, int32_t n_keys)
{
    if (n_keys < 0 || (n_keys > 0 && !keys)) return S2M_ERR_INVALID_ARG;
    for (int32_t k = 0; k < n_keys; k++)
        if (keys[k] < 0 || keys[k] >= n_variables) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

int s2m_pg_marginals(s2m_handle h, const int32_t* keys, int32_t n_keys, double* cov)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (s2m_pg_marginals_check_args((int32_t)pg_n(h), keys, n_keys) || (n_keys > 0 && !cov))
        return fail(h, S2M_ERR_INVALID_ARG, "marginals: a key outside the pose graph, or a null array");
    if (n_keys == 0) return S2M_OK;
    int rc = prepare(h);
    if (rc) return rc;
    s2m_pg_params prm;
    s2m_pg_default_params(&prm);
    constexpr int kKeys = kPgBlockCols / 6;                 // keys per pass
    PgDev db;
    PgCols c;
    if ((rc = prepare_block(h, 6 * std::min<int>(n_keys, kKeys), db, c))) return rc;
    S2M_HIP(h, pg_linearize(h->stream, h->pg.dev, h->pg.dev.X));
    double rows[12 * kPgBlockCols];
    for (int32_t k0 = 0; k0 < n_keys; k0 += kKeys) {
        const int nk = std::min<int>(kKeys, n_keys - k0);
        PgColAt at{}, ka{}, kb{};
        for (int q = 0; q < 6 * nk; q++) { ka.v[q] = keys[k0 + q / 6]; at.v[q] = 6 * ka.v[q] + q % 6; kb.v[q] = -1; }
        c.cols = 6 * nk;
        if ((rc = solve_pass(h, db, c, prm, at, ka, kb, rows))) return rc;
        for (int q = 0; q < 6 * nk; q++)                    // column q % 6 of key q / 6's block
            for (int b = 0; b < 6; b++) cov[36 * (size_t)(k0 + q / 6) + b * 6 + q % 6] = rows[12 * q + b];
    }
    return S2M_OK;
}

int s2m_pg_joint_marginal(s2m_handle h, int32_t key_a, int32_t key_b, double cov[144])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    const int32_t keys[2] = { key_a, key_b };
    if (s2m_pg_marginals_check_args((int32_t)pg_n(h), keys, 2) || key_a == key_b || !cov)
        return fail(h, S2M_ERR_INVALID_ARG, "joint marginal: two different keys of the pose graph");
    int rc = prepare(h);
    if (rc) return rc;
    s2m_pg_params prm;
    s2m_pg_default_params(&prm);
    PgDev db;
    PgCols c;
    if ((rc = prepare_block(h, 12, db, c))) return rc;
    S2M_HIP(h, pg_linearize(h->stream, h->pg.dev, h->pg.dev.X));
    PgColAt at{}, ka{}, kb{};
    for (int q = 0; q < 12; q++) { at.v[q] = 6 * keys[q / 6] + q % 6; ka.v[q] = key_a; kb.v[q] = key_b; }
    double rows[12 * 12];
    if ((rc = solve_pass(h, db, c, prm, at, ka, kb, rows))) return rc;
    for (int q = 0; q < 12; q++)
        for (int b = 0; b < 12; b++) cov[b * 12 + q] = rows[12 * q + b];
    return S2M_OK;
}

int s2m_pg_apply_to_store(s2m_handle h, int32_t first, int32_t count)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->pg.pending) return pg_busy(h);
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > pg_n(h) || (size_t)first + (size_t)count > h->kf.time.size())
        return fail(h, S2M_ERR_INVALID_ARG, "pose range outside the pose graph or the key-frame store");
    if (count == 0) return S2M_OK;
    int rc = upload_state(h, (size_t)first, (size_t)count);
    if (rc) return rc;
    // Pose vectors and cached transforms are computed on the device into a staging block (the host libm's sinf / cosf are
    // restated there, so each transform is bit for bit s2m_kf_set_poses'); one copy brings the block and its not-finite flag
    // to the store's host mirror; only then a second launch writes positions and transforms into the store. A failure up
    // to the flag leaves the store as it was; nothing is uploaded.
    const size_t nf = 18 * (size_t)count;
    if ((rc = ensure(h, h->pg.poses, sizeof(float) * nf + sizeof(int32_t)))) return rc;
    float* stage = h->pg.poses.as<float>();
    int32_t* bad = reinterpret_cast<int32_t*>(stage + nf);
    std::vector<float> back(nf + 1);
    S2M_HIP(h, hipMemsetAsync(bad, 0, sizeof(int32_t), h->stream));
    S2M_HIP(h, pg_store_stage(h->stream, h->pg.est.as<double>(), first, count, stage, bad));
    S2M_HIP(h, hipMemcpyAsync(back.data(), stage, sizeof(float) * nf + sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    int32_t flag;
    memcpy(&flag, &back[nf], sizeof(flag));
    if (flag) return fail(h, S2M_ERR_INVALID_ARG, "pose graph: an estimate is not finite; the key-frame store is unchanged");
    S2M_HIP(h, pg_store_write(h->stream, stage, count, h->kf.pos.as<float4>() + first, h->kf.frames.as<KfFrame>() + first));
    for (int k = 0; k < count; k++) {
        const float* q = back.data() + 18 * (size_t)k;
        std::copy(q, q + 6, h->kf.pose.begin() + 6 * (size_t)(first + k));
        std::copy(q + 6, q + 18, h->kf.frame[(size_t)(first + k)].T);
    }
    return S2M_OK;
}
