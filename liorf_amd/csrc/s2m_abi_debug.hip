// s2m_abi_debug.hip — the observation and timing hooks of the registration path (include/liorf_s2m_debug.h and the s2m_time_* /
// s2m_surf_optimization / s2m_normal_eq entry points): single stages and launches of the LM loop run on their own, the scan
// preparation run again, the restated libm pinned - and the copy-out of the last key-frame selection's stages.  It reaches the loop through the host functions s2m_abi.hip defines
// (s2m_context.hpp) and never includes s2m_kernels.hpp / s2m_register.hpp: a second unit that instantiates k_register would
// compile every build twice.  Its two kernels include s2m_device.hpp, so the trig they pin is the one k_register compiles.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <limits>
#include <vector>

#include "s2m_context.hpp"
#include "s2m_device.hpp"

using namespace s2m;
using namespace s2m::host;

namespace s2m {

// Observation hook: the device's sinf / cosf of n arguments (tests compare them with the host's libm).
__global__ __launch_bounds__(256) void k_debug_sincos(const float* __restrict__ x, int n, float* __restrict__ s, float* __restrict__ c,
                                                      float* __restrict__ a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { s[i] = glibc_sincosf(x[i], 0); c[i] = glibc_sincosf(x[i], 1); if (a) a[i] = glibc_atanf(x[i]); }
}

// Observation hook: the hypotf of eigen6_sym's Jacobi rotations on n argument pairs (tests compare with the host's libm).
__global__ __launch_bounds__(256) void k_debug_hypot(const float* __restrict__ x, const float* __restrict__ y, int n, float* __restrict__ r)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i] = glibc_hypotf(x[i], y[i]);
}

}  // namespace s2m

extern "C" {

int s2m_surf_optimization(s2m_handle h, const float pose[6], int32_t* idx5, float* d2_5, uint8_t* flag, float* coeff4)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t n = h->reg.n_q;
    if (n == 0) return S2M_OK;
    if (h->reg.n_m == 0) {          // no map: nothing is ever gated
        if (idx5) for (size_t i = 0; i < 5 * n; i++) idx5[i] = -1;
        if (d2_5) for (size_t i = 0; i < 5 * n; i++) d2_5[i] = INFINITY;
        if (flag) memset(flag, 0, n);
        if (coeff4) memset(coeff4, 0, sizeof(float) * 4 * n);
        return S2M_OK;
    }
    int rc;
    if ((rc = ensure(h, h->reg.dbg_idx5, sizeof(int32_t) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_d2, sizeof(float) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_flag, n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_coeff, sizeof(float) * 4 * n))) return rc;
    h->hctx.dbg_idx5 = h->reg.dbg_idx5.as<int32_t>(); h->hctx.dbg_d2 = h->reg.dbg_d2.as<float>();
    h->hctx.dbg_flag = h->reg.dbg_flag.as<uint8_t>(); h->hctx.dbg_coeff = h->reg.dbg_coeff.as<float>();
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    launch_fused(h, shape_of(h), true, 0, 0);
    S2M_HIP(h, hipGetLastError());
    if (idx5) S2M_HIP(h, hipMemcpyAsync(idx5, h->reg.dbg_idx5.p, sizeof(int32_t) * 5 * n, hipMemcpyDeviceToHost, h->stream));
    if (d2_5) S2M_HIP(h, hipMemcpyAsync(d2_5, h->reg.dbg_d2.p, sizeof(float) * 5 * n, hipMemcpyDeviceToHost, h->stream));
    if (flag) S2M_HIP(h, hipMemcpyAsync(flag, h->reg.dbg_flag.p, n, hipMemcpyDeviceToHost, h->stream));
    if (coeff4) S2M_HIP(h, hipMemcpyAsync(coeff4, h->reg.dbg_coeff.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    h->hctx.dbg_idx5 = nullptr; h->hctx.dbg_d2 = nullptr; h->hctx.dbg_flag = nullptr; h->hctx.dbg_coeff = nullptr;
    h->ctx_dirty = true;
    return upload_ctx(h);
}

int s2m_debug_wave_profile(s2m_handle h, const float pose[6], int launches, uint64_t* out, size_t cap_waves)
{
    if (!h || !pose || !out || launches == 0) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t nwaves = (size_t)h->hctx.nblocks * (size_t)h->hctx.wpb;   // one record per wave of the grid
    int rc;
    if ((rc = ensure(h, h->reg.dbg_clk, sizeof(uint64_t) * kProfWords * nwaves))) return rc;
    S2M_HIP(h, hipMemsetAsync(h->reg.dbg_clk.p, 0, sizeof(uint64_t) * kProfWords * nwaves, h->stream));
    h->hctx.dbg_clk = h->reg.dbg_clk.as<unsigned long long>();
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    if (launches < 0) {
        // a real loop as enqueue_loop issues it (density re-split, R0 F0 R1 R2' ...); the recorded launch is number
        // N = -launches - 1 (N = 0: the first launch of a scan), closing the iteration before it when the loop is fused
        const LoopShape sh = shape_of(h);
        const int nblocks = h->hctx.nblocks, N = -launches - 1;
        const bool fuse = h->tune.fuse_solve && nblocks <= h->tune.fuse_max_blocks;
        if (h->tune.density_raw > 0) launch_density(h, sh);
        h->hctx.density_pending = 0;                      // cleared on the device by the kernel: keep the host copy in step
        for (int L = 0; L < N; L++) {
            launch_iteration(h, sh, L, (fuse && L >= 2) ? 1 : 0);
            if (!fuse || L == 0) launch_finalize(h, sh, L, 0);
        }
        launch_fused(h, sh, true, N, (fuse && N >= 2) ? 1 : 0);
    }
    for (int rep = 0; rep < launches; rep++)
        launch_fused(h, shape_of(h), true, 0, 0);
    S2M_HIP(h, hipGetLastError());
    const size_t n = nwaves < cap_waves ? nwaves : cap_waves;
    S2M_HIP(h, hipMemcpyAsync(out, h->reg.dbg_clk.p, sizeof(uint64_t) * kProfWords * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    h->hctx.dbg_clk = nullptr;
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    return (int)n;
}

int s2m_debug_device_trig(s2m_handle h, const float* x, size_t n, float* s, float* c, float* a)
{
    if (!h || (n > 0 && (!x || !s || !c)) || n > (size_t)0x3fffffff) return S2M_ERR_INVALID_ARG;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure(h, h->voxel.in, sizeof(float) * 4 * n);
    if (rc) return rc;
    float* d = h->voxel.in.as<float>();
    S2M_HIP(h, hipMemcpyAsync(d, x, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_debug_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)d, (int)n, d + n, d + 2 * n,
                       a ? d + 3 * n : (float*)nullptr);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(s, d + n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(c, d + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    if (a) S2M_HIP(h, hipMemcpyAsync(a, d + 3 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_device_hypot(s2m_handle h, const float* x, const float* y, size_t n, float* r)
{
    if (!h || (n > 0 && (!x || !y || !r)) || n > (size_t)0x3fffffff) return S2M_ERR_INVALID_ARG;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure(h, h->voxel.in, sizeof(float) * 3 * n);
    if (rc) return rc;
    float* d = h->voxel.in.as<float>();
    S2M_HIP(h, hipMemcpyAsync(d, x, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(d + n, y, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_debug_hypot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)d, (const float*)(d + n), (int)n, d + 2 * n);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(r, d + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_lm_close_check_args(int form, int iter, int max_iter, const double* rows, int n_rows, const float pose0[6],
                                  const float matP_in[36], const s2m_debug_lm_close_out* out)
{
    if (n_rows < 0 || (n_rows > 0 && !rows) || !pose0 || !matP_in || !out) return S2M_ERR_INVALID_ARG;
    if (form != 0 && form != 1) return S2M_ERR_INVALID_ARG;
    if (iter < 0 || iter >= max_iter) return S2M_ERR_INVALID_ARG;
    if (form == 1 && iter == 0) return S2M_ERR_INVALID_ARG;     // launch 1 never closes: iteration 0 needs the degeneracy analysis
    return S2M_OK;
}

int s2m_debug_lm_close(s2m_handle h, int form, int iter, const double* rows, int n_rows, const float pose0[6],
                       int degen_in, const float matP_in[36], s2m_debug_lm_close_out* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_debug_lm_close_check_args(form, iter, h->prm.max_iter, rows, n_rows, pose0, matP_in, out))
        return fail(h, S2M_ERR_INVALID_ARG, "null argument, form outside {0, 1}, iter outside 0 .. max_iter-1, or form 1 at iter 0");
    if (h->reg.pending != Reg::kNone) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;                   // (the parameters of the last s2m_set_params with it)
    // the rows a close reads: one per workgroup the wave table of the resident scan needs (k_finalize, k_register)
    ensure_wave_table(h);
    int32_t n_waves = 0;
    S2M_HIP(h, hipMemcpyAsync(&n_waves, h->reg.n_waves.p, sizeof(n_waves), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const int nblocks = h->hctx.nblocks, wpb = h->hctx.wpb;
    const int nb_act = std::min((n_waves + wpb - 1) / wpb, nblocks);
    if (n_rows > nb_act) return fail(h, S2M_ERR_INVALID_ARG, "more rows than the resident scan has active workgroups");
    std::vector<double> part((size_t)2 * (size_t)nblocks * kAcc, std::numeric_limits<double>::quiet_NaN());
    double* slot = part.data() + (size_t)(iter & 1) * (size_t)nblocks * kAcc;
    for (size_t k = 0; k < (size_t)nb_act * kAcc; k++) slot[k] = k < (size_t)n_rows * kAcc ? rows[k] : 0.0;
    S2M_HIP(h, hipMemcpyAsync(h->reg.partials.p, part.data(), sizeof(double) * part.size(), hipMemcpyHostToDevice, h->stream));
    DevState s;
    fill_state(h, &s, pose0);
    for (int k = 0; k < 6; k++) { s.pose2[iter & 1][k] = pose0[k]; s.pose2[(iter + 1) & 1][k] = NAN; }
    s.T_valid = 0;
    s.isDegenerate = degen_in;
    memcpy(s.matP, matP_in, sizeof(s.matP));
    store_state(h, s, nullptr);
    S2M_HIP(h, hipMemsetAsync(h->hctx.trace + iter, 0xff, sizeof(s2m_iter_trace), h->stream));
    const LoopShape sh = shape_of(h);
    if (form == 0) launch_finalize(h, sh, iter, 0);
    else           launch_fused(h, sh, false, iter + 1, 1);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_trace[iter], h->hctx.trace + iter, sizeof(s2m_iter_trace), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const DevState& r = h->reg.h_state[1];
    memcpy(out->AtA, r.AtA, sizeof(out->AtA));
    memcpy(out->AtB, r.AtB, sizeof(out->AtB));
    out->n_sel_last = r.n_sel_last;
    out->trace = h->reg.h_trace[iter];
    memcpy(out->pose, r.pose, 24);
    memcpy(out->pose_next, r.pose2[(iter + 1) & 1], 24);
    out->iters_run = r.iters_run; out->converged = r.converged; out->done = r.done; out->stalled = r.stalled;
    out->is_degenerate = r.isDegenerate;
    out->n_rows_active = nb_act;
    memcpy(out->matP, r.matP, sizeof(out->matP));
    return S2M_OK;
}

int s2m_debug_lm_rows_check_args(const float pose[6], int launch, int max_iter, int early_exit, const double* rows, int cap_rows,
                                 const s2m_debug_lm_rows_out* out)
{
    if (!pose || !out || cap_rows < 0 || (cap_rows > 0 && !rows)) return S2M_ERR_INVALID_ARG;
    if (launch < 0 || launch >= max_iter) return S2M_ERR_INVALID_ARG;
    if (launch > 0 && early_exit) return S2M_ERR_INVALID_ARG;  // a loop that may end before launch N has no launch N
    return S2M_OK;
}

int s2m_debug_lm_rows(s2m_handle h, const float pose[6], int launch, double* rows, int cap_rows, s2m_debug_lm_rows_out* out,
                      int32_t* wave_table)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_debug_lm_rows_check_args(pose, launch, h->prm.max_iter, h->prm.early_exit, rows, cap_rows, out))
        return fail(h, S2M_ERR_INVALID_ARG, "null argument, launch outside 0 .. max_iter-1, or launch > 0 with early_exit on");
    if (h->batch.parent) return fail(h, S2M_ERR_INVALID_ARG, "a scan slot of a batch has no loop of its own to observe");
    if (h->reg.pending != Reg::kNone) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    const bool resplit = launch > 0 && h->hctx.density_pending && h->tune.density_raw > 0;   // the hook's loop consumes the scan's re-split
    if ((rc = push_state(h, pose))) return rc;
    const LoopShape sh = shape_of(h);
    if (launch == 0) launch_fused(h, sh, false, 0, 0);      // (s2m_normal_eq's first launch)
    else {
        // enqueue_loop's launches 0 .. N, without the k_finalize behind launch N
        const bool fuse = h->tune.fuse_solve && sh.nblocks * sh.nslots <= h->tune.fuse_max_blocks;
        if (h->tune.density_raw > 0) launch_density(h, sh);
        h->hctx.density_pending = 0;                      // cleared on the device by the kernel: keep the host copy in step
        for (int L = 0; L <= launch; L++) {
            launch_iteration(h, sh, L, (fuse && L >= 2) ? 1 : 0, fuse);
            if (L < launch && (!fuse || L == 0)) launch_finalize(h, sh, L, 0);
        }
    }
    S2M_HIP(h, hipGetLastError());
    int32_t nw = 0;
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(&nw, h->reg.n_waves.p, sizeof(nw), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (resplit) {                                          // back to where s2m_set_scan left the scan: the table is rebuilt from chunk_parts on demand
        h->hctx.density_pending = 1;
        h->reg.table_stale = true;
        h->ctx_dirty = true;
    }
    if (nw < 0 || nw > h->hctx.table_cap) return fail(h, S2M_ERR_HIP, "wave count outside the table");
    const DevState& r = h->reg.h_state[1];
    const int nblocks = h->hctx.nblocks, wpb = h->hctx.wpb;
    const int nb_act = std::min((nw + wpb - 1) / wpb, nblocks);
    out->n_rows_active = nb_act; out->wpb = wpb; out->nblocks = nblocks; out->n_waves = nw;
    memcpy(out->pose_used, launch == 0 ? pose : r.pose2[launch & 1], 24);
    out->done = r.done;
    if (cap_rows < nb_act) return fail(h, S2M_ERR_INVALID_ARG, "fewer rows offered than the resident scan has active workgroups");
    const double* slot = h->reg.partials.as<double>() + (size_t)(launch & 1) * (size_t)nblocks * kAcc;
    if (nb_act > 0) S2M_HIP(h, hipMemcpyAsync(rows, slot, sizeof(double) * (size_t)nb_act * kAcc, hipMemcpyDeviceToHost, h->stream));
    if (wave_table && nw > 0) S2M_HIP(h, hipMemcpyAsync(wave_table, h->reg.wave_table.p, sizeof(int2) * (size_t)nw, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_normal_eq(s2m_handle h, const float pose[6], float AtA[36], float AtB[6], int32_t* n_sel)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    if (h->reg.n_m == 0 || h->reg.n_q == 0) {
        if (AtA) memset(AtA, 0, sizeof(float) * 36);
        if (AtB) memset(AtB, 0, sizeof(float) * 6);
        if (n_sel) *n_sel = 0;
        return S2M_OK;
    }
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    {
        const LoopShape sh = shape_of(h);
        launch_fused(h, sh, false, 0, 0);
        launch_finalize(h, sh, 0, 1);
    }
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (AtA) memcpy(AtA, h->reg.h_state[1].AtA, sizeof(float) * 36);
    if (AtB) memcpy(AtB, h->reg.h_state[1].AtB, sizeof(float) * 6);
    if (n_sel) *n_sel = h->reg.h_state[1].n_sel_last;
    return S2M_OK;
}

int s2m_debug_scan_prep(s2m_handle h, int32_t chain, const float pose[6], int32_t* qperm, float* qxyz, int32_t* chunk_parts,
                        int32_t* chunk_factor, int32_t* wave_table, int32_t* n_waves)
{
    if (!h || chain < S2M_DEBUG_PREP_READ || chain > S2M_DEBUG_PREP_LEGACY) return S2M_ERR_INVALID_ARG;
    if (h->batch.parent) return fail(h, S2M_ERR_INVALID_ARG, "a scan slot of a batch keeps the six-kernel chain");
    if (h->reg.pending != Reg::kNone) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    const size_t n = h->reg.n_q;
    if (n == 0) { if (n_waves) *n_waves = 0; return S2M_OK; }
    if (pose && chain != S2M_DEBUG_PREP_READ && h->reg.n_m == 0) return fail(h, S2M_ERR_NO_SCAN, "the density pass needs a map");
    S2M_HIP(h, hipSetDevice(h->device));
    const int n_chunks = h->hctx.n_chunks;
    if (chain != S2M_DEBUG_PREP_READ) {
        const bool legacy = chain == S2M_DEBUG_PREP_LEGACY;
        PrepTable t;
        t.s[0] = h->reg.prep_slot;
        S2M_HIP(h, hipMemsetAsync(h->reg.chunk_factor.p, 0, sizeof(int32_t) * (size_t)(n_chunks + 1), h->stream));
        launch_scan_prep(h->stream, t, 1, !legacy);
        S2M_HIP(h, hipGetLastError());
        h->reg.table_stale = !legacy;
        h->hctx.density_pending = 1;
        h->ctx_dirty = true;
        if (pose) {
            const LoopShape sh = shape_of(h);
            if (legacy) {
                int rc = push_state(h, pose);
                if (rc) return rc;
                launch_density_wishes(h, sh);
            } else {
                launch_density_state(h, pose, nullptr);
                h->ctx_dirty = false;
                h->reg.table_stale = false;
            }
            S2M_HIP(h, hipGetLastError());
            // the wishes before k_chunk_table_density consumes them
            if (chunk_factor) S2M_HIP(h, hipMemcpyAsync(chunk_factor, h->reg.chunk_factor.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
            launch_density_table(h, sh);
            S2M_HIP(h, hipGetLastError());
            h->hctx.density_pending = 0;                  // cleared on the device by the kernel: keep the host copy in step
        } else if (wave_table || n_waves)
            ensure_wave_table(h);
    }
    if ((!pose || chain == S2M_DEBUG_PREP_READ) && chunk_factor)
        S2M_HIP(h, hipMemcpyAsync(chunk_factor, h->reg.chunk_factor.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
    if (qperm) S2M_HIP(h, hipMemcpyAsync(qperm, h->reg.qperm.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    if (qxyz) {
        S2M_HIP(h, hipMemcpyAsync(qxyz, h->reg.qx.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipMemcpyAsync(qxyz + n, h->reg.qy.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipMemcpyAsync(qxyz + 2 * n, h->reg.qz.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    }
    if (chunk_parts) S2M_HIP(h, hipMemcpyAsync(chunk_parts, h->reg.chunk_parts.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
    int32_t nw = 0;
    const bool have_table = !h->reg.table_stale;
    if (have_table) S2M_HIP(h, hipMemcpyAsync(&nw, h->reg.n_waves.p, sizeof(nw), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (nw < 0 || nw > h->hctx.table_cap) return fail(h, S2M_ERR_HIP, "wave count outside the table");
    if (wave_table && nw > 0) {
        S2M_HIP(h, hipMemcpyAsync(wave_table, h->reg.wave_table.p, sizeof(int2) * (size_t)nw, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (n_waves) *n_waves = have_table ? nw : -1;
    return S2M_OK;
}

// Diagnostics: workgroups the certify kernels of the last collected loop handed to the search kernel (0 for a fused loop;
// slot >= 0: that scan slot of the last batch).
int s2m_debug_deferred(s2m_handle h, int slot)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (slot >= 0) { if (slot >= (int)h->batch.kids.size()) return S2M_ERR_INVALID_ARG; h = h->batch.kids[(size_t)slot]; }
    return h->reg.h_state ? h->reg.h_state[1].deferred_total : 0;
}

static int time_iterations_impl(s2m_handle h, const float pose[6], int reps, float* ms_mean, float* ms_per_iter)
{
    if (!h || !pose || reps < 1) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    const int nit = h->prm.max_iter;
    if (h->reg.iter_events.size() < (size_t)(2 * nit)) {
        const size_t old = h->reg.iter_events.size();
        h->reg.iter_events.resize(2 * nit);
        for (size_t k = old; k < h->reg.iter_events.size(); k++) S2M_HIP(h, hipEventCreate(&h->reg.iter_events[k]));
    }
    std::vector<double> per_iter((size_t)nit, 0.0);
    for (int rep = 0; rep < reps; rep++) {
        // a new scan starts without a prior or cached planes (what s2m_set_scan leaves behind)
        S2M_HIP(h, hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream));
        S2M_HIP(h, hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream));
        if ((rc = push_state(h, pose))) return rc;
        enqueue_loop(h, shape_of(h), h->reg.iter_events.data());     // the real loop, launched one by one between event pairs
        h->hctx.density_pending = 0;
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (int it = 0; it < nit; it++) {
            float ms = 0;
            S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.iter_events[2 * it], h->reg.iter_events[2 * it + 1]));
            per_iter[(size_t)it] += ms;
        }
    }
    double total = 0.0;
    for (int it = 0; it < nit; it++) {
        total += per_iter[(size_t)it];
        if (ms_per_iter) ms_per_iter[it] = (float)(per_iter[(size_t)it] / reps);
    }
    if (ms_mean) *ms_mean = (float)(total / ((double)reps * nit));
    return S2M_OK;
}

// Diagnostics: one full loop from `pose` (max_iter iterations, so early_exit should be off), then `reps` back-to-back
// replays of the loop's last registration launch in the state the loop ended in (nearly every point certified):
// solve_prev = 1 closes the iteration before it in its prologue each time (the steady launch of the fused loop),
// 0 rebuilds the transform only.  Returns the mean time per replayed launch, gaps included.
int s2m_debug_time_steady(s2m_handle h, const float pose[6], int reps, int solve_prev, float* us_per_launch)
{
    if (!h || !pose || reps < 1 || !us_per_launch) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    float p[6];
    memcpy(p, pose, 24);
    s2m_result r;
    int rc = s2m_optimize_resident(h, p, nullptr, &r);
    if (rc) return rc;
    if (r.skipped || r.iters_run != h->prm.max_iter) return fail(h, S2M_ERR_INVALID_ARG, "the loop ended early: switch early_exit off");
    const LoopShape sh = shape_of(h);
    const int L = h->prm.max_iter;
    S2M_HIP(h, hipEventRecord(h->reg.ev_c, h->stream));
    for (int k = 0; k < reps; k++)
        launch_iteration(h, sh, sh.split ? L + (k & 1) : L, solve_prev ? 1 : 0);   // (split: the worklist slots alternate with the launch parity)
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipEventRecord(h->reg.ev_d, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.ev_c, h->reg.ev_d));
    *us_per_launch = ms * 1e3f / (float)reps;
    return S2M_OK;
}

// Mean duration of a k_register launch over `reps` whole LM loops (max_iter >= 5, fused loop), gaps between the back-to-back
// launches included: HIP events on the handle's stream around launch 0, launch 1, the run of launches 2 .. n-2 and launch n-1.
int s2m_time_loop_launches(s2m_handle h, const float pose[6], int reps, float* us_per_launch)
{
    if (!h || !pose || reps < 1 || !us_per_launch) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    const int nit = h->prm.max_iter;
    if (nit < 5) return fail(h, S2M_ERR_INVALID_ARG, "needs max_iter >= 5");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    while (h->reg.iter_events.size() < 8) { hipEvent_t e; S2M_HIP(h, hipEventCreate(&e)); h->reg.iter_events.push_back(e); }
    double total_ms = 0.0;
    for (int rep = 0; rep < reps; rep++) {
        S2M_HIP(h, hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream));      // a new scan: no certificates, no neighbourhoods
        S2M_HIP(h, hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream));
        if ((rc = push_state(h, pose))) return rc;
        enqueue_loop(h, shape_of(h), h->reg.iter_events.data(), true);
        h->hctx.density_pending = 0;
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.iter_events[2 * k], h->reg.iter_events[2 * k + 1]));
            total_ms += ms;
        }
    }
    *us_per_launch = (float)(total_ms * 1e3 / ((double)reps * nit));
    return S2M_OK;
}

int s2m_time_iteration_kernel(s2m_handle h, const float pose[6], int reps, float* ms_per_launch)
{
    if (!ms_per_launch) return S2M_ERR_INVALID_ARG;
    return time_iterations_impl(h, pose, reps, ms_per_launch, nullptr);
}

int s2m_time_iterations(s2m_handle h, const float pose[6], int reps, float* ms_per_iter, int cap)
{
    if (!h || !ms_per_iter || cap < h->prm.max_iter) return S2M_ERR_INVALID_ARG;
    return time_iterations_impl(h, pose, reps, nullptr, ms_per_iter);
}

int s2m_debug_kf_select_last_check_args(const s2m_debug_kf_select_out* out)
{
    if (!out) return S2M_ERR_INVALID_ARG;
    if (out->cent_cap > 0 && (!out->cent || !out->nn)) return S2M_ERR_INVALID_ARG;
    if (out->frames_cap > 0 && (!out->keys || !out->offsets)) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

// Observation hook: the stages the last kf_select on the handle's workspace left resident (s2m_voxel.hpp, KfLast), copied out as they
// stand.  No kernel runs; the float4 centroids are narrowed to xyz on the host.
int s2m_debug_kf_select_last(s2m_handle h, s2m_debug_kf_select_out* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_debug_kf_select_last_check_args(out)) return fail(h, S2M_ERR_INVALID_ARG, "null output, or a null array with a capacity above 0");
    KfLast last;
    if (!kf_select_last(h->voxel.ws, &last)) return fail(h, S2M_ERR_NO_SCAN, "no key-frame selection has run on the handle");
    out->path = last.path;
    out->n_cand = last.sel.n_cand; out->n_cent = last.sel.n_cent; out->n_frames = last.sel.n_frames;
    out->n_points = last.sel.n_points;
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t n_cent = (size_t)last.sel.n_cent, n_frames = (size_t)last.sel.n_frames;
    const size_t nc = std::min(n_cent, out->cent_cap), nf = std::min(n_frames, out->frames_cap);
    std::vector<float> c4(4 * nc);
    if (nc > 0) {
        S2M_HIP(h, hipMemcpyAsync(c4.data(), last.cent, sizeof(float) * 4 * nc, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipMemcpyAsync(out->nn, last.nn, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    }
    if (nf > 0) S2M_HIP(h, hipMemcpyAsync(out->keys, last.tab.keys, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, h->stream));
    if (out->frames_cap > 0 && nf == n_frames)
        S2M_HIP(h, hipMemcpyAsync(out->offsets, last.tab.offsets, sizeof(int32_t) * (n_frames + 1), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < nc; k++) memcpy(out->cent + 3 * k, c4.data() + 4 * k, sizeof(float) * 3);
    if (n_cent > out->cent_cap || n_frames > out->frames_cap) return fail(h, S2M_ERR_CAPACITY, "fewer centroids or frames offered than the selection holds");
    return S2M_OK;
}

// Host only: a copy of the notes the batch entry points took where they issued their launches (s2m_context::Batch::last).
int s2m_debug_batch_last(s2m_handle h, s2m_debug_batch_last_out* out)
{
    if (!h || !out) return S2M_ERR_INVALID_ARG;
    const s2m_context::Batch::Last& last = h->batch.last;
    memset(out, 0, sizeof(*out));
    out->n_scans = last.n_scans; out->n_live = last.n_live;
    out->ctx_launches = last.ctx_launches; out->init_launches = last.init_launches; out->prep_launches = last.prep_launches;
    out->ranges_issued = last.ranges_issued;
    out->graph_cached = last.graph_hits > 0 && last.graph_captures == 0;
    out->n_loops = last.n_loops;
    for (int j = 0; j < 2; j++) {
        const LoopIssued& l = last.loop[j];
        out->loop[j].wpb = l.wpb; out->loop[j].nslots = l.nslots; out->loop[j].nblocks = l.nblocks;
        out->loop[j].fused = l.fused; out->loop[j].first_split = l.first_split;
    }
    return S2M_OK;
}

}  // extern "C"
