// s2m_abi.hip — host side of the gfx950 scan-to-map LM loop and the part of the C ABI (include/liorf_s2m.h) that launches its
// kernels: create / destroy / params, the context and state uploads, the loop and its graphs, launch / collect of a single
// scan.  The only translation unit that includes s2m_kernels.hpp / s2m_register.hpp.
//
// Runs the whole <= max_iter LM loop as one captured hipGraph (enqueue_loop) so that a scan costs one graph launch and one
// synchronisation.  The map index and the scan preparation in front of it are s2m_prep.hip's, batches and slots
// s2m_abi_batch.hip's, the observation and timing hooks s2m_abi_debug.hip's (both launch the loop's kernels through the
// functions s2m_context.hpp declares for this unit), ScanContext s2m_sc.hip's and s2m_abi_sc.hip's.  The handle is
// s2m_context.hpp's; the entry points that only orchestrate other units' stages live in s2m_abi_voxel.hip,
// s2m_abi_keyframes.hip, s2m_abi_loop.hip, s2m_abi_icp.hip, s2m_abi_reloc.hip and s2m_abi_front_end.hip.  There is no CPU fallback: without a gfx950 device every
// entry point fails with S2M_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "s2m_context.hpp"
#include "s2m_kernels.hpp"

using namespace s2m;
using namespace s2m::host;

// milliseconds between two device stamps of the pinned block (valid once the stream has been synchronised behind the kernels
// that wrote them)
float s2m::host::stamps_ms(const s2m_context* h, int from, int to)
{
    const unsigned long long a = h->reg.h_stamps[from], b = h->reg.h_stamps[to];
    return (b > a && h->reg.wall_clock_khz > 0) ? (float)((double)(b - a) / (double)h->reg.wall_clock_khz) : 0.0f;
}

// the partial rows of a launch (two slots, by launch parity) and, behind them, the search kernel's worklist
int s2m::host::ensure_rows(s2m_context* h, int nblocks)
{
    const size_t rows = sizeof(double) * 2 * kAcc * (size_t)nblocks;
    int rc = ensure(h, h->reg.partials, rows + 64 + sizeof(int32_t) * 2 * (size_t)nblocks);
    if (rc) return rc;
    h->hctx.partials = h->reg.partials.as<double>();
    h->hctx.wl_count = reinterpret_cast<int32_t*>(h->reg.partials.as<unsigned char>() + rows);
    h->hctx.wl_items = h->hctx.wl_count + 16;
    h->ctx_dirty = true;
    return S2M_OK;
}

int s2m::host::upload_ctx(s2m_context* h)
{
    if (!h->ctx_dirty) return S2M_OK;
    hipLaunchKernelGGL(k_set_ctx, dim3(1), dim3(64), 0, h->stream, h->reg.dctx.as<DevCtx>(), h->hctx);
    S2M_HIP(h, hipGetLastError());
    h->ctx_dirty = false;
    return S2M_OK;
}

void s2m::host::fill_state(s2m_context* h, DevState* s, const float pose[6])
{
    memset(s, 0, sizeof(*s));
    memcpy(s->pose, pose, 24);
    memcpy(s->pose2[0], pose, 24);       // launch 0 runs with slot 0
    host_pose_to_transform(pose, s->T, s->sc);
    s->T_valid = 1;
    memcpy(s->matP, h->reg.persist_matP, sizeof(s->matP));
    s->isDegenerate = h->reg.persist_degenerate;
}

// `s` as the loop state, with the wave count of the resident scan folded in (k_set_state)
// `stamp` (pinned, may be null): where the kernel leaves the wall clock once the state is stored
void s2m::host::store_state(s2m_context* h, const DevState& s, unsigned long long* stamp)
{
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, h->stream, h->reg.state.as<DevState>(), s,
                       (const int32_t*)h->reg.n_waves.as<int32_t>(), stamp);
}

int s2m::host::push_state(s2m_context* h, const float pose[6], unsigned long long* stamp)
{
    DevState s;
    fill_state(h, &s, pose);
    ensure_wave_table(h);                                 // (k_set_state copies the wave count)
    if (h->ctx_dirty) {
        hipLaunchKernelGGL(k_set_ctx_state, dim3(1), dim3(64), 0, h->stream, h->reg.dctx.as<DevCtx>(), h->hctx, h->reg.state.as<DevState>(), s,
                           (const int32_t*)h->reg.n_waves.as<int32_t>(), stamp);
        h->ctx_dirty = false;
    } else
        store_state(h, s, stamp);
    S2M_HIP(h, hipGetLastError());
    return S2M_OK;
}

// The density wishes of a single scan's first optimisation from `pose`, with the DevCtx block and the loop state it starts from
// (k_wave_density_state: one plain launch, no wave table needed); `stamp` as push_state's
void s2m::host::launch_density_state(s2m_context* h, const float pose[6], unsigned long long* stamp)
{
    DensityStateArgs a;
    a.c = h->hctx;
    fill_state(h, &a.v, pose);
    a.cdst = h->reg.dctx.as<DevCtx>(); a.sdst = h->reg.state.as<DevState>();
    a.stamp = stamp;
    a.raw_limit = h->tune.density_raw;
    hipLaunchKernelGGL(k_wave_density_state, dim3((h->hctx.n_chunks + 3) / 4 + 1), dim3(256), 0, h->stream, a);       // (+ 1: the workgroup that stores the blocks)
}

void s2m::host::launch_chunk_table(hipStream_t stream, const PrepTable& t, int nslots)
{
    hipLaunchKernelGGL(k_chunk_table, dim3(1, nslots), dim3(1024), 0, stream, t);
}

void s2m::host::launch_set_ctxs(hipStream_t stream, CtxTable& t, int n, int* issued)
{
    for (int j = n; j < kCtxSlots; j++) t.dst[j] = nullptr;
    hipLaunchKernelGGL(k_set_ctxs, dim3(n), dim3(64), 0, stream, t);
    if (issued) ++*issued;
}

void s2m::host::launch_init_states(hipStream_t stream, StateInitTable& t, int n, int* issued)
{
    for (int j = n; j < kInitSlots; j++) t.s[j].dst = nullptr;
    hipLaunchKernelGGL(k_init_states, dim3(n), dim3(256), 0, stream, t);
    if (issued) ++*issued;
}

// The LM loop (:1304-1315) as a launch sequence.  One iteration L is either one launch of the fused kernel R(L), or -
// split - the certify kernel C(L) followed by the search kernel S(L) for the workgroups C put on its worklist (launch 0 of a
// scan, where nothing is certified yet: S alone, over every workgroup).  When the whole grid is co-resident iterations
// 1..n-2 are closed inside the prologue of the following R / C (solve_prev): every workgroup repeats the small solve, and
// a kernel boundary plus a one-workgroup kernel disappear from every iteration:
//   R0 F0 R1 R2' R3' ... R(n-1)' F(n-1)        (' = closes the iteration before it)
//   S0 F0 C1 S1 C2' S2 ... C(n-1)' S(n-1) F(n-1)
// The plain form  R0 F0 R1 F1 ...  remains for A/B measurements (S2M_NO_FUSE=1).
// Several scan slots (a batch) advance in lockstep: every launch has one grid row per slot.
constexpr int kFuseMaxBlocks = 512;
static_assert(sizeof(CtxTable) <= 4096 && sizeof(StateInitTable) <= 4096 && sizeof(PrepTable) <= 4096 && sizeof(SlotTable) <= 4096 &&
              sizeof(DensityStateArgs) <= 4096,
              "kernel arguments are limited to 4 KB");

LoopShape s2m::host::shape_of(s2m_context* h)
{
    LoopShape sh;
    memset(&sh.tbl, 0, sizeof(sh.tbl));
    sh.tbl.ctx[0] = h->reg.dctx.as<DevCtx>();
    sh.tbl.st[0] = h->reg.state.as<DevState>();
    sh.nslots = 1; sh.nblocks = h->hctx.nblocks; sh.table_cap = h->hctx.table_cap; sh.wpb = h->hctx.wpb;
    sh.batch = h->batch.parent != nullptr && h->reg.pending != Reg::kSlot;    // (a slot's own loop is a single scan's)
    sh.split = h->tune.split_mode == 1;
    return sh;
}

namespace {

template <bool HOOK, int NW, int MINW, int MODE, int CNW>
inline void launch_k(hipStream_t s, const LoopShape& sh, int L, int flags, int grid_x = 0)
{
    hipLaunchKernelGGL((k_register<HOOK, NW, MINW, MODE, CNW>), dim3(grid_x > 0 ? std::min(grid_x, sh.nblocks) : sh.nblocks, sh.nslots), dim3(NW * 64), 0, s,
                       sh.tbl, L, flags);
}

// the search kernel S(L): over the worklist C(L) left, or (all) over every workgroup
// (small_grid: late in a loop the list is short - a few workgroups per slot walk it instead of one workgroup per row)
inline void launch_search(s2m_context* h, const LoopShape& sh, int L, bool all, bool small_grid = false)
{
    constexpr int NW = kBlock / 64;
    const bool close_after = small_grid && !all && h->tune.close_in_search;     // one workgroup per slot walks the list and closes the iteration
    const int fl = (all ? kFlagAll : 0) | (close_after ? kFlagCloseAfter : 0);
    const int gx = close_after ? 1 : ((small_grid && !all) ? h->tune.search_grid : 0);
    if (sh.wpb == kBigWaves) launch_k<false, NW, 2, kSearch, kBigWaves>(h->stream, sh, L, fl, gx);
    else if (sh.batch && h->tune.batch_minw == 4) launch_k<false, NW, 4, kSearch, NW>(h->stream, sh, L, fl, gx);
    else                     launch_k<false, NW, 2, kSearch, NW>(h->stream, sh, L, fl, gx);
}

inline void launch_certify(s2m_context* h, const LoopShape& sh, int L, int solve_prev, bool fused_loop)
{
    constexpr int NW = kBlock / 64;
    const int fl = solve_prev ? kFlagSolvePrev : 0;
    if (!fused_loop && sh.wpb == NW && h->tune.lean_certify)      // iterations closed by k_finalize: the 64-register kernel
        hipLaunchKernelGGL((k_certify_lean<NW, 1, kCertifyLeanWaves>), dim3(sh.nblocks, sh.nslots), dim3(NW * 64), 0, h->stream, sh.tbl, L);
    else if (sh.wpb == kBigWaves) launch_k<false, kBigWaves, kCertifyWavesBig, kCertify, kBigWaves>(h->stream, sh, L, fl);
    else                     launch_k<false, NW, kCertifyWaves, kCertify, NW>(h->stream, sh, L, fl);
}

}  // namespace

// one fused launch R(L) in the workgroup shape of the scan (DevCtx::wpb); `hook`: the observation variant
void s2m::host::launch_fused(s2m_context* h, const LoopShape& sh, bool hook, int L, int solve_prev)
{
    constexpr int NW = kBlock / 64;
    const int fl = solve_prev ? kFlagSolvePrev : 0;
    if (sh.wpb == kBigWaves) {
        if (hook) launch_k<true, kBigWaves, 4, kFused, kBigWaves>(h->stream, sh, L, fl);
        else      launch_k<false, kBigWaves, 4, kFused, kBigWaves>(h->stream, sh, L, fl);
    } else if (sh.batch && h->tune.batch_minw == 4 && !hook) {
        launch_k<false, NW, 4, kFused, NW>(h->stream, sh, L, fl);          // two workgroups per CU (spills in the search path)
    } else {
        if (hook) launch_k<true, NW, 2, kFused, NW>(h->stream, sh, L, fl);
        else      launch_k<false, NW, 2, kFused, NW>(h->stream, sh, L, fl);
    }
}

// iteration L of the loop: R(L), or C(L) S(L)
void s2m::host::launch_iteration(s2m_context* h, const LoopShape& sh, int L, int solve_prev, bool fused_loop)
{
    if (!sh.split) { launch_fused(h, sh, false, L, solve_prev); return; }
    if (L == 0) { launch_search(h, sh, 0, true); return; }
    launch_certify(h, sh, L, solve_prev, fused_loop);
    launch_search(h, sh, L, false, sh.late);
    if (h->reg.last_loop.first_split < 0) h->reg.last_loop.first_split = L;
}

// ends_range: the last launch of the range (it hands the record over, see LoopShape::out)
void s2m::host::launch_finalize(s2m_context* h, const LoopShape& sh, int L, int mode, bool ends_range)
{
    hipLaunchKernelGGL(k_finalize, dim3(1, sh.nslots), dim3(kFinThreads), 0, h->stream, sh.tbl, L, mode,
                       ends_range ? sh.out : (DevState*)nullptr, ends_range ? sh.stamp : (unsigned long long*)nullptr);
}

// the two launches of launch_density: the wishes of every wave-table entry, and the table rebuilt from them
void s2m::host::launch_density_wishes(s2m_context* h, const LoopShape& sh)
{
    hipLaunchKernelGGL(k_wave_density, dim3((sh.table_cap + 3) / 4, sh.nslots), dim3(256), 0, h->stream, sh.tbl, h->tune.density_raw);
}
void s2m::host::launch_density_table(s2m_context* h, const LoopShape& sh)
{
    hipLaunchKernelGGL(k_chunk_table_density, dim3(1, sh.nslots), dim3(1024), 0, h->stream, sh.tbl);
}

void s2m::host::launch_density(s2m_context* h, const LoopShape& sh)
{
    // re-split the wave table for the map density at the initial guess (the transform k_set_state just stored);
    // both kernels take everything from the DevCtx block, so the captured graph stays valid from scan to scan
    if (!sh.wishes_done) launch_density_wishes(h, sh);
    launch_density_table(h, sh);
}

// Launches L0 .. L1-1 of the loop.  A range that starts after launch 0 begins like launch 1 does (transform rebuilt from the
// pose the k_finalize before it stored), and a range that ends before the last launch closes its last iteration with a
// k_finalize of its own: with early exit on, the loop is issued in two ranges and the second only if the first did not converge.
// `events`, if given, holds 2*n events recorded around every iteration's launches; with `coarse` only four pairs are recorded - around
// launch 0, launch 1, the run of back-to-back launches 2 .. n-2 (slots 4, 5) and launch n-1 (slots 6, 7) - so that the event
// packets do not break up the loop's back-to-back dispatch.
void s2m::host::enqueue_loop(s2m_context* h, const LoopShape& sh_in, hipEvent_t* events, bool coarse, int L0, int L1)
{
    const int n = h->prm.max_iter;
    if (L1 < 0) L1 = n;
    const bool fuse = h->tune.fuse_solve && sh_in.nblocks * sh_in.nslots <= h->tune.fuse_max_blocks;     // the whole grid co-resident (see above)
    LoopShape sh = sh_in;
    h->reg.last_loop = LoopIssued{ sh.wpb, sh.nslots, sh.nblocks, fuse ? 1 : 0, -1 };       // (launch_iteration notes the first certify + search)
    // S2M_SPLIT=2: from launch `split_from` on (the first launches search most points: there the certify kernel is only one
    // more launch in front of the search) the iterations of a loop closed by k_finalize run certify (lean) + search
    const bool split_late = sh.split_auto && !fuse && sh.wpb == kBlock / 64 && h->tune.lean_certify;   // (with early exit on these launches are the second range: issued only for scans that need them)
    if (h->tune.density_raw > 0 && L0 == 0) launch_density(h, sh);
    for (int L = L0; L < L1; L++) {
        const int slot = !coarse ? 2 * L : (L == 0 ? 0 : (L == 1 ? 2 : (L == n - 1 ? 6 : 4)));
        const bool open = events && (!coarse || L <= 2 || L == n - 1), close = events && (!coarse || L <= 1 || L >= n - 2);
        if (open) (void)hipEventRecord(events[slot], h->stream);
        sh.split = sh_in.split || (split_late && L >= h->tune.split_from);
        sh.late = !sh_in.split && sh.split;
        launch_iteration(h, sh, L, (fuse && L >= 2 && L != L0) ? 1 : 0, fuse);
        if (close) (void)hipEventRecord(events[slot + 1], h->stream);
        if ((!fuse || L == 0 || L == L1 - 1) && !(sh.late && h->tune.close_in_search)) launch_finalize(h, sh, L, 0, L == L1 - 1);   // (late split: the search launch closes)
    }
}

namespace {

// part 0: the whole loop; 1: launches 0 .. seg-1; 2: launches seg .. max_iter-1
int get_graph(s2m_context* h, int nblocks, int part, hipGraphExec_t* out)
{
    // table_cap fixes both grids in the captured loop: k_register's (nblocks) and k_wave_density's
    LoopShape sh = shape_of(h);
    // Loop state + trace come back from inside the graph, into the pinned mirror (its address never changes).  The last launch
    // of a single scan's range is always a k_finalize (only the late split of a lockstep batch closes in the search kernel):
    // it writes the record there itself.  (A copy node as the graph's last: 4.4 us and a boundary; a copy issued behind the
    // graph starts ~10 us after the graph's last kernel.)  The first range - the whole loop, mostly - also stamps its end.
    sh.out = &h->reg.h_state[1];
    sh.stamp = part == 2 ? nullptr : h->reg.h_stamps + kStampLoop1;
    sh.wishes_done = h->batch.parent == nullptr;          // a single scan: k_wave_density_state ran as a plain launch in front of the graph
    const long long key = (((long long)h->hctx.table_cap * 4 + part) * 256 + (part ? h->tune.seg_iters : 0)) * 4 + (sh.split ? 1 : 0) + (sh.wpb == kBigWaves ? 2 : 0);
    auto it = h->reg.graphs.find(key);
    if (it != h->reg.graphs.end()) { *out = it->second; return S2M_OK; }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    S2M_HIP(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    enqueue_loop(h, sh, nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (e != hipSuccess || !graph) return fail(h, S2M_ERR_HIP, "hipStreamEndCapture", e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "hipGraphInstantiate", e);
    h->reg.graphs[key] = exec;
    *out = exec;
    return S2M_OK;
}

int launch_loop(s2m_context* h, int part = 0)
{
    const int nblocks = h->hctx.nblocks;
    // The first range is timed by device stamps: its start by the state upload before it (optimize_launch), its end by the
    // k_finalize that closes it.  The second range, issued only for a scan that did not converge in the first, keeps an event
    // pair (second_range).
    if (h->tune.use_graph) {
        hipGraphExec_t exec = nullptr;
        int rc = get_graph(h, nblocks, part, &exec);
        if (rc == S2M_OK) {
            S2M_HIP(h, hipGraphLaunch(exec, h->stream));
            h->hctx.density_pending = 0;                  // cleared on the device by k_chunk_table_density: keep the host copy in step
            return S2M_OK;
        }
        h->tune.use_graph = false;       // capture unsupported here: fall back to plain launches
    }
    LoopShape sh = shape_of(h);
    sh.stamp = part == 2 ? nullptr : h->reg.h_stamps + kStampLoop1;
    sh.wishes_done = h->batch.parent == nullptr;
    enqueue_loop(h, sh, nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState) + sizeof(s2m_iter_trace) * h->prm.max_iter, hipMemcpyDeviceToHost, h->stream));
    h->hctx.density_pending = 0;
    return S2M_OK;
}

// the parameters the kernels read, into the host copy of the DevCtx block
void params_to_ctx(s2m_context* h, const s2m_params& prm)
{
    h->hctx.gate_f = nextafterf((float)prm.gate_sq, INFINITY);
    h->hctx.gate_r = nextafterf(sqrtf((float)prm.gate_sq), 0.0f);
    h->hctx.gate_sq = prm.gate_sq; h->hctx.plane_tol = prm.plane_tol; h->hctx.weight_scale = prm.weight_scale;
    h->hctx.weight_min = prm.weight_min; h->hctx.conv_deg = prm.conv_deg; h->hctx.conv_cm = prm.conv_cm;
    h->hctx.eig_thresh = prm.eig_thresh; h->hctx.min_corr = prm.min_corr; h->hctx.max_iter = prm.max_iter;
    h->hctx.early_exit = prm.early_exit;
    h->ctx_dirty = true;
}

}  // namespace

// the soft conditions in front of the loop (:1297, :1300)
bool s2m::host::optimize_gate(s2m_context* k, const float pose[6])
{
    memcpy(k->reg.pending_pose_in, pose, 24);
    k->reg.pending_skipped = k->reg.n_m == 0 ? 1 : ((int)k->reg.n_q <= k->prm.min_feats ? 2 : 0);
    return k->reg.pending_skipped == 0;
}

int s2m::host::optimize_launch(s2m_context* h, const float pose[6], Reg::Pending kind)
{
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    const bool runs = optimize_gate(h, pose);
    h->reg.pending = kind;                                // (nothing refuses from here on; shape_of reads the kind)
    if (!runs) return S2M_OK;
    PendingGuard undo(h);
    int rc;
    if (!h->batch.parent && h->hctx.density_pending && h->tune.density_raw > 0) {
        // the first optimisation of a single scan: the density wishes, the DevCtx block and the loop state in one plain launch
        // (k_wave_density_state needs no wave table; the graph behind it starts with k_chunk_table_density)
        launch_density_state(h, pose, h->reg.h_stamps + kStampLoop0);
        S2M_HIP(h, hipGetLastError());
        h->ctx_dirty = false;
        h->reg.table_stale = false;                       // k_chunk_table_density emits the table
    } else if ((rc = push_state(h, pose, h->reg.h_stamps + kStampLoop0))) return rc;      // (with the DevCtx block when that changed)
    h->reg.seg_pending = two_ranges(h);
    if ((rc = launch_loop(h, h->reg.seg_pending ? 1 : 0))) return rc;        // (state + trace come back with it)
    undo.release();
    return S2M_OK;
}

void s2m::host::collect_record(s2m_context* k, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    s2m_result r;
    memset(&r, 0, sizeof(r));
    r.skipped = k->reg.pending_skipped;
    k->reg.last_trace_n = 0;
    float t[6];
    memcpy(t, k->reg.pending_pose_in, 24);
    if (!r.skipped) {
        const DevState& s = k->reg.h_state[1];
        memcpy(t, s.pose, 24);
        r.iters_run = s.iters_run; r.converged = s.converged; r.is_degenerate = s.isDegenerate;
        r.n_sel_last = s.n_sel_last;
        k->reg.persist_degenerate = s.isDegenerate;
        memcpy(k->reg.persist_matP, s.matP, sizeof(s.matP));
        // trace: executed iterations; a loop that stalled at iteration k (fewer than min_corr correspondences,
        // pose unchanged, :1178-1180) repeats that no-op record for the iterations the reference would still run
        int n_exec = s.iters_run, stall_at = -1;
        for (int i = 0; i < n_exec && i < kMaxIter; i++) {
            if (stall_at >= 0) { k->reg.last_trace[i] = k->reg.last_trace[stall_at]; continue; }
            k->reg.last_trace[i] = k->reg.h_trace[i];
            if (s.stalled && !k->reg.h_trace[i].stepped) stall_at = i;
        }
        k->reg.last_trace_n = n_exec < kMaxIter ? n_exec : kMaxIter;
        host_transform_update(k->prm, imu, t, r.affine);                           // :1317
    } else {
        host_pose_to_transform(t, r.affine, nullptr);
        r.is_degenerate = k->reg.persist_degenerate;
    }
    memcpy(r.pose, t, 24);
    memcpy(pose, t, 24);
    if (out) *out = r;
}

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* s2m_version(void) { return "liorf_amd s2m 0.1 (gfx950)"; }

int s2m_default_params(s2m_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(s2m_params);
    p->device_id = 0; p->stream = nullptr;
    p->k_neighbors = 5; p->gate_sq = 1.0; p->plane_tol = 0.2; p->weight_scale = 0.9; p->weight_min = 0.1;
    p->min_corr = 50; p->min_feats = 30; p->max_iter = 30; p->eig_thresh = 100.0f;
    p->conv_deg = 0.05; p->conv_cm = 0.05; p->z_tol = FLT_MAX; p->rot_tol = FLT_MAX;
    p->imu_type = 0; p->imu_rpy_weight = 0.01f; p->early_exit = 1;
    return S2M_OK;
}

int s2m_create(const s2m_params* p, s2m_handle* out)
{
    if (!out) return S2M_ERR_INVALID_ARG;
    *out = nullptr;
    s2m_params prm;
    if (p) {
        if (p->struct_size != sizeof(s2m_params)) return S2M_ERR_INVALID_ARG;
        prm = *p;
    } else s2m_default_params(&prm);
    if (prm.k_neighbors != 5 || prm.max_iter < 1 || prm.max_iter > kMaxIter || !(prm.gate_sq > 0.0)) return S2M_ERR_INVALID_ARG;

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || prm.device_id < 0 || prm.device_id >= count)
        return S2M_ERR_NO_DEVICE;
    if (hipSetDevice(prm.device_id) != hipSuccess) return S2M_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, prm.device_id) != hipSuccess) return S2M_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return S2M_ERR_NO_DEVICE;   // kernels are built for gfx950 only

    s2m_context* h = new (std::nothrow) s2m_context();
    if (!h) return S2M_ERR_HIP;
    h->prm = prm; h->device = prm.device_id;
    if (const char* e = getenv("S2M_NO_GRAPH")) h->tune.use_graph = !(e[0] == '1');
    if (const char* e = getenv("S2M_NO_FUSE")) h->tune.fuse_solve = !(e[0] == '1');
    if (const char* e = getenv("S2M_DENSITY_RAW")) h->tune.density_raw = atoi(e);
    if (const char* e = getenv("S2M_BIG_BLOCKS")) h->tune.big_blocks = !(e[0] == '0');
    if (const char* e = getenv("S2M_SEGMENT")) h->tune.seg_iters = atoi(e);
    if (const char* e = getenv("S2M_SPLIT")) h->tune.split_mode = atoi(e);
    if (const char* e = getenv("S2M_LOCKSTEP")) h->tune.lockstep = !(e[0] == '0');
    if (const char* e = getenv("S2M_SPLIT_FROM")) h->tune.split_from = std::max(1, atoi(e));
    if (const char* e = getenv("S2M_SEARCH_GRID")) h->tune.search_grid = std::max(1, atoi(e));
    if (const char* e = getenv("S2M_CLOSE_IN_SEARCH")) h->tune.close_in_search = (e[0] == '1');
    if (const char* e = getenv("S2M_BATCH_MINW")) h->tune.batch_minw = atoi(e);
    if (const char* e = getenv("S2M_BATCH_ENTRIES")) h->tune.batch_entries = atoi(e);
    if (const char* e = getenv("S2M_LEAN")) h->tune.lean_certify = !(e[0] == '0');
    h->tune.fuse_max_blocks = kFuseMaxBlocks;
    if (const char* e = getenv("S2M_FUSE_MAX")) h->tune.fuse_max_blocks = atoi(e);

    auto bail = [&](int code) { s2m_destroy(h); return code; };
    if (prm.stream) { h->stream = static_cast<hipStream_t>(prm.stream); h->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(S2M_ERR_HIP);
        h->own_stream = true;
    }
    if (hipEventCreate(&h->reg.ev_a) != hipSuccess || hipEventCreate(&h->reg.ev_b) != hipSuccess ||
        hipEventCreate(&h->reg.ev_c) != hipSuccess || hipEventCreate(&h->reg.ev_d) != hipSuccess ||
        hipEventCreate(&h->reg.ev_a2) != hipSuccess || hipEventCreate(&h->reg.ev_b2) != hipSuccess ||
        hipEventCreateWithFlags(&h->reg.ev_up, hipEventDisableTiming) != hipSuccess) return bail(S2M_ERR_HIP);
    static_assert(sizeof(DevState) % 8 == 0, "the trace follows the state block");
    if (hipHostMalloc((void**)&h->reg.h_state, sizeof(DevState) + kSlotStateStride) != hipSuccess) return bail(S2M_ERR_HIP);
    h->reg.h_trace = reinterpret_cast<s2m_iter_trace*>(h->reg.h_state + 2);
    if (hipHostMalloc((void**)&h->reg.h_mm, 64) != hipSuccess) return bail(S2M_ERR_HIP);
    if (hipHostMalloc((void**)&h->reg.h_stamps, sizeof(unsigned long long) * kStampCount) != hipSuccess) return bail(S2M_ERR_HIP);
    memset(h->reg.h_stamps, 0, sizeof(unsigned long long) * kStampCount);
    {   // the constant-frequency counter behind wall_clock64(); a runtime that does not tell its rate leaves the timings at zero
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, prm.device_id) != hipSuccess || khz <= 0) { khz = 0; (void)hipGetLastError(); }
        h->reg.wall_clock_khz = khz;
    }
    if (hipHostMalloc((void**)&h->sc.h_stage, sizeof(double) * 1220) != hipSuccess) return bail(S2M_ERR_HIP);
    if (ensure(h, h->reg.state, kSlotStateStride) ||                                          // loop state, then the trace
        ensure(h, h->reg.dctx, sizeof(DevCtx)) || ensure(h, h->reg.mm, 64 + sizeof(uint32_t) * 8 * 1024) ||
        ensure(h, h->sc.bins, sizeof(uint32_t) * 1200) || ensure(h, h->sc.out, sizeof(double) * 1220) ||
        ensure(h, h->reg.q_counts, sizeof(int32_t) * kPolarCells))
        return bail(S2M_ERR_HIP);
    if (hipMemsetAsync(h->reg.q_counts.p, 0, sizeof(int32_t) * kPolarCells, h->stream) != hipSuccess) return bail(S2M_ERR_HIP);

    if (!(h->voxel.ws = vox_create())) return bail(S2M_ERR_HIP);
    if (!(h->loop.icp = icp_create())) return bail(S2M_ERR_HIP);

    memset(&h->hctx, 0, sizeof(h->hctx));
    h->hctx.nblocks = kBlocksQuantum;
    h->hctx.wpb = kBlock / 64;
    if (ensure_rows(h, kBlocksQuantum)) return bail(S2M_ERR_HIP);
    h->hctx.state = h->reg.state.as<DevState>();
    h->hctx.trace = reinterpret_cast<s2m_iter_trace*>(h->reg.state.as<DevState>() + 1);
    params_to_ctx(h, prm);
    if (const char* e = getenv("S2M_ABLATE")) h->hctx.ablate = atoi(e);
    h->hctx.tune[0] = 0; h->hctx.tune[1] = 0; h->hctx.tune[2] = 0; h->hctx.tune[3] = 2;      // tune[0..2] are spare: no kernel reads them
    if (const char* e = getenv("S2M_TUNE")) { (void)sscanf(e, "%d,%d,%d,%d", &h->hctx.tune[0], &h->hctx.tune[1], &h->hctx.tune[2], &h->hctx.tune[3]); h->tune.tune_env = true; }
    h->ctx_dirty = true;
    if (upload_ctx(h) != S2M_OK) return bail(S2M_ERR_HIP);
    *out = h;
    return S2M_OK;
}

int s2m_destroy(s2m_handle h)
{
    if (!h) return S2M_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    loop_drop_pending(h, true);                                                         // (a launched loop closure uses the loop buffers)
    pg_drop_pending(h, true);                                                           // (a launched optimise uses the pose graph's)
    for (hipStream_t st : h->batch.branch_streams) (void)hipStreamSynchronize(st);      // (slot work in flight uses the slots' buffers)
    if (h->gmap.copy_stream) (void)hipStreamSynchronize(h->gmap.copy_stream);
    for (s2m_context* k : h->batch.kids) (void)s2m_destroy(k);
    h->batch.kids.clear();
    if (h->batch.state_borrowed) { h->reg.state.forget(); h->reg.h_state = nullptr; }    // (the parent's blocks)
    for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second.exec);
    for (auto& kv : h->reg.graphs) (void)hipGraphExecDestroy(kv.second);
    for (const std::vector<hipEvent_t>* evs : { &h->batch.branch_events, &h->batch.prep_events, &h->reg.iter_events })
        for (hipEvent_t e : *evs) (void)hipEventDestroy(e);
    for (hipEvent_t e : { h->batch.ev_fork, h->batch.ev_prep, h->gmap.ev_xf[0], h->gmap.ev_xf[1], h->gmap.ev_cp[0], h->gmap.ev_cp[1],
                          h->reg.ev_a, h->reg.ev_b, h->reg.ev_a2, h->reg.ev_b2, h->reg.ev_c, h->reg.ev_d, h->reg.ev_up })
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : h->batch.branch_streams) (void)hipStreamDestroy(st);
    if (h->gmap.copy_stream) (void)hipStreamDestroy(h->gmap.copy_stream);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    vox_destroy(h->voxel.ws);
    icp_destroy(h->loop.icp);
    for (void* p : { (void*)h->batch.h_kid_states, (void*)h->reg.h_state, (void*)h->reg.h_mm, (void*)h->reg.h_stamps, (void*)h->sc.h_stage, (void*)h->sc.h_many, (void*)h->ldet.h_pass, (void*)h->proj.h_count,
                     (void*)h->pg.h_sc, (void*)h->pgc.h_io, (void*)h->sess.h_chunk[0], (void*)h->sess.h_chunk[1] })
        if (p) (void)hipHostFree(p);
    delete h;                                              // every DevBuf and the key-frame arena go with their owners
    return S2M_OK;
}

const char* s2m_last_error(s2m_handle h) { return h ? h->err.c_str() : "null handle"; }

int s2m_get_params(s2m_handle h, s2m_params* out)
{
    if (!h || !out) return S2M_ERR_INVALID_ARG;
    *out = h->prm;
    return S2M_OK;
}

int s2m_set_params(s2m_handle h, const s2m_params* p)
{
    if (!h || !p) return S2M_ERR_INVALID_ARG;
    if (p->struct_size != sizeof(s2m_params)) return fail(h, S2M_ERR_INVALID_ARG, "s2m_params.struct_size does not match this library");
    if (p->device_id != h->prm.device_id || p->stream != h->prm.stream || p->k_neighbors != h->prm.k_neighbors ||
        p->gate_sq != h->prm.gate_sq)
        return fail(h, S2M_ERR_INVALID_ARG, "device_id, stream, k_neighbors and gate_sq are fixed at s2m_create (the search grid is built for the gate)");
    if (p->max_iter < 1 || p->max_iter > kMaxIter) return fail(h, S2M_ERR_INVALID_ARG, "max_iter out of range");
    if (h->reg.pending != Reg::kNone || slots_pending(h))   // (a slot in flight runs on a stream of its own, off the graphs dropped below)
        return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (p->max_iter != h->prm.max_iter) {               // the captured loops hold max_iter launches
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (auto& kv : h->reg.graphs) (void)hipGraphExecDestroy(kv.second);
        h->reg.graphs.clear();
        for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second.exec);     // (every branch of a batch graph is such a loop)
        h->batch.graphs.clear();
    }
    h->prm = *p;
    params_to_ctx(h, h->prm);                           // uploaded by the next call that launches anything
    return S2M_OK;
}

int s2m_set_map(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{ return set_map_impl(h, pts, n, stride_bytes, false); }
int s2m_set_map_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes)
{ return set_map_impl(h, d_pts, n, stride_bytes, true); }
int s2m_set_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{ return set_scan_impl(h, pts, n, stride_bytes, false); }
int s2m_set_scan_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes)
{ return set_scan_impl(h, d_pts, n, stride_bytes, true); }

int s2m_optimize_launch(s2m_handle h, const float pose[6])
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    return optimize_launch(h, pose, Reg::kSingle);
}

int s2m_optimize_collect(s2m_handle h, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (h->reg.pending == Reg::kNone) return fail(h, S2M_ERR_INVALID_ARG, "no optimize launch pending");
    PendingGuard done(h);
    if (!h->reg.pending_skipped) {
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        h->reg.t_optimize_ms = stamps_ms(h, kStampLoop0, kStampLoop1);
        if (h->reg.seg_pending && !h->reg.h_state[1].done) {       // the first range did not converge: the rest of the loop
            const int rc = second_range(h, [&] { return launch_loop(h, 2); });
            if (rc) return rc;
        }
    }
    collect_record(h, pose, imu, out);
    return S2M_OK;
}

int s2m_optimize_resident(s2m_handle h, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    int rc = s2m_optimize_launch(h, pose);
    if (rc) return rc;
    return s2m_optimize_collect(h, pose, imu, out);
}

int s2m_optimize(s2m_handle h, const void* scan, size_t n, size_t stride_bytes, float pose[6],
                 const s2m_imu_init* imu, s2m_result* out)
{
    int rc = s2m_set_scan(h, scan, n, stride_bytes);
    if (rc) return rc;
    return s2m_optimize_resident(h, pose, imu, out);
}

int s2m_get_trace(s2m_handle h, s2m_iter_trace* out, int cap)
{
    if (!h || (!out && cap > 0)) return S2M_ERR_INVALID_ARG;
    int n = h->reg.last_trace_n < cap ? h->reg.last_trace_n : cap;
    for (int i = 0; i < n; i++) out[i] = h->reg.last_trace[i];
    return n;
}

// set_scan_ms: from the start of the first ordering kernel to the end of the last.  optimize_ms: from the end of the state upload
// of s2m_optimize_launch to the end of the k_finalize that closes the loop (with early exit on: its first range; the second
// range, where one was needed, is added from an event pair of its own).  Both intervals of a single scan are read from
// wall_clock64() stamps the bracketing kernels store in pinned memory - event records around them cost GPU time in every step -
// so optimize_ms no longer includes the idle time between an event's packet and the first kernel behind it.  A batch is still
// timed by an event pair around its graph; set_map_ms by events.  Synchronises if a scan preparation is still to be timed.
int s2m_last_timing(s2m_handle h, float* optimize_ms, float* set_map_ms, float* set_scan_ms)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->reg.scan_timing_pending) {
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        h->reg.t_set_scan_ms = stamps_ms(h, kStampPrep0, kStampPrep1);
        h->reg.scan_timing_pending = false;
    }
    if (optimize_ms) *optimize_ms = h->reg.t_optimize_ms;
    if (set_map_ms) *set_map_ms = h->reg.t_set_map_ms;
    if (set_scan_ms) *set_scan_ms = h->reg.t_set_scan_ms;
    return S2M_OK;
}


}  // extern "C"
