// s2m_abi_batch.hip — the batch and slot entry points of the C ABI (include/liorf_s2m.h): n scans against one resident map in
// one captured graph (s2m_optimize_batch and its steps), and a stream of scans through slots with a stream each (s2m_slot_*).
// A slot is a child context of the handle (s2m_context::Batch); what is in flight on it is s2m_context::Registration::pending,
// whose rules every launch and collect here keeps.  Host only: the loop's kernels are s2m_abi.hip's and the scan preparation
// s2m_prep.hip's, reached through the functions s2m_context.hpp declares for them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <algorithm>
#include <vector>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

// field by field (the struct has padding): everything a slot has to take over from its parent
bool same_params_but_stream(const s2m_params& a, const s2m_params& b)
{
    return a.struct_size == b.struct_size && a.device_id == b.device_id && a.k_neighbors == b.k_neighbors && a.gate_sq == b.gate_sq &&
           a.plane_tol == b.plane_tol && a.weight_scale == b.weight_scale && a.weight_min == b.weight_min && a.min_corr == b.min_corr &&
           a.min_feats == b.min_feats && a.max_iter == b.max_iter && a.eig_thresh == b.eig_thresh && a.conv_deg == b.conv_deg &&
           a.conv_cm == b.conv_cm && a.z_tol == b.z_tol && a.rot_tol == b.rot_tol && a.imu_type == b.imu_type &&
           a.imu_rpy_weight == b.imu_rpy_weight && a.early_exit == b.early_exit;
}

// child b borrows the parent's map index (no copy) and its per-scan certificates are void when the index changed
int adopt_map(s2m_context* h, s2m_context* k)
{
    if (k->batch.adopted_epoch == h->batch.map_epoch) return S2M_OK;
    k->reg.n_m = h->reg.n_m;
    k->hctx.n_m = h->hctx.n_m;
    k->hctx.g = h->hctx.g;
    k->hctx.map_sorted = h->hctx.map_sorted;
    k->hctx.cell_start = h->hctx.cell_start;
    k->ctx_dirty = true;
    k->batch.adopted_epoch = h->batch.map_epoch;
    if (k->reg.have_scan && k->reg.n_q > 0 && k->reg.cert.p) {
        S2M_HIP(k, hipMemsetAsync(k->reg.cert.p, 0, sizeof(float4) * k->reg.n_q, k->stream));
        S2M_HIP(k, hipMemsetAsync(k->reg.aux.p, 0, sizeof(int4) * k->reg.n_q, k->stream));
    }
    return S2M_OK;
}

// slot k follows its parent before a launch: any parameter changed on the parent since the slot was made, and the map index
int sync_slot(s2m_context* h, s2m_context* k)
{
    int rc = S2M_OK;
    if (!same_params_but_stream(k->prm, h->prm)) {
        s2m_params p = h->prm;
        p.stream = k->prm.stream;
        rc = s2m_set_params(k, &p);
    }
    if (!rc) rc = adopt_map(h, k);
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int ensure_kids(s2m_context* h, int n)
{
    while ((int)h->batch.kids.size() < n) {
        const size_t slot = h->batch.kids.size();
        // the slots' loop states and traces live in one block of the parent's
        if (!h->batch.h_kid_states &&
            (ensure(h, h->batch.kid_states, kSlotStateStride * kMaxSlots) != S2M_OK ||
             hipHostMalloc((void**)&h->batch.h_kid_states, sizeof(DevState) + kSlotStateStride * kMaxSlots) != hipSuccess))
            return fail(h, S2M_ERR_HIP, "batch: state block allocation failed");
        s2m_params p = h->prm;
        p.stream = h->stream;                              // everything outside the captured graph is ordered on the parent's stream
        s2m_context* k = nullptr;
        const int rc = s2m_create(&p, &k);
        if (rc) return fail(h, rc, "batch: could not create a scan slot");
        k->batch.parent = h;
        k->hctx.ablate = h->hctx.ablate;
        memcpy(k->hctx.tune, h->hctx.tune, sizeof(h->hctx.tune));
        (void)k->reg.state.reset();                        // from here on an alias: forgotten, not freed, in s2m_destroy
        (void)hipHostFree(k->reg.h_state);
        k->reg.state.p = h->batch.kid_states.as<unsigned char>() + kSlotStateStride * slot; k->reg.state.cap = kSlotStateStride;
        k->reg.h_state = reinterpret_cast<DevState*>(h->batch.h_kid_states + kSlotStateStride * slot);      // [1] = the download area of this slot
        k->reg.h_trace = reinterpret_cast<s2m_iter_trace*>(k->reg.h_state + 2);
        k->batch.state_borrowed = true;
        k->hctx.state = k->reg.state.as<DevState>();
        k->hctx.trace = reinterpret_cast<s2m_iter_trace*>(k->reg.state.as<DevState>() + 1);
        k->ctx_dirty = true;
        // The streams of neighbouring slots get different priorities.  HIP deals a process's streams of one priority onto a small
        // pool of hardware queues in creation order (GPU_MAX_HW_QUEUES, default 4), and two streams that land on one queue run
        // strictly one after the other: with other streams alive in the process (a ROS node has them) the two slots of a stream
        // of scans could end up sharing a queue and lose the overlap of one's preparation with the other's loop.  Streams of
        // different priority never share a hardware queue, whatever else the process has created.
        hipStream_t st = nullptr;
        hipEvent_t ev = nullptr, ev2 = nullptr;
        if (create_stream(h, &st, !(slot & 1), "a scan slot's stream") != S2M_OK || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev2, hipEventDisableTiming) != hipSuccess) {
            if (ev) (void)hipEventDestroy(ev);
            if (st) (void)hipStreamDestroy(st);
            (void)s2m_destroy(k);
            return fail(h, S2M_ERR_HIP, "batch: stream / event creation failed");
        }
        h->batch.kids.push_back(k);
        h->batch.branch_streams.push_back(st);
        h->batch.branch_events.push_back(ev);
        h->batch.prep_events.push_back(ev2);
        h->batch.prep_pending.push_back(0);
    }
    if (!h->batch.ev_fork && hipEventCreateWithFlags(&h->batch.ev_fork, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    if (!h->batch.ev_prep && hipEventCreateWithFlags(&h->batch.ev_prep, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    return S2M_OK;
}

// One graph for the whole batch in flight (h->batch.live).  Lockstep (default): the slots' loops advance together, every launch
// of the loop has one grid row per slot (slots of different workgroup shape form groups, one loop per group on a branch of its
// own).  Otherwise (S2M_LOCKSTEP=0, A/B measurements): a fork, one branch per scan with that scan's loop, a join.
// part 0: the whole loop; 1: launches 0 .. seg-1; 2: launches seg .. max_iter-1 (as a single scan's graph)
int get_batch_graph(s2m_context* h, int part, const s2m_context::Batch::Graph** out)
{
    const std::vector<int>& live = h->batch.live;
    std::vector<int> key;
    key.push_back(part); key.push_back(part ? h->tune.seg_iters : 0);
    for (int b : live) { key.push_back(b); key.push_back(h->batch.kids[(size_t)b]->hctx.table_cap); key.push_back(h->batch.kids[(size_t)b]->hctx.wpb); }
    auto it = h->batch.graphs.find(key);
    if (it != h->batch.graphs.end()) { h->batch.last.graph_hits++; *out = &it->second; return S2M_OK; }
    h->batch.last.graph_captures++;
    std::vector<LoopIssued> issued;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // the loops to run: (shape, stream to run it on)
    std::vector<LoopShape> loops;
    if (h->tune.lockstep) {
        for (int wpb : { kBlock / 64, kBigWaves }) {
            LoopShape sh;
            memset(&sh.tbl, 0, sizeof(sh.tbl));
            sh.nslots = 0; sh.wpb = wpb; sh.batch = true;
            for (int b : live) {
                s2m_context* k = h->batch.kids[(size_t)b];
                if (k->hctx.wpb != wpb) continue;
                sh.tbl.ctx[sh.nslots] = k->reg.dctx.as<DevCtx>();
                sh.tbl.st[sh.nslots] = k->reg.state.as<DevState>();
                sh.nslots++;
                sh.nblocks = std::max(sh.nblocks, k->hctx.nblocks);
                sh.table_cap = std::max(sh.table_cap, k->hctx.table_cap);
            }
            sh.split = h->tune.split_mode == 1;         // (default: decided in enqueue_loop - split where the loop is not fused)
            sh.split_auto = h->tune.split_mode == 2 || h->tune.split_mode < 0;   // (default: certify (lean) + search from launch split_from on, where k_finalize closes the iterations)
            if (sh.nslots) loops.push_back(sh);
        }
    } else
        for (int b : live) loops.push_back(shape_of(h->batch.kids[(size_t)b]));
    S2M_HIP(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    bool ok = hipEventRecord(h->batch.ev_fork, h->stream) == hipSuccess;
    for (size_t j = 0; j < loops.size(); j++) {
        hipStream_t br = h->batch.branch_streams[j];
        ok = ok && hipStreamWaitEvent(br, h->batch.ev_fork, 0) == hipSuccess;
        {
            OnStream on(h, br);                               // (enqueue_loop launches on the handle's stream; settings are the parent's)
            enqueue_loop(h, loops[j], nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
            issued.push_back(h->reg.last_loop);
        }
        ok = ok && hipEventRecord(h->batch.branch_events[j], br) == hipSuccess;
        ok = ok && hipStreamWaitEvent(h->stream, h->batch.branch_events[j], 0) == hipSuccess;
    }
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (!ok || e != hipSuccess || !graph) return fail(h, S2M_ERR_HIP, "batch: stream capture failed", e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: hipGraphInstantiate", e);
    s2m_context::Batch::Graph& g = h->batch.graphs[key];
    g.exec = exec; g.loops = std::move(issued);
    *out = &g;
    return S2M_OK;
}

// range `part` of the batch in flight on the handle's stream, and state + trace of every slot up to the last live one back in one
// copy (the slots' blocks are contiguous)
int launch_batch_graph(s2m_context* h, int part)
{
    const s2m_context::Batch::Graph* g = nullptr;
    const int rc = get_batch_graph(h, part, &g);
    if (rc) return rc;
    S2M_HIP(h, hipGraphLaunch(g->exec, h->stream));
    // (s2m_debug_batch_last: the loops of this range as enqueue_loop noted them; a second range adds its certify + search launch)
    s2m_context::Batch::Last& last = h->batch.last;
    last.n_loops = (int)g->loops.size();
    for (size_t j = 0; j < g->loops.size() && j < 2; j++) {
        const int split_before = last.ranges_issued ? last.loop[j].first_split : -1;
        last.loop[j] = g->loops[j];
        if (split_before >= 0) last.loop[j].first_split = split_before;
    }
    last.ranges_issued++;
    return S2M_OK;
}
int fetch_slot_states(s2m_context* h)
{
    const size_t upto = (size_t)h->batch.live.back() + 1;
    S2M_HIP(h, hipMemcpyAsync(h->batch.h_kid_states + sizeof(DevState), h->batch.kid_states.p, kSlotStateStride * upto, hipMemcpyDeviceToHost, h->stream));
    return S2M_OK;
}

}  // namespace

extern "C" {

int s2m_batch_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device)
{
    if (!h || slot < 0 || slot >= kMaxSlots) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure_kids(h, slot + 1);
    if (rc) return rc;
    s2m_context* k = h->batch.kids[(size_t)slot];
    if ((rc = adopt_map(h, k))) return fail(h, rc, k->err.c_str());
    // The ordering of one slot's scan does not depend on the others': it runs on the slot's own stream, behind everything
    // issued on the handle's stream so far (the previous batch read the slot's buffers), and the batch launch waits for it.
    hipStream_t br = h->batch.branch_streams[(size_t)slot];
    S2M_HIP(h, hipEventRecord(h->batch.ev_prep, h->stream));
    S2M_HIP(h, hipStreamWaitEvent(br, h->batch.ev_prep, 0));
    {
        OnStream on(k, br);
        rc = set_scan_impl(k, pts, n, stride_bytes, on_device != 0);
    }
    if (rc) { (void)hipStreamSynchronize(br); return fail(h, rc, k->err.c_str()); }
    S2M_HIP(h, hipEventRecord(h->batch.prep_events[(size_t)slot], br));
    h->batch.prep_pending[(size_t)slot] = 1;
    return S2M_OK;
}

int s2m_batch_set_scans(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes, int on_device)
{
    if (!h || n_scans < 1 || n_scans > kMaxSlots || !scans || !sizes) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure_kids(h, n_scans);
    if (rc) return rc;
    // Work still queued on a slot's own stream (a preparation from s2m_batch_set_scan, a loop from s2m_slot_optimize_launch)
    // uses the buffers this call rewrites: the handle's stream waits for it first.
    for (int b = 0; b < n_scans; b++) {
        S2M_HIP(h, hipEventRecord(h->batch.prep_events[(size_t)b], h->batch.branch_streams[(size_t)b]));
        S2M_HIP(h, hipStreamWaitEvent(h->stream, h->batch.prep_events[(size_t)b], 0));
        h->batch.prep_pending[(size_t)b] = 0;
    }
    h->batch.last.prep_launches = 0;
    for (int b0 = 0; b0 < n_scans; b0 += kPrepSlots) {
        PrepTable t;
        const int nb = std::min(kPrepSlots, n_scans - b0);
        for (int j = 0; j < nb; j++) {
            s2m_context* k = h->batch.kids[(size_t)(b0 + j)];
            if ((rc = adopt_map(h, k)) == S2M_OK) rc = scan_slot_prepare(k, scans[b0 + j], sizes[b0 + j], stride_bytes, on_device != 0, &t.s[j]);
            if (rc) {
                // no slot of this call holds a scan after a failure: the groups before this one were ordered, but a batch
                // of which some scans are missing is of no use to the caller
                for (int q = 0; q <= b0 + j; q++) h->batch.kids[(size_t)q]->reg.have_scan = false;
                (void)hipStreamSynchronize(h->stream);
                return fail(h, rc, k->err.c_str());
            }
            k->reg.t_set_scan_ms = 0; k->reg.scan_timing_pending = false;
        }
        launch_scan_prep(h->stream, t, nb, false, &h->batch.last.prep_launches);
        S2M_HIP(h, hipGetLastError());
    }
    if (!on_device) S2M_HIP(h, hipStreamSynchronize(h->stream));       // the callers' buffers are free again
    return S2M_OK;
}

// ---- a stream of scans: slot k's preparation and loop run on slot k's own stream, so that the ordering of scan i+1 (slot B)
// overlaps the LM loop of scan i (slot A) - the reference does the two strictly one after the other (:257-265) ----------
int s2m_slot_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device)
{ return s2m_batch_set_scan(h, slot, pts, n, stride_bytes, on_device); }

int s2m_slot_optimize_launch(s2m_handle h, int slot, const float pose[6])
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size() || !pose) return S2M_ERR_INVALID_ARG;
    s2m_context* k = h->batch.kids[(size_t)slot];
    if (h->batch.pend_n) return fail(h, S2M_ERR_INVALID_ARG, "a batch launch is pending: collect it first");
    if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_slot_set_scan has not been called for this slot");
    S2M_HIP(h, hipSetDevice(h->device));
    OnStream on(k, h->batch.branch_streams[(size_t)slot]);
    int rc = sync_slot(h, k);
    if (rc) return rc;
    h->batch.prep_pending[(size_t)slot] = 0;                       // (the preparation is ahead of the loop on the same stream)
    rc = optimize_launch(k, pose, Reg::kSlot);
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_slot_optimize_collect(s2m_handle h, int slot, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size() || !pose) return S2M_ERR_INVALID_ARG;
    s2m_context* k = h->batch.kids[(size_t)slot];
    if (k->reg.pending != Reg::kSlot) return fail(h, S2M_ERR_INVALID_ARG, "no slot launch pending on this slot");
    OnStream on(k, h->batch.branch_streams[(size_t)slot]);
    const int rc = s2m_optimize_collect(k, pose, imu, out);
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_optimize_batch_launch(s2m_handle h, int n_scans, const float* poses)
{
    if (!h || n_scans < 1 || n_scans > kMaxSlots || !poses) return S2M_ERR_INVALID_ARG;
    if ((int)h->batch.kids.size() < n_scans) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
    if (h->batch.pend_n) return fail(h, S2M_ERR_INVALID_ARG, "a batch launch is pending: collect it first");
    for (int b = 0; b < n_scans; b++) {
        const s2m_context* k = h->batch.kids[(size_t)b];
        if (k->reg.pending != Reg::kNone) return fail(h, S2M_ERR_INVALID_ARG, "a slot launch is pending on a slot of the batch: collect it first");
        if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
    }
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    for (size_t b = 0; b < h->batch.prep_pending.size(); b++)
        if (h->batch.prep_pending[b]) { S2M_HIP(h, hipStreamWaitEvent(h->stream, h->batch.prep_events[b], 0)); h->batch.prep_pending[b] = 0; }
    for (int b = 0; b < n_scans; b++)
        if ((rc = sync_slot(h, h->batch.kids[(size_t)b]))) return rc;
    // nothing refuses from here on: the batch and its slots are pending, and a failure below un-marks them
    PendingGuard undo(h, n_scans);
    std::vector<int>& live = h->batch.live;
    h->batch.pend_n = n_scans;
    s2m_context::Batch::Last& last = h->batch.last;
    const int prep_launches = last.prep_launches;          // (of the s2m_batch_set_scans before this launch)
    last = s2m_context::Batch::Last();
    last.prep_launches = prep_launches;
    last.n_scans = n_scans;
    live.clear();
    for (int b = 0; b < n_scans; b++) {
        s2m_context* k = h->batch.kids[(size_t)b];
        k->reg.pending = Reg::kBatch;
        if (optimize_gate(k, poses + 6 * (size_t)b)) { live.push_back(b); last.n_live++; }
    }
    {   // DevCtx blocks that changed and the loop state every live slot starts from: one launch per kCtxSlots / kInitSlots slots
        CtxTable ct; int nc = 0;
        for (int b = 0; b < n_scans; b++) {
            s2m_context* k = h->batch.kids[(size_t)b];
            if (!k->ctx_dirty) continue;
            ct.dst[nc] = k->reg.dctx.as<DevCtx>(); ct.v[nc] = k->hctx;
            k->ctx_dirty = false;
            if (++nc == kCtxSlots) { launch_set_ctxs(h->stream, ct, nc, &last.ctx_launches); nc = 0; }
        }
        if (nc) launch_set_ctxs(h->stream, ct, nc, &last.ctx_launches);
        StateInitTable it; int ni = 0;
        for (int b : live) {
            s2m_context* k = h->batch.kids[(size_t)b];
            DevState s0;
            fill_state(k, &s0, poses + 6 * (size_t)b);
            StateInit& si = it.s[ni];
            si.dst = k->reg.state.as<DevState>(); si.n_waves = k->reg.n_waves.as<int32_t>();
            memcpy(si.pose, s0.pose, sizeof(si.pose)); memcpy(si.T, s0.T, sizeof(si.T)); memcpy(si.sc, s0.sc, sizeof(si.sc));
            memcpy(si.matP, s0.matP, sizeof(si.matP)); si.isDegenerate = s0.isDegenerate;
            if (++ni == kInitSlots) { launch_init_states(h->stream, it, ni, &last.init_launches); ni = 0; }
        }
        if (ni) launch_init_states(h->stream, it, ni, &last.init_launches);
        S2M_HIP(h, hipGetLastError());
    }
    // With early exit on the loops are issued as launches 0 .. seg-1 and, only if some slot has not converged by then, the rest
    // (s2m_optimize_batch_collect looks at the slots' `done` flags, which come back with the states anyway): the launches behind
    // the convergence of every slot - idle, but a kernel boundary and a k_finalize each - were a fifth of an early-exit batch.
    h->batch.seg_pending = two_ranges(h);
    S2M_HIP(h, hipEventRecord(h->reg.ev_a, h->stream));
    if (!live.empty() && (rc = launch_batch_graph(h, h->batch.seg_pending ? 1 : 0))) return rc;
    S2M_HIP(h, hipEventRecord(h->reg.ev_b, h->stream));
    for (int b : live) h->batch.kids[(size_t)b]->hctx.density_pending = 0;
    if (!live.empty() && (rc = fetch_slot_states(h))) return rc;
    undo.release();
    return S2M_OK;
}

int s2m_optimize_batch_collect(s2m_handle h, int n_scans, float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || !poses) return S2M_ERR_INVALID_ARG;
    if (!h->batch.pend_n) return fail(h, S2M_ERR_INVALID_ARG, "no batch launch pending");
    if (n_scans != h->batch.pend_n) return fail(h, S2M_ERR_INVALID_ARG, "n_scans differs from the pending batch launch's");
    PendingGuard done(h, n_scans);
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    S2M_HIP(h, hipEventElapsedTime(&h->reg.t_optimize_ms, h->reg.ev_a, h->reg.ev_b));
    bool all_done = true;
    for (int b : h->batch.live) all_done = all_done && h->batch.kids[(size_t)b]->reg.h_state[1].done != 0;
    if (h->batch.seg_pending && !all_done) {
        // some slot needs more than the first range: the rest of the loop for all of them (a converged slot's launches return at once)
        const int rc = second_range(h, [&] { const int rc2 = launch_batch_graph(h, 2); return rc2 ? rc2 : fetch_slot_states(h); });
        if (rc) return rc;
    }
    for (int b : h->batch.live) h->batch.kids[(size_t)b]->reg.t_optimize_ms = h->reg.t_optimize_ms;      // the batch was timed as a whole
    for (int b = 0; b < n_scans; b++)
        collect_record(h->batch.kids[(size_t)b], poses + 6 * (size_t)b, imu ? imu + b : nullptr, out ? out + b : nullptr);
    return S2M_OK;
}

int s2m_optimize_batch(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes,
                       float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || n_scans > kMaxSlots || !scans || !sizes || !poses) return S2M_ERR_INVALID_ARG;
    int rc = s2m_batch_set_scans(h, n_scans, scans, sizes, stride_bytes, 0);
    if (rc) return rc;
    rc = s2m_optimize_batch_launch(h, n_scans, poses);
    if (rc) return rc;
    return s2m_optimize_batch_collect(h, n_scans, poses, imu, out);
}

int s2m_batch_get_trace(s2m_handle h, int slot, s2m_iter_trace* out, int cap)
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size()) return S2M_ERR_INVALID_ARG;
    return s2m_get_trace(h->batch.kids[(size_t)slot], out, cap);
}

}  // extern "C"
