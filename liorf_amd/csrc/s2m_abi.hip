// s2m_abi.hip — host side of the gfx950 scan-to-map LM loop and the part of the C ABI (include/liorf_s2m.h) that launches its
// kernels: create / destroy / params, the context and state uploads, the loop and its graphs, launch / collect, batches and
// slots.  The only translation unit that includes s2m_kernels.hpp / s2m_register.hpp.
//
// Runs the whole <= max_iter LM loop as one captured hipGraph (enqueue_loop) so that a scan costs one graph launch and one
// synchronisation.  The map index and the scan preparation in front of it are s2m_prep.hip's, the observation and timing hooks
// s2m_abi_debug.hip's (they launch the loop's kernels through the functions s2m_context.hpp declares for this unit),
// ScanContext s2m_sc.hip's and s2m_abi_sc.hip's.  The handle is s2m_context.hpp's; the entry points that only orchestrate
// other units' stages live in s2m_abi_voxel.hip, s2m_abi_keyframes.hip, s2m_abi_loop.hip and s2m_abi_front_end.hip.  There is
// no CPU fallback: without a gfx950 device every entry point fails with S2M_ERR_NO_DEVICE.
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
    sh.batch = h->batch.parent != nullptr && !h->batch.slot_mode;
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
    // The first range is timed by device stamps: its start by the state upload before it (s2m_optimize_launch), its end by the
    // k_finalize that closes it.  The second range, issued only for a scan that did not converge in the first, keeps an event pair.
    if (h->tune.use_graph) {
        hipGraphExec_t exec = nullptr;
        int rc = get_graph(h, nblocks, part, &exec);
        if (rc == S2M_OK) {
            if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
            S2M_HIP(h, hipGraphLaunch(exec, h->stream));
            if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
            h->hctx.density_pending = 0;                  // cleared on the device by k_chunk_table_density: keep the host copy in step
            return S2M_OK;
        }
        h->tune.use_graph = false;       // capture unsupported here: fall back to plain launches
    }
    LoopShape sh = shape_of(h);
    sh.stamp = part == 2 ? nullptr : h->reg.h_stamps + kStampLoop1;
    sh.wishes_done = h->batch.parent == nullptr;
    if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
    enqueue_loop(h, sh, nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
    S2M_HIP(h, hipGetLastError());
    if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
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
    static_assert((sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter) % 64 == 0, "a batch's state blocks (kid_states) all start on a 64-byte line");
    if (hipHostMalloc((void**)&h->reg.h_state, sizeof(DevState) * 2 + sizeof(s2m_iter_trace) * kMaxIter) != hipSuccess) return bail(S2M_ERR_HIP);
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
    if (ensure(h, h->reg.state, sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter) ||      // loop state, then the trace
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
    for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second);
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
    for (void* p : { (void*)h->batch.h_kid_states, (void*)h->reg.h_state, (void*)h->reg.h_mm, (void*)h->reg.h_stamps, (void*)h->sc.h_stage, (void*)h->proj.h_count,
                     (void*)h->pg.h_sc })
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
    if (h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (p->max_iter != h->prm.max_iter) {               // the captured loops hold max_iter launches
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (auto& kv : h->reg.graphs) (void)hipGraphExecDestroy(kv.second);
        h->reg.graphs.clear();
        for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second);     // (every branch of a batch graph is such a loop)
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
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    memcpy(h->reg.pending_pose_in, pose, 24);
    h->reg.opt_pending = true;
    h->reg.pending_skipped = 0;
    if (h->reg.n_m == 0) { h->reg.pending_skipped = 1; return S2M_OK; }                    // :1297
    if ((int)h->reg.n_q <= h->prm.min_feats) { h->reg.pending_skipped = 2; return S2M_OK; } // :1300
    int rc;
    if (!h->batch.parent && h->hctx.density_pending && h->tune.density_raw > 0) {
        // the first optimisation of a single scan: the density wishes, the DevCtx block and the loop state in one plain launch
        // (k_wave_density_state needs no wave table; the graph behind it starts with k_chunk_table_density)
        launch_density_state(h, pose, h->reg.h_stamps + kStampLoop0);
        S2M_HIP(h, hipGetLastError());
        h->ctx_dirty = false;
        h->reg.table_stale = false;                       // k_chunk_table_density emits the table
    } else if ((rc = push_state(h, pose, h->reg.h_stamps + kStampLoop0))) return rc;      // (with the DevCtx block when that changed)
    h->reg.seg_pending = h->prm.early_exit && h->tune.seg_iters > 1 && h->tune.seg_iters < h->prm.max_iter;
    if ((rc = launch_loop(h, h->reg.seg_pending ? 1 : 0))) return rc;        // (state + trace come back with it)
    return S2M_OK;
}

int s2m_optimize_collect(s2m_handle h, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "no optimize launch pending");
    h->reg.opt_pending = false;
    s2m_result r;
    memset(&r, 0, sizeof(r));
    r.skipped = h->reg.pending_skipped;
    h->reg.last_trace_n = 0;
    float t[6];
    memcpy(t, h->reg.pending_pose_in, 24);
    if (!r.skipped) {
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        if (h->batch.parent && !h->batch.slot_mode) h->reg.t_optimize_ms = h->batch.parent->reg.t_optimize_ms;      // a slot of a batch: the batch was timed as a whole
        else h->reg.t_optimize_ms = stamps_ms(h, kStampLoop0, kStampLoop1);
        if (h->reg.seg_pending && !h->reg.h_state[1].done) {
            // the first range did not converge: the rest of the loop
            int rc2 = launch_loop(h, 2);
            if (rc2) return rc2;
            S2M_HIP(h, hipStreamSynchronize(h->stream));
            float t2 = 0.0f;
            S2M_HIP(h, hipEventElapsedTime(&t2, h->reg.ev_a2, h->reg.ev_b2));
            h->reg.t_optimize_ms += t2;
        }
        h->reg.seg_pending = false;
        const DevState& s = h->reg.h_state[1];
        memcpy(t, s.pose, 24);
        r.iters_run = s.iters_run; r.converged = s.converged; r.is_degenerate = s.isDegenerate;
        r.n_sel_last = s.n_sel_last;
        h->reg.persist_degenerate = s.isDegenerate;
        memcpy(h->reg.persist_matP, s.matP, sizeof(s.matP));
        // trace: executed iterations; a loop that stalled at iteration k (fewer than min_corr correspondences,
        // pose unchanged, :1178-1180) repeats that no-op record for the iterations the reference would still run
        int n_exec = s.iters_run, stall_at = -1;
        for (int i = 0; i < n_exec && i < kMaxIter; i++) {
            if (stall_at >= 0) { h->reg.last_trace[i] = h->reg.last_trace[stall_at]; continue; }
            h->reg.last_trace[i] = h->reg.h_trace[i];
            if (s.stalled && !h->reg.h_trace[i].stepped) stall_at = i;
        }
        h->reg.last_trace_n = n_exec < kMaxIter ? n_exec : kMaxIter;
        host_transform_update(h->prm, imu, t, r.affine);                           // :1317
    } else {
        host_pose_to_transform(t, r.affine, nullptr);
        r.is_degenerate = h->reg.persist_degenerate;
    }
    memcpy(r.pose, t, 24);
    memcpy(pose, t, 24);
    if (out) *out = r;
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

// ---- a batch of scans against one resident map -------------------------------------------------------
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

int ensure_kids(s2m_context* h, int n)
{
    while ((int)h->batch.kids.size() < n) {
        s2m_params p = h->prm;
        p.stream = h->stream;                              // everything outside the captured graph is ordered on the parent's stream
        s2m_context* k = nullptr;
        const int rc = s2m_create(&p, &k);
        if (rc) return fail(h, rc, "batch: could not create a scan slot");
        k->batch.parent = h;
        k->hctx.ablate = h->hctx.ablate;
        memcpy(k->hctx.tune, h->hctx.tune, sizeof(h->hctx.tune));
        {   // the slot's loop state and trace live in the parent's block
            constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
            if (!h->batch.kid_states.p) {
                if (ensure(h, h->batch.kid_states, kStride * kMaxSlots) != S2M_OK ||
                    hipHostMalloc((void**)&h->batch.h_kid_states, sizeof(DevState) + kStride * kMaxSlots) != hipSuccess) {
                    (void)s2m_destroy(k);
                    return fail(h, S2M_ERR_HIP, "batch: state block allocation failed");
                }
            }
            const size_t slot = h->batch.kids.size();
            (void)k->reg.state.reset();                        // from here on an alias: forgotten, not freed, in s2m_destroy
            (void)hipHostFree(k->reg.h_state);
            k->reg.state.p = h->batch.kid_states.as<unsigned char>() + kStride * slot; k->reg.state.cap = kStride;
            k->reg.h_state = reinterpret_cast<DevState*>(h->batch.h_kid_states + kStride * slot);      // [1] = the download area of this slot
            k->reg.h_trace = reinterpret_cast<s2m_iter_trace*>(k->reg.h_state + 2);
            k->batch.state_borrowed = true;
            k->hctx.state = k->reg.state.as<DevState>();
            k->hctx.trace = reinterpret_cast<s2m_iter_trace*>(k->reg.state.as<DevState>() + 1);
            k->ctx_dirty = true;
        }
        h->batch.kids.push_back(k);
        hipStream_t st = nullptr;
        hipEvent_t ev = nullptr, ev2 = nullptr;
        // The streams of neighbouring slots get different priorities.  HIP deals a process's streams of one priority onto a small
        // pool of hardware queues in creation order (GPU_MAX_HW_QUEUES, default 4), and two streams that land on one queue run
        // strictly one after the other: with other streams alive in the process (a ROS node has them) the two slots of a stream
        // of scans could end up sharing a queue and lose the overlap of one's preparation with the other's loop.  Streams of
        // different priority never share a hardware queue, whatever else the process has created.
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        const int prio = (h->batch.kids.size() & 1) ? prio_greatest : prio_least;
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev2, hipEventDisableTiming) != hipSuccess)
            return fail(h, S2M_ERR_HIP, "batch: stream / event creation failed");
        h->batch.branch_streams.push_back(st);
        h->batch.branch_events.push_back(ev);
        h->batch.prep_events.push_back(ev2);
        h->batch.prep_pending.push_back(0);
    }
    if (!h->batch.ev_fork && hipEventCreateWithFlags(&h->batch.ev_fork, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    if (!h->batch.ev_prep && hipEventCreateWithFlags(&h->batch.ev_prep, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    return S2M_OK;
}

// One graph for the whole batch.  Lockstep (default): the slots' loops advance together, every launch of the loop has one
// grid row per slot (slots of different workgroup shape form groups, one loop per group on a branch of its own).  Otherwise
// (S2M_LOCKSTEP=0, A/B measurements): a fork, one branch per scan with that scan's loop, a join.
// part 0: the whole loop; 1: launches 0 .. seg-1; 2: launches seg .. max_iter-1 (as get_graph)
int get_batch_graph(s2m_context* h, const std::vector<int>& live, int part, hipGraphExec_t* out)
{
    std::vector<int> key;
    key.push_back(part); key.push_back(part ? h->tune.seg_iters : 0);
    for (int b : live) { key.push_back(b); key.push_back(h->batch.kids[(size_t)b]->hctx.table_cap); key.push_back(h->batch.kids[(size_t)b]->hctx.wpb); }
    auto it = h->batch.graphs.find(key);
    if (it != h->batch.graphs.end()) { *out = it->second; return S2M_OK; }
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
    hipStream_t keep = h->stream;
    for (size_t j = 0; j < loops.size(); j++) {
        hipStream_t br = h->batch.branch_streams[j];
        ok = ok && hipStreamWaitEvent(br, h->batch.ev_fork, 0) == hipSuccess;
        h->stream = br;                                       // (enqueue_loop launches on the handle's stream; settings are the parent's)
        enqueue_loop(h, loops[j], nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
        h->stream = keep;
        ok = ok && hipEventRecord(h->batch.branch_events[j], br) == hipSuccess;
        ok = ok && hipStreamWaitEvent(h->stream, h->batch.branch_events[j], 0) == hipSuccess;
    }
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (!ok || e != hipSuccess || !graph) return fail(h, S2M_ERR_HIP, "batch: stream capture failed", e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: hipGraphInstantiate", e);
    h->batch.graphs[key] = exec;
    *out = exec;
    return S2M_OK;
}

}  // namespace

int s2m_batch_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device)
{
    if (!h || slot < 0 || slot >= 64) return S2M_ERR_INVALID_ARG;
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
    k->stream = br;
    rc = set_scan_impl(k, pts, n, stride_bytes, on_device != 0);
    k->stream = h->stream;
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
        launch_scan_prep(h->stream, t, nb);
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
    if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_slot_set_scan has not been called for this slot");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if (!same_params_but_stream(k->prm, h->prm)) {
        s2m_params p = h->prm;
        p.stream = k->prm.stream;
        if ((rc = s2m_set_params(k, &p))) return fail(h, rc, k->err.c_str());
    }
    h->batch.prep_pending[(size_t)slot] = 0;                       // (the preparation is ahead of the loop on the same stream)
    k->stream = h->batch.branch_streams[(size_t)slot];
    k->batch.slot_mode = true;
    rc = adopt_map(h, k);
    if (!rc) rc = s2m_optimize_launch(k, pose);
    k->stream = h->stream;
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_slot_optimize_collect(s2m_handle h, int slot, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size() || !pose) return S2M_ERR_INVALID_ARG;
    s2m_context* k = h->batch.kids[(size_t)slot];
    k->stream = h->batch.branch_streams[(size_t)slot];
    const int rc = s2m_optimize_collect(k, pose, imu, out);
    k->stream = h->stream;
    k->batch.slot_mode = false;
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_optimize_batch_launch(s2m_handle h, int n_scans, const float* poses)
{
    if (!h || n_scans < 1 || n_scans > 64 || !poses) return S2M_ERR_INVALID_ARG;
    if ((int)h->batch.kids.size() < n_scans) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
    S2M_HIP(h, hipSetDevice(h->device));
    std::vector<int> live;
    int rc;
    for (size_t b = 0; b < h->batch.prep_pending.size(); b++)
        if (h->batch.prep_pending[b]) { S2M_HIP(h, hipStreamWaitEvent(h->stream, h->batch.prep_events[b], 0)); h->batch.prep_pending[b] = 0; }
    for (int b = 0; b < n_scans; b++) {
        s2m_context* k = h->batch.kids[(size_t)b];
        if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
        if (!same_params_but_stream(k->prm, h->prm)) {     // any parameter changed on the parent since the slot was made
            s2m_params p = h->prm;
            p.stream = k->prm.stream;
            if ((rc = s2m_set_params(k, &p))) return fail(h, rc, k->err.c_str());
        }
        if ((rc = adopt_map(h, k))) return fail(h, rc, k->err.c_str());
        memcpy(k->reg.pending_pose_in, poses + 6 * (size_t)b, 24);
        k->reg.opt_pending = true;
        k->reg.pending_skipped = 0;
        if (k->reg.n_m == 0) { k->reg.pending_skipped = 1; continue; }                            // :1297
        if ((int)k->reg.n_q <= k->prm.min_feats) { k->reg.pending_skipped = 2; continue; }         // :1300
        live.push_back(b);
    }
    {   // DevCtx blocks that changed and the loop state every live slot starts from: one launch per kCtxSlots / kInitSlots slots
        CtxTable ct; int nc = 0;
        auto flush_ctx = [&]() { if (nc) { for (int j = nc; j < kCtxSlots; j++) ct.dst[j] = nullptr; hipLaunchKernelGGL(k_set_ctxs, dim3(nc), dim3(64), 0, h->stream, ct); nc = 0; } };
        for (int b = 0; b < n_scans; b++) {
            s2m_context* k = h->batch.kids[(size_t)b];
            if (!k->ctx_dirty) continue;
            ct.dst[nc] = k->reg.dctx.as<DevCtx>(); ct.v[nc] = k->hctx; nc++;
            k->ctx_dirty = false;
            if (nc == kCtxSlots) flush_ctx();
        }
        flush_ctx();
        StateInitTable it; int ni = 0;
        auto flush_init = [&]() { if (ni) { for (int j = ni; j < kInitSlots; j++) it.s[j].dst = nullptr; hipLaunchKernelGGL(k_init_states, dim3(ni), dim3(256), 0, h->stream, it); ni = 0; } };
        for (int b : live) {
            s2m_context* k = h->batch.kids[(size_t)b];
            DevState s0;
            fill_state(k, &s0, poses + 6 * (size_t)b);
            StateInit& si = it.s[ni++];
            si.dst = k->reg.state.as<DevState>(); si.n_waves = k->reg.n_waves.as<int32_t>();
            memcpy(si.pose, s0.pose, sizeof(si.pose)); memcpy(si.T, s0.T, sizeof(si.T)); memcpy(si.sc, s0.sc, sizeof(si.sc));
            memcpy(si.matP, s0.matP, sizeof(si.matP)); si.isDegenerate = s0.isDegenerate;
            if (ni == kInitSlots) flush_init();
        }
        flush_init();
        S2M_HIP(h, hipGetLastError());
    }
    // With early exit on the loops are issued as launches 0 .. seg-1 and, only if some slot has not converged by then, the rest
    // (s2m_optimize_batch_collect looks at the slots' `done` flags, which come back with the states anyway): the launches behind
    // the convergence of every slot - idle, but a kernel boundary and a k_finalize each - were a fifth of an early-exit batch.
    h->batch.seg_pending = h->prm.early_exit && h->tune.seg_iters > 1 && h->tune.seg_iters < h->prm.max_iter;
    h->batch.live = live;
    S2M_HIP(h, hipEventRecord(h->reg.ev_a, h->stream));
    if (!live.empty()) {
        hipGraphExec_t exec = nullptr;
        if ((rc = get_batch_graph(h, live, h->batch.seg_pending ? 1 : 0, &exec))) return rc;
        S2M_HIP(h, hipGraphLaunch(exec, h->stream));
    }
    S2M_HIP(h, hipEventRecord(h->reg.ev_b, h->stream));
    for (int b : live) h->batch.kids[(size_t)b]->hctx.density_pending = 0;
    if (!live.empty()) {
        // state + trace of every slot up to the last live one, in one copy (the slots' blocks are contiguous)
        constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
        const size_t upto = (size_t)live.back() + 1;
        S2M_HIP(h, hipMemcpyAsync(h->batch.h_kid_states + sizeof(DevState), h->batch.kid_states.p, kStride * upto, hipMemcpyDeviceToHost, h->stream));
    }
    return S2M_OK;
}

int s2m_optimize_batch_collect(s2m_handle h, int n_scans, float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || (int)h->batch.kids.size() < n_scans || !poses) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    S2M_HIP(h, hipEventElapsedTime(&h->reg.t_optimize_ms, h->reg.ev_a, h->reg.ev_b));
    if (h->batch.seg_pending && !h->batch.live.empty()) {
        h->batch.seg_pending = false;
        bool all_done = true;
        for (int b : h->batch.live) all_done = all_done && h->batch.kids[(size_t)b]->reg.h_state[1].done != 0;
        if (!all_done) {
            // some slot needs more than the first range: the rest of the loop for all of them (a converged slot's launches return at once)
            hipGraphExec_t exec = nullptr;
            int rc2 = get_batch_graph(h, h->batch.live, 2, &exec);
            if (rc2) return rc2;
            S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
            S2M_HIP(h, hipGraphLaunch(exec, h->stream));
            S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
            constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
            const size_t upto = (size_t)h->batch.live.back() + 1;
            S2M_HIP(h, hipMemcpyAsync(h->batch.h_kid_states + sizeof(DevState), h->batch.kid_states.p, kStride * upto, hipMemcpyDeviceToHost, h->stream));
            S2M_HIP(h, hipStreamSynchronize(h->stream));
            float t2 = 0.0f;
            S2M_HIP(h, hipEventElapsedTime(&t2, h->reg.ev_a2, h->reg.ev_b2));
            h->reg.t_optimize_ms += t2;
        }
    }
    for (int b = 0; b < n_scans; b++) {
        s2m_context* k = h->batch.kids[(size_t)b];
        const int rc = s2m_optimize_collect(k, poses + 6 * (size_t)b, imu ? imu + b : nullptr, out ? out + b : nullptr);
        if (rc) return fail(h, rc, k->err.c_str());
    }
    return S2M_OK;
}

int s2m_optimize_batch(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes,
                       float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || n_scans > 64 || !scans || !sizes || !poses) return S2M_ERR_INVALID_ARG;
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
