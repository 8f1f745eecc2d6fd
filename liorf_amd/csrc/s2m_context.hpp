// s2m_context.hpp — the handle behind the C ABI (struct s2m_context) and the host helpers that more than one stage uses.
// Internal: included by the s2m_abi*.hip translation units, s2m_prep.hip and s2m_sc.hip only, never installed, and nothing declared
// here leaves the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "s2m_types.h"
#include "s2m_host_math.hpp"
#include "s2m_voxel.hpp"
#include "s2m_icp.hpp"
#include "s2m_project.hpp"
#include "s2m_pose_graph.hpp"

namespace s2m {
namespace host __attribute__((visibility("hidden"))) {

// A device allocation and its one owner: declaring a DevBuf member is all a new buffer needs, the destructor frees it.
// A DevBuf that points into memory it does not own (a slot's `state`) is made to forget() it before it goes.
struct DevBuf {
    void*  p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)reset(); }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    // frees what is held and takes q (cap bytes) instead; the old memory is dropped whatever hipFree says, never freed twice
    hipError_t reset(void* q = nullptr, size_t bytes = 0)
    {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = q; cap = bytes;
        return e;
    }
    void forget() { p = nullptr; cap = 0; }
};

constexpr size_t kDsStride = 32;       // filtered clouds are kept as pcl::PointXYZI records

// s2m_context::Registration::h_stamps: k_polar_count starts, k_chunk_parts ends (consecutive: PrepSlot::stamps), the state
// upload of s2m_optimize_launch ends, the k_finalize that closes the loop's (first) range ends
enum { kStampPrep0 = 0, kStampPrep1 = 1, kStampLoop0 = 2, kStampLoop1 = 3, kStampCount = 4 };

// What enqueue_loop issued, noted as it decided it: the grid (nblocks x nslots workgroups of wpb waves), whether the iterations
// close inside the registration kernel (fused) or by k_finalize, and the first launch that ran certify + search (-1: none)
struct LoopIssued { int wpb = 0, nslots = 0, nblocks = 0, fused = 0, first_split = -1; };

}  // namespace host
}  // namespace s2m

struct __attribute__((visibility("hidden"))) s2m_context {
    using DevBuf = s2m::host::DevBuf;

    s2m_params prm{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    s2m::DevCtx hctx{};                // host copy of the DevCtx block; ctx_dirty: it has to go to the device before the next launch
    bool ctx_dirty = true;

    // registration: the map index, the ordered scan, the LM loop's state and its captured graphs
    struct Registration {
        // map side
        DevBuf raw_map, map_sorted, m_counts, m_cell_start, m_cell_of, m_rank_of;
        // scan side
        DevBuf raw_scan, qx, qy, qz, qperm, npos, front, cert, aux, plane_cache, plane_alt, npos_alt, chunk_parts, chunk_factor, wave_table, n_waves, q_counts, q_cell_start, q_cell_of, q_rank_of, q_block_hist;
        // shared: scan scratch, partial rows + worklist, loop state + trace, the DevCtx block, bounding box, the debug outputs
        DevBuf block_sums, partials, state, dctx, mm, dbg_idx5, dbg_d2, dbg_flag, dbg_coeff, dbg_clk;
        size_t n_m = 0, n_q = 0;
        bool have_scan = false;

        // pinned host staging
        s2m::DevState* h_state = nullptr;  // [2]: [0] upload, [1] download
        s2m_iter_trace* h_trace = nullptr; // [kMaxIter], directly behind h_state[1]: state and trace come back in one copy
        uint32_t* h_mm = nullptr;          // [6]
        // [kStampCount] wall_clock64() values the kernels that bracket a single scan's preparation and its loop leave behind
        // (device-visible: the kernels store them directly), and the counter's rate
        unsigned long long* h_stamps = nullptr;
        int wall_clock_khz = 0;

        // state that persists across scans in the reference node (:139-140)
        int persist_degenerate = 0;
        float persist_matP[36] = { 0 };

        std::map<long long, hipGraphExec_t> graphs;
        s2m::host::LoopIssued last_loop;   // of the last enqueue_loop on this context (a batch keeps them with its graphs)
        std::vector<hipEvent_t> iter_events;
        hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr, ev_up = nullptr;
        hipEvent_t ev_a2 = nullptr, ev_b2 = nullptr;     // around the second range of launches
        float t_optimize_ms = 0, t_set_map_ms = 0, t_set_scan_ms = 0;
        int base_parts = 1;
        // The one pending optimise of this context: what a launch queued and no collect has brought back yet. kSingle: the
        // handle's own loop (s2m_optimize_launch). A slot is pending as kSlot - a loop of its own on its own stream
        // (s2m_slot_optimize_launch) - or as kBatch, a row of the parent's batch; the parent records that batch in Batch::pend_n,
        // live and seg_pending. The rules, for every launch and collect:
        //  - A launch marks a context pending only after everything that can refuse has passed (arguments, have_scan, the
        //    parameter sync and adopt_map, for every slot of the call): a refused call marks nothing. A call that fails after
        //    marking (capture, graph launch, a HIP error) un-marks what it marked before it returns.
        //  - A collect clears what it collects on every exit (PendingGuard): pending and seg_pending, and for a batch the
        //    parent's record and every slot of that batch.
        //  - s2m_optimize_launch twice without a collect stays allowed: the collect brings back the most recent launch.
        //  - A batch and a slot's own loop do not cross: no batch launch over a slot pending as kSlot or under a pending batch, no
        //    slot launch under a pending batch, and no s2m_set_params on a parent while one of its slots is pending.
        enum Pending { kNone, kSingle, kSlot, kBatch } pending = kNone;
        bool seg_pending = false;          // the launch in flight was the first range only
        bool scan_timing_pending = false;
        s2m::PrepSlot prep_slot{};         // the resident scan's row of the ordering kernels' table (s2m_debug_scan_prep runs them again)
        bool table_stale = false;          // a single scan is resident whose extent-only wave table has not been built (ensure_wave_table)
        int pending_skipped = 0;
        float pending_pose_in[6] = { 0 };
        s2m_iter_trace last_trace[s2m::kMaxIter];
        int last_trace_n = 0;
    } reg;

    // batch of scans against this handle's map (s2m_optimize_batch): one child context per scan slot.  A child owns its scan-side
    // buffers and DevCtx block, borrows the parent's map index, keeps its loop state and trace in the parent's block (kid_states)
    // and runs on the parent's stream; inside the captured batch graph the slots advance in lockstep, one grid row each, or
    // (S2M_LOCKSTEP=0) every child's loop is a branch of its own.
    struct Batch {
        s2m_context* parent = nullptr;
        std::vector<s2m_context*> kids;
        std::vector<hipStream_t> branch_streams;
        std::vector<hipEvent_t> branch_events;
        std::vector<hipEvent_t> prep_events;  // a slot's scan preparation runs on the slot's branch stream, next to the other slots': done when this fires
        std::vector<char> prep_pending;
        hipEvent_t ev_fork = nullptr, ev_prep = nullptr;
        // loop state + trace of every slot in one block (device) with a pinned mirror: one copy brings all of a batch's results back
        DevBuf kid_states;
        unsigned char* h_kid_states = nullptr;
        bool state_borrowed = false;       // (a slot: `reg.state` and `reg.h_state` point into the parent's blocks)
        struct Graph { hipGraphExec_t exec = nullptr; std::vector<s2m::host::LoopIssued> loops; };   // (loops: what enqueue_loop noted at the capture)
        std::map<std::vector<int>, Graph> graphs;
        // What the last s2m_batch_set_scans (prep_launches) and the last batch launch / collect issued, each count taken where
        // the launch is issued or the decision falls (s2m_debug_batch_last): observation only, nothing reads it back.
        struct Last {
            int n_scans = 0, n_live = 0;
            int ctx_launches = 0, init_launches = 0, prep_launches = 0;
            int ranges_issued = 0, graph_hits = 0, graph_captures = 0;
            int n_loops = 0;
            s2m::host::LoopIssued loop[2];
        } last;
        int pend_n = 0;                    // n_scans of the batch in flight (0: none); its slots 0 .. pend_n-1 are pending as kBatch
        std::vector<int> live;             // the slots of the batch in flight that run a loop
        bool seg_pending = false;          // the batch in flight was issued as its first range of launches only (early exit on)
        unsigned long long map_epoch = 0;  // bumped by every s2m_set_map: children re-adopt the index when it changed
        unsigned long long adopted_epoch = 0;
    } batch;

    // tuning switches, read from the environment once in s2m_create
    struct Tuning {
        bool use_graph = true;
        bool fuse_solve = true;            // env S2M_NO_FUSE=1 keeps one k_finalize per iteration (A/B measurements)
        int  fuse_max_blocks = 0;          // largest grid that closes iterations inside k_register (env S2M_FUSE_MAX overrides)
        int  seg_iters = 8;                // with early exit on, the loop is issued as launches 0..seg-1 and, only if those did not converge, the rest (env S2M_SEGMENT, 0 = one piece)
        int  split_mode = -1;              // env S2M_SPLIT: 1 = every loop runs certify + search kernels, 0 = every loop the fused kernel, 2 (and the default)
                                           // = a lockstep batch whose iterations are closed by k_finalize runs the fused kernel up to launch split_from
                                           // and k_certify_lean + the search kernel from there on; everything else the fused kernel
        bool tune_env = false;             // S2M_TUNE given (DevCtx::tune holds the caller's values)
        bool lean_certify = true;          // env S2M_LEAN=0: the certify role by the general kernel even where the 64-register one applies
        int  batch_entries = 1;            // env S2M_BATCH_ENTRIES: wave-table entries per wave in the scan slots of a batch (fewer, longer-running workgroups)
        int  batch_minw = 4;               // env S2M_BATCH_MINW=4: the search / fused kernel of batch slots in the 128-register build
        bool close_in_search = false;      // env S2M_CLOSE_IN_SEARCH=1: late split iterations without a k_finalize launch - ONE search workgroup per slot walks the
                                           // worklist and closes the iteration (1 % faster on the benchmark batch, but a slot with several deferred workgroups then
                                           // works them off one after the other: 70 us in a launch that had three)
        int  search_grid = 8;              // env S2M_SEARCH_GRID: workgroups per slot of a late search launch
        int  split_from = 8;               // env S2M_SPLIT_FROM: first launch that runs certify + search under S2M_SPLIT=2
        bool lockstep = true;              // env S2M_LOCKSTEP=0: the scans of a batch as parallel branches of the graph instead of one grid row each (A/B measurements)
        bool big_blocks = true;            // env S2M_BIG_BLOCKS=0: 8-wave workgroups whatever the scan size (A/B measurements)
        int  density_raw = 320;            // box points above which a wave asks for a finer cut (env S2M_DENSITY_RAW, 0 = off)
    } tune;

    // voxel-grid stages that feed the path (section 8(f) F1/F2): staging for host clouds, the filter's output for the host,
    // transformed key frames, and the two filtered clouds that stay resident as the registration's scan and map
    struct Voxel {
        DevBuf in, out, frames_xf, scan_ds, map_ds;
        s2m::VoxWorkspace* ws = nullptr;
        size_t scan_ds_n = 0;              // records s2m_downsample_scan left in scan_ds
        bool have_scan_ds = false;
    } voxel;

    // ScanContext (SCManager's containers, section 8(f) F3): the polar bins and descriptor + ring key of the cloud in hand, then
    // the store - descriptors, fp32 ring keys, sector keys, by key-frame index - and the candidate list of s2m_sc_distance; the place
    // query's slot (descriptor + sector key of the query) and the workgroups' lists of their best hits
    struct ScanContext {
        DevBuf bins, out;
        DevBuf store_desc, store_ring, store_sector, cand;
        DevBuf query, query_part;
        // the many-query's pass (s2m_sc_many.hpp): the queries' keys or descriptors + sector keys, their column norms, the
        // (query, tile group) lists, the rows; together at most kScManyScratchMax.  h_many: pinned, the pass's upload | rows
        DevBuf many_in, many_qnorm, many_part, many_out;
        unsigned char* h_many = nullptr;
        size_t h_many_cap = 0;
        // pass: queries per pass, 0: as many as the scratch bound allows (s2m_debug_sc_query_many_pass / s2m_debug_sc_ring_pass);
        // last_*: of the last call, its passes and the device bytes of one pass
        struct ScPassState { int pass = 0; int last_passes = 0; size_t last_scratch = 0; };
        ScPassState many;
        // the ring-key prefilter's pass (s2m_sc_ring.hpp): the queries' keys or descriptors + sector keys + fp32 ring keys, the
        // neighbour lists and their sizes, the candidates' distances and shifts, the rows; together at most kScManyScratchMax.
        // The pinned block of a pass is h_many.
        DevBuf ring_in, ring_cand, ring_dist, ring_out;
        ScPassState ring;
        size_t n = 0, cap = 0, n_search = 0;
        int    counter = 0;                // tree_making_period_conter (include/Scancontext.cpp:270-283)
        double* h_stage = nullptr;         // pinned [1200 + 20]: descriptor + ring key, or the detection's result, or the query's hits
    } sc;

    // key-frame store (cloudKeyPoses3D / cloudKeyPoses6D / surfCloudKeyFrames, :93-100): every key's 32-byte records in an arena of
    // blocks that are never moved (the frame table holds raw pointers into them), and per key its position, KfFrame (transform,
    // records, count) and time on the device; poses, times and frames mirrored on the host
    struct KeyFrames {
        DevBuf pos, frames, tdev;          // tdev: every key's time (double), read by the loop detection
        std::vector<void*> blocks;
        size_t block_used = 0, block_cap = 0, cap = 0;
        std::vector<float> pose;           // 6 per key: x, y, z, roll, pitch, yaw
        std::vector<double> time;
        std::vector<s2m::KfFrame> frame;
        KeyFrames() = default;
        KeyFrames(const KeyFrames&) = delete;
        KeyFrames& operator=(const KeyFrames&) = delete;
        ~KeyFrames() { for (void* b : blocks) (void)hipFree(b); }
    } kf;

    // loop closure: the ICP alignment (section 8(f) F4) with its staging of host clouds, and against the store loopIndexContainer
    // (:146), the transformed frames, the source submap (cur) and the target submaps: candidate 0's in prev - the only one of the
    // synchronous and the single launched closure, and where s2m_loop_near_keyframes builds - and candidates 1.. in ver_prev
    struct LoopClosure {
        s2m::IcpWorkspace* icp = nullptr;
        DevBuf icp_src, icp_tgt;
        std::map<int32_t, int32_t> index;
        DevBuf xf, cur, prev, ver_prev[S2M_LOOP_MAX_CANDIDATES - 1];
        DevBuf& target(int i) { return i == 0 ? prev : ver_prev[i - 1]; }
        // the stream a launched closure's ICP runs on (lowest priority, created at the first launch) and the event on the handle's
        // stream behind the submap writes
        hipStream_t stream = nullptr;
        hipEvent_t ev_submaps = nullptr;
        // The one pending closure: what a launch queued on the loop stream and no poll or collect has brought back yet, and the
        // family of calls that launched it - s2m_loop_*_launch (kSingle: one candidate) or s2m_loop_verify_launch (kVerify) - which
        // is the family that may poll it. Its records in the caller's order, the slot of the device loop each one runs in (-1:
        // decided at launch, it took none), and what the result needs from launch time, as the reference copies copy_cloudKeyPoses6D.
        enum Pending { kNone, kSingle, kVerify } pending = kNone;
        int32_t pend_n = 0;                // records of the pending closure
        s2m_loop_result pend_rec[S2M_LOOP_MAX_CANDIDATES]{};
        int32_t pend_slot[S2M_LOOP_MAX_CANDIDATES] = { 0 };
        float pend_pose_pre[S2M_LOOP_MAX_CANDIDATES][6] = { { 0 } };   // kf.pose[key_pre] of every candidate at launch
        float snap_T[12] = { 0 };          // kf.frame[key_cur].T at launch
        float pend_fitness = 0.0f;         // s2m_loop_params::fitness_score of the launch
        int32_t pend_base_key = -1;
        s2m::IcpTuning tune{ 0.0f, s2m::kIcpShellCap, s2m::kIcpUseGrid ? 1 : 0 };   // cell: edge in units of the leaf (s2m_debug_icp_tuning)
        // s2m_loop_verify_many: the submaps of one pass, all held at once - a source per row, a target per pair - back to back in
        // one arena: a submap is built in cur / target(i) as ever and its filtered records are copied behind the ones before
        // (many_used bytes so far). The arena grows to the largest pass it has held and is kept.
        // pairs_per_pass: s2m_debug_loop_verify_many_pass (0: kIcpMaxPairs); last_*: what the call made last did.
        DevBuf many_arena;
        size_t many_used = 0;
        int32_t many_pairs_per_pass = 0;
        int32_t many_last_passes = 0, many_last_pairs = 0;
    } loop;

    // loop detection by position for many keys (s2m_loop_detect_keys, s2m_loop_detect.hpp): buffers of its own - the pass's keys and
    // times, the (query, split) lists, the rows - together at most kScManyScratchMax, and the pinned block of a pass (upload |
    // rows).  pass: queries per pass, 0: as many as the bound allows (s2m_debug_loop_detect_pass); max_splits: a cap on the store
    // splits of a grid, 0: the plan's own (s2m_debug_loop_detect_splits); last_*: of the last call.
    struct LoopDetect {
        DevBuf in, part, out;
        unsigned char* h_pass = nullptr;
        size_t h_pass_cap = 0;
        int pass = 0, max_splits = 0, last_passes = 0;
        size_t last_scratch = 0;
    } ldet;

    // the global map and the saved map from the store: transformed frames, the filtered cloud, the chunked copy-out (frame table,
    // two staging buffers that take turns, a copy stream and its events)
    struct GlobalMap {
        DevBuf xf, out, tab, stage[2];
        hipStream_t copy_stream = nullptr;
        hipEvent_t ev_xf[2] = { nullptr, nullptr }, ev_cp[2] = { nullptr, nullptr };
    } gmap;

    // imageProjection's filter and deskew (s2m_project_scan): staging of host records, the survivor masks, the per-workgroup
    // counts, the IMU table, transStartInverse, and cloud_deskewed - the resident result the next stages read
    struct Projection {
        DevBuf in, mask, part, table, start, cloud_deskewed;
        size_t deskewed_n = 0;
        bool have_deskewed = false;
        s2m::ProjCount* h_count = nullptr; // pinned: the count, written by the device
    } proj;

    // the pose graph beside the key-frame store (saveKeyFramesAndFactor / correctPoses, :1386-1642): factors and a mirror of the
    // estimates on the host, the estimates (R, t in fp64), the linearisation, the two chain scans and the CG vectors on the device
    struct PoseGraph {
        std::vector<s2m::PgFactor> factors;        // in the order they were added
        std::vector<double> X;                     // 12 per variable: R row-major, t
        std::vector<char> has_init, dirty;         // dirty: the host value is newer than the device's
        bool dev_newer = false;                    // an accepted step: the device's estimates are newer than X
        bool topo_dirty = true;                    // factors were added since the device tables were built
        size_t n_dev = 0;                          // variables the device arrays hold
        DevBuf est, trial, chain, extra, inc_start, inc, Binv, Aof, rc, Ji, Jj, rx, ferr, fw, vecs, partial, sc, poses;
        DevBuf scan_M[2], scan_Pre[2], scan_loc[2], scan_C0[2];
        DevBuf blk_vecs, blk_loc[2], blk_partial, blk_sc, blk_rows;   // the block solve's columns (s2m_pg_marginals, s2m_pg_joint_marginal)
        s2m::PgScalars* h_sc = nullptr;            // pinned
        s2m::PgDev dev{};
        // the launched optimise (s2m_pg_optimize_launch): the stream its solve runs on (lowest priority, created at the first
        // launch), the event on the handle's stream behind the launch's uploads, the event behind the range in flight, the
        // record on the device and its pinned copy (written at the end of every range), and what the result needs from launch time
        hipStream_t stream = nullptr;
        hipEvent_t ev_ready = nullptr, ev_range = nullptr;
        DevBuf rec;
        s2m::PgRecord* h_rec = nullptr;            // pinned
        bool pending = false;
        size_t n_l = 0, f_l = 0;                   // variables and factors of the pending solve
        s2m_pg_params pend_prm{};
        int pend_max_cg = 0;
        double a_launch[12] = { 0 };               // variable n_l - 1 at launch
    } pg;

    // the mutually consistent loops among many candidates (s2m_pg_consistent_loops, s2m_pg_consistency.hpp): buffers of its own, all
    // grow-only - the chain length and its block sums, the candidate table, the matrix in the caller's and in rank order, ranks |
    // order | set sizes, the block of the one download (selected | degree | record) - and the pinned block (the table up | that
    // block down).  It reads pg.est and writes nothing else of the handle.
    struct PgConsistency {
        DevBuf s, blk, cand, mat, mat_rank, rank, out;
        unsigned char* h_io = nullptr;
        size_t h_io_cap = 0;
    } pgc;

    // saving and loading a session (s2m_abi_session.hip): the segment table of a section on the device, the workgroups' checksum
    // partials, and two pinned chunks that take turns with gmap's two device staging buffers on gmap's copy stream
    struct Session {
        DevBuf tab, partial;
        unsigned char* h_chunk[2] = { nullptr, nullptr };      // pinned, h_chunk_cap bytes each
        size_t h_chunk_cap = 0;
        size_t chunk_bytes = 0;                                // 0: the default (s2m_debug_session_chunk sets a small one)
        // the session appended last (s2m_session_append): its keys [app_first, app_first + app_count) and the index of its
        // junction factor (-1: none); k_session_place's input and staging blocks
        int32_t app_first = -1, app_count = 0, app_junction = -1;
        DevBuf place_in, place_out;
        void forget_appended() { app_first = -1; app_count = 0; app_junction = -1; }
    } sess;
};

namespace s2m {
namespace host __attribute__((visibility("hidden"))) {

using Reg = s2m_context::Registration;

inline int fail(s2m_context* h, int code, const char* what, hipError_t e = hipSuccess)
{
    if (h) {
        h->err = what;
        if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); }
    }
    return code;
}

#define S2M_HIP(h, call)                                                     \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return fail((h), S2M_ERR_HIP, #call, e__);   \
    } while (0)

inline int ensure(s2m_context* h, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return S2M_OK;
    size_t want = bytes + bytes / 4 + 256;          // grow-only with slack
    S2M_HIP(h, b.reset());
    S2M_HIP(h, hipMalloc(&b.p, want));
    b.cap = want;
    h->ctx_dirty = true;
    return S2M_OK;
}

// host records -> `buf` (grown to hold them), on the handle's stream
inline int stage_host_records(s2m_context* h, DevBuf& buf, const void* pts, size_t bytes)
{
    int rc = ensure(h, buf, bytes);
    if (rc) return rc;
    S2M_HIP(h, hipMemcpyAsync(buf.p, pts, bytes, hipMemcpyHostToDevice, h->stream));
    return S2M_OK;
}

inline int check_records(s2m_context* h, const void* pts, size_t n, size_t stride)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (n > 0 && !pts) return fail(h, S2M_ERR_INVALID_ARG, "null point buffer");
    if (stride < 12 || (stride & 3)) return fail(h, S2M_ERR_INVALID_ARG, "stride_bytes must be >= 12 and a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(pts) & 3) != 0) return fail(h, S2M_ERR_INVALID_ARG, "point buffer must be 4-byte aligned");
    if (n > (size_t)0x3fffffff) return fail(h, S2M_ERR_CAPACITY, "too many points");
    return S2M_OK;
}

inline int check_leaf(s2m_context* h, float leaf)
{
    if (!(leaf > 0.0f) || !std::isfinite(leaf)) return fail(h, S2M_ERR_INVALID_ARG, "leaf size must be positive and finite");
    return S2M_OK;
}

// an output buffer that is asked for (cap > 0) and cannot take records
inline bool bad_out(const void* out, size_t out_stride, size_t cap) { return cap > 0 && (!out || out_stride < 12 || (out_stride & 3)); }

// transCur = pcl::getTransformation(x, y, z, roll, pitch, yaw) of a key pose (:317) as a row-major 3x4
inline void xyzrpy_to_transform(const float p[6], float T[12])
{
    const float rpyxyz[6] = { p[3], p[4], p[5], p[0], p[1], p[2] };
    host_pose_to_transform(rpyxyz, T, nullptr);
}

// A stream at the highest (`high`) or the lowest priority the device offers: the slots' streams alternate between the two, a
// loop closure and a pose-graph solve run at the lowest so that they yield to the registration kernels. A device that reports
// no range (or an error) gives a stream of the default priority; that is said on stderr, `who` naming the stream.
inline int create_stream(s2m_context* h, hipStream_t* out, bool high, const char* who)
{
    int least = 0, greatest = 0;
    const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess || least == greatest) {
        (void)hipGetLastError();
        fprintf(stderr, "liorf_s2m: no stream priority range on device %d (%s): %s runs at the default priority\n", h->device,
                e != hipSuccess ? hipGetErrorString(e) : "least == greatest", who);
        S2M_HIP(h, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    } else {
        S2M_HIP(h, hipStreamCreateWithPriority(out, hipStreamNonBlocking, high ? greatest : least));
    }
    return S2M_OK;
}

// puts a context on another stream for a scope (a slot on its own stream, the parent on a branch of the batch graph's capture)
struct OnStream {
    s2m_context* h;
    hipStream_t keep;
    OnStream(s2m_context* h_, hipStream_t s) : h(h_), keep(h_->stream) { h->stream = s; }
    OnStream(const OnStream&) = delete;
    ~OnStream() { h->stream = keep; }
};

// Forgets the pending optimise of `h` when the scope ends - with n_slots > 0 the batch of n_slots slots that `h` is the parent
// of. A collect holds one for its whole body; a launch from its first mark on, release()d when everything is queued.
struct PendingGuard {
    s2m_context* h;
    int n_slots;
    explicit PendingGuard(s2m_context* h_, int n_slots_ = 0) : h(h_), n_slots(n_slots_) {}
    PendingGuard(const PendingGuard&) = delete;
    void release() { h = nullptr; }
    ~PendingGuard()
    {
        if (!h) return;
        if (n_slots == 0) { h->reg.pending = Reg::kNone; h->reg.seg_pending = false; return; }
        for (int b = 0; b < n_slots; b++) { PendingGuard slot(h->batch.kids[(size_t)b]); }
        h->batch.pend_n = 0; h->batch.seg_pending = false; h->batch.live.clear();
    }
};

// ---- s2m_abi.hip (the LM loop: the only unit that launches kernels of s2m_kernels.hpp / s2m_register.hpp; the scan preparation,
// the batches and slots and the observation and timing hooks reach them through these) ----
float stamps_ms(const s2m_context* h, int from, int to);
int ensure_rows(s2m_context* h, int nblocks);
int upload_ctx(s2m_context* h);
void fill_state(s2m_context* h, DevState* s, const float pose[6]);
void store_state(s2m_context* h, const DevState& s, unsigned long long* stamp);
int push_state(s2m_context* h, const float pose[6], unsigned long long* stamp = nullptr);
void launch_density_state(s2m_context* h, const float pose[6], unsigned long long* stamp);
// k_chunk_table, the extent-only wave table of `nslots` prepared slots (it shares chunk_table_body with k_chunk_table_density)
void launch_chunk_table(hipStream_t stream, const PrepTable& t, int nslots);
// k_set_ctxs / k_init_states over the first n entries of a table (a batch launch: the DevCtx blocks that changed, the loop
// states its live slots start from); the entries behind them are marked unused here.  `issued`, if given, counts the launch.
void launch_set_ctxs(hipStream_t stream, CtxTable& t, int n, int* issued = nullptr);
void launch_init_states(hipStream_t stream, StateInitTable& t, int n, int* issued = nullptr);
// what one loop launches over: the scan slots (one for a single scan), the widest grid among them, their common workgroup shape
struct LoopShape {
    SlotTable tbl;
    int nslots = 1;
    int nblocks = 0;        // grid.x of the registration kernels: the largest DevCtx::nblocks among the slots
    int table_cap = 0;      // the largest wave-table capacity among the slots (grid of k_wave_density)
    int wpb = kBlock / 64;  // waves per workgroup (DevCtx::wpb, the same for every slot)
    bool batch = false;     // scan slots of a batch
    bool split = false;     // C + S per iteration instead of R
    bool late = false;      // the split iterations of this loop come late (few rows on the worklist): small search grid
    bool split_auto = false; // split if the loop's iterations are closed by k_finalize and the lean certify kernel applies
    bool wishes_done = false; // the density wishes of a pending re-split are in chunk_factor already (s2m_optimize_launch): the loop starts with k_chunk_table_density
    // a captured single-scan loop: the k_finalize that ends the range copies state + trace to `out` (the pinned mirror) and
    // stamps the wall clock at `stamp`; both null: the caller copies (plain launches, batches, diagnostics)
    DevState* out = nullptr;
    unsigned long long* stamp = nullptr;
};
LoopShape shape_of(s2m_context* h);
void launch_fused(s2m_context* h, const LoopShape& sh, bool hook, int L, int solve_prev);
void launch_iteration(s2m_context* h, const LoopShape& sh, int L, int solve_prev, bool fused_loop = true);
void launch_finalize(s2m_context* h, const LoopShape& sh, int L, int mode, bool ends_range = false);
void launch_density_wishes(s2m_context* h, const LoopShape& sh);
void launch_density_table(s2m_context* h, const LoopShape& sh);
void launch_density(s2m_context* h, const LoopShape& sh);
void enqueue_loop(s2m_context* h, const LoopShape& sh_in, hipEvent_t* events, bool coarse = false, int L0 = 0, int L1 = -1);
// The launch and the collect of one context's loop, shared by the single-scan, slot and batch entry points.
// optimize_gate: the soft conditions :1297 / :1300 for the optimisation of k's resident scan from `pose` (pending_pose_in,
// pending_skipped); true: a loop runs.  two_ranges: with early exit on a loop is issued as launches 0 .. seg-1 and, only for
// what has not converged by then, the rest.  optimize_launch: s2m_optimize_launch with the kind it is pending as.
// collect_record: the host-only half of a collect, once the record is in the pinned mirror - result, persistent state, trace,
// transformUpdate (:1317), or the skipped case.
bool optimize_gate(s2m_context* k, const float pose[6]);
inline bool two_ranges(const s2m_context* h) { return h->prm.early_exit && h->tune.seg_iters > 1 && h->tune.seg_iters < h->prm.max_iter; }
int optimize_launch(s2m_context* h, const float pose[6], Reg::Pending kind);
void collect_record(s2m_context* k, float pose[6], const s2m_imu_init* imu, s2m_result* out);
// The second range, for what did not converge in the first: `issue` queues it on h's stream with whatever brings the record
// back; it is waited for and timed by an event pair of its own, added to t_optimize_ms.
template <typename Issue> int second_range(s2m_context* h, Issue issue)
{
    S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
    const int rc = issue();
    if (rc) return rc;
    S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    float t2 = 0.0f;
    S2M_HIP(h, hipEventElapsedTime(&t2, h->reg.ev_a2, h->reg.ev_b2));
    h->reg.t_optimize_ms += t2;
    return S2M_OK;
}

// a slot of `h` has an optimise pending, of its own or as a row of a batch (s2m_set_params would pull the graphs from under it)
inline bool slots_pending(const s2m_context* h)
{
    for (const s2m_context* k : h->batch.kids)
        if (k->reg.pending != Reg::kNone) return true;
    return false;
}

// ---- s2m_prep.hip (the map index and the scan preparation: kernels of s2m_prep.hpp) ----
int set_map_impl(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device);
int set_scan_impl(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device);
int scan_slot_prepare(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device, PrepSlot* ps);
void launch_scan_prep(hipStream_t stream, const PrepTable& t, int nslots, bool single = false, int* issued = nullptr);
void ensure_wave_table(s2m_context* h);

// ---- s2m_sc.hip ----
// SCManager::makeScancontext + ring key of a cloud into h->sc.out (device); then: append them as key frame sc.n
int sc_build_descriptor(s2m_context* h, const void* pts, size_t n, size_t stride_bytes, bool on_device = false);
int sc_append_from_out(s2m_context* h);
// the store's three arrays hold `want` descriptors (grow-with-copy)
int sc_reserve(s2m_context* h, size_t want);

// ---- s2m_abi_sc_query.hip ----
// s2m_sc_query_scan with the scan on the device (n records of stride_bytes): hits has room for p->top_k records
int sc_query_device_scan(s2m_context* h, const void* d_pts, size_t n, size_t stride_bytes, const s2m_sc_query_params* p, s2m_sc_hit* hits,
                         int32_t* n_hits);

// ---- s2m_abi_loop.hip ----
// S2M_ERR_BUSY while a launched loop closure is pending (the calls that use its buffers start with this)
int loop_busy(s2m_context* h);
// waits for the loop stream and forgets the pending closure (s2m_kf_reset, s2m_destroy); `destroy`: the stream and event go too
void loop_drop_pending(s2m_context* h, bool destroy);
// what the loop closure shares with the alignment of host clouds (s2m_abi_icp.hip) and the relocalisation (s2m_abi_reloc.hip):
// the loop stream and its event exist; the handle's tuning of the device loop at a leaf; the caller's ICP parameters (null: the
// defaults) and an initial guess, validated; a result in the ABI's form
int loop_stream(s2m_context* h);
s2m::IcpTuning loop_tuning(const s2m_context* h, float leaf);
int icp_params_in(s2m_context* h, const s2m_icp_params* p, s2m::IcpParams* ip);
int guess_ok(s2m_context* h, const float* g);
void icp_result_out(const s2m::IcpResult& r, s2m_icp_result* out);
// the caller's loop parameters (null: the defaults), validated; the ICP parameters of a closure; a key of a store of N
int loop_params(s2m_context* h, const s2m_loop_params* p, s2m_loop_params* prm);
s2m::IcpParams loop_icp_params(const s2m_loop_params& prm);
bool loop_key_ok(int32_t k, size_t N);
int loop_submap(s2m_context* h, int32_t key, int32_t search_num, int32_t loop_index, float leaf, DevBuf& dst, VoxResult* res,
                long long clamp_lo = 0, long long clamp_hi = -1);
// The alignments a caller wants run together, in the form it names (s2m::IcpSet): it adds them as its gates leave them open and
// reads res[k] of alignment k once they have run. who[k]: the caller's own index of alignment k - its candidate, its record -
// so that no caller keeps a table beside the list. The slot form takes the same source with every add. arena: the clouds are
// offsets (add_at) in this buffer, which may move while it grows, and become addresses when the set is made.
struct IcpList {
    const s2m::IcpForm form;
    const size_t       stride;
    const DevBuf*      arena;
    int                n = 0;
    uintptr_t          src[s2m::kIcpMaxPairs], tgt[s2m::kIcpMaxPairs];
    size_t             n_src[s2m::kIcpMaxPairs], n_tgt[s2m::kIcpMaxPairs], who[s2m::kIcpMaxPairs];
    const float*       guess[s2m::kIcpMaxPairs];
    s2m::IcpResult     res[s2m::kIcpMaxPairs];
    const unsigned char *d_src[s2m::kIcpMaxPairs], *d_tgt[s2m::kIcpMaxPairs];       // (made by set())
    IcpList(s2m::IcpForm f, size_t stride_bytes, const DevBuf* in = nullptr) : form(f), stride(stride_bytes), arena(in) {}
    // the alignment's index
    int add_at(uintptr_t s, size_t ns, uintptr_t t, size_t nt, const float* g, size_t w)
    {
        src[n] = s; n_src[n] = ns; tgt[n] = t; n_tgt[n] = nt; guess[n] = g; who[n] = w;
        return n++;
    }
    int add(const void* s, size_t ns, const void* t, size_t nt, const float* g, size_t w)
    {
        return add_at(reinterpret_cast<uintptr_t>(s), ns, reinterpret_cast<uintptr_t>(t), nt, g, w);
    }
    s2m::IcpSet set()
    {
        const uintptr_t base = arena ? reinterpret_cast<uintptr_t>(arena->p) : 0;
        for (int k = 0; k < n; k++) {
            d_src[k] = reinterpret_cast<const unsigned char*>(base + src[k]);
            d_tgt[k] = reinterpret_cast<const unsigned char*>(base + tgt[k]);
        }
        return s2m::IcpSet{ form, n, d_src, n_src, d_tgt, n_tgt, guess, stride };
    }
};
int icp_list_align(s2m_context* h, hipStream_t stream, IcpList& al, const s2m::IcpParams& ip, float leaf, const char* what);
// `bytes` of src (kind: from the host or from the device) to the end of the many-keys arena, on `stream`, a stretch rounded up to
// 256 bytes; *off: where they start. The many_used bytes the arena holds are kept when it grows (the caller starts at 0).
int arena_put(s2m_context* h, hipStream_t stream, const void* src, hipMemcpyKind kind, size_t bytes, size_t* off);

// ---- s2m_abi_pose_graph.hip ----
// waits for the pose-graph stream and forgets the pending optimise (s2m_pg_reset, s2m_destroy); `destroy`: stream, events and the
// pinned record go too
void pg_drop_pending(s2m_context* h, bool destroy);
// the host mirror of the estimates holds the newest values (the device's, where an accepted step made them newer)
int pg_host_current(s2m_context* h);
// Rot3::RzRyRx(roll, pitch, yaw) and t of a float pose in fp64 with libm, as s2m_pg_set_initial makes an estimate of it
void pg_pose_to_state(const float pose_xyzrpy[6], double X[12]);
// pg.est holds the newest estimate of every variable, as an optimise finds it (S2M_ERR_INVALID_ARG: a variable without a value)
int pg_device_current(s2m_context* h);

// ---- s2m_abi_keyframes.hip ----
// gmap's copy stream and its two pairs of events exist (the chunked copy-out of the saved map and of a session share them)
int copy_pipeline(s2m_context* h);
// n keys behind the N0 the store holds, in one go (a session load: N0 = 0; an append): poses {x, y, z, roll, pitch, yaw}, times
// and point counts; every key gets its place in the arena, as n s2m_kf_add would give them, and its transform and position by
// the path of s2m_kf_add, with one upload per device array.  The records themselves are written by the caller, to
// frame[N0 + k].src.  A failure leaves the store for s2m_kf_reset, or for kf_truncate to a KfMark taken before the call.
int kf_install_keys(s2m_context* h, size_t n, const float* pose_xyzrpy, const double* time, const int32_t* counts);
// The store's extent - keys, arena blocks, the last block's fill and size - and the way back to it: blocks taken since are
// released (nothing on a stream may still write to them), the host mirrors shrink.  The device arrays only ever grew.
struct KfMark { size_t n_keys, n_blocks, block_used, block_cap; };
inline KfMark kf_mark(const s2m_context* h) { return KfMark{ h->kf.time.size(), h->kf.blocks.size(), h->kf.block_used, h->kf.block_cap }; }
void kf_truncate(s2m_context* h, const KfMark& m);

// ---- s2m_abi_voxel.hip ----
// VoxelGrid of a device cloud into `dst` (grown to hold one record per input point, the worst case).
int voxel_into(s2m_context* h, const unsigned char* d_in, size_t n, size_t stride, float leaf, DevBuf& dst, VoxResult* res);
// strided device records -> caller's host buffer (min(n, cap) records)
int download_records(s2m_context* h, const DevBuf& src, size_t n, void* out, size_t out_stride, size_t cap);
// the end of a stage that left res.n_out records in `src`: the host copy if one is asked for (cap > 0), the capacity error with
// the stage's message, the leaf warning
int finish_cloud(s2m_context* h, const DevBuf& src, const VoxResult& res, void* out, size_t out_stride, size_t cap, const char* too_small);

// the host side of a frame table: clouds on the device, each with its 3x4 transform, to be written back to back
struct FrameTable {
    std::vector<const unsigned char*> src;
    std::vector<int32_t> offsets{ 0 };
    std::vector<float> T;
    size_t total = 0;
    void push(const unsigned char* d_src, size_t n, const float t[12])
    {
        total += n;
        src.push_back(d_src);
        offsets.push_back((int32_t)total);
        T.insert(T.end(), t, t + 12);
    }
    // transformPointCloud (:310-329) of every frame (records of `stride` bytes) into `dst`; `what` names the step in an error
    int transform_into(s2m_context* h, DevBuf& dst, size_t stride, const char* what) const;
};

}  // namespace host
}  // namespace s2m
