// s2m_abi_loop.hip — C ABI of the loop closure against the key-frame store: detection, submaps, gates and judge, the closure and
// its launched form (launch / poll / collect), the verification of one key against several candidates and of many keys at once.
// Host orchestration of s2m_icp.hip's and s2m_voxel.hip's stages only.  What the alignment of host clouds (s2m_abi_icp.hip) and
// the relocalisation (s2m_abi_reloc.hip) share with it is defined first: the loop stream, the parameters, the submap, the list of
// alignments with its waited run, the arena.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "s2m_context.hpp"
#include "s2m_loop_detect_plan.hpp"    // loop_radius_time_ok: the radius and time test shared with s2m_loop_detect_keys

using namespace s2m;
using namespace s2m::host;

void s2m::host::icp_result_out(const IcpResult& r, s2m_icp_result* out)
{
    memcpy(out->T, r.T, sizeof(r.T));
    out->converged = r.converged; out->iterations = r.iterations; out->fitness_score = r.fitness;
}

static_assert(S2M_ICP_RANGE == kIcpRange, "include/liorf_s2m_debug.h states the range length of the device loop");
static_assert(S2M_LOOP_MAX_CANDIDATES == kIcpMaxSlots, "include/liorf_s2m.h states the slots of the device loop");

int s2m::host::loop_busy(s2m_context* h)
{
    return h->loop.pending != s2m_context::LoopClosure::kNone ? fail(h, S2M_ERR_BUSY, "a launched loop closure is pending: s2m_loop_poll / s2m_loop_collect it first") : S2M_OK;
}

void s2m::host::loop_drop_pending(s2m_context* h, bool destroy)
{
    if (h->loop.stream) (void)hipStreamSynchronize(h->loop.stream);
    if (h->loop.icp) icp_dev_cancel(h->loop.icp);
    h->loop.pending = s2m_context::LoopClosure::kNone;
    if (!destroy) return;
    if (h->loop.ev_submaps) (void)hipEventDestroy(h->loop.ev_submaps);
    if (h->loop.stream) (void)hipStreamDestroy(h->loop.stream);
    h->loop.ev_submaps = nullptr; h->loop.stream = nullptr;
}

// The loop stream: the lowest priority the device offers (create_stream), so that a closure yields to the registration kernels.
int s2m::host::loop_stream(s2m_context* h)
{
    if (h->loop.stream) return S2M_OK;
    const int rc = create_stream(h, &h->loop.stream, false, "the loop-closure stream");
    if (rc) return rc;
    S2M_HIP(h, hipEventCreateWithFlags(&h->loop.ev_submaps, hipEventDisableTiming));
    return S2M_OK;
}

IcpTuning s2m::host::loop_tuning(const s2m_context* h, float leaf)
{
    IcpTuning t = h->loop.tune;
    t.cell = (t.cell > 0.0f ? t.cell : kIcpCellLeaves) * leaf;
    return t;
}

// the caller's ICP parameters (null: the defaults), validated
int s2m::host::icp_params_in(s2m_context* h, const s2m_icp_params* p, IcpParams* ip)
{
    s2m_icp_params prm;
    if (p) prm = *p; else s2m_icp_default_params(&prm);
    if (!(prm.max_correspondence_distance > 0.0) || prm.max_iterations < 1)
        return fail(h, S2M_ERR_INVALID_ARG, "ICP needs a positive correspondence distance and at least one iteration");
    *ip = IcpParams{ prm.max_correspondence_distance, prm.max_iterations, prm.transformation_epsilon, prm.euclidean_fitness_epsilon };
    return S2M_OK;
}

// an initial guess as align(output, guess) takes one: finite, last row 0 0 0 1
int s2m::host::guess_ok(s2m_context* h, const float* g)
{
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(g[i])) return fail(h, S2M_ERR_INVALID_ARG, "the ICP guess has an entry that is not finite");
    if (g[12] != 0.0f || g[13] != 0.0f || g[14] != 0.0f || g[15] != 1.0f)
        return fail(h, S2M_ERR_INVALID_ARG, "the last row of the ICP guess must be 0 0 0 1");
    return S2M_OK;
}

// ---- loop closure against the key-frame store (:542-844) --------------------------------------------------

int s2m_loop_default_params(s2m_loop_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    p->search_radius = 10.0f;       // historyKeyframeSearchRadius    include/utility.h:245
    p->time_diff_s = 30.0f;         // historyKeyframeSearchTimeDiff  include/utility.h:246
    p->search_num = 25;             // historyKeyframeSearchNum       include/utility.h:247
    p->fitness_score = 0.3f;        // historyKeyframeFitnessScore    include/utility.h:248
    p->icp_leaf = 0.3f;             // loopClosureICPSurfLeafSize     include/utility.h:239
    return S2M_OK;
}

int s2m::host::loop_params(s2m_context* h, const s2m_loop_params* p, s2m_loop_params* prm)
{
    if (p) *prm = *p; else s2m_loop_default_params(prm);
    if (!loop_radius_time_ok(prm->search_radius, prm->time_diff_s) || prm->search_num < 0 || std::isnan(prm->fitness_score))
        return fail(h, S2M_ERR_INVALID_ARG, "loop search radius must be positive, time window finite, search_num >= 0");
    return check_leaf(h, prm->icp_leaf);
}

// loopFindNearKeyframes(key, search_num, loop_index) (:821-844) into `dst`: the frame table from the host mirror of the store, then
// the transform and the VoxelGrid of s2m_extract_cloud. An empty concatenation is not filtered (res->n_out = 0).
// With a clamp [clamp_lo, clamp_hi) the neighbours stay inside it (clamp_hi < 0: the whole store, as the reference): a submap at
// the boundary of an appended, still unplaced session takes no key of the other one (s2m_relocalize_key).
int s2m::host::loop_submap(s2m_context* h, int32_t key, int32_t search_num, int32_t loop_index, float leaf, DevBuf& dst, VoxResult* res,
                           long long clamp_lo, long long clamp_hi)
{
    *res = VoxResult{};
    const long long N = (long long)h->kf.time.size();
    const long long end = clamp_hi < 0 ? N : std::min(N, clamp_hi);
    const long long lo = std::max(std::max(0LL, clamp_lo), (long long)key - search_num), hi = std::min(end - 1, (long long)key + search_num);
    FrameTable tab;
    for (long long k = lo; k <= hi; k++) {                  // i = -search_num .. search_num, keyNear outside [0, N) skipped
        const KfFrame& f = h->kf.frame[(size_t)k];
        const KfFrame& tf = h->kf.frame[(size_t)(loop_index != -1 ? (long long)loop_index : k)];
        if (tab.total + (size_t)f.n > (size_t)0x3fffffff) return fail(h, S2M_ERR_CAPACITY, "too many points in the loop submap");
        tab.push(f.src, (size_t)f.n, tf.T);
    }
    if (tab.total == 0) return S2M_OK;                      // nearKeyframes->empty(): returned unfiltered (:837-838)
    int rc = tab.transform_into(h, h->loop.xf, kDsStride, "loop submap transform");
    if (rc) return rc;
    return voxel_into(h, h->loop.xf.as<unsigned char>(), tab.total, kDsStride, leaf, dst, res);   // (waits for the counts)
}

// s2m_icp_align's path on the device submaps: historyKeyframeSearchRadius*2 (a float), 100, 1e-6, 1e-6 (:572-576)
IcpParams s2m::host::loop_icp_params(const s2m_loop_params& prm) { return IcpParams{ (double)(prm.search_radius * 2.0f), 100, 1e-6, 1e-6 }; }

bool s2m::host::loop_key_ok(int32_t k, size_t N) { return k >= 0 && (size_t)k < N; }

// The list's alignments begun on `stream` and advanced with waits to their end, then the stream waited for: al.res[k] is the
// result of alignment k. An empty list only waits for the stream. what: the caller's words for a failure, after which the stream
// has been drained and nothing is in flight.
int s2m::host::icp_list_align(s2m_context* h, hipStream_t stream, IcpList& al, const IcpParams& ip, float leaf, const char* what)
{
    if (al.n) {
        hipError_t e = icp_dev_begin(h->loop.icp, stream, al.set(), ip, loop_tuning(h, leaf));
        bool done = false;
        if (e == hipSuccess) e = icp_dev_advance(h->loop.icp, stream, true, &done, al.res, kIcpMaxPairs);
        if (e != hipSuccess || !done) {
            (void)hipStreamSynchronize(stream);
            icp_dev_cancel(h->loop.icp);
            return fail(h, S2M_ERR_HIP, what, e);
        }
    }
    S2M_HIP(h, hipStreamSynchronize(stream));
    return S2M_OK;
}

// Room for `need` bytes in the arena of a pass, the many_used bytes it holds kept (a larger arena takes them over). stream: the
// stream the arena is written on.
static int arena_reserve(s2m_context* h, hipStream_t stream, size_t need)
{
    s2m_context::LoopClosure& L = h->loop;
    if (need <= L.many_arena.cap) return S2M_OK;
    const size_t want = std::max(need + need / 2, (size_t)1 << 20);
    void* q = nullptr;
    S2M_HIP(h, hipMalloc(&q, want));
    hipError_t e = L.many_used ? hipMemcpyAsync(q, L.many_arena.p, L.many_used, hipMemcpyDeviceToDevice, stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipFree(q); return fail(h, S2M_ERR_HIP, "the submaps of a verification pass", e); }
    S2M_HIP(h, L.many_arena.reset(q, want));
    return S2M_OK;
}

int s2m::host::arena_put(s2m_context* h, hipStream_t stream, const void* src, hipMemcpyKind kind, size_t bytes, size_t* off)
{
    s2m_context::LoopClosure& L = h->loop;
    const size_t room = (bytes + 255) / 256 * 256;
    const int rc = arena_reserve(h, stream, L.many_used + room);
    if (rc) return rc;
    *off = L.many_used;
    S2M_HIP(h, hipMemcpyAsync(L.many_arena.as<unsigned char>() + L.many_used, src, bytes, kind, stream));
    L.many_used += room;
    return S2M_OK;
}

namespace {

void loop_result_init(s2m_loop_result* o)
{
    memset(o, 0, sizeof(*o));
    o->status = S2M_LOOP_NONE;
    o->key_cur = o->key_pre = -1;
}

// The gates of one key against n_cand candidates (:565-566, :641-661): the container test, the source submap once, then a target
// submap (loop.target(i)) and the size gate per candidate. rec: n_cand records as loop_result_init leaves them; one that the gates
// decide is final (ALREADY_CLOSED, TOO_FEW_POINTS), the others keep S2M_LOOP_NONE and are what *open counts.
int loop_gates(s2m_context* h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params& prm,
               s2m_loop_result* rec, int32_t* open)
{
    s2m_context::LoopClosure& L = h->loop;
    *open = 0;
    const bool closed = L.index.count(key_cur) != 0;
    for (int32_t i = 0; i < n_cand; i++) {
        rec[i].key_cur = key_cur;
        rec[i].key_pre = key_pre[i];
        if (closed) rec[i].status = S2M_LOOP_ALREADY_CLOSED;
    }
    if (closed) return S2M_OK;
    VoxResult rc_cur;
    int rc = loop_submap(h, key_cur, 0, base_key, prm.icp_leaf, L.cur, &rc_cur);
    if (rc) return rc;
    for (int32_t i = 0; i < n_cand; i++) {
        VoxResult rc_prev;
        if ((rc = loop_submap(h, key_pre[i], prm.search_num, base_key, prm.icp_leaf, L.target(i), &rc_prev))) return rc;
        rec[i].n_cur = (int32_t)rc_cur.n_out;
        rec[i].n_prev = (int32_t)rc_prev.n_out;
        if (rc_cur.n_out < 300 || rc_prev.n_out < 1000) rec[i].status = S2M_LOOP_TOO_FEW_POINTS;
        else ++*open;
    }
    return S2M_OK;
}

// the fitness gate and the pose result (:585-620, :707-715). T_cur, pose_pre: transCur of key_cur and the pose of
// key_pre - the store's for the synchronous call, the launch-time snapshot for a launched closure
void loop_judge(const IcpResult& r, int32_t base_key, float fitness_score, const float T_cur[12], const float pose_pre[6], s2m_loop_result* out)
{
    icp_result_out(r, &out->icp);
    if (!r.converged || r.fitness > (double)fitness_score) { out->status = S2M_LOOP_REJECTED; return; }   // (:585)
    if (base_key == -1) {
        float t_correct[12];                                // correctionLidarFrame * tWrong (:597-601)
        host_affine_mul(r.T, T_cur, t_correct);
        host_translation_and_euler(t_correct, 4, out->pose_from);
        memcpy(out->pose_to, pose_pre, sizeof(out->pose_to));
    } else {
        host_translation_and_euler(r.T, 4, out->pose_from);  // (:707); poseTo is the identity (:709)
    }
    out->status = S2M_LOOP_ACCEPTED;
}

// the accepted record with the least (icp.fitness_score, position), or -1
int32_t verify_best(const s2m_loop_result* rec, int32_t n)
{
    int32_t best = -1;
    for (int32_t i = 0; i < n; i++)
        if (rec[i].status == S2M_LOOP_ACCEPTED && (best < 0 || rec[i].icp.fitness_score < rec[best].icp.fitness_score)) best = i;
    return best;
}

// the container test, both submaps, the size gate, ICP, the fitness gate, the pose result and the container (:565-621, :641-715)
int loop_align_impl(s2m_context* h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params& prm, s2m_loop_result* out)
{
    int32_t open;
    int rc = loop_gates(h, key_cur, &key_pre, 1, base_key, prm, out, &open);
    if (rc || !open) return rc;
    IcpResult r;
    hipError_t e = icp_align(h->loop.icp, h->stream, h->loop.cur.as<unsigned char>(), (size_t)out->n_cur, h->loop.target(0).as<unsigned char>(),
                             (size_t)out->n_prev, kDsStride, loop_icp_params(prm), &r);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "loop ICP alignment", e);
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    loop_judge(r, base_key, prm.fitness_score, h->kf.frame[(size_t)key_cur].T, &h->kf.pose[6 * (size_t)key_pre], out);
    if (out->status == S2M_LOOP_ACCEPTED) h->loop.index[key_cur] = key_pre;               // loopIndexContainer[loopKeyCur] = loopKeyPre (:621)
    return S2M_OK;
}

// The launched form: the same gates, then the alignments of the candidates that are left queued in lockstep on the loop stream,
// behind the submap writes. rec: n_cand records; who: the family of the call, which may poll the closure and names it in an error.
int loop_launch(s2m_context* h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params& prm,
                s2m_loop_result* rec, s2m_context::LoopClosure::Pending who)
{
    s2m_context::LoopClosure& L = h->loop;
    int32_t slots;
    int rc = loop_gates(h, key_cur, key_pre, n_cand, base_key, prm, rec, &slots);
    if (rc || !slots) return rc;
    IcpList al(IcpForm::kSlots, kDsStride);
    for (int32_t i = 0; i < n_cand; i++)
        L.pend_slot[i] = rec[i].status != S2M_LOOP_NONE ? -1 : al.add(L.cur.p, (size_t)rec[0].n_cur, L.target(i).p, (size_t)rec[i].n_prev, nullptr, i);
    if ((rc = loop_stream(h))) return rc;
    S2M_HIP(h, hipEventRecord(L.ev_submaps, h->stream));
    S2M_HIP(h, hipStreamWaitEvent(L.stream, L.ev_submaps, 0));
    const hipError_t e = icp_dev_begin(L.icp, L.stream, al.set(), loop_icp_params(prm), loop_tuning(h, prm.icp_leaf));
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(L.stream);               // (whatever was queued before the failure ends before the buffers are used again)
        return fail(h, S2M_ERR_HIP, who == L.kSingle ? "loop ICP launch" : "loop verification launch", e);
    }
    for (int32_t i = 0; i < n_cand; i++) {
        if (L.pend_slot[i] >= 0) rec[i].status = S2M_LOOP_PENDING;
        L.pend_rec[i] = rec[i];
        memcpy(L.pend_pose_pre[i], &h->kf.pose[6 * (size_t)key_pre[i]], sizeof(L.pend_pose_pre[i]));
    }
    L.pend_n = n_cand;
    L.pend_fitness = prm.fitness_score;
    L.pend_base_key = base_key;
    memcpy(L.snap_T, h->kf.frame[(size_t)key_cur].T, sizeof(L.snap_T));
    L.pending = who;
    return S2M_OK;
}

int loop_launch_single(s2m_context* h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params& prm, s2m_loop_result* early)
{
    return loop_launch(h, key_cur, &key_pre, 1, base_key, prm, early, s2m_context::LoopClosure::kSingle);
}

// A step of the pending closure: the device loop advanced (wait: to its end). Once it has ended the records that took a slot are
// judged, the accepted one with the least fitness - of one record, that record if it was accepted - goes into the container (only
// the winner is a closure, :621), *best names it and nothing is pending any more. The records are loop.pend_rec[0 .. pend_n).
int loop_advance(s2m_context* h, bool wait, int32_t* best)
{
    s2m_context::LoopClosure& L = h->loop;
    S2M_HIP(h, hipSetDevice(h->device));
    bool done = false;
    IcpResult r[S2M_LOOP_MAX_CANDIDATES];
    const hipError_t e = icp_dev_advance(L.icp, L.stream, wait, &done, r, S2M_LOOP_MAX_CANDIDATES);
    if (e != hipSuccess) {
        const char* what = L.pending == L.kSingle ? "loop ICP on the loop stream" : "loop verification on the loop stream";
        loop_drop_pending(h, false);
        return fail(h, S2M_ERR_HIP, what, e);
    }
    if (!done) return S2M_OK;
    for (int32_t i = 0; i < L.pend_n; i++) {
        if (L.pend_slot[i] < 0) continue;
        L.pend_rec[i].status = S2M_LOOP_NONE;
        loop_judge(r[L.pend_slot[i]], L.pend_base_key, L.pend_fitness, L.snap_T, L.pend_pose_pre[i], &L.pend_rec[i]);
    }
    *best = verify_best(L.pend_rec, L.pend_n);
    if (*best >= 0) L.index[L.pend_rec[*best].key_cur] = L.pend_rec[*best].key_pre;
    L.pending = L.kNone;
    return S2M_OK;
}

int loop_poll_impl(s2m_context* h, s2m_loop_result* out, bool wait)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    s2m_context::LoopClosure& L = h->loop;
    if (L.pending == L.kVerify)
        return fail(h, S2M_ERR_BUSY, "a launched verification is pending: s2m_loop_verify_poll / s2m_loop_verify_collect it");
    loop_result_init(out);
    if (L.pending == L.kNone) return S2M_OK;                // S2M_LOOP_NONE, keys -1
    int32_t best;
    const int rc = loop_advance(h, wait, &best);
    if (rc) return rc;
    *out = L.pend_rec[0];                                   // S2M_LOOP_PENDING, or the result
    return S2M_OK;
}

}  // namespace

int s2m_loop_near_keyframes(s2m_handle h, int32_t key, int32_t search_num, int32_t loop_index, float leaf,
                            void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    int rc = loop_busy(h);
    if (rc) return rc;
    *n_out = 0;
    if ((rc = check_leaf(h, leaf))) return rc;
    if (search_num < 0) return fail(h, S2M_ERR_INVALID_ARG, "search_num must be >= 0");
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;
    if (!loop_key_ok(key, N) || (loop_index != -1 && !loop_key_ok(loop_index, N)))
        return fail(h, S2M_ERR_INVALID_ARG, "key or loop_index outside the key-frame store");
    S2M_HIP(h, hipSetDevice(h->device));
    VoxResult res;
    if ((rc = loop_submap(h, key, search_num, loop_index, leaf, h->loop.prev, &res))) return rc;
    *n_out = res.n_out;
    if ((rc = download_records(h, h->loop.prev, res.n_out, out, out_stride_bytes, cap))) return rc;
    if (res.n_out > cap) return fail(h, S2M_ERR_CAPACITY, "output buffer too small for the loop submap");
    return res.leaf_too_small ? S2M_WARN_LEAF_TOO_SMALL : S2M_OK;
}

namespace {

using LoopImpl = int (*)(s2m_context*, int32_t, int32_t, int32_t, const s2m_loop_params&, s2m_loop_result*);

int loop_align_front(s2m_context* h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params* p, s2m_loop_result* out,
                     LoopImpl impl)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    int rc = loop_busy(h);
    if (rc) return rc;
    loop_result_init(out);
    s2m_loop_params prm;
    if ((rc = loop_params(h, p, &prm))) return rc;
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;                             // cloudKeyPoses3D->points.empty() (:544-545, :627-628)
    if (!loop_key_ok(key_cur, N) || !loop_key_ok(key_pre, N) || (base_key != -1 && !loop_key_ok(base_key, N)))
        return fail(h, S2M_ERR_INVALID_ARG, "loop keys outside the key-frame store");
    S2M_HIP(h, hipSetDevice(h->device));
    return impl(h, key_cur, key_pre, base_key, prm, out);
}

int loop_closure_rs_front(s2m_context* h, double time_cur, const s2m_loop_params* p, s2m_loop_result* out, LoopImpl impl)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    int rc = loop_busy(h);
    if (rc) return rc;
    loop_result_init(out);
    s2m_loop_params prm;
    if ((rc = loop_params(h, p, &prm))) return rc;
    if (!std::isfinite(time_cur)) return fail(h, S2M_ERR_INVALID_ARG, "time_cur must be finite");
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;                             // (:544-545)
    const int32_t key_cur = (int32_t)N - 1;
    if (h->loop.index.count(key_cur)) {                    // (:737-739)
        out->key_cur = key_cur;
        out->status = S2M_LOOP_ALREADY_CLOSED;
        return S2M_OK;
    }
    S2M_HIP(h, hipSetDevice(h->device));
    int key_pre = -1;
    hipError_t e = loop_detect(h->voxel.ws, h->stream, h->kf.pos.as<float4>(), h->kf.tdev.as<double>(), (int)N, prm.search_radius,
                               time_cur, (double)prm.time_diff_s, &key_pre);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "loop detection", e);
    if (key_pre == -1 || key_pre == key_cur) return S2M_OK;                 // (:761-762)
    return impl(h, key_cur, key_pre, -1, prm, out);
}

}  // namespace

int s2m_loop_align(s2m_handle h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params* p, s2m_loop_result* out)
{
    return loop_align_front(h, key_cur, key_pre, base_key, p, out, loop_align_impl);
}

int s2m_loop_closure_rs(s2m_handle h, double time_cur, const s2m_loop_params* p, s2m_loop_result* out)
{
    return loop_closure_rs_front(h, time_cur, p, out, loop_align_impl);
}

int s2m_loop_align_launch(s2m_handle h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params* p, s2m_loop_result* early)
{
    return loop_align_front(h, key_cur, key_pre, base_key, p, early, loop_launch_single);
}

int s2m_loop_closure_rs_launch(s2m_handle h, double time_cur, const s2m_loop_params* p, s2m_loop_result* early)
{
    return loop_closure_rs_front(h, time_cur, p, early, loop_launch_single);
}

int s2m_loop_poll(s2m_handle h, s2m_loop_result* out) { return loop_poll_impl(h, out, false); }

int s2m_loop_collect(s2m_handle h, s2m_loop_result* out) { return loop_poll_impl(h, out, true); }

// ---- verification: one key against several candidates, aligned in lockstep ------------------------------------------------

namespace {

// the checks of the candidate list that need no handle. *empty: the store is empty (S2M_OK, S2M_LOOP_NONE records)
int verify_args(s2m_context* h, size_t N, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params* p,
                s2m_loop_params* prm, bool* empty)
{
    *empty = false;
    if (!key_pre || n_cand < 1 || n_cand > S2M_LOOP_MAX_CANDIDATES)
        return fail(h, S2M_ERR_INVALID_ARG, "a verification takes 1 .. S2M_LOOP_MAX_CANDIDATES candidates");
    const int rc = loop_params(h, p, prm);
    if (rc) return rc;
    if (N == 0) { *empty = true; return S2M_OK; }
    if (!loop_key_ok(key_cur, N) || (base_key != -1 && !loop_key_ok(base_key, N)))
        return fail(h, S2M_ERR_INVALID_ARG, "loop keys outside the key-frame store");
    for (int32_t i = 0; i < n_cand; i++) {
        if (!loop_key_ok(key_pre[i], N)) return fail(h, S2M_ERR_INVALID_ARG, "loop keys outside the key-frame store");
        if (key_pre[i] == key_cur) return fail(h, S2M_ERR_INVALID_ARG, "a candidate is key_cur itself");
        for (int32_t j = 0; j < i; j++)
            if (key_pre[j] == key_pre[i]) return fail(h, S2M_ERR_INVALID_ARG, "a candidate is listed twice");
    }
    return S2M_OK;
}

int verify_launch_front(s2m_context* h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params* p,
                        s2m_loop_result* early, int32_t* best)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!early || !best) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    int rc = loop_busy(h);
    if (rc) return rc;
    *best = -1;
    s2m_loop_params prm;
    bool empty;
    if ((rc = verify_args(h, h->kf.time.size(), key_cur, key_pre, n_cand, base_key, p, &prm, &empty))) return rc;
    for (int32_t i = 0; i < n_cand; i++) loop_result_init(&early[i]);
    if (empty) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    return loop_launch(h, key_cur, key_pre, n_cand, base_key, prm, early, s2m_context::LoopClosure::kVerify);
}

int verify_poll_impl(s2m_context* h, s2m_loop_result* out, int32_t cap, int32_t* n_out, int32_t* best, bool wait)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!n_out || !best || cap < 0 || (cap > 0 && !out)) return fail(h, S2M_ERR_INVALID_ARG, "bad loop result buffer");
    s2m_context::LoopClosure& L = h->loop;
    if (L.pending == L.kSingle)
        return fail(h, S2M_ERR_BUSY, "a launched loop closure is pending: s2m_loop_poll / s2m_loop_collect it first");
    *n_out = 0; *best = -1;
    if (L.pending == L.kNone) return S2M_OK;
    const int rc = loop_advance(h, wait, best);
    if (rc) return rc;
    const int32_t n = L.pend_n;
    *n_out = n;
    for (int32_t i = 0; i < std::min(n, cap); i++) out[i] = L.pend_rec[i];
    if (cap < n) return fail(h, S2M_ERR_CAPACITY, "output buffer too small for the verification's records");
    return S2M_OK;
}

}  // namespace

int s2m_loop_verify_check_args(int32_t n_stored, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params* p)
{
    if (n_stored < 0) return S2M_ERR_INVALID_ARG;
    s2m_loop_params prm;
    bool empty;
    return verify_args(nullptr, (size_t)n_stored, key_cur, key_pre, n_cand, base_key, p, &prm, &empty);
}

int s2m_loop_verify_launch(s2m_handle h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params* p,
                           s2m_loop_result* early, int32_t* best)
{
    return verify_launch_front(h, key_cur, key_pre, n_cand, base_key, p, early, best);
}

int s2m_loop_verify_poll(s2m_handle h, s2m_loop_result* out, int32_t cap, int32_t* n_out, int32_t* best)
{
    return verify_poll_impl(h, out, cap, n_out, best, false);
}

int s2m_loop_verify_collect(s2m_handle h, s2m_loop_result* out, int32_t cap, int32_t* n_out, int32_t* best)
{
    return verify_poll_impl(h, out, cap, n_out, best, true);
}

int s2m_loop_verify(s2m_handle h, int32_t key_cur, const int32_t* key_pre, int32_t n_cand, int32_t base_key, const s2m_loop_params* p,
                    s2m_loop_result* out, int32_t* best)
{
    const int rc = verify_launch_front(h, key_cur, key_pre, n_cand, base_key, p, out, best);
    if (rc || h->loop.pending == s2m_context::LoopClosure::kNone) return rc;
    int32_t n = 0;
    return verify_poll_impl(h, out, n_cand, &n, best, true);
}

// ---- verification of many keys: the pairs of a pass aligned in lockstep through the pair table ---------------------------

static_assert(S2M_LOOP_MANY_MAX_PAIRS == kIcpMaxPairs, "include/liorf_s2m.h states the pairs of a pass");

namespace {

int many_pairs_per_pass(int32_t asked)
{
    return asked <= 0 ? kIcpMaxPairs : std::min(std::max((int)asked, (int)S2M_LOOP_MAX_CANDIDATES), kIcpMaxPairs);
}

// The plan: consecutive rows while the sum of their n_cand stays within pairs_per_pass, a row never split, a row without
// candidates taking no room. first[k] .. first[k + 1]: the rows of pass k (first: m + 1 entries at most). A function of the
// arguments alone: what the gates leave does not enter it.
int32_t many_plan(const int32_t* n_cand, int32_t m, int pairs_per_pass, int32_t* first)
{
    int32_t n_pass = 0, used = 0;
    for (int32_t r = 0; r < m; r++) {
        if (r == 0 || used + n_cand[r] > pairs_per_pass) { first[n_pass++] = r; used = 0; }
        used += n_cand[r];
    }
    first[n_pass] = m;
    return n_pass;
}

// every check of s2m_loop_verify_many that needs no handle. *empty: the store is empty
int many_args(s2m_context* h, size_t N, const int32_t* key_cur, const int32_t* key_pre, const int32_t* n_cand, int32_t m, int32_t row_stride,
              int32_t base_key, const s2m_loop_params* p, s2m_loop_params* prm, bool* empty)
{
    *empty = N == 0;
    if (m < 0) return fail(h, S2M_ERR_INVALID_ARG, "a negative number of rows");
    if (row_stride < 1 || row_stride > S2M_LOOP_MAX_CANDIDATES)
        return fail(h, S2M_ERR_INVALID_ARG, "row_stride must be 1 .. S2M_LOOP_MAX_CANDIDATES");
    int rc = loop_params(h, p, prm);
    if (rc) return rc;
    if (m == 0) return S2M_OK;
    if (!key_cur || !key_pre || !n_cand) return fail(h, S2M_ERR_INVALID_ARG, "null row arrays");
    for (int32_t r = 0; r < m; r++) {
        if (n_cand[r] < 0 || n_cand[r] > row_stride) return fail(h, S2M_ERR_INVALID_ARG, "a row has more candidates than row_stride, or fewer than none");
        if (n_cand[r] == 0) continue;
        s2m_loop_params row_prm;
        bool row_empty;
        if ((rc = verify_args(h, N, key_cur[r], key_pre + (size_t)r * row_stride, n_cand[r], base_key, p, &row_prm, &row_empty))) return rc;
    }
    // the rows must not depend on one another's results: key_cur distinct over the rows that have candidates
    std::vector<int32_t> keys;
    for (int32_t r = 0; r < m; r++) if (n_cand[r]) keys.push_back(key_cur[r]);
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return fail(h, S2M_ERR_INVALID_ARG, "a key_cur is named by two rows");
    return S2M_OK;
}

// One pass: rows [r0, r1). The gates and submaps of every row by the path of the single call - built where the single call builds
// them, the filtered records of the pairs the gates left open then copied into the pass's arena, behind the stream's order, before
// the next row builds over them; one lockstep alignment of those pairs; the judge, the best rule and the container per row.
int many_pass(s2m_context* h, const int32_t* key_cur, const int32_t* key_pre, const int32_t* n_cand, int32_t r0, int32_t r1, int32_t row_stride,
              int32_t base_key, const s2m_loop_params& prm, s2m_loop_result* out, int32_t* best)
{
    s2m_context::LoopClosure& L = h->loop;
    IcpList al(IcpForm::kTable, kDsStride, &L.many_arena);  // (the arena may move while it grows: the list keeps offsets)
    int cands = 0, rc;
    L.many_used = 0;
    for (int32_t r = r0; r < r1; r++) {
        if (!n_cand[r]) continue;
        if (cands + n_cand[r] > kIcpMaxPairs) return fail(h, S2M_ERR_CAPACITY, "a pass of more than kIcpMaxPairs pairs");   // not reached
        s2m_loop_result* rec = out + (size_t)r * row_stride;
        int32_t open;
        if ((rc = loop_gates(h, key_cur[r], key_pre + (size_t)r * row_stride, n_cand[r], base_key, prm, rec, &open))) return rc;
        size_t row_src = 0, tgt = 0;                        // (n_cur: the same in every record of the row)
        if (open && (rc = arena_put(h, h->stream, L.cur.p, hipMemcpyDeviceToDevice, (size_t)rec[0].n_cur * kDsStride, &row_src))) return rc;
        for (int32_t i = 0; open && i < n_cand[r]; i++) {
            if (rec[i].status != S2M_LOOP_NONE) continue;
            if ((rc = arena_put(h, h->stream, L.target(i).p, hipMemcpyDeviceToDevice, (size_t)rec[i].n_prev * kDsStride, &tgt))) return rc;
            al.add_at(row_src, (size_t)rec[i].n_cur, tgt, (size_t)rec[i].n_prev, nullptr, (size_t)(&rec[i] - out));
        }
        cands += n_cand[r];
    }
    if (al.n) {
        if ((rc = icp_list_align(h, h->stream, al, loop_icp_params(prm), prm.icp_leaf, "loop verification of many keys"))) return rc;
        for (int k = 0; k < al.n; k++) {
            s2m_loop_result* o = &out[al.who[k]];
            loop_judge(al.res[k], base_key, prm.fitness_score, h->kf.frame[(size_t)o->key_cur].T, &h->kf.pose[6 * (size_t)o->key_pre], o);
        }
        L.many_last_pairs += al.n;
    }
    for (int32_t r = r0; r < r1; r++) {
        if (!n_cand[r]) continue;
        const s2m_loop_result* rec = out + (size_t)r * row_stride;
        best[r] = verify_best(rec, n_cand[r]);
        if (best[r] >= 0) L.index[rec[best[r]].key_cur] = rec[best[r]].key_pre;           // only the winner is a closure (:621)
    }
    return S2M_OK;
}

}  // namespace

int s2m_loop_verify_many_check_args(int32_t n_stored, const int32_t* key_cur, const int32_t* key_pre, const int32_t* n_cand, int32_t m,
                                    int32_t row_stride, int32_t base_key, const s2m_loop_params* p)
{
    if (n_stored < 0) return S2M_ERR_INVALID_ARG;
    s2m_loop_params prm;
    bool empty;
    return many_args(nullptr, (size_t)n_stored, key_cur, key_pre, n_cand, m, row_stride, base_key, p, &prm, &empty);
}

int s2m_loop_verify_many(s2m_handle h, const int32_t* key_cur, const int32_t* key_pre, const int32_t* n_cand, int32_t m, int32_t row_stride,
                         int32_t base_key, const s2m_loop_params* p, s2m_loop_result* out, int32_t* best)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (m > 0 && (!out || !best)) return fail(h, S2M_ERR_INVALID_ARG, "null loop results");
    int rc = loop_busy(h);
    if (rc) return rc;
    s2m_loop_params prm;
    bool empty;
    if ((rc = many_args(h, h->kf.time.size(), key_cur, key_pre, n_cand, m, row_stride, base_key, p, &prm, &empty))) return rc;
    s2m_context::LoopClosure& L = h->loop;
    L.many_last_passes = L.many_last_pairs = 0;
    if (m == 0) return S2M_OK;
    for (int32_t r = 0; r < m; r++) {
        best[r] = -1;
        for (int32_t i = 0; i < n_cand[r]; i++) loop_result_init(&out[(size_t)r * row_stride + i]);
    }
    if (empty) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    std::vector<int32_t> first((size_t)m + 1);
    const int32_t n_pass = many_plan(n_cand, m, many_pairs_per_pass(L.many_pairs_per_pass), first.data());
    for (int32_t k = 0; k < n_pass; k++) {
        rc = many_pass(h, key_cur, key_pre, n_cand, first[k], first[k + 1], row_stride, base_key, prm, out, best);
        if (rc) {                                           // the rows of the passes before keep what they have; this pass's rows as the later ones
            for (int32_t r = first[k]; r < first[k + 1]; r++) {
                best[r] = -1;
                for (int32_t i = 0; i < n_cand[r]; i++) loop_result_init(&out[(size_t)r * row_stride + i]);
            }
            return rc;
        }
        L.many_last_passes++;
    }
    return S2M_OK;
}

int s2m_debug_loop_verify_many_pass(s2m_handle h, int32_t pairs_per_pass)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (pairs_per_pass < 0) return fail(h, S2M_ERR_INVALID_ARG, "pairs per pass must not be negative");
    h->loop.many_pairs_per_pass = pairs_per_pass == 0 ? 0 : many_pairs_per_pass(pairs_per_pass);
    return S2M_OK;
}

int s2m_debug_loop_verify_many_last(s2m_handle h, int32_t* passes, int32_t* pairs_aligned, size_t* bytes)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (passes) *passes = h->loop.many_last_passes;
    if (pairs_aligned) *pairs_aligned = h->loop.many_last_pairs;
    if (bytes) *bytes = h->loop.many_arena.cap;
    return S2M_OK;
}

int s2m_debug_loop_verify_many_plan(const int32_t* n_cand, int32_t m, int32_t pairs_per_pass, int32_t* first_row_of_pass, int32_t* n_pass)
{
    if (m < 0 || pairs_per_pass < 0 || !first_row_of_pass || !n_pass || (m > 0 && !n_cand)) return S2M_ERR_INVALID_ARG;
    for (int32_t r = 0; r < m; r++) if (n_cand[r] < 0 || n_cand[r] > S2M_LOOP_MAX_CANDIDATES) return S2M_ERR_INVALID_ARG;
    *n_pass = many_plan(n_cand, m, many_pairs_per_pass(pairs_per_pass), first_row_of_pass);
    return S2M_OK;
}

