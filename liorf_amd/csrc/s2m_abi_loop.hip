// s2m_abi_loop.hip — C ABI of the loop closure: the ICP alignment of two host clouds (section 8(f) row F4) and detection, submaps
// and alignment against the key-frame store.  Host orchestration of s2m_icp.hip's and s2m_voxel.hip's stages only.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

static void icp_result_out(const IcpResult& r, s2m_icp_result* out)
{
    memcpy(out->T, r.T, sizeof(r.T));
    out->converged = r.converged; out->iterations = r.iterations; out->fitness_score = r.fitness;
}

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
    int rc = check_records(h, src, n_src, stride_bytes);
    if (rc) return rc;
    if ((rc = check_records(h, tgt, n_tgt, stride_bytes))) return rc;
    if (!out) return S2M_ERR_INVALID_ARG;
    s2m_icp_params prm;
    if (p) prm = *p; else s2m_icp_default_params(&prm);
    if (!(prm.max_correspondence_distance > 0.0) || prm.max_iterations < 1)
        return fail(h, S2M_ERR_INVALID_ARG, "ICP needs a positive correspondence distance and at least one iteration");
    S2M_HIP(h, hipSetDevice(h->device));
    if (n_src && (rc = stage_host_records(h, h->loop.icp_src, src, n_src * stride_bytes))) return rc;
    if (n_tgt && (rc = stage_host_records(h, h->loop.icp_tgt, tgt, n_tgt * stride_bytes))) return rc;
    IcpParams ip{ prm.max_correspondence_distance, prm.max_iterations, prm.transformation_epsilon, prm.euclidean_fitness_epsilon };
    IcpResult r;
    hipError_t e = icp_align(h->loop.icp, h->stream, h->loop.icp_src.as<unsigned char>(), n_src, h->loop.icp_tgt.as<unsigned char>(), n_tgt,
                             stride_bytes, ip, &r);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "ICP alignment", e);
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    icp_result_out(r, out);
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

namespace {

int loop_params(s2m_context* h, const s2m_loop_params* p, s2m_loop_params* prm)
{
    if (p) *prm = *p; else s2m_loop_default_params(prm);
    if (!(prm->search_radius > 0.0f) || !std::isfinite(prm->search_radius) || !std::isfinite(prm->time_diff_s) ||
        prm->search_num < 0 || std::isnan(prm->fitness_score))
        return fail(h, S2M_ERR_INVALID_ARG, "loop search radius must be positive, time window finite, search_num >= 0");
    return check_leaf(h, prm->icp_leaf);
}

void loop_result_init(s2m_loop_result* o)
{
    memset(o, 0, sizeof(*o));
    o->status = S2M_LOOP_NONE;
    o->key_cur = o->key_pre = -1;
}

// loopFindNearKeyframes(key, search_num, loop_index) (:821-844) into `dst`: the frame table from the host mirror of the store, then
// the transform and the VoxelGrid of s2m_extract_cloud. An empty concatenation is not filtered (res->n_out = 0).
int loop_submap(s2m_context* h, int32_t key, int32_t search_num, int32_t loop_index, float leaf, DevBuf& dst, VoxResult* res)
{
    *res = VoxResult{};
    const long long N = (long long)h->kf.time.size();
    const long long lo = std::max(0LL, (long long)key - search_num), hi = std::min(N - 1, (long long)key + search_num);
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

// the container test, both submaps, the size gate, ICP, the fitness gate and the pose result (:565-621, :641-715)
int loop_align_impl(s2m_context* h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params& prm, s2m_loop_result* out)
{
    out->key_cur = key_cur;
    out->key_pre = key_pre;
    if (h->loop.index.count(key_cur)) { out->status = S2M_LOOP_ALREADY_CLOSED; return S2M_OK; }
    VoxResult rc_cur, rc_prev;
    int rc = loop_submap(h, key_cur, 0, base_key, prm.icp_leaf, h->loop.cur, &rc_cur);
    if (rc) return rc;
    if ((rc = loop_submap(h, key_pre, prm.search_num, base_key, prm.icp_leaf, h->loop.prev, &rc_prev))) return rc;
    out->n_cur = (int32_t)rc_cur.n_out;
    out->n_prev = (int32_t)rc_prev.n_out;
    if (rc_cur.n_out < 300 || rc_prev.n_out < 1000) { out->status = S2M_LOOP_TOO_FEW_POINTS; return S2M_OK; }
    // s2m_icp_align's path on the device submaps: historyKeyframeSearchRadius*2 (a float), 100, 1e-6, 1e-6 (:572-576)
    const IcpParams ip{ (double)(prm.search_radius * 2.0f), 100, 1e-6, 1e-6 };
    IcpResult r;
    hipError_t e = icp_align(h->loop.icp, h->stream, h->loop.cur.as<unsigned char>(), rc_cur.n_out, h->loop.prev.as<unsigned char>(),
                             rc_prev.n_out, kDsStride, ip, &r);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "loop ICP alignment", e);
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    icp_result_out(r, &out->icp);
    if (!r.converged || r.fitness > (double)prm.fitness_score) { out->status = S2M_LOOP_REJECTED; return S2M_OK; }   // (:585)
    if (base_key == -1) {
        float t_correct[12];                                // correctionLidarFrame * tWrong (:597-601)
        host_affine_mul(r.T, h->kf.frame[(size_t)key_cur].T, t_correct);
        host_translation_and_euler(t_correct, 4, out->pose_from);
        memcpy(out->pose_to, &h->kf.pose[6 * (size_t)key_pre], sizeof(out->pose_to));
    } else {
        host_translation_and_euler(r.T, 4, out->pose_from);  // (:707); poseTo is the identity (:709)
    }
    out->status = S2M_LOOP_ACCEPTED;
    h->loop.index[key_cur] = key_pre;                       // loopIndexContainer[loopKeyCur] = loopKeyPre (:621)
    return S2M_OK;
}

bool loop_key_ok(int32_t k, size_t N) { return k >= 0 && (size_t)k < N; }

}  // namespace

int s2m_loop_near_keyframes(s2m_handle h, int32_t key, int32_t search_num, int32_t loop_index, float leaf,
                            void* out, size_t out_stride_bytes, size_t cap, size_t* n_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!n_out || bad_out(out, out_stride_bytes, cap)) return fail(h, S2M_ERR_INVALID_ARG, "bad output buffer");
    *n_out = 0;
    int rc = check_leaf(h, leaf);
    if (rc) return rc;
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

int s2m_loop_align(s2m_handle h, int32_t key_cur, int32_t key_pre, int32_t base_key, const s2m_loop_params* p, s2m_loop_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    loop_result_init(out);
    s2m_loop_params prm;
    int rc = loop_params(h, p, &prm);
    if (rc) return rc;
    const size_t N = h->kf.time.size();
    if (N == 0) return S2M_OK;                             // cloudKeyPoses3D->points.empty() (:544-545, :627-628)
    if (!loop_key_ok(key_cur, N) || !loop_key_ok(key_pre, N) || (base_key != -1 && !loop_key_ok(base_key, N)))
        return fail(h, S2M_ERR_INVALID_ARG, "loop keys outside the key-frame store");
    S2M_HIP(h, hipSetDevice(h->device));
    return loop_align_impl(h, key_cur, key_pre, base_key, prm, out);
}

int s2m_loop_closure_rs(s2m_handle h, double time_cur, const s2m_loop_params* p, s2m_loop_result* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out) return fail(h, S2M_ERR_INVALID_ARG, "null loop result");
    loop_result_init(out);
    s2m_loop_params prm;
    int rc = loop_params(h, p, &prm);
    if (rc) return rc;
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
    return loop_align_impl(h, key_cur, key_pre, -1, prm, out);
}
