// s2m_abi_reloc.hip — C ABI of the relocalisation: a scan that is no key, or a stored key, against the stored map (place query,
// guessed alignment of its hits in lockstep).  Host orchestration only; the submaps, the parameters and the list of alignments
// are the loop closure's (s2m_abi_loop.hip, declared in s2m_context.hpp).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "s2m_context.hpp"

using namespace s2m;
using namespace s2m::host;

int s2m_reloc_default_params(s2m_reloc_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    s2m_sc_query_default_params(&p->query);
    p->query.top_k = 4;
    p->query.align = S2M_SC_ALIGN_FULL;
    s2m_loop_default_params(&p->loop);
    p->use_yaw = 1;
    return S2M_OK;
}

namespace {

int reloc_args(s2m_context* h, int64_t n_sc, int64_t n_kf, const s2m_reloc_params* p, s2m_reloc_params* prm)
{
    if (p) *prm = *p; else s2m_reloc_default_params(prm);
    if (n_sc < 0 || n_kf < 0 || n_sc > INT32_MAX) return fail(h, S2M_ERR_INVALID_ARG, "relocalisation: a negative store size");
    if (prm->query.top_k < 1 || prm->query.top_k > S2M_LOOP_MAX_CANDIDATES)
        return fail(h, S2M_ERR_INVALID_ARG, "a relocalisation aligns the top 1 .. S2M_LOOP_MAX_CANDIDATES hits");
    if (s2m_sc_query_check_args((int32_t)n_sc, &prm->query) != S2M_OK)
        return fail(h, S2M_ERR_INVALID_ARG, "relocalisation: the query's align, max_dist or range is invalid");
    s2m_loop_params lp;
    const int rc = loop_params(h, &prm->loop, &lp);
    return rc;
}

// G = T(pose[key]) * Rz(-yaw): the key's stored 3x4 times the turn that takes a query point back onto the candidate's (the
// descriptor's shift says query ~ Rz(+yaw) * candidate), in float, each entry ((a0 b0 + a1 b1) + a2 b2)
void reloc_guess(const float T_key[12], float yaw_diff_rad, bool use_yaw, float G[16])
{
    const float a = use_yaw ? -yaw_diff_rad : 0.0f;
    const float c = cosf(a), s = sinf(a);
    const float Rz[12] = { c, -s, 0.0f, 0.0f,   s, c, 0.0f, 0.0f,   0.0f, 0.0f, 1.0f, 0.0f };
    if (use_yaw) host_affine_mul(T_key, Rz, G); else memcpy(G, T_key, sizeof(float) * 12);
    G[12] = G[13] = G[14] = 0.0f; G[15] = 1.0f;
}

// Steps 2 to 6 of a relocalisation, from the query's hits on: the source (n records on the device, in their own frame) through the
// VoxelGrid, a target submap - its neighbours inside [clamp_lo, clamp_hi), see loop_submap - and a guess per hit, the alignments in
// lockstep, the gates, both pose forms and *best.
int reloc_from_hits(s2m_context* h, const s2m_reloc_params& prm, const unsigned char* d_pts, size_t n, size_t stride_bytes, const s2m_sc_hit* hits,
                    int32_t n_hits, long long clamp_lo, long long clamp_hi, s2m_reloc_candidate* out, int32_t* n_out, int32_t* best)
{
    int rc;
    s2m_context::LoopClosure& L = h->loop;
    if (n_hits == 0) return S2M_OK;
    const size_t N = h->kf.time.size();
    for (int32_t i = 0; i < n_hits; i++)
        if (!loop_key_ok(hits[i].key, N))
            return fail(h, S2M_ERR_INVALID_ARG, "relocalisation: a hit names a key the key-frame store does not hold (the two stores are out of step)");
    // 2. the source: the scan in its own frame through the VoxelGrid at icp_leaf, once, into the loop's source buffer
    VoxResult vs;
    if ((rc = voxel_into(h, d_pts, n, stride_bytes, prm.loop.icp_leaf, L.cur, &vs))) return rc;
    // 3. + 4. a target submap and a guess per hit; the size gates decide who takes a slot
    IcpList al(IcpForm::kSlots, kDsStride);
    for (int32_t i = 0; i < n_hits; i++) {
        s2m_reloc_candidate& c = out[i];
        memset(&c, 0, sizeof(c));
        c.hit = hits[i];
        c.icp.T[0] = c.icp.T[5] = c.icp.T[10] = c.icp.T[15] = 1.0f;
        c.n_src = (int32_t)vs.n_out;
        reloc_guess(h->kf.frame[(size_t)hits[i].key].T, hits[i].yaw_diff_rad, prm.use_yaw != 0, c.guess);
        c.status = S2M_LOOP_TOO_FEW_POINTS;
        if (vs.n_out < 300) continue;
        VoxResult vt;
        if ((rc = loop_submap(h, hits[i].key, prm.loop.search_num, -1, prm.loop.icp_leaf, L.target(i), &vt, clamp_lo, clamp_hi))) return rc;
        c.n_tgt = (int32_t)vt.n_out;
        if (vt.n_out < 1000) continue;
        if ((rc = guess_ok(h, c.guess))) return rc;
        c.status = S2M_LOOP_NONE;
        al.add(L.cur.p, vs.n_out, L.target(i).p, vt.n_out, c.guess, (size_t)i);
    }
    *n_out = n_hits;
    if (!al.n) return S2M_OK;
    // 5. the alignments in lockstep on the device loop, waited for
    if ((rc = icp_list_align(h, h->stream, al, loop_icp_params(prm.loop), prm.loop.icp_leaf, "relocalisation ICP"))) return rc;
    // 6. the fitness gate, both pose forms, the best record by (fitness, position)
    for (int k = 0; k < al.n; k++) {
        const int32_t i = (int32_t)al.who[k];
        s2m_reloc_candidate& c = out[i];
        const IcpResult& ri = al.res[k];
        icp_result_out(ri, &c.icp);
        if (!ri.converged || ri.fitness > (double)prm.loop.fitness_score) { c.status = S2M_LOOP_REJECTED; continue; }
        c.status = S2M_LOOP_ACCEPTED;
        host_translation_and_euler(ri.T, 4, c.pose_xyzrpy);
        for (int a = 0; a < 3; a++) { c.pose_tobemapped[a] = c.pose_xyzrpy[3 + a]; c.pose_tobemapped[3 + a] = c.pose_xyzrpy[a]; }
        if (*best < 0 || c.icp.fitness_score < out[*best].icp.fitness_score) *best = i;
    }
    return S2M_OK;
}

}  // namespace

int s2m_relocalize_check_args(int32_t n_sc, int32_t n_kf, const s2m_reloc_params* p)
{
    s2m_reloc_params prm;
    return reloc_args(nullptr, n_sc, n_kf, p, &prm);
}

int s2m_relocalize_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes, int on_device, const s2m_reloc_params* p,
                        s2m_reloc_candidate* out, int32_t* n_out, int32_t* best)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out || !n_out || !best) return fail(h, S2M_ERR_INVALID_ARG, "null relocalisation outputs");
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if ((rc = loop_busy(h))) return rc;
    *n_out = 0; *best = -1;
    s2m_reloc_params prm;
    if ((rc = reloc_args(h, (int64_t)h->sc.n, (int64_t)h->kf.time.size(), p, &prm))) return rc;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    s2m_context::LoopClosure& L = h->loop;
    // the scan in the loop's staging buffer (a host scan), where the query's descriptor and the source filter both read it
    const unsigned char* d_pts = static_cast<const unsigned char*>(pts);
    if (!on_device) {
        if ((rc = stage_host_records(h, L.icp_src, pts, n * stride_bytes))) return rc;
        d_pts = L.icp_src.as<unsigned char>();
    }
    // 1. the query: s2m_sc_query_scan's hits
    s2m_sc_hit hits[S2M_LOOP_MAX_CANDIDATES];
    int32_t n_hits = 0;
    if ((rc = sc_query_device_scan(h, d_pts, n, stride_bytes, &prm.query, hits, &n_hits))) return rc;
    return reloc_from_hits(h, prm, d_pts, n, stride_bytes, hits, n_hits, 0, -1, out, n_out, best);
}

int s2m_relocalize_key(s2m_handle h, int32_t key, const s2m_reloc_params* p, s2m_reloc_candidate* out, int32_t* n_out, int32_t* best)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!out || !n_out || !best) return fail(h, S2M_ERR_INVALID_ARG, "null relocalisation outputs");
    int rc = loop_busy(h);
    if (rc) return rc;
    *n_out = 0; *best = -1;
    s2m_reloc_params prm;
    if ((rc = reloc_args(h, (int64_t)h->sc.n, (int64_t)h->kf.time.size(), p, &prm))) return rc;
    if (key < 0 || (size_t)key >= h->kf.time.size() || (size_t)key >= h->sc.n)
        return fail(h, S2M_ERR_INVALID_ARG, "relocalisation: the key is outside the key-frame store or has no descriptor");
    const KfFrame& f = h->kf.frame[(size_t)key];
    if (f.n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    // 1. the query: the key's stored descriptor against the searched range
    s2m_sc_hit hits[S2M_LOOP_MAX_CANDIDATES];
    int32_t n_hits = 0;
    if ((rc = s2m_sc_query_key(h, key, &prm.query, hits, &n_hits))) return rc;
    // 2 .. 6 with the key's own records, straight from the arena, as the source, and submaps that stay inside the searched range
    const long long lo = prm.query.first, hi = prm.query.count < 0 ? (long long)h->sc.n : lo + prm.query.count;
    return reloc_from_hits(h, prm, f.src, (size_t)f.n, kDsStride, hits, n_hits, lo, hi, out, n_out, best);
}
