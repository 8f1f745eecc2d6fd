"""Model of the relocalisation (include/liorf_s2m.h, "Relocalisation", "ICP with an initial guess", "The local map around a given
position") on the oracle: ScanContext distances, the VoxelGrid and ICP are the oracle's; the guess, the fp32 move of the source,
the composition with the guess and the judgement are restated here in numpy. Shared by test_relocalize_cpu.py and
test_relocalize_gpu.py; the expensive results are computed once per process.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import sc_query_ref as Q
from liorf_amd import s2m
from oracle import oracle as O
from test_loop_closure_cpu import local_cloud, near_submap, scene, scripted_revisit, transformation64, translation_and_euler64

F = np.float32

# the parameters of the issue's fixture
R, SEARCH_NUM, LEAF, FITNESS, TOP_K = 15.0, 2, 0.5, 0.3, 4
MAX_CORR = float(F(R) * F(2))


def rz64(a):
    c, s = np.cos(float(a)), np.sin(float(a))
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])


def guess64(pose_xyzrpy, yaw_diff_rad, use_yaw=True):
    """G = T(pose[key]) * Rz(-yaw_diff_rad) in float64 (use_yaw False: T(pose[key]))."""
    T = transformation64(pose_xyzrpy)
    return T @ rz64(-float(yaw_diff_rad)) if use_yaw else T


def move32(cloud, G):
    """The source under a guess as the library moves it: fp32, m0*x + m1*y + m2*z + m3 per row, left to right, no contraction."""
    m = np.asarray(G, F).reshape(4, 4)
    x, y, z = (np.asarray(cloud, F)[:, k] for k in range(3))
    out = np.array(cloud, F, copy=True)
    for r in range(3):
        out[:, r] = ((m[r, 0] * x + m[r, 1] * y).astype(F) + m[r, 2] * z).astype(F) + m[r, 3]
    return out


def icp_guess(src, tgt, G, max_corr_dist=MAX_CORR, max_iter=100):
    """align(output, guess) with the oracle: its ICP from the identity on the fp32-moved source, composed with G in float64.
    Returns (T 4x4 float64, converged, fitness, iterations, the oracle's own T)."""
    T, conv, fit, its = O.icp_align(move32(src, G), tgt, max_corr_dist=max_corr_dist, max_iter=max_iter)
    T = np.asarray(T, np.float64).reshape(4, 4)
    return T @ np.asarray(G, F).astype(np.float64).reshape(4, 4), bool(conv), float(fit), int(its), T


def select_at(P, c, R=50.0, D=1.0):
    """The keys of s2m_extract_surrounding_at, in order: select_global (tests/test_global_map_cpu.py) with the free centre c in
    place of P[N-1] - (b) d2(P[i], c) < (float)(R*R) in ascending (d2, i), (c) the VoxelGrid of those key poses with leaf D,
    (d) the nearest key of every centroid among all keys (ties: the lower index), (f) dropped when sqrtf(|centroid - c|^2) > R."""
    P = np.asarray(P, F).reshape(-1, 3)
    if P.shape[0] == 0:
        return []
    q = np.asarray(c, F).reshape(3)
    R = F(R)

    def d2(a, b):
        d = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
    dq = d2(P, q)
    cand = np.flatnonzero(dq < R * R)
    order = cand[np.lexsort((cand, dq[cand]))]
    if order.size == 0:
        return []
    rec = np.zeros((order.size, 8), F)
    rec[:, :3] = P[order]
    rec[:, 3] = 1.0
    rec[:, 4] = order.astype(F)
    cents, _ = O.voxel_grid(rec, float(D))
    keys = []
    for ce in cents[:, :3]:
        k = int(np.argmin(d2(P, ce)))
        d = (np.asarray(ce, F) - q).astype(F)
        if np.sqrt(F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) > R:
            continue
        keys.append(k)
    return keys


# ---- the fixture: the scripted revisit as a stored map, two query scans near key 8 ----------------------------------------

@functools.lru_cache(maxsize=None)
def revisit():
    clouds, poses, times, true = scripted_revisit()
    descs = [O.make_scancontext(c)[0] for c in clouds]
    return clouds, poses, times, true, descs


QUERY_OFFSETS = {"Q1": ((0.8, -0.5, 0.0), np.deg2rad(-90.0)), "Q2": ((1.5, 1.0, 0.0), np.deg2rad(132.0))}
TRUE_KEY = 8


@functools.lru_cache(maxsize=None)
def query_scan(name):
    """(scan records in the scan's own frame, true pose x y z roll pitch yaw float64)."""
    true = revisit()[3]
    (dx, dy, dz), dyaw = QUERY_OFFSETS[name]
    pose = true[TRUE_KEY].copy()
    pose[:3] += (dx, dy, dz)
    pose[5] += dyaw
    return local_cloud(scene(0), pose), pose


@functools.lru_cache(maxsize=None)
def model(name, use_yaw=True):
    """The relocalisation of query `name` from the oracle alone: dict(hits, records, best). A record: dict(key, status, n_src,
    n_tgt, guess (float64 4x4), T, converged, fitness, iterations, pose (x y z roll pitch yaw, accepted records))."""
    clouds, poses, _, _, descs = revisit()
    scan, _ = query_scan(name)
    hits = Q.query(descs, O.make_scancontext(scan)[0], top_k=TOP_K, align=Q.ALIGN_FULL, max_dist=0.3)
    src, _ = O.voxel_grid(scan, LEAF)
    recs = []
    for h in hits:
        key = int(h["key"])
        tgt = near_submap(clouds, poses, key, SEARCH_NUM, -1, LEAF)
        G = guess64(poses[key], h["yaw_diff_rad"], use_yaw)
        r = dict(key=key, n_src=src.shape[0], n_tgt=tgt.shape[0], guess=G, src=src, tgt=tgt)
        if src.shape[0] < 300 or tgt.shape[0] < 1000:
            r["status"] = s2m.S2M_LOOP_TOO_FEW_POINTS
        else:
            T, conv, fit, its, _ = icp_guess(src, tgt, G)
            ok = conv and not fit > float(F(FITNESS))
            r.update(T=T, converged=conv, fitness=fit, iterations=its, status=s2m.S2M_LOOP_ACCEPTED if ok else s2m.S2M_LOOP_REJECTED)
            if ok:
                r["pose"] = translation_and_euler64(T)
        recs.append(r)
    ranked = sorted((r["fitness"], i) for i, r in enumerate(recs) if r["status"] == s2m.S2M_LOOP_ACCEPTED)
    return dict(hits=hits, records=recs, best=ranked[0][1] if ranked else -1)


def pose_error(pose_xyzrpy, true_pose):
    """(position error in m, yaw error in rad) of a pose against the truth."""
    p, t = np.asarray(pose_xyzrpy, np.float64), np.asarray(true_pose, np.float64)
    dyaw = (p[5] - t[5] + np.pi) % (2 * np.pi) - np.pi
    return float(np.linalg.norm(p[:3] - t[:3])), float(abs(dyaw))
