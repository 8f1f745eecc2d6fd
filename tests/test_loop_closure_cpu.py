"""CPU side of the loop closure against the key-frame store (include/liorf_s2m.h, s2m_loop_*): a numpy restatement of
detectLoopClosureDistance() (reference src/mapOptmization.cpp:732-765), of loopFindNearKeyframes() (:821-844) and of the
pose result of performRSLoopClosure() / performSCLoopClosure() (:597-606, :707-709), pins of it, the expected result of a
small scripted revisit from the oracle, and the ABI checks that need no GPU.
The GPU tests (test_loop_closure_gpu.py) hold the library against these functions.
"""
import ctypes as C
import os
import re

import numpy as np

from liorf_amd import s2m
from oracle import oracle as O

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _d2(a, b):
    """FLANN L2_Simple in fp32: ((dx*dx + dy*dy) + dz*dz), a: (n, 3), b: (3,)."""
    d = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def detect_loop(P, t, time_cur, R=10.0, W=30.0, variant=None):
    """(key_cur, key_pre) of detectLoopClosureDistance(), or (-1, -1) for no loop. `variant` names a plausible but wrong
    detection: "radius_le" (d2 <= R*R), "time_ge" (|dt| >= W), "first_by_index" (candidates in key order), "key_time"
    (t[N-1] instead of time_cur), "int_abs" (abs truncating |dt| to an int)."""
    P = np.asarray(P, F).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1)
    N = P.shape[0]
    if N == 0:
        return -1, -1
    d2 = _d2(P, P[N - 1])
    r2 = F(R) * F(R)
    cand = np.flatnonzero(d2 <= r2 if variant == "radius_le" else d2 < r2)
    if variant != "first_by_index":
        cand = cand[np.lexsort((cand, d2[cand]))]                  # FLANN's sorted result: ascending (d2, i)
    tc = t[N - 1] if variant == "key_time" else float(time_cur)
    W = float(F(W))
    pre = -1
    for i in cand:
        dt = abs(t[i] - tc)                                        # std::abs(double)
        if variant == "int_abs":
            dt = float(abs(int(t[i] - tc)))
        if (dt >= W) if variant == "time_ge" else (dt > W):
            pre = int(i)
            break
    if pre == -1 or pre == N - 1:
        return -1, -1
    return N - 1, pre


def near_frames(key, search_num, N, loop_index=-1):
    """loopFindNearKeyframes' frame list: [(keyNear, key whose pose transforms it)] in i order."""
    out = []
    for i in range(-search_num, search_num + 1):
        k = key + i
        if 0 <= k < N:
            out.append((k, loop_index if loop_index != -1 else k))
    return out


def near_submap(clouds, poses, key, search_num, loop_index, leaf):
    """The submap restated with the oracle: transformPointCloud of every frame, concatenated, VoxelGrid."""
    fr = near_frames(key, search_num, len(clouds), loop_index)
    parts = [O.transform_point_cloud(clouds[k], poses[p]) for k, p in fr if len(clouds[k])]
    if not parts:
        return np.zeros((0, 8), F)
    out, _ = O.voxel_grid(np.concatenate(parts), leaf)
    return out


def transformation64(pose_xyzrpy):
    """pcl::getTransformation in float64 (4x4)."""
    x, y, z, r, p, w = [float(v) for v in pose_xyzrpy]
    A, B, Cc, D, E, Fs = np.cos(w), np.sin(w), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    return np.array([[A * Cc, A * D * Fs - B * E, B * Fs + A * D * E, x],
                     [B * Cc, A * E + B * D * Fs, B * D * E - A * Fs, y],
                     [-D, Cc * Fs, Cc * E, z],
                     [0, 0, 0, 1.0]])


def translation_and_euler64(T):
    """pcl::getTranslationAndEulerAngles: x, y, z, roll, pitch, yaw."""
    T = np.asarray(T, np.float64)
    return np.array([T[0, 3], T[1, 3], T[2, 3], np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0])])


def pose_from64(icp_T, pose_cur=None):
    """RS (pose_cur given): of correction * tWrong (:597-604); SC: of the correction (:707)."""
    T = np.asarray(icp_T, np.float64).reshape(4, 4)
    return translation_and_euler64(T if pose_cur is None else T @ transformation64(pose_cur))


# ---- a scripted revisit -------------------------------------------------------------------------------------

def scene(seed=0):
    """Ground, four walls and a few poles in a 80 m square: enough structure for ICP to fix all six degrees."""
    rng = np.random.default_rng(seed)
    parts = [np.c_[rng.uniform(-40, 40, (12000, 2)), rng.normal(0, 0.01, 12000)]]
    for s in (-1, 1):
        parts.append(np.c_[np.full(3000, 30.0 * s), rng.uniform(-30, 30, 3000), rng.uniform(0, 6, 3000)])
        parts.append(np.c_[rng.uniform(-30, 30, 3000), np.full(3000, 30.0 * s), rng.uniform(0, 6, 3000)])
    for c in rng.uniform(-25, 25, (12, 2)):
        a = rng.uniform(0, 2 * np.pi, 300)
        parts.append(np.c_[c[0] + 0.3 * np.cos(a), c[1] + 0.3 * np.sin(a), rng.uniform(0, 4, 300)])
    return np.concatenate(parts)


def local_cloud(world, true_pose, reach=25.0):
    """The points within `reach` of the key, in the key's frame (PointXYZI records)."""
    T = transformation64(true_pose)
    w = world[np.linalg.norm(world[:, :2] - np.asarray(true_pose[:2], np.float64), axis=1) < reach]
    loc = (w - T[:3, 3]) @ T[:3, :3]
    rec = np.zeros((loc.shape[0], 8), F)
    rec[:, :3] = loc
    rec[:, 3] = 1.0
    rec[:, 4] = np.arange(loc.shape[0]) % 7
    return rec


REVISIT_DRIFT = np.array([0.35, -0.25, 0.05, 0.0, 0.0, 0.03])


def scripted_revisit(n=32, radius=20.0, seed=0):
    """n keys 1 s apart on a circle that ends where it started; the last key's stored pose carries REVISIT_DRIFT.
    Returns (clouds, stored poses (float32, x y z roll pitch yaw), times, true poses)."""
    world = scene(seed)
    a = 2 * np.pi * np.arange(n) / (n - 1)
    true = np.c_[radius * np.cos(a) - radius, radius * np.sin(a), np.zeros(n), np.zeros(n), np.zeros(n), a + np.pi / 2]
    true[-1, 5] = true[0, 5]
    clouds = [local_cloud(world, p) for p in true]
    stored = true.copy()
    stored[-1] += REVISIT_DRIFT
    return clouds, stored.astype(F), np.arange(n, dtype=np.float64), true


def expected_loop(clouds, poses, times, time_cur, R=15.0, W=30.0, search_num=25, leaf=0.5, fitness=0.3, base_key=-1):
    """The LoopResult of performRSLoopClosure (base_key -1) restated with the oracle: a dict."""
    kc, kp = detect_loop(poses[:, :3], times, time_cur, R, W)
    out = dict(status=s2m.S2M_LOOP_NONE, key_cur=kc, key_pre=kp, n_cur=0, n_prev=0)
    if kp == -1:
        return out
    cur = near_submap(clouds, poses, kc, 0, base_key, leaf)
    prev = near_submap(clouds, poses, kp, search_num, base_key, leaf)
    out.update(n_cur=cur.shape[0], n_prev=prev.shape[0], cur=cur, prev=prev)
    if cur.shape[0] < 300 or prev.shape[0] < 1000:
        out["status"] = s2m.S2M_LOOP_TOO_FEW_POINTS
        return out
    T, conv, fit, its = O.icp_align(cur, prev, max_corr_dist=float(F(R) * F(2)), max_iter=100)
    out.update(T=T, converged=conv, fitness=fit, iterations=its)
    if not conv or fit > float(F(fitness)):
        out["status"] = s2m.S2M_LOOP_REJECTED
        return out
    out["status"] = s2m.S2M_LOOP_ACCEPTED
    out["pose_from"] = pose_from64(T, poses[kc] if base_key == -1 else None)
    out["pose_to"] = poses[kp] if base_key == -1 else np.zeros(6, F)
    return out


# ---- pins of the restatement ------------------------------------------------------------------------------

def test_key_exactly_on_the_radius_is_excluded():
    P = [[10.0, 0, 0], [0, 0, 0]]
    assert detect_loop(P, [0, 100], 100.0) == (-1, -1)
    assert detect_loop(P, [0, 100], 100.0, variant="radius_le") == (1, 0)
    P = [[float(np.nextafter(F(10), F(0))), 0, 0], [0, 0, 0]]
    assert detect_loop(P, [0, 100], 100.0) == (1, 0)


def test_equidistant_candidates_go_to_the_lower_id():
    P = [[0, 3.0, 0], [3.0, 0, 0], [0, -3.0, 0], [0, 0, 0]]
    assert detect_loop(P, [0, 0, 0, 100], 100.0) == (3, 0)
    P = [[5.0, 0, 0], [0, 3.0, 0], [3.0, 0, 0], [0, 0, 0]]
    assert detect_loop(P, [0, 0, 0, 100], 100.0) == (3, 1)                            # nearest first, then lower id
    assert detect_loop(P, [0, 0, 0, 100], 100.0, variant="first_by_index") == (3, 0)


def test_time_window_is_strict_and_abs_is_the_double_overload():
    P = [[1.0, 0, 0], [2.0, 0, 0], [0, 0, 0]]
    assert detect_loop(P, [70.0, 0.0, 100.0], 100.0) == (2, 1)                        # |dt| == 30 excluded, 100 selected
    assert detect_loop(P, [70.0, 0.0, 100.0], 100.0, variant="time_ge") == (2, 0)
    # |dt| = W + 0.5: selected; an int abs would truncate it to 30 and refuse it
    assert detect_loop(P, [69.5, 99.0, 100.0], 100.0) == (2, 0)
    assert detect_loop(P, [69.5, 99.0, 100.0], 100.0, variant="int_abs") == (-1, -1)


def test_time_cur_earlier_than_the_key_times():
    P = [[1.0, 0, 0], [2.0, 0, 0], [0, 0, 0]]
    assert detect_loop(P, [100.0, 40.0, 20.0], 5.0) == (2, 0)                         # |100 - 5| > 30
    assert detect_loop(P, [100.0, 40.0, 20.0], 45.0) == (2, 0)
    assert detect_loop(P, [30.0, 40.0, 20.0], 5.0) == (2, 1)                          # 35 > 30; key 0: 25
    assert detect_loop(P, [30.0, 40.0, 20.0], 5.0, variant="key_time") == (-1, -1)    # from t[N-1] = 20 nothing is 30 s away


def test_nearest_passing_candidate_being_the_current_key_gives_no_loop():
    P = [[1.0, 0, 0], [0, 0, 0]]
    assert detect_loop(P, [0.0, 0.0], 100.0) == (-1, -1)        # key 1 (d2 0) passes first: loopKeyCur == loopKeyPre
    assert detect_loop(P, [0.0, 0.0], 10.0) == (-1, -1)         # nothing passes


def test_near_frames_clip_and_loop_index():
    assert near_frames(1, 3, 5) == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    assert near_frames(0, 2, 5) == [(0, 0), (1, 1), (2, 2)]
    assert near_frames(4, 2, 5) == [(2, 2), (3, 3), (4, 4)]
    assert near_frames(4, 0, 5) == [(4, 4)]
    assert near_frames(3, 1, 5, loop_index=0) == [(2, 0), (3, 0), (4, 0)]


# Boundary stores (R 10, W 30), each with the query times at which it is read. The newest key sits at the origin.
BOUNDARY = [
    # key 0 passes but is far, key 1 sits exactly on the radius, key 2 is exactly W away at 100, key 3 passes at 5 m
    ([[7.0, 0, 0], [10.0, 0, 0], [3.0, 0, 0], [5.0, 0, 0], [0, 0, 0]], [0.0, 0.0, 70.0, 160.0, 100.0], [100.0, 107.0, 40.0]),
    # only the key on the radius would pass
    ([[10.0, 0, 0], [4.0, 0, 0], [0, 0, 0]], [0.0, 95.0, 100.0], [100.0, 99.5]),
]


def test_boundary_stores_tell_the_wrong_variants_apart():
    told = set()
    for P, t, tcs in BOUNDARY:
        for tc in tcs:
            right = detect_loop(P, t, tc)
            for v in ("radius_le", "time_ge", "first_by_index", "key_time"):
                if detect_loop(P, t, tc, variant=v) != right:
                    told.add(v)
    assert told == {"radius_le", "time_ge", "first_by_index", "key_time"}
    P, t, _ = BOUNDARY[0]
    assert detect_loop(P, t, 100.0) == (4, 3) and detect_loop(P, t, 107.0) == (4, 2)
    assert detect_loop(*BOUNDARY[1][:2], 100.0) == (-1, -1)


def test_pose_composition_of_an_exact_correction():
    pose = np.array([1.0, 2.0, 0.5, 0.01, -0.02, 0.3])
    C_ = transformation64([0.2, -0.1, 0.0, 0.0, 0.0, -0.05])
    got = pose_from64(C_, pose)
    want = translation_and_euler64(C_ @ transformation64(pose))
    assert np.allclose(got, want)
    assert np.allclose(pose_from64(np.eye(4), pose), pose)                              # identity correction: the pose itself
    assert np.allclose(pose_from64(C_), [0.2, -0.1, 0.0, 0.0, 0.0, -0.05])               # SC: the correction's own pose


def test_scripted_revisit_expected_result():
    clouds, poses, times, true = scripted_revisit()
    e = expected_loop(clouds, poses, times, times[-1], R=15.0, search_num=2, leaf=0.5)
    assert (e["key_cur"], e["key_pre"]) == (len(clouds) - 1, 0)
    assert e["status"] == s2m.S2M_LOOP_ACCEPTED and e["converged"]
    assert e["n_cur"] >= 300 and e["n_prev"] >= 1000
    # the correction takes the drifted pose of the last key back to its true pose
    assert np.abs(e["pose_from"][:3] - true[-1, :3]).max() < 0.05
    assert abs(e["pose_from"][5] - true[-1, 5]) < 0.005
    assert np.array_equal(e["pose_to"], poses[0])


def test_revisit_submap_uses_loop_index_pose():
    clouds, poses, times, _ = scripted_revisit(n=8)
    a = near_submap(clouds, poses, 3, 1, 0, 0.5)
    b = np.concatenate([O.transform_point_cloud(clouds[k], poses[0]) for k in (2, 3, 4)])
    assert np.array_equal(a, O.voxel_grid(b, 0.5)[0])


# ---- ABI checks without a GPU -----------------------------------------------------------------------------

NEW = ["s2m_loop_default_params", "s2m_loop_near_keyframes", "s2m_loop_align", "s2m_loop_closure_rs"]


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liorf_s2m.h")).read(), flags=re.S)
    lib = C.CDLL(s2m.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in s2m.ABI_SYMBOLS
        assert hasattr(lib, n)
    assert C.sizeof(s2m.LoopResult) == 152


def test_loop_default_params_are_the_reference_constants():
    p = s2m.default_loop_params()
    assert (p.search_radius, p.time_diff_s, p.search_num) == (10.0, 30.0, 25)
    assert p.fitness_score == F(0.3) and p.icp_leaf == F(0.3)
    assert s2m.load_library().s2m_loop_default_params(None) == -1


def test_null_handle_calls_are_rejected():
    lib = s2m.load_library()
    r = s2m.LoopResult()
    n = C.c_size_t(7)
    out = (C.c_float * 8)()
    assert lib.s2m_loop_closure_rs(None, 0.0, None, C.byref(r)) == -1
    assert lib.s2m_loop_align(None, 0, 0, -1, None, C.byref(r)) == -1
    assert lib.s2m_loop_near_keyframes(None, 0, 0, -1, 0.3, out, 32, 1, C.byref(n)) == -1
