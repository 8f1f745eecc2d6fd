"""CPU side of the resident key-frame store (include/liorf_s2m.h, s2m_kf_* / s2m_extract_surrounding): a numpy
restatement of extractSurroundingKeyFrames()'s selection (reference src/mapOptmization.cpp:1046-1059 -> extractNearby
:975-1010 -> extractCloud :1012-1044), hand-built pins of it, and the ABI checks that need no GPU.
The GPU tests (test_keyframes_gpu.py) hold the library's key lists against select_surrounding().
"""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m
from oracle import oracle as O

F = np.float32


def _d2(a, b):
    """FLANN L2_Simple in fp32: ((dx*dx + dy*dy) + dz*dz), a: (n, 3), b: (3,)."""
    d = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def select_surrounding(P, t, time_cur, R=50.0, D=1.0, W=10.0, variant=None):
    """Key ids concatenated into the local map, in order: (b) radius search, (c) VoxelGrid of the key positions,
    (d) nearest key of every centroid, (e) recent keys, (f) distance filter (centroid for (d), key pose for (e)).
    `variant` gives two plausible but wrong selections, used to show that a test input tells them apart:
    "filter_at_key" tests the chosen key's pose in (f), "nn_among_candidates" runs (d) over the radius candidates only."""
    P = np.asarray(P, F).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1)
    N = P.shape[0]
    if N == 0:
        return []
    q = P[N - 1]
    R = F(R)
    d2 = _d2(P, q)
    cand = np.flatnonzero(d2 < R * R)                               # (b) strict '<' against (float)(R*R)
    order = cand[np.lexsort((cand, d2[cand]))]                      # ascending (d2, i)
    entries = []                                                     # (key, point tested by (f))
    if order.size:
        rec = np.zeros((order.size, 8), F)
        rec[:, :3] = P[order]
        rec[:, 3] = 1.0
        rec[:, 4] = order.astype(F)                                 # intensity = key id
        cents, _ = O.voxel_grid(rec, float(D))                      # (c), leaf-too-small: input unchanged
        pool = np.sort(order) if variant == "nn_among_candidates" else np.arange(N)
        for c in cents[:, :3]:
            k = int(pool[np.argmin(_d2(P[pool], c))])               # (d) over all N keys; argmin: lower index on ties
            entries.append((k, P[k] if variant == "filter_at_key" else c))
    for i in range(N - 1, -1, -1):                                  # (e)
        if not (time_cur - t[i] < W):
            break
        entries.append((i, P[i]))
    keys = []
    for k, x in entries:                                             # (f) pointDistance(x, P[N-1]) > R: dropped
        d = (np.asarray(x, F) - q).astype(F)
        if not (np.sqrt(F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) > R):
            keys.append(k)
    return keys


# ---- pins of the restatement ------------------------------------------------------------------------

def test_key_exactly_on_the_radius_is_excluded():
    P = [[50.0, 0, 0], [0, 0, 0]]
    assert select_surrounding(P, [0, 0], 100.0, R=50.0) == [1]
    P = [[np.nextafter(F(50), F(0)), 0, 0], [0, 0, 0]]
    assert select_surrounding(P, [0, 0], 100.0, R=50.0) == [1, 0]       # two voxels, ascending index


def test_equidistant_keys_go_to_the_lower_id():
    # one voxel of leaf 10 holding all three; centroid (5, 5, 6) is d2 = 2 from keys 0 and 1, 4 from key 2
    P = [[4.0, 5, 5], [6.0, 5, 5], [5.0, 5, 8]]
    assert select_surrounding(P, [0, 0, 0], 100.0, D=10.0) == [0]
    P = [[6.0, 5, 5], [4.0, 5, 5], [5.0, 5, 8]]
    assert select_surrounding(P, [0, 0, 0], 100.0, D=10.0) == [0]


def test_recent_key_chosen_twice():
    assert select_surrounding([[1.0, 2, 3]], [5.0], 6.0) == [0, 0]


def test_recent_window_is_strict_and_stops_at_the_first_failure():
    P = [[0.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0]]
    keys = select_surrounding(P, [15.0, 10.0, 12.0], 20.0, D=1.0)
    assert keys == [0, 1, 2, 2]                 # three voxels, then key 2 (8 s); key 1 is exactly 10.0 s old: stop


def boundary_store(n=3000, seed=2, R=50.0):
    """Keys on a shell from R - 3 to R + 1 around the newest key (at the origin): voxels of leaf 4 straddle the sphere,
    so some centroids inside R have their nearest key outside R (no radius candidate, its own pose beyond R)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    P = (v * rng.uniform(R - 3.0, R + 1.0, (n, 1))).astype(F)
    P[-1] = 0
    return P, np.zeros(n)


BOUNDARY_D = 4.0


def test_boundary_store_tells_the_wrong_variants_apart():
    P, t = boundary_store()
    right = select_surrounding(P, t, 100.0, D=BOUNDARY_D)
    assert select_surrounding(P, t, 100.0, D=BOUNDARY_D, variant="filter_at_key") != right
    assert select_surrounding(P, t, 100.0, D=BOUNDARY_D, variant="nn_among_candidates") != right


def test_distance_filter_tests_the_centroid_not_the_key():
    # keys 0, 1 within R = 10 share a voxel; their centroid (9.9, 0.3, 0) is nearest to key 2, which lies beyond R
    P = [[9.9, 0.0, 0], [9.9, 0.6, 0], [10.05, 0.3, 0], [0.0, 0, 0]]
    keys = select_surrounding(P, [0, 0, 0, 0], 100.0, R=10.0, D=1.0)
    assert keys == [3, 2]                       # kept on the centroid's distance (the key's own is 10.05 > R)
    # the converse for the recent keys: those are tested at their own pose, and a recent key beyond R is dropped
    keys = select_surrounding(P, [0, 0, 99.0, 99.0], 100.0, R=10.0, D=1.0)
    assert keys == [3, 2, 3]
    # the store also separates the wrong variants: key 2 is no radius candidate, and its own pose lies beyond R
    assert select_surrounding(P, [0, 0, 0, 0], 100.0, R=10.0, D=1.0, variant="filter_at_key") == [3]
    assert select_surrounding(P, [0, 0, 0, 0], 100.0, R=10.0, D=1.0, variant="nn_among_candidates") == [3, 0]
    # Not pinned: a centroid beyond R whose nearest key lies within R. The centroid of keys within R lies within R (the
    # ball is convex), so only rounding of the fp32 sum and division could move it across, and a key inside R with
    # sqrtf(d2) > R does not exist either (fl(x*x) < fl(R*R) implies sqrtf(fl(x*x)) <= R, both being monotone and
    # correctly rounded). A search over random boundary clusters found no such input.


def test_leaf_too_small_passes_the_key_poses_through():
    rng = np.random.default_rng(5)
    P = rng.uniform(-40, 40, (60, 3)).astype(F)
    P[-1] = 0
    d2 = _d2(P, P[-1])
    cand = np.flatnonzero(d2 < F(50) * F(50))
    order = cand[np.lexsort((cand, d2[cand]))]
    assert select_surrounding(P, np.zeros(60), 100.0, D=1e-6) == order.tolist()


def test_restatement_on_a_random_trajectory_is_sane():
    rng = np.random.default_rng(2)
    P = np.cumsum(rng.normal(0, 1.5, (300, 3)), 0).astype(F)
    t = np.arange(300, dtype=np.float64)
    keys = select_surrounding(P, t, 299.5, R=20.0, D=2.0)
    q = P[-1]
    recent = [i for i in range(299, 289, -1) if np.linalg.norm(P[i] - q) <= 20.0]
    assert keys and keys[len(keys) - len(recent):] == recent
    for k in keys:
        assert np.linalg.norm(P[k] - q) < 25.0


# ---- ABI checks without a GPU -------------------------------------------------------------------------

NEW = ["s2m_kf_default_params", "s2m_kf_reset", "s2m_kf_size", "s2m_kf_add", "s2m_kf_set_poses", "s2m_extract_surrounding"]


def test_new_symbols_declared_bound_and_exported():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "liorf_s2m.h")).read(), flags=re.S)
    lib = C.CDLL(s2m.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in s2m.ABI_SYMBOLS
        assert hasattr(lib, n)


def test_kf_default_params_are_the_reference_constants():
    p = s2m.default_kf_params()
    assert (p.search_radius, p.density, p.recent_window_s) == (50.0, 1.0, 10.0)
    assert p.map_leaf == F(0.2)
    assert s2m.load_library().s2m_kf_default_params(None) == -1


def test_null_handle_calls_are_rejected():
    lib = s2m.load_library()
    pose = (C.c_float * 6)()
    pts = (C.c_float * 8)()
    n_out, n_keys = C.c_size_t(7), C.c_size_t(7)
    keys = (C.c_int32 * 4)()
    assert lib.s2m_kf_reset(None) == -1
    assert lib.s2m_kf_size(None) == -1
    assert lib.s2m_kf_add(None, pose, 0.0, pts, 1, 32, s2m.S2M_KF_FROM_HOST) == -1
    assert lib.s2m_kf_add(None, None, 0.0, None, 0, 32, s2m.S2M_KF_FROM_LAST_DOWNSAMPLE) == -1
    assert lib.s2m_kf_set_poses(None, 0, 1, pose) == -1
    assert lib.s2m_extract_surrounding(None, 0.0, None, None, 32, 0, C.byref(n_out), keys, 4, C.byref(n_keys)) == -1
