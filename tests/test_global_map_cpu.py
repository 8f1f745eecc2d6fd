"""CPU side of s2m_global_map / s2m_kf_map_cloud (include/liorf_s2m.h): a numpy restatement of publishGlobalMap()'s selection
(reference src/mapOptmization.cpp:453-502), a boundary store it tells apart from plausible wrong variants, and the ABI checks
that need no GPU. The GPU tests (test_global_map_gpu.py) hold the library's key lists against select_global().
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


def select_global(P, R=1e3, D=10.0, variant=None):
    """Key ids concatenated into globalMapKeyFrames, in order (:463-496):
    radiusSearch(cloudKeyPoses3D->back(), R) -> ascending (d2, i) with d2 < (float)(R*R);
    VoxelGrid of those key poses with leaf D (intensity = key id; leaf too small: the poses unchanged);
    nearestKSearch(centroid, 1) over all keys (equal distances: the lower index);
    pointDistance(centroid, back()) > R: dropped.
    Wrong variants, used to show that a store tells them apart:
      "nn_among_candidates"  the nearest key among the radius candidates only
      "filter_at_key"        the distance test at the chosen key instead of the centroid
      "filter_ge"            a centroid at exactly R dropped too
      "ties_to_higher"       equal distances to the higher index."""
    P = np.asarray(P, F).reshape(-1, 3)
    N = P.shape[0]
    if N == 0:
        return []
    q = P[N - 1]
    R = F(R)
    d2 = _d2(P, q)
    cand = np.flatnonzero(d2 < R * R)
    order = cand[np.lexsort((cand, d2[cand]))]
    rec = np.zeros((order.size, 8), F)
    rec[:, :3] = P[order]
    rec[:, 3] = 1.0
    rec[:, 4] = order.astype(F)
    cents, _ = O.voxel_grid(rec, float(D))
    pool = np.sort(order) if variant == "nn_among_candidates" else np.arange(N)
    keys = []
    for c in cents[:, :3]:
        dd = _d2(P[pool], c)
        if variant == "ties_to_higher":
            k = int(pool[len(dd) - 1 - int(np.argmin(dd[::-1]))])
        else:
            k = int(pool[np.argmin(dd)])
        x = P[k] if variant == "filter_at_key" else c
        d = (np.asarray(x, F) - q).astype(F)
        dist = np.sqrt(F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if (dist >= R) if variant == "filter_ge" else (dist > R):
            continue
        keys.append(k)
    return keys


# ---- the boundary store -----------------------------------------------------------------------------------

AT_R = (F(9.999999), F(0.001954))       # fp32 d2 = pred(100) < 10*10, and sqrtf of it rounds to 10.0 exactly
BOUNDARY_R, BOUNDARY_D = 10.0, 1.0


def boundary_store():
    """Around the newest key (the origin), R = 10, D = 1:
      key 0       alone in its voxel at sqrtf distance exactly R: a radius candidate whose centroid is itself, kept by '> R'
      keys 1..3   three keys at one position (equal d2, one voxel): the centroid's nearest key is the lowest of them
      keys 4, 5   one voxel inside R whose centroid (-9.9, 0.3, 0) is nearest to key 6
      key 6       (-10.05, 0.3, 0): beyond R, no candidate; its own pose fails the distance test, the centroid passes it
      key 7       the newest key"""
    P = np.array([[AT_R[0], AT_R[1], 0.0],
                  [3.3, 4.4, -1.2], [3.3, 4.4, -1.2], [3.3, 4.4, -1.2],
                  [-9.9, 0.0, 0.0], [-9.9, 0.6, 0.0], [-10.05, 0.3, 0.0],
                  [0.0, 0.0, 0.0]], F)
    return P


def test_boundary_store_pins_the_rules():
    P = boundary_store()
    d2 = _d2(P, P[-1])
    assert d2[0] < F(100) and np.sqrt(d2[0]) == F(10)
    keys = select_global(P, R=BOUNDARY_R, D=BOUNDARY_D)
    assert 0 in keys                                   # a centroid exactly at R is kept
    assert 1 in keys and 2 not in keys and 3 not in keys
    assert 6 in keys and 4 not in keys and 5 not in keys
    assert sorted(keys) == [0, 1, 6, 7]


def test_boundary_store_tells_the_wrong_variants_apart():
    P = boundary_store()
    right = select_global(P, R=BOUNDARY_R, D=BOUNDARY_D)
    for v in ("nn_among_candidates", "filter_at_key", "filter_ge", "ties_to_higher"):
        assert select_global(P, R=BOUNDARY_R, D=BOUNDARY_D, variant=v) != right, v


def test_global_selection_is_the_surrounding_one_without_recent_keys():
    from test_keyframes_cpu import select_surrounding
    rng = np.random.default_rng(3)
    P = np.cumsum(rng.normal(0, 2.0, (400, 3)) * [1, 1, 0.1], 0).astype(F)
    for R, D in ((1e3, 10.0), (1e3, 3.0), (30.0, 2.0)):
        # a time window that no key passes: (e) adds nothing
        assert select_global(P, R=R, D=D) == select_surrounding(P, np.zeros(400), 1e9, R=R, D=D, W=10.0)


def test_all_candidate_store_and_leaf_too_small():
    ang = np.arange(5000) * 0.05
    P = np.c_[20 * np.cos(ang), 20 * np.sin(ang), np.zeros(5000)].astype(F)
    keys = select_global(P, R=1e3, D=3.0)
    assert len(keys) == len(set(keys)) and 0 < len(keys) < 5000
    # a pose density far too small for the extent: the key poses pass through, every candidate in (d2, i) order is chosen
    d2 = _d2(P, P[-1])
    order = np.lexsort((np.arange(5000), d2))
    P2 = P.copy()
    P2[:, 2] = np.linspace(-1e4, 1e4, 5000)
    keys2 = select_global(P2, R=1e5, D=1e-4)
    order2 = np.lexsort((np.arange(5000), _d2(P2, P2[-1])))
    assert keys2 == order2.tolist()
    assert order.size == 5000


def test_empty_and_single_key():
    assert select_global(np.zeros((0, 3))) == []
    assert select_global([[1.0, 2.0, 3.0]]) == [0]


# ---- ABI checks without a GPU -------------------------------------------------------------------------

NEW = {"s2m_gmap_default_params": 1, "s2m_global_map": 9, "s2m_kf_map_cloud": 8}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liorf_s2m.h")).read(), flags=re.S)


def test_new_symbols_declared_bound_and_exported():
    txt = _header()
    lib = s2m.load_library()
    raw = C.CDLL(s2m.LIB_PATH)
    for n, nargs in NEW.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        assert m.group(1).count(",") + 1 == nargs, n
        assert n in s2m.ABI_SYMBOLS
        assert hasattr(raw, n)
        assert len(getattr(lib, n).argtypes) == nargs, n


def test_argtypes_match_the_declarations():
    lib = s2m.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    g = lib.s2m_global_map.argtypes
    assert g[0] is vp and g[2] is vp and g[3] is sz and g[4] is sz and g[7] is sz
    assert g[1]._type_ is s2m.GmapParams and g[5]._type_ is sz and g[6]._type_ is C.c_int32 and g[8]._type_ is sz
    k = lib.s2m_kf_map_cloud.argtypes
    assert k[0] is vp and k[1] is C.c_int and k[2] is C.c_int and k[3] is C.c_float
    assert k[4] is vp and k[5] is sz and k[6] is sz and k[7]._type_ is sz
    assert C.sizeof(s2m.GmapParams) == 12


def test_gmap_default_params_are_the_reference_constants():
    p = s2m.default_gmap_params()
    assert (p.search_radius, p.pose_density, p.leaf) == (1000.0, 10.0, 1.0)
    assert s2m.load_library().s2m_gmap_default_params(None) == -1


def test_null_handle_calls_are_rejected():
    lib = s2m.load_library()
    n_out, n_keys = C.c_size_t(7), C.c_size_t(7)
    keys = (C.c_int32 * 4)()
    assert lib.s2m_global_map(None, None, None, 32, 0, C.byref(n_out), keys, 4, C.byref(n_keys)) == -1
    assert lib.s2m_kf_map_cloud(None, 0, 0, 0.0, None, 32, 0, C.byref(n_out)) == -1


def test_mirrors_carry_the_new_methods():
    assert callable(getattr(s2m.MapOptimizationS2M, "publishGlobalMap"))
    assert callable(getattr(s2m.MapOptimizationS2M, "globalMapCloud"))
    hpp = open(os.path.join(ROOT, "liorf_amd", "host", "map_optimization_s2m.hpp")).read()
    assert "void publishGlobalMap()" in hpp and "void globalMapCloud(" in hpp
    assert "--global-map" in open(os.path.join(ROOT, "liorf_amd", "host", "s2m_harness.cpp")).read()
