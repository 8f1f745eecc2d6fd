"""CPU side of the stage-by-stage check of the key-frame selection (kf_select, liorf_amd/csrc/s2m_voxel.hip): the staged
restatement tests/ref/kf_select_ref.py against the two key-list restatements the suite already has, the conditions the GPU
tests (test_kf_select_gpu.py) put on their inputs - exact candidate counts, a store that tells a wrong tie order and a wrong
summation order apart, voxel indices that reach the third radix digit - and the argument checks of s2m_debug_kf_select_last.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import kf_select_ref as K
import relocalize_ref as M
from liorf_amd import s2m
from test_keyframes_cpu import BOUNDARY_D, boundary_store, select_surrounding

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["s2m_debug_kf_select_last", "s2m_debug_kf_select_last_check_args"]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the hook without a device --------------------------------------------------------------------------------------------

def test_hook_symbols_declared_bound_and_exported():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, dbg = strip("liorf_s2m.h"), strip("liorf_s2m_debug.h")
    raw, lib = C.CDLL(s2m.LIB_PATH), s2m.load_library()
    for n, nargs in zip(NEW, (2, 1)):
        assert re.search(r"\b%s\s*\(" % n, dbg) and not re.search(r"\b%s\s*\(" % n, main), n
        assert n in s2m.ABI_SYMBOLS and hasattr(raw, n) and len(getattr(lib, n).argtypes) == nargs, n
    body = dbg[dbg.index("typedef struct s2m_debug_kf_select_out"):dbg.index("} s2m_debug_kf_select_out;")]
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [f for f, _ in s2m.KfSelectOut._fields_]              # the ctypes mirror, field by field
    assert (s2m.S2M_DEBUG_KF_NARROW, s2m.S2M_DEBUG_KF_PRE, s2m.S2M_DEBUG_KF_WIDE) == (K.PATH_NARROW, K.PATH_PRE, K.PATH_WIDE) == (0, 1, 2)
    for name, v in (("NARROW", 0), ("PRE", 1), ("WIDE", 2)):
        assert re.search(r"#define\s+S2M_DEBUG_KF_%s\s+%d\b" % (name, v), dbg)


def test_hook_argument_checks_need_no_device():
    lib = s2m.load_library()
    chk = lib.s2m_debug_kf_select_last_check_args
    bad, i32 = -1, C.POINTER(C.c_int32)                        # S2M_ERR_INVALID_ARG
    cent, nn, keys, off = np.zeros((4, 3), F), np.zeros(4, np.int32), np.zeros(9, np.int32), np.zeros(10, np.int32)
    full = dict(cent_cap=4, cent=s2m._fp(cent), nn=nn.ctypes.data_as(i32), frames_cap=9, keys=keys.ctypes.data_as(i32),
                offsets=off.ctypes.data_as(i32))
    assert chk(None) == bad
    assert chk(C.byref(s2m.KfSelectOut(**full))) == 0
    assert chk(C.byref(s2m.KfSelectOut())) == 0                             # no room offered: the counts alone
    for drop in ("cent", "nn", "keys", "offsets"):
        assert chk(C.byref(s2m.KfSelectOut(**{k: v for k, v in full.items() if k != drop}))) == bad, drop
    assert chk(C.byref(s2m.KfSelectOut(**{**full, "cent_cap": 0, "cent": None, "nn": None}))) == 0
    assert lib.s2m_debug_kf_select_last(None, C.byref(s2m.KfSelectOut(**full))) == bad
    assert lib.s2m_debug_kf_select_last(None, None) == bad


# ---- the staged restatement against select_surrounding and select_at ---------------------------------------------------

def _n_recent(t, time_cur, W=10.0):
    n = 0
    for i in range(len(t) - 1, -1, -1):
        if not (time_cur - t[i] < W):
            break
        n += 1
    return n


_NN_FAR = [[9.9, 0.0, 0], [9.9, 0.6, 0], [10.05, 0.3, 0], [0.0, 0, 0]]
HAND = [  # the hand-built pins of test_keyframes_cpu: (positions, times, time_cur, R, D)
    ([[50.0, 0, 0], [0, 0, 0]], [0, 0], 100.0, 50.0, 1.0),
    ([[float(np.nextafter(F(50), F(0))), 0, 0], [0, 0, 0]], [0, 0], 100.0, 50.0, 1.0),
    ([[4.0, 5, 5], [6.0, 5, 5], [5.0, 5, 8]], [0, 0, 0], 100.0, 50.0, 10.0),
    ([[6.0, 5, 5], [4.0, 5, 5], [5.0, 5, 8]], [0, 0, 0], 100.0, 50.0, 10.0),
    ([[1.0, 2, 3]], [5.0], 6.0, 50.0, 1.0),
    ([[0.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0]], [15.0, 10.0, 12.0], 20.0, 50.0, 1.0),
    (_NN_FAR, [0, 0, 0, 0], 100.0, 10.0, 1.0),
    (_NN_FAR, [0, 0, 99.0, 99.0], 100.0, 10.0, 1.0),
]


def _random_stores():
    rng = np.random.default_rng(2)
    P = np.cumsum(rng.normal(0, 1.5, (300, 3)), 0).astype(F)
    yield P, np.arange(300, dtype=np.float64), 299.5, 20.0, 2.0               # test_restatement_on_a_random_trajectory_is_sane
    rng = np.random.default_rng(5)
    P = rng.uniform(-40, 40, (60, 3)).astype(F)
    P[-1] = 0
    yield P, np.zeros(60), 100.0, 50.0, 1e-6                                  # test_leaf_too_small_passes_the_key_poses_through
    yield P, np.zeros(60), 5.0, 50.0, 3.0                                     # ... with every key recent
    P, t = boundary_store()
    yield P, t, 100.0, 50.0, BOUNDARY_D
    yield P, t, 5.0, 50.0, BOUNDARY_D


def test_staged_keys_equal_select_surrounding_on_the_existing_stores():
    for P, t, tc, R, D in HAND + list(_random_stores()):
        P, t = np.asarray(P, F), np.asarray(t, np.float64)
        st = K.stages(P, P[-1], R, D, n_recent=_n_recent(t, tc))
        assert st["keys"].tolist() == select_surrounding(P, t, tc, R=R, D=D), (P.shape, tc, R, D)
        assert st["n_frames"] == len(st["keys"]) and st["n_cent"] == len(st["nn"]) == st["cent"].shape[0]


def test_staged_keys_equal_select_at_on_the_existing_stores():
    for P, _, _, R, D in HAND + list(_random_stores()):
        P = np.asarray(P, F)
        for c in (P[0], P[-1] + F(0.37), [1.5, -2.25, 0.5]):
            assert K.stages(P, c, R, D)["keys"].tolist() == M.select_at(P, c, R=R, D=D), (P.shape, R, D)


@pytest.mark.parametrize("n", [1, 2, 1025, 4097, K.N_KEYS])
def test_staged_keys_equal_both_restatements_on_the_new_store(n):
    P, sizes, _ = K.store()
    Pn = P[:n]
    for D in (2.0, 0.5):
        st = K.store_stages(n, 50.0, D)
        assert st["keys"].tolist() == M.select_at(Pn, K.CENTRE, R=50.0, D=D)
        assert st["offsets"][0] == 0 and st["offsets"][-1] == st["n_points"] == int(sizes[st["keys"]].sum())
    # around the newest key, with recent keys: times 1 s apart, a window that takes 0, 1 and min(n, 1500) keys
    t = np.arange(n, dtype=np.float64)
    for n_recent in sorted({0, 1, min(n, 1500)}):
        tc = t[-1] + 10.0 - n_recent + 0.5 if n_recent else t[-1] + 10.0
        assert _n_recent(t, tc) == n_recent
        st = K.stages(Pn, Pn[-1], 50.0, 2.0, n_recent=n_recent)
        assert st["keys"].tolist() == select_surrounding(Pn, t, tc, R=50.0, D=2.0)


def test_store_is_seeded_and_planted_as_described():
    K.store.cache_clear()
    P, sizes, info = K.store()
    K.store.cache_clear()
    P2, sizes2, _ = K.store()
    assert np.array_equal(_bits(P), _bits(P2)) and np.array_equal(sizes, sizes2)            # one seed, one store
    assert P.shape == (K.N_KEYS, 3) and sizes.min() == 0 and sizes.max() == 7 and (sizes == 0).sum() == 1
    assert all(0 <= t < 500 for t in info["trials"])                                           # found within a few hundred trials
    d2 = K.d2_of(P, K.CENTRE)
    for cl in (K.CLUSTER_A, K.CLUSTER_B):
        four, early = list(cl[:4]), cl[4]
        assert len(set(_bits(d2[four]).tolist())) == 1 and d2[early] < d2[four[0]] and early > max(four)
        for D in (2.0, 0.5):
            assert len({tuple(K._cell(P[k], D)) for k in cl}) == 1
    assert max(K.CLUSTER_A) < 4096 and K.CLUSTER_B[1] == 4095 and K.CLUSTER_B[2] == 4096
    a, b = K.NEAREST_PAIR
    assert b - a > 256 and (a % 256) // 64 != (b % 256) // 64                                  # different waves of k_kf_select_nearest
    c = ((P[a] + P[b]).astype(F) / F(2)).astype(F)
    e = K.d2_of(P, c)
    assert _bits(e[a]) == _bits(e[b]) and np.sort(e)[2] > e[a]


# ---- the conditions on the GPU tests' inputs -------------------------------------------------------------------------

@pytest.mark.parametrize("m", K.COUNTS)
def test_radius_for_hits_the_count_exactly(m):
    P, _, _ = K.store()
    R = K.radius_for(P, K.CENTRE, m)
    assert R.dtype == F and R > 0
    assert int((K.d2_of(P, K.CENTRE) < R * R).sum()) == m
    assert K.store_stages(K.N_KEYS, R, 2.0)["n_cand"] == m


def test_radius_for_hits_the_counts_of_the_path_comparison_on_the_first_4096_keys():
    P, _, _ = K.store()
    for m in (1025, 2048, 4096):
        R = K.radius_for(P[:4096], K.CENTRE, m)
        assert int((K.d2_of(P[:4096], K.CENTRE) < R * R).sum()) == m and R < 1e3      # (the key parked at 1e4 m is no candidate)


def test_radius_for_fails_loudly():
    P, _, _ = K.store()
    with pytest.raises(RuntimeError):
        K.radius_for(P, K.CENTRE, int(np.searchsorted(np.sort(K.d2_of(P, K.CENTRE)), K.d2_of(P, K.CENTRE)[K.CLUSTER_A[0]])) + 2)   # a cut inside the tie
    with pytest.raises(ValueError):
        K.radius_for(P, K.CENTRE, K.N_KEYS + 1)


@pytest.mark.parametrize("D", [2.0, 0.5])
@pytest.mark.parametrize("m", [4096, 4097])
def test_new_store_tells_the_wrong_variants_apart(m, D):
    """At a radius with at most 4 096 candidates and at one with more: a tie order the other way round and sums taken in key order
    each change the bits of at least one centroid; the tie order also changes a nearest key."""
    P, _, _ = K.store()
    R = K.radius_for(P, K.CENTRE, m)
    right = K.store_stages(K.N_KEYS, R, D)
    assert right["n_cand"] == m and (right["path"] == K.PATH_WIDE) == (m > K.TILE)
    for v in ("ties_descending", "sum_in_key_order"):
        wrong = K.store_stages(K.N_KEYS, R, D, variant=v)
        assert wrong["n_cent"] == right["n_cent"]
        assert (_bits(wrong["cent"]) != _bits(right["cent"])).any(), v
        if v == "ties_descending":
            assert (wrong["nn"] != right["nn"]).any()
            # the planted pair is one of the places: its centroid goes to the lower key, the variant takes the higher
            c = ((P[K.NEAREST_PAIR[0]] + P[K.NEAREST_PAIR[1]]).astype(F) / F(2)).astype(F)
            at = np.flatnonzero((_bits(right["cent"]) == _bits(c)).all(axis=1))
            assert at.size == 1 and right["nn"][at[0]] == K.NEAREST_PAIR[0] and wrong["nn"][at[0]] == K.NEAREST_PAIR[1]
        else:
            assert np.array_equal(wrong["order"], right["order"])


def test_one_more_candidate_than_the_tile_adds_one_voxel_of_its_own():
    """What the pre-against-wide comparison of the GPU tests rests on: the 4 097th candidate shares no voxel, so every centroid
    of the 4 096-candidate selection is a centroid of the 4 097-candidate one, bit for bit."""
    P, _, _ = K.store()
    for D in (2.0, 0.5):
        a = K.store_stages(K.N_KEYS, K.radius_for(P, K.CENTRE, 4096), D)
        b = K.store_stages(K.N_KEYS, K.radius_for(P, K.CENTRE, 4097), D)
        new = P[b["order"][-1]]
        assert b["n_cent"] == a["n_cent"] + 1
        rest = b["cent"][~(_bits(b["cent"]) == _bits(new)).all(axis=1)]
        assert np.array_equal(_bits(rest), _bits(a["cent"]))


def test_full_store_reaches_the_third_radix_digit_and_the_leaf_too_small_case():
    P, _, _ = K.store()
    full = K.store_stages(K.N_KEYS, 1e3, 0.5)
    assert full["n_cand"] == K.N_KEYS and not full["leaf_too_small"]
    assert K.max_voxel_index(P, full["order"], 0.5) > 2 ** 22                # bits 22 and up: the third 11-bit pass moves keys
    tiny = K.store_stages(K.N_KEYS, 1e3, 1e-6)
    assert tiny["leaf_too_small"] and tiny["n_cent"] == tiny["n_cand"] == K.N_KEYS
    assert np.array_equal(_bits(tiny["cent"]), _bits(P[tiny["order"]]))      # the candidate positions in rank order
