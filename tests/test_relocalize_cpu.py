"""CPU side of localising a scan in the stored map (include/liorf_s2m.h: "ICP with an initial guess", "Relocalisation", "The local
map around a given position"): the model on the oracle (tests/ref/relocalize_ref.py) with its pins - the sign of the yaw, the
scripted revisit's expected records, the selection around a free centre - and the ABI checks that need no GPU.
The GPU tests (test_relocalize_gpu.py) hold the library against this model.

Figures of the model on the scripted revisit (search_radius 15, search_num 2, icp_leaf 0.5, fitness_score 0.3, top_k 4, all 60
shifts), hit order and fitness:
  Q1  8: 0.00802 (9 it., 5 mm)   23: 0.19318 (40 m off)   15: 9.693 rejected   24: 0.19317 (40 m off)      best = key 8
  Q2  23: 0.20470 (40 m off)     8: 0.0092909 (2.1 mm)    15: 10.41 rejected   7: 0.0092838 (2.4 mm)
Key 7 and key 8 are neighbours on the circle: their submaps (keys 5..9, keys 6..10) both hold the true place, both alignments end
2 mm from the truth and their fitness differs in the fifth digit, 7e-6 in key 7's favour. By the rule of *best - the least
(fitness, position), as s2m_loop_verify - the best record of Q2 is therefore key 7 at position 3, not key 8 at position 1 as a
table rounded to four digits suggests. What the tests hold is what that figure stood for: *best follows the rule, it is not the
descriptor's first hit (the mirror place, key 23), it is a record of the true place (key 7 or key 8) within the pose bar, and
key 8's own record is accepted within the same bar.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import relocalize_ref as M
import sc_query_ref as Q

from liorf_amd import s2m
from oracle import oracle as O
from test_global_map_cpu import AT_R, BOUNDARY_D, BOUNDARY_R, boundary_store, select_global

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = s2m.S2M_OK, -1
A, RJ = s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_REJECTED
POS_BAR, YAW_BAR = 0.05, 0.005      # ten times what the reference alone reaches (0.005 m, 2e-4 rad)


# ---- the model and its pins ---------------------------------------------------------------------------------

def test_yaw_sign_a_cloud_turned_by_plus_12_degrees_gives_shift_2_and_rz_minus_yaw_brings_it_back():
    cloud = M.revisit()[0][M.TRUE_KEY]
    turned = M.move32(cloud, M.rz64(np.deg2rad(12.0)))
    dq, dc = O.make_scancontext(turned)[0], O.make_scancontext(cloud)[0]
    for align in (Q.ALIGN_SECTOR_KEY, Q.ALIGN_FULL):
        assert Q.distance(dq, dc, align) == (0.0, 2), align
    yaw = Q.yaw_of_shift(2)
    assert abs(float(yaw) - np.deg2rad(12.0)) < 1e-6
    back = M.move32(turned, M.rz64(-float(yaw)))
    # two fp32 rotations of coordinates up to 25 m, and the yaw itself rounded to fp32
    assert np.abs(back[:, :3] - cloud[:, :3]).max() < 2e-5
    wrong = M.move32(turned, M.rz64(+float(yaw)))
    assert np.abs(wrong[:, :3] - cloud[:, :3]).max() > 1.0


def test_guess_is_the_key_pose_times_the_turn_back():
    pose = np.array([3.0, -2.0, 0.5, 0.0, 0.0, 0.7])
    G = M.guess64(pose, 0.2)
    assert np.allclose(G, M.transformation64([3.0, -2.0, 0.5, 0.0, 0.0, 0.5]))
    assert np.array_equal(M.guess64(pose, 0.2, use_yaw=False), M.transformation64(pose))


@pytest.mark.parametrize("name,keys,statuses", [
    ("Q1", [8, 23, 15, 24], [A, A, RJ, A]),
    ("Q2", [23, 8, 15, 7], [A, A, RJ, A]),
])
def test_model_on_the_scripted_revisit(name, keys, statuses):
    m = M.model(name)
    _, true = M.query_scan(name)
    recs = m["records"]
    assert [r["key"] for r in recs] == keys
    assert [r["status"] for r in recs] == statuses
    for r in recs:
        print(name, "key", r["key"], "fitness", r["fitness"], "iterations", r["iterations"], "pose error", M.pose_error(r["pose"], true) if "pose" in r else None)
        # no status is a matter of rounding: no fitness within a factor 1.4 of the gate
        assert r["fitness"] < M.FITNESS / 1.4 or r["fitness"] > M.FITNESS * 1.4, r["key"]
        assert r["n_src"] >= 300 and r["n_tgt"] >= 1000
    best = m["best"]
    # *best by the rule, and no matter of rounding either: the runner-up is more than twice the ICP fitness bar (1e-6) behind
    fits = sorted(r["fitness"] for r in recs if r["status"] == A)
    assert recs[best]["fitness"] == fits[0] and fits[1] - fits[0] > 2e-6
    assert recs[best]["key"] in (7, 8)
    if name == "Q1":
        assert best == 0 and recs[best]["key"] == 8
    else:
        assert best != 0 and recs[0]["key"] == 23                 # the descriptor's first hit is the mirror place
        assert best == 3 and recs[best]["key"] == 7               # (see the module docstring)
    # the records of the true place are within a tenth of the bar; the mirror place passes the gate 40 m off
    for r in recs:
        if r["key"] in (7, 8):
            pe, ye = M.pose_error(r["pose"], true)
            assert pe < POS_BAR / 10 + 1e-3 and ye < YAW_BAR / 10, (r["key"], pe, ye)
        elif r["status"] == A:
            assert M.pose_error(r["pose"], true)[0] > 30.0
    k8 = recs[keys.index(8)]
    assert k8["status"] == A and k8["fitness"] < 0.01 and k8["iterations"] < 30


def test_without_the_yaw_the_true_place_is_rejected():
    for name in ("Q1", "Q2"):
        m = M.model(name, use_yaw=False)
        k8 = [r for r in m["records"] if r["key"] == 8][0]
        assert k8["status"] == RJ and k8["iterations"] == 100 and 1.4 * M.FITNESS < k8["fitness"], (name, k8["fitness"])
        assert m["best"] == -1 or m["records"][m["best"]]["key"] != 8


def test_select_at_the_newest_key_is_select_global():
    rng = np.random.default_rng(3)
    P = np.cumsum(rng.normal(0, 2.0, (400, 3)) * [1, 1, 0.1], 0).astype(F)
    for R, D in ((1e3, 10.0), (1e3, 3.0), (30.0, 2.0)):
        assert M.select_at(P, P[-1], R, D) == select_global(P, R=R, D=D)
    B = boundary_store()
    assert M.select_at(B, B[-1], BOUNDARY_R, BOUNDARY_D) == select_global(B, R=BOUNDARY_R, D=BOUNDARY_D)
    assert M.select_at(np.zeros((0, 3)), [0, 0, 0]) == []


def free_centre_store():
    """boundary_store() without its newest key, read from the origin as a free centre (no key sits there, and the newest key is
    now key 6, 10.05 m away): key 0 at sqrtf distance exactly R, keys 1..3 at one position, keys 4 and 5 with a centroid that
    is nearest to key 6, which is beyond R."""
    return boundary_store()[:-1].copy(), np.zeros(3, F)


def test_boundary_pin_for_a_centre_that_is_no_key():
    P, c = free_centre_store()
    d = (P[0] - c).astype(F)
    d2 = F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert d2 < F(100) and np.sqrt(d2) == F(10) and tuple(P[0][:2]) == AT_R
    keys = M.select_at(P, c, BOUNDARY_R, BOUNDARY_D)
    assert 0 in keys                                   # a centroid at exactly R is kept
    assert sorted(keys) == [0, 1, 6]                   # lowest of the equal keys; key 6 through its neighbours' centroid
    # a key exactly at R is excluded from the radius search
    P2 = np.array([[10.0, 0, 0], [4.0, 0, 0], [30.0, 0, 0]], F)
    assert M.select_at(P2, c, BOUNDARY_R, BOUNDARY_D) == [1]
    P2[0, 0] = np.nextafter(F(10), F(0))
    assert sorted(M.select_at(P2, c, BOUNDARY_R, BOUNDARY_D)) == [0, 1]
    # the centre matters: from the newest key the selection is another one
    assert sorted(select_global(P, R=BOUNDARY_R, D=BOUNDARY_D)) != sorted(keys)


# ---- ABI checks without a GPU -----------------------------------------------------------------------------

NEW = {"s2m_icp_align_guess": 9, "s2m_reloc_default_params": 1, "s2m_relocalize_check_args": 3, "s2m_relocalize_scan": 9,
       "s2m_extract_surrounding_at": 10}
NEW_DEBUG = {"s2m_debug_icp_align_guess_many_device": 10}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_declared_bound_and_exported():
    lib = s2m.load_library()
    raw = C.CDLL(s2m.LIB_PATH)
    for hdr, table in (("liorf_s2m.h", NEW), ("liorf_s2m_debug.h", NEW_DEBUG)):
        txt = _header(hdr)
        for n, nargs in table.items():
            m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
            assert m, n
            assert m.group(1).count(",") + 1 == nargs, n
            assert n in s2m.ABI_SYMBOLS
            assert hasattr(raw, n)
            assert len(getattr(lib, n).argtypes) == nargs, n


def test_argtypes_match_the_declarations():
    lib = s2m.load_library()
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    g = lib.s2m_icp_align_guess.argtypes
    assert g[0] is vp and g[1] is vp and g[2] is sz and g[3] is vp and g[4] is sz and g[5] is sz
    assert g[6]._type_ is C.c_float and g[7]._type_ is s2m.IcpParams and g[8]._type_ is s2m.IcpResult
    r = lib.s2m_relocalize_scan.argtypes
    assert r[0] is vp and r[1] is vp and r[2] is sz and r[3] is sz and r[4] is C.c_int
    assert r[5]._type_ is s2m.RelocParams and r[6]._type_ is s2m.RelocCandidate and r[7]._type_ is i32 and r[8]._type_ is i32
    c = lib.s2m_relocalize_check_args.argtypes
    assert c[0] is i32 and c[1] is i32 and c[2]._type_ is s2m.RelocParams
    e = lib.s2m_extract_surrounding_at.argtypes
    assert e[0] is vp and e[1]._type_ is C.c_float and e[2]._type_ is s2m.KfParams and e[3] is vp and e[4] is sz and e[5] is sz
    assert e[6]._type_ is sz and e[7]._type_ is i32 and e[8] is sz and e[9]._type_ is sz
    d = lib.s2m_debug_icp_align_guess_many_device.argtypes
    assert d[0] is vp and d[1] is vp and d[2] is sz and d[3]._type_ is vp and d[4]._type_ is sz and d[5]._type_ is C.c_float
    assert d[6] is i32 and d[7] is sz and d[8]._type_ is s2m.IcpParams and d[9]._type_ is s2m.IcpResult
    # the layout the header's declarations give on this ABI
    assert C.sizeof(s2m.RelocParams) == 64 and s2m.RelocParams.loop.offset == 32 and s2m.RelocParams.use_yaw.offset == 52
    assert C.sizeof(s2m.RelocCandidate) == 232 and s2m.RelocCandidate.guess.offset == 36 and s2m.RelocCandidate.icp.offset == 104
    assert s2m.RelocCandidate.pose_xyzrpy.offset == 184 and s2m.RelocCandidate.pose_tobemapped.offset == 208


def test_defaults():
    p = s2m.default_reloc_params()
    q, d = p.query, s2m.default_sc_query_params()
    assert (q.first, q.count, q.exclude_lo, q.exclude_hi, q.max_dist) == (d.first, d.count, d.exclude_lo, d.exclude_hi, d.max_dist)
    assert (q.top_k, q.align) == (4, s2m.S2M_SC_ALIGN_FULL)
    lp, ld = p.loop, s2m.default_loop_params()
    assert (lp.search_radius, lp.time_diff_s, lp.search_num, lp.fitness_score, lp.icp_leaf) == (
        ld.search_radius, ld.time_diff_s, ld.search_num, ld.fitness_score, ld.icp_leaf)
    assert (p.use_yaw, p.reserved) == (1, 0)
    assert s2m.load_library().s2m_reloc_default_params(None) == INVALID


def test_null_handle_calls_are_rejected():
    lib = s2m.load_library()
    r = s2m.IcpResult()
    pts = (C.c_float * 8)()
    assert lib.s2m_icp_align_guess(None, pts, 1, pts, 1, 32, None, None, C.byref(r)) == INVALID
    recs = (s2m.RelocCandidate * 8)()
    n, best = C.c_int32(7), C.c_int32(7)
    assert lib.s2m_relocalize_scan(None, pts, 1, 32, 0, None, recs, C.byref(n), C.byref(best)) == INVALID
    n_out, n_keys = C.c_size_t(7), C.c_size_t(7)
    keys = (C.c_int32 * 4)()
    c = (C.c_float * 3)()
    assert lib.s2m_extract_surrounding_at(None, c, None, None, 32, 0, C.byref(n_out), keys, 4, C.byref(n_keys)) == INVALID
    ptrs, ns = (C.c_void_p * 1)(), (C.c_size_t * 1)(1)
    assert lib.s2m_debug_icp_align_guess_many_device(None, pts, 1, ptrs, ns, None, 1, 32, None, C.byref(r)) == INVALID


# (n_sc, n_kf, fields, status)
ARG_TABLE = [
    (32, 32, {}, OK), (0, 0, {}, OK), (33, 32, {}, OK),                     # (stores out of step show at a hit, not here)
    (32, 32, {"query_top_k": 0}, INVALID), (32, 32, {"query_top_k": 1}, OK), (32, 32, {"query_top_k": 8}, OK),
    (32, 32, {"query_top_k": 9}, INVALID), (32, 32, {"query_top_k": 32}, INVALID), (32, 32, {"query_top_k": -1}, INVALID),
    (32, 32, {"query_align": 0}, OK), (32, 32, {"query_align": 2}, INVALID),
    (32, 32, {"query_max_dist": 0.0}, INVALID), (32, 32, {"query_max_dist": float("nan")}, INVALID), (32, 32, {"query_max_dist": 1e-9}, OK),
    (32, 32, {"query_first": 33}, INVALID), (32, 32, {"query_first": 8, "query_count": 24}, OK), (32, 32, {"query_count": 33}, INVALID),
    (32, 32, {"loop_search_radius": 0.0}, INVALID), (32, 32, {"loop_search_radius": float("inf")}, INVALID),
    (32, 32, {"loop_search_num": -1}, INVALID), (32, 32, {"loop_search_num": 0}, OK),
    (32, 32, {"loop_icp_leaf": 0.0}, INVALID), (32, 32, {"loop_icp_leaf": float("nan")}, INVALID),
    (32, 32, {"loop_fitness_score": float("nan")}, INVALID), (32, 32, {"loop_fitness_score": -1.0}, OK),
    (32, 32, {"loop_time_diff_s": float("nan")}, INVALID),                   # (unused, but held to the loop's own rules)
    (32, 32, {"use_yaw": 0}, OK), (32, 32, {"use_yaw": 1}, OK),
    (-1, 32, {}, INVALID), (32, -1, {}, INVALID),
]


@pytest.mark.parametrize("n_sc,n_kf,fields,status", ARG_TABLE)
def test_argument_table(n_sc, n_kf, fields, status):
    assert s2m.relocalize_check_args(n_sc, n_kf, s2m.default_reloc_params(**fields)) == status


def test_null_params_are_the_defaults():
    assert s2m.relocalize_check_args(32, 32, None) == OK and s2m.relocalize_check_args(-1, 0, None) == INVALID


def test_mirrors_carry_the_new_methods():
    for name in ("icpAlignGuess", "relocalizeScan", "extractSurroundingKeyFramesAt", "localizeInStoredMap", "debugIcpAlignGuessManyDevice"):
        assert callable(getattr(s2m.MapOptimizationS2M, name)), name
    hpp = open(os.path.join(ROOT, "liorf_amd", "host", "map_optimization_s2m.hpp")).read()
    assert "bool icpAlignGuess(" in hpp and "bool relocalizeScan(" in hpp and "void extractSurroundingKeyFramesAt(" in hpp
