"""CPU side of appending a saved session and placing it (include/liorf_s2m.h, "Appending a saved session"; DESIGN.md section
21): the model (tests/ref/session_append_ref.py) held against the library's host-only entry points - the blob checker on a merged
blob, the precondition table, the anchor from pairs bit for bit - and the end-to-end condition of the GPU test checked on the
oracle alone. The GPU tests (test_session_append_gpu.py) hold the library against this model.

session_ref.scripted() names keys 20 .. 39 in its loop pairs and factors, so the 12- and 9-key sessions here come from
session_append_ref.scripted(), the same recipe with those placed by proportion.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import session_append_ref as AM
import session_ref as M

from liorf_amd import s2m

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = s2m.S2M_OK, -1
ANCHOR = [3.0, -2.0, 0.5, 0.02, -0.03, 0.7]            # all six components non-zero
POS_BAR, YAW_BAR = 0.05, 0.005                          # tests/test_relocalize_cpu.py

NEW = {"s2m_session_append_check_args": 4, "s2m_session_append": 6, "s2m_session_append_file": 5, "s2m_session_place": 2,
       "s2m_session_appended": 3, "s2m_session_anchor_from_pairs": 8, "s2m_relocalize_key": 6}


def test_new_symbols_declared_bound_and_exported():
    lib = s2m.load_library()
    raw = C.CDLL(s2m.LIB_PATH)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liorf_s2m.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m and m.group(1).count(",") + 1 == nargs, n
        assert n in s2m.ABI_SYMBOLS and hasattr(raw, n) and len(getattr(lib, n).argtypes) == nargs, n
    assert C.sizeof(s2m.SessionAppendInfo) == C.sizeof(s2m.SessionInfo) + 8
    for name in ("sessionAppend", "sessionAppendFile", "sessionPlace", "sessionAppended", "relocalizeKey", "mergeSession"):
        assert callable(getattr(s2m.MapOptimizationS2M, name)), name
    assert callable(s2m.anchorFromPairs)
    hpp = open(os.path.join(ROOT, "liorf_amd", "host", "map_optimization_s2m.hpp")).read()
    for sig in ("sessionAppend(", "void sessionPlace(", "bool relocalizeKey(", "anchorFromPairs(", "int mergeSession("):
        assert sig in hpp, sig


# ---- the merged blob is a session -----------------------------------------------------------------------------

@pytest.mark.parametrize("anchor", [None, ANCHOR])
def test_the_checker_accepts_the_models_merged_blob(anchor):
    a, b = AM.scripted(12, 12, seed=11), AM.scripted(9, 9, seed=5)
    for s in (a, b):
        s2m.session_check(M.write(s))
    m = AM.merge(a, b, anchor)
    info = s2m.session_check(M.write(m))
    ca, cb = a.counts(), b.counts()
    assert (info.n_keys, info.n_descriptors, info.n_loop_pairs, info.n_variables, info.n_points) == tuple(
        ca[k] + cb[k] for k in ("n_keys", "n_descriptors", "n_loop_pairs", "n_variables", "n_points"))
    assert info.n_factors == ca["n_factors"] + cb["n_factors"] + 1
    # re-keyed pairs stay ascending
    cur = [c for c, _ in m.pairs]
    assert cur == sorted(cur) and len(set(cur)) == len(cur) and m.pairs[len(a.pairs):] == [(c + 12, p + 12) for c, p in b.pairs]
    # the junction is the first factor that names variable N0, and it names it as the next variable
    j = m.factors[m.junction]
    assert (m.junction, j["type"], j["i"], j["j"], j["rows"], j["k"]) == (ca["n_factors"], M.BETWEEN, 11, 12, 6, 0.0)
    assert j["sw"] == [1.0] * 6
    assert all(max(f["i"], f["j"]) < 12 for f in m.factors[:m.junction])
    # its residual at the appended estimates is rounding-sized
    assert AM.junction_residual(m) < 1e-12
    # the counters stay the handle's
    assert (m.n_search, m.counter) == (a.n_search, a.counter)
    if anchor is None:                                   # nothing composed: every bit of b is there
        assert np.array_equal(m.poses[12:].view(np.uint32), b.poses.view(np.uint32))
        assert np.array_equal(m.X[12:].view(np.uint64), b.X.view(np.uint64))
        assert [f["R"] + f["t"] for f in m.factors[m.junction + 1:]] == [f["R"] + f["t"] for f in b.factors]
    else:                                                # a GPS factor's variances and rotation block stay, its position moves
        g0 = next(f for f in b.factors if f["type"] == M.GPS)
        g1 = next(f for f in m.factors[m.junction:] if f["type"] == M.GPS)
        assert g1["sw"] == g0["sw"] and g1["R"] == g0["R"] and g1["t"] != g0["t"] and g1["i"] == g0["i"] + 12
        A = M.state_of(anchor)
        assert np.allclose(g1["t"], np.array(A[:9]).reshape(3, 3) @ np.array(g0["t"]) + np.array(A[9:]), rtol=0, atol=1e-12)


def test_append_then_place_is_append_with_the_anchor_in_the_model():
    a, b = AM.scripted(12, 12, seed=11), AM.scripted(9, 9, seed=5)
    assert M.write(AM.place(AM.merge(a, b, None), ANCHOR)) == M.write(AM.merge(a, b, ANCHOR))
    # and a -0.0 survives the NULL anchor but not an identity anchor
    b.poses[3, 1] = F(-0.0)
    assert np.signbit(AM.merge(a, b, None).poses[12 + 3, 1]) and not np.signbit(AM.merge(a, b, [0] * 6).poses[12 + 3, 1])


# ---- the preconditions -------------------------------------------------------------------------------------------

def info(keys, desc, var):
    return s2m.SessionInfo(version=1, n_keys=keys, n_descriptors=desc, n_loop_pairs=0, n_variables=var, n_factors=0, n_points=0, bytes=224)


NAN, INF = float("nan"), float("inf")
PRECONDITIONS = [
    # have (keys, descriptors, variables), blob (keys, descriptors, variables), anchor, junction_var, status
    ((5, 5, 5), (3, 3, 3), None, None, OK),
    ((5, 5, 5), (3, 3, 3), ANCHOR, [1.0] * 6, OK),
    ((0, 0, 0), (3, 3, 3), None, None, INVALID),                     # an empty handle is s2m_session_load's
    ((1, 1, 1), (3, 3, 3), None, None, OK),
    ((5, 5, 5), (0, 0, 0), None, None, OK),
    (((1 << 24) - 3, 0, 0), (3, 0, 0), None, None, OK),              # N0 + nK <= 2^24
    (((1 << 24) - 3, 0, 0), (4, 0, 0), None, None, INVALID),
    ((5, 4, 5), (3, 3, 3), None, None, INVALID),                     # descriptors in the blob: the store holds exactly N0
    ((5, 6, 5), (3, 3, 3), None, None, INVALID),
    ((5, 4, 5), (3, 0, 3), None, None, OK),                          # none in the blob: the store is not asked
    ((5, 5, 5), (3, 4, 3), None, None, INVALID),                     # nD <= nK
    ((5, 5, 5), (3, 2, 3), None, None, OK),
    ((5, 5, 4), (3, 3, 3), None, None, INVALID),                     # variables in the blob: the graph holds exactly N0
    ((5, 5, 6), (3, 3, 3), None, None, INVALID),
    ((5, 5, 0), (3, 3, 0), None, None, OK),
    ((5, 5, 5), (3, 3, 4), None, None, INVALID),                     # nV <= nK
    ((5, 5, 5), (3, 3, 2), None, None, OK),
    ((5, 5, 5), (3, 3, 3), [0, 0, 0, 0, NAN, 0], None, INVALID),     # a finite anchor
    ((5, 5, 5), (3, 3, 3), [INF, 0, 0, 0, 0, 0], None, INVALID),
    ((5, 5, 5), (3, 3, 3), None, [1, 1, 1, 1, 1, 0.0], INVALID),     # positive finite variances
    ((5, 5, 5), (3, 3, 3), None, [1, -1, 1, 1, 1, 1], INVALID),
    ((5, 5, 5), (3, 3, 3), None, [1, 1, INF, 1, 1, 1], INVALID),
    ((5, 5, 5), (3, 3, 3), None, [1, 1, 1, NAN, 1, 1], INVALID),
    ((5, 5, 5), (3, 3, 3), None, [1e-9, 1e8, 1, 1, 1, 1], OK),
]


@pytest.mark.parametrize("have,blob,anchor,var,status", PRECONDITIONS)
def test_precondition_table(have, blob, anchor, var, status):
    assert s2m.session_append_check_args(info(*have), info(*blob), anchor, var) == status


def test_null_arguments():
    lib = s2m.load_library()
    i = info(5, 5, 5)
    assert lib.s2m_session_append_check_args(None, C.byref(i), None, None) == INVALID
    assert lib.s2m_session_append_check_args(C.byref(i), None, None, None) == INVALID
    assert lib.s2m_session_append(None, s2m.SESSION_READ_FN(lambda *a: 0), None, None, None, None) == INVALID
    assert lib.s2m_session_append_file(None, b"x", None, None, None) == INVALID
    assert lib.s2m_session_place(None, None) == INVALID
    assert lib.s2m_session_appended(None, None, None) == INVALID
    recs = (s2m.RelocCandidate * 8)()
    n, best = C.c_int32(7), C.c_int32(7)
    assert lib.s2m_relocalize_key(None, 0, None, recs, C.byref(n), C.byref(best)) == INVALID


# ---- the anchor from pairs ---------------------------------------------------------------------------------------

def pairs_from(anchors, seed=2):
    """Poses in the session's frame and, per pair, its pose in the map under that pair's anchor (as the float read-out)."""
    rng = np.random.default_rng(seed)
    sess = np.c_[rng.uniform(-20, 20, (len(anchors), 3)), rng.uniform(-0.1, 0.1, (len(anchors), 2)), rng.uniform(-3, 3, len(anchors))].astype(F)
    in_map = np.array([AM.readout(AM.compose(M.state_of(a), M.state_of(p))) for a, p in zip(anchors, sess)], F)
    return sess, in_map


def both(sess, in_map, tol_m, tol_rad):
    want = AM.anchor_from_pairs(sess, in_map, tol_m, tol_rad)
    got = s2m.anchorFromPairs(sess, in_map, tol_m, tol_rad)
    assert got[0].dtype == F and got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], (got, want)
    return got


def test_anchor_five_consistent_pairs_and_two_mirror_outliers():
    true = np.array([12.0, -7.0, 0.4, 0.01, -0.02, np.deg2rad(25.0)])
    rng = np.random.default_rng(4)
    anchors = [true + np.r_[rng.normal(0, 0.004, 3), rng.normal(0, 2e-4, 3)] for _ in range(5)]
    mirror = true + np.array([-40.0, 3.0, 0.0, 0.0, 0.0, np.pi])
    anchors = anchors[:2] + [mirror] + anchors[2:4] + [mirror + np.array([0.01, 0, 0, 0, 0, 0])] + anchors[4:]
    anchor, n, chosen = both(*pairs_from(anchors), 0.05, 0.005)
    assert n == 5 and chosen not in (2, 5)
    assert np.abs(anchor[:3] - true[:3]).max() < 0.02 and abs(anchor[5] - true[5]) < 1e-3
    # no averaging: the anchor is one pair's own, to the float
    sess, in_map = pairs_from(anchors)
    assert anchor.tobytes() == AM.readout(AM.compose(M.state_of(in_map[chosen]), AM.inverse(M.state_of(sess[chosen])))).tobytes()


def test_anchor_ties():
    base = np.array([1.0, 2.0, 0.0, 0.0, 0.0, 0.3])
    # two camps of two: {0, 1} 0.04 m apart, {2, 3} 0.01 m apart - the closer camp wins, its lower index
    anchors = [base, base + [0.04, 0, 0, 0, 0, 0], base + [5, 0, 0, 0, 0, 0], base + [5.01, 0, 0, 0, 0, 0]]
    _, n, chosen = both(*pairs_from(anchors), 0.05, 0.01)
    assert (n, chosen) == (2, 2)
    # all alone (tolerance 0 m between distinct anchors): every pair has itself, sum 0 - the lower index
    anchors = [base + [k, 0, 0, 0, 0, 0] for k in range(4)]
    _, n, chosen = both(*pairs_from(anchors), 0.05, 0.01)
    assert (n, chosen) == (1, 0)
    # m = 1
    _, n, chosen = both(*pairs_from(anchors[:1]), 0.05, 0.01)
    assert (n, chosen) == (1, 0)


def test_anchor_error_rows():
    lib = s2m.load_library()
    a = np.zeros((2, 6), F)
    out = np.zeros(6, F)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    call = lambda s, m, n, tm=0.1, tr=0.1, o=out: lib.s2m_session_anchor_from_pairs(s, m, n, tm, tr, fp(o) if o is not None else None, None, None)
    assert call(fp(a), fp(a), 2) == OK
    assert call(fp(a), fp(a), 0) == INVALID and call(fp(a), fp(a), -1) == INVALID
    assert call(None, fp(a), 2) == INVALID and call(fp(a), None, 2) == INVALID and call(fp(a), fp(a), 2, o=None) == INVALID
    for bad in (NAN, INF, -INF):
        b = a.copy()
        b[1, 4] = bad
        assert call(fp(b), fp(a), 2) == INVALID and call(fp(a), fp(b), 2) == INVALID
        assert call(fp(a), fp(a), 2, tm=bad) == INVALID and call(fp(a), fp(a), 2, tr=bad) == INVALID
    assert call(fp(a), fp(a), 2, tm=-1.0) == INVALID
    with pytest.raises(s2m.S2MError):
        s2m.anchorFromPairs(np.full((1, 6), NAN, F), a[:1])


# ---- the end-to-end condition, on the oracle alone --------------------------------------------------------------

def test_the_probe_keys_place_session_b_within_a_tenth_of_the_bar_on_the_oracle():
    import relocalize_ref as R
    clouds, stored, _, true, _ = AM.session_b()
    in_session, in_map = [], []
    for k, name in zip(AM.B_PROBES, ("Q1", "Q2")):
        assert np.array_equal(clouds[k], R.query_scan(name)[0])
        m = R.model(name)
        assert m["best"] >= 0
        in_session.append(stored[k])
        in_map.append(np.asarray(m["records"][m["best"]]["pose"], F))
    anchor, n, chosen = both(np.array(in_session, F), np.array(in_map, F), POS_BAR, YAW_BAR)
    print("anchor", anchor, "supporters", n, "chosen", chosen)
    assert n == 2
    A = M.state_of(anchor)
    for k in range(len(clouds)):
        placed = AM.readout(AM.compose(A, M.state_of(stored[k])))
        pe, ye = R.pose_error(placed, true[k])
        print("key", k, "position error", pe, "yaw error", ye)
        assert pe < POS_BAR / 10 + 1e-3 and ye < YAW_BAR / 10, (k, pe, ye)
