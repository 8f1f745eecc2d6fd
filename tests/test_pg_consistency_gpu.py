"""GPU tests of the mutually consistent loops (s2m_pg_consistent_loops) against the model
tests/ref/pg_consistency_ref.py: matrix, degrees, selection and the result record bit for bit at the word and tile edges and at
the cap, thresholds met exactly, the chain length across scan blocks, far from the origin, read-only and busy, and the scene that
motivates the call end to end.  The estimates are set with s2m_debug_pg_set_estimate, so the model sees the same 12 doubles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pg_consistency_ref as R  # noqa: E402
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m  # noqa: E402

pytestmark = pytest.mark.gpu
OK, PENDING = s2m.S2M_OK, s2m.S2M_PG_PENDING


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def gpu(pair):
    return pair[0]


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _set_estimates(g, X):
    g.pgReset()
    for k, x in enumerate(np.asarray(X, np.float64).reshape(-1, 12)):
        g.pgSetEstimate(k, x[:9], x[9:])


def _params(prm):
    return s2m.default_pg_consistency_params(**prm) if prm else None


def _compare(g, X, kf, kt, rel, prm=None, chunk=512):
    """The call on the estimates X against the model: every output bit for bit.  Returns the model's dict."""
    _set_estimates(g, X)
    sel, deg, rec, words = g.pgConsistentLoops(kf, kt, rel, _params(prm), matrix=True)
    want = R.run(X, kf, kt, rel, R.params(**prm) if prm else None)
    m = len(kf)
    print("m", m, "pairs", rec.n_consistent_pairs, want["n_consistent_pairs"], "selected", rec.n_selected, want["n_selected"], "start", rec.start,
          want["start"], "largest degree", int(deg.max()) if m else 0)
    assert words.shape == want["words"].shape
    for r0 in range(0, m, chunk):                                           # in row chunks, so a failure names its rows
        assert np.array_equal(words[r0:r0 + chunk], want["words"][r0:r0 + chunk]), (r0, int((words[r0:r0 + chunk] != want["words"][r0:r0 + chunk]).sum()))
    assert np.array_equal(deg, want["degree"])
    assert np.array_equal(sel, want["selected"])
    assert (rec.n_candidates, rec.n_selected, rec.start, rec.reserved, rec.n_consistent_pairs) == \
           (m, want["n_selected"], want["start"], 0, want["n_consistent_pairs"])
    return want


# ---- bit for bit against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_outputs_are_the_models_bit_for_bit(gpu, m):
    """Word and tile edges, a partial last word, more than one tile in both directions: 300 keys with random SE(3) estimates of
    moderate drift; about half the candidates are true loops with noise, half random."""
    X, kf, kt, rel = R.random_scene(m)
    want = _compare(gpu, X, kf, kt, rel)
    if m >= 63:
        assert 2 <= want["n_selected"] < m and want["matrix"].any()          # a scene with something to decide


def test_outputs_are_the_models_at_the_cap(gpu):
    """m = S2M_PG_CONSISTENCY_MAX: 64 words a row, 64 x 64 tiles; families of loops that agree within and not across."""
    X, kf, kt, rel = R.structured_scene()
    assert len(kf) == s2m.S2M_PG_CONSISTENCY_MAX
    want = _compare(gpu, X, kf, kt, rel)
    assert want["n_selected"] > 64


def test_empty_call_and_optional_outputs(gpu):
    X, kf, kt, rel = R.random_scene(65)
    _set_estimates(gpu, X)
    sel, deg, rec = gpu.pgConsistentLoops([], [], np.zeros((0, 6), np.float32))
    assert len(sel) == 0 and (rec.n_candidates, rec.n_selected, rec.start, rec.n_consistent_pairs) == (0, 0, -1, 0)
    want = R.run(X, kf, kt, rel)
    out = np.zeros(65, np.uint8)
    i32p = C.POINTER(C.c_int32)
    rc = gpu.lib.s2m_pg_consistent_loops(gpu.h, kf.ctypes.data_as(i32p), kt.ctypes.data_as(i32p), rel.ctypes.data_as(C.POINTER(C.c_float)), 65,
                                         None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None)
    assert rc == OK and np.array_equal(out.astype(bool), want["selected"])
    # a variable without a value, a key outside the graph: refused with the outputs as they were
    n = X.shape[0]
    out[:] = 7
    bad = kt.copy()
    bad[64] = n
    rc = gpu.lib.s2m_pg_consistent_loops(gpu.h, kf.ctypes.data_as(i32p), bad.ctypes.data_as(i32p), rel.ctypes.data_as(C.POINTER(C.c_float)), 65,
                                         None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None)
    assert rc == -1 and (out == 7).all()
    gpu.pgAddPrior(n, np.zeros(6, np.float32), np.ones(6))                  # variable n exists now, without a value
    rc = gpu.lib.s2m_pg_consistent_loops(gpu.h, kf.ctypes.data_as(i32p), kt.ctypes.data_as(i32p), rel.ctypes.data_as(C.POINTER(C.c_float)), 65,
                                         None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None)
    assert rc == -1 and (out == 7).all()


# ---- thresholds met exactly ------------------------------------------------------------------------------------------

def _identity_chain(n, step=(1.0, 0.0, 0.0)):
    X = np.zeros((n, 12))
    X[:, [0, 4, 8]] = 1.0
    X[:, 9:] = np.arange(n)[:, None] * np.asarray(step)[None, :]
    return X


def test_translation_threshold_is_met_exactly(gpu):
    """Pure translations by small integers: all arithmetic is exact.  Candidate 0 agrees with the estimates, candidate 1 is off
    by (3, 4, 0): d2 = 25.  tol_m = 5 keeps the pair (d2 == tol_m^2), the next double below 5 does not."""
    X = _identity_chain(8)
    kf, kt = np.array([0, 1], np.int32), np.array([4, 5], np.int32)
    rel = np.array([[4, 0, 0, 0, 0, 0], [7, 4, 0, 0, 0, 0]], np.float32)
    for tol, bit in ((5.0, True), (np.nextafter(5.0, 0.0), False), (np.nextafter(5.0, 9.0), True)):
        prm = dict(tol_m=float(tol), tol_chord=0.5, rate_m=0.0, rate_chord=0.0)
        want = _compare(gpu, X, kf, kt, rel, prm)
        assert bool(want["matrix"][0, 1]) == bit and want["n_selected"] == (2 if bit else 1)


def test_chord_threshold_is_met_exactly(gpu):
    """Rotations by 90 degrees about z in the estimates (entries 0 and +-1, exact), identity measurements: the cycle of the two
    candidates is a rotation by 180 degrees, rho2 = 4.  tol_chord = 2 keeps the pair, the next double below 2 does not."""
    def rz(q):                                        # q quarter turns
        c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q % 4]
        return [c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    X = np.array([rz(0), rz(0), rz(1), rz(3)])
    kf, kt = np.array([0, 2], np.int32), np.array([1, 3], np.int32)
    rel = np.zeros((2, 6), np.float32)
    for tol, bit in ((2.0, True), (np.nextafter(2.0, 0.0), False)):
        prm = dict(tol_m=1.0, tol_chord=float(tol), rate_m=0.0, rate_chord=0.0)
        want = _compare(gpu, X, kf, kt, rel, prm)
        assert bool(want["matrix"][0, 1]) == bit


def test_chain_length_loosens_the_far_pair_only(gpu):
    """1500 keys a metre apart (more than one block of the prefix sum).  Candidates 1 and 2 are both off by one metre against
    candidate 0; candidate 1 lies 4 m of chain from it, candidate 2 lies 2600 m away.  At rate_m = 0.001 only the far pair passes."""
    X = _identity_chain(1500)
    kf, kt = np.array([10, 12, 1310], np.int32), np.array([20, 22, 1320], np.int32)
    rel = np.array([[10, 0, 0, 0, 0, 0], [11, 0, 0, 0, 0, 0], [11, 0, 0, 0, 0, 0]], np.float32)
    s = R.chain_length(X)
    assert s[1024] == 1024 * 10 ** 6 and s[-1] == 1499 * 10 ** 6
    want = _compare(gpu, X, kf, kt, rel, dict(tol_m=0.5, tol_chord=0.01, rate_m=0.001, rate_chord=0.0))
    M = want["matrix"]
    assert not M[0, 1] and M[0, 2] and M[1, 2]
    want = _compare(gpu, X, kf, kt, rel, dict(tol_m=0.5, tol_chord=0.01, rate_m=0.0, rate_chord=0.0))
    assert not want["matrix"][0, 1] and not want["matrix"][0, 2]


def test_far_from_the_origin_the_model_still_holds(gpu):
    """The m = 65 scene 100 km away: the device's bits are the model's at that place (the model is the contract, not translation
    invariance)."""
    X, kf, kt, rel = R.random_scene(65, offset=(1e5, -1e5, 50.0))
    assert np.abs(X[:, 9:11]).min() > 9e4
    _compare(gpu, X, kf, kt, rel)


# ---- read-only and busy --------------------------------------------------------------------------------------------------

def _candidates_of(g):
    return (np.array([l[0] for l in g.loops], np.int32), np.array([l[1] for l in g.loops], np.int32), np.array([l[2] for l in g.loops], np.float32))


def test_the_call_changes_nothing_an_optimise_reads(pair):
    a, b = pair
    g = CS.build("loops_200")
    CS.load_into(a, g)
    CS.load_into(b, g)
    kf, kt, rel = _candidates_of(g)
    first = a.pgConsistentLoops(kf, kt, rel)
    ra, rb = a.pgOptimize(), b.pgOptimize()
    assert ra.iterations >= 1 and _bytes(ra) == _bytes(rb) and np.array_equal(a.pgPoses(), b.pgPoses())
    second = a.pgConsistentLoops(kf, kt, rel)                               # on the optimised estimates, device-side
    ra, rb = a.pgOptimize(), b.pgOptimize()
    assert _bytes(ra) == _bytes(rb) and np.array_equal(a.pgPoses(), b.pgPoses())
    assert a.pgSize() == b.pgSize()
    print("selected before the optimise", int(first[0].sum()), "after", int(second[0].sum()), "of", len(kf))
    assert second[0].all()                                                  # the loops the graph was optimised with agree on its estimates


def test_busy_while_a_launched_optimise_is_pending(pair):
    a, _ = pair
    g = CS.build("loops_200")
    CS.load_into(a, g)
    kf, kt, rel = _candidates_of(g)
    m = len(kf)
    i32p = C.POINTER(C.c_int32)
    sel, deg = np.full(m, 7, np.uint8), np.full(m, -5, np.int32)
    mat = np.full((m, 1), 0xABCD, np.uint64)
    rec = s2m.PgConsistencyResult()
    rec.n_candidates = -9

    def call():
        return a.lib.s2m_pg_consistent_loops(a.h, kf.ctypes.data_as(i32p), kt.ctypes.data_as(i32p), rel.ctypes.data_as(C.POINTER(C.c_float)), m, None,
                                             sel.ctypes.data_as(C.POINTER(C.c_uint8)), deg.ctypes.data_as(i32p), mat.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             C.byref(rec))
    code, _ = a.pgOptimizeLaunch()
    assert code == PENDING
    assert call() == s2m.S2M_ERR_BUSY
    assert (sel == 7).all() and (deg == -5).all() and (mat == 0xABCD).all() and rec.n_candidates == -9
    code, res = a.pgOptimizeCollect()
    assert code == OK and res.iterations >= 1
    assert call() == OK
    assert rec.n_candidates == m and sel.max() <= 1 and rec.n_selected == int(sel.sum()) and (deg >= 0).all()


# ---- end to end on the motivating scene ------------------------------------------------------------------------------

def test_selected_loops_give_the_graph_that_never_saw_the_false_ones(pair):
    a, b = pair
    sc = R.motivating_scene()
    g = sc["graph"]
    CS.load_into(a, g)
    CS.load_into(b, g)
    records = []
    for i, j, rel in sc["cand"]:
        r = s2m.LoopResult()
        r.status, r.key_cur, r.key_pre = s2m.S2M_LOOP_ACCEPTED, i, j
        r.pose_to[:] = [float(v) for v in rel]                             # pose_from is the identity: between() gives rel back
        records.append(r)
    kept = a.selectConsistentLoops(records)
    assert [(r.key_cur, r.key_pre) for r in kept] == [(c[0], c[1]) for c, t in zip(sc["cand"], sc["true"]) if t]
    var = np.full(6, 0.3)
    for r in kept:
        a.addLoopFactor(r.key_cur, r.key_pre, np.array(r.pose_from), np.array(r.pose_to), var)
    for r, t in zip(records, sc["true"]):
        if t:
            b.addLoopFactor(r.key_cur, r.key_pre, np.array(r.pose_from), np.array(r.pose_to), var)
    ra, rb = a.pgOptimize(), b.pgOptimize()
    print("iterations", ra.iterations, "error", ra.error_before, "->", ra.error_after)
    assert ra.iterations >= 1 and _bytes(ra) == _bytes(rb) and np.array_equal(a.pgPoses(), b.pgPoses())
