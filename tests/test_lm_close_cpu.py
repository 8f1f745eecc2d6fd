"""CPU companions of tests/test_lm_close_gpu.py: the argument checks of the hook, the oracle's close as one function, and
the proof that the shared cases (tests/ref/lm_close_cases.py) sit where they claim to sit - independent of the device and,
where it matters, of the oracle (numpy fp64 / fp32 restatements)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import lm_close_cases as LC  # noqa: E402

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the hook's boundary ---------------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    lib = s2m.load_library()
    rows = np.zeros((2, 28))
    rp = rows.ctypes.data_as(C.POINTER(C.c_double))
    pose, matP, out = np.zeros(6, F32), np.eye(6, dtype=F32), s2m.LmCloseOut()
    fp = C.POINTER(C.c_float)
    pp, mp = pose.ctypes.data_as(fp), matP.ctypes.data_as(fp)
    chk = lib.s2m_debug_lm_close_check_args
    assert chk(0, 0, 30, rp, 2, pp, mp, C.byref(out)) == 0
    assert chk(1, 1, 30, rp, 2, pp, mp, C.byref(out)) == 0
    assert chk(0, 29, 30, rp, 2, pp, mp, C.byref(out)) == 0
    assert chk(0, 3, 30, None, 0, pp, mp, C.byref(out)) == 0          # no rows at all: every active row is zero
    for bad in ((2, 1), (-1, 1), (1, 0), (0, -1), (0, 30), (1, 30)):   # form, iter
        assert chk(bad[0], bad[1], 30, rp, 2, pp, mp, C.byref(out)) == -1, bad
    assert chk(0, 4, 4, rp, 2, pp, mp, C.byref(out)) == -1            # iter == max_iter
    assert chk(0, 1, 30, None, 2, pp, mp, C.byref(out)) == -1
    assert chk(0, 1, 30, rp, -1, pp, mp, C.byref(out)) == -1
    assert chk(0, 1, 30, rp, 2, None, mp, C.byref(out)) == -1
    assert chk(0, 1, 30, rp, 2, pp, None, C.byref(out)) == -1
    assert chk(0, 1, 30, rp, 2, pp, mp, None) == -1
    assert lib.s2m_debug_lm_close(None, 0, 1, rp, 2, pp, 0, mp, C.byref(out)) == -1
    assert lib.s2m_debug_device_hypot(None, pp, pp, 1, pp) == -1


def test_out_struct_matches_the_header():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "liorf_s2m_debug.h")).read()
    body = txt[txt.index("typedef struct s2m_debug_lm_close_out"):txt.index("} s2m_debug_lm_close_out;")]
    order = [n for n, _ in s2m.LmCloseOut._fields_]
    assert order == ["AtA", "AtB", "n_sel_last", "trace", "pose", "pose_next", "iters_run", "converged", "done", "stalled",
                     "is_degenerate", "n_rows_active", "matP"]
    pos = [body.index(n) for n in order]
    assert pos == sorted(pos)
    assert C.sizeof(s2m.LmCloseOut) == 4 * (36 + 6 + 1 + 16 + 6 + 6 + 6 + 36)


# ---- the oracle's close as one function ------------------------------------------------------------------------------
def test_the_loop_runs_orc_lm_close(cfg_tiny):
    """orc_LMOptimization's records are what orc_lm_close gives on the loop's own normal equations (the committed golden
    vectors pin the loop itself)."""
    m, s = synth.to_xyzi(cfg_tiny["map"]), synth.to_xyzi(cfg_tiny["scan"])
    orc = O.Oracle(knn_backend=1)
    orc.set_map(m)
    orc.set_scan(s)
    pose = cfg_tiny["pose_init"].copy()
    orc.set_pose(pose)
    dg, matP = 0, np.zeros((6, 6), F32)
    for it in range(4):
        orc.surfOptimization()
        AtA, AtB, n = orc.normal_eq()
        conv, pose2, dg, matP, tr = O.lm_close(AtA, AtB, n, it, orc.p, orc.get_pose(), dg, matP)
        c2 = orc.LMOptimization(it)
        t2 = orc.trace()[-1]
        assert c2 == conv and bytes(t2) == bytes(tr)
        assert np.array_equal(_bits(orc.get_pose()), _bits(pose2))
        m2, d2 = orc.matP()
        assert d2 == dg and np.array_equal(_bits(m2), _bits(matP))


def test_below_min_corr_nothing_moves():
    P = np.arange(36, dtype=F32).reshape(6, 6)
    for it in (0, 3):
        conv, pose, dg, matP, tr = O.lm_close(np.eye(6, dtype=F32), np.ones(6, F32), 49, it, O.default_params(), LC.POSE0, 1, P)
        assert conv == 0 and tr.stepped == 0 and tr.n_sel == 49 and dg == 1
        assert np.array_equal(_bits(pose), _bits(LC.POSE0)) and np.array_equal(_bits(matP), _bits(P))
        assert np.array_equal(_bits(tr.pose), _bits(LC.POSE0)) and not any(tr.delta)


def test_hypotf_of_the_host_is_the_double_expression():
    """What glibc_hypotf restates: the host's hypotf is (float)sqrt((double)x * x + (double)y * y)."""
    libm = C.CDLL("libm.so.6")
    libm.hypotf.restype = C.c_float
    libm.hypotf.argtypes = [C.c_float, C.c_float]
    rng = np.random.default_rng(12)
    n = 100000
    p = (10.0 ** rng.uniform(-7, 6, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    y = np.where(rng.random(n) < 0.5, p * rng.uniform(0.25, 4.0, n), 10.0 ** rng.uniform(-9, 7, n)).astype(F32)
    want = np.array([libm.hypotf(a, b) for a, b in zip(p.tolist(), y.tolist())], F32)
    pd, yd = p.astype(np.float64), y.astype(np.float64)
    got = np.sqrt(pd * pd + yd * yd).astype(F32)
    assert np.array_equal(_bits(got), _bits(want))
    assert libm.hypotf(float("inf"), float("nan")) == math.inf and libm.hypotf(float("nan"), float("-inf")) == math.inf


# ---- the cases -------------------------------------------------------------------------------------------------------
def test_case_counts():
    fam = {}
    for c in LC.all_cases():
        fam[c.fam] = fam.get(c.fam, 0) + 1
    assert fam == {"a": 22, "b": 336, "c": 145, "d": 13, "e": 34}
    f1 = {}
    for c in LC.all_cases():
        if not c.inexact and LC.form1_ok(c, LC.oracle_close(O, c)[1]):
            f1[c.fam] = f1.get(c.fam, 0) + 1
    assert f1 == {"a": 19, "b": 327, "d": 13, "e": 34}              # what the GPU file runs in form 1 (rows permitting)
    assert all(c.it == 0 and c.form0_only for c in LC.all_cases() if c.fam == "c")


def test_sums_are_exact_in_any_order():
    rng = np.random.default_rng(1)
    for c in LC.all_cases():
        if c.inexact or c.rows.shape[0] < 2 or not np.all(np.isfinite(c.rows)):
            continue
        exact = np.array([math.fsum(c.rows[:, k]) for k in range(28)])
        for _ in range(3):
            r = c.rows[rng.permutation(c.rows.shape[0])]
            assert np.array_equal(np.cumsum(r, 0)[-1], exact), c.name                 # left to right
            assert np.array_equal(np.sum(r, 0), exact), c.name                        # numpy's pairwise tree
    a = next(c for c in LC.all_cases() if c.name == "a_rows512")
    AtA, AtB, n = LC.intended(a.rows)
    vals = np.concatenate([AtA[np.triu_indices(6)], AtB])
    assert len(set(vals.tolist())) == 27 and n == 4512, "28 distinct sums: any mis-mapped index shows"
    assert np.array_equal(AtA, AtA.T)
    big = next(c for c in LC.all_cases() if c.name == "a_count_2p24p1")
    assert LC.intended(big.rows)[2] == 2 ** 24 + 1 and int(F32(2 ** 24 + 1)) == 2 ** 24        # exact as an int, not as a float


def test_the_inexact_case_is_inexact_and_its_bar_is_tight():
    c = next(c for c in LC.all_cases() if c.inexact)
    lo, hi = LC.inexact_bounds(c.rows)
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(20):
        s = np.cumsum(c.rows[rng.permutation(c.rows.shape[0])], 0)[-1][:27]
        seen.add(s.tobytes())
        assert np.all(s.astype(F32) >= lo) and np.all(s.astype(F32) <= hi)
    assert len(seen) > 1
    assert np.all(hi.astype(np.float64) - lo < 1.0) and np.abs(c.rows[:, :27]).max(0).min() > 1e11   # one lost or doubled row is 1e11 outside


def _np_qr32(A):
    """hal::QR32f's reflectors in numpy fp32, one rounding per operation: R's diagonal and the leading entry each reflector met."""
    A = np.array(A, F32)
    lead = []
    with np.errstate(all="ignore"):
        for l in range(6):
            vl = A[l:, l].copy()
            nrm = F32(0)
            for v in vl:
                nrm = F32(nrm + F32(v * v))
            lead.append(vl[0])
            t = vl[0]
            vl[0] = F32(vl[0] + F32((F32(1) if vl[0] >= 0 else F32(-1)) * np.sqrt(nrm)))
            nrm = np.sqrt(F32(F32(nrm + F32(vl[0] * vl[0])) - F32(t * t)))
            vl = (vl / nrm).astype(F32)
            for j in range(l, 6):
                v = F32(0)
                for i in range(l, 6):
                    v = F32(v + F32(vl[i - l] * A[i, j]))
                for i in range(l, 6):
                    A[i, j] = F32(A[i, j] - F32(F32(F32(2) * vl[i - l]) * v))
    return np.diag(A).copy(), lead


def test_qr_cases_sit_on_their_edges():
    by = {c.name: c for c in LC.all_cases()}
    n_well = 0
    for c in LC.all_cases():
        if not c.name.startswith("b_rand"):
            continue
        AtA, AtB, n = LC.intended(c.rows)
        _, _, _, _, tr = LC.oracle_close(O, c)
        ref = np.linalg.solve(AtA.astype(np.float64), AtB.astype(np.float64))
        cond = np.linalg.cond(AtA.astype(np.float64))
        assert np.abs(np.array(tr.delta) - ref).max() <= 3e-6 * cond * np.abs(ref).max(), c.name
        d = np.sqrt(np.diag(AtA).astype(np.float64))
        assert d[:3].min() > 10 * d[3:].max(), "rotation columns tens of times the translation columns"
        n_well += 1
    assert n_well >= 300
    for i in (5, 2):
        for tag, k, singular in (("prev", -1, True), ("at", 0, False), ("next", 1, False)):
            c = by[f"b_pivot_{tag}_i{i}"]
            AtA, AtB, n = LC.intended(c.rows)
            R, _ = _np_qr32(AtA)
            assert _bits(np.abs(R[i])) == _bits(LC.nxt(LC.QR_TINY, k)), c.name
            conv, _, _, _, tr = LC.oracle_close(O, c)
            assert (not any(tr.delta)) == singular and conv == (1 if singular else 0), c.name
    assert _bits(LC.QR_TINY) == _bits(F32(1.1920929e-06))
    for l in range(6):
        for tag, lead in (("neg", F32(-7.0)), ("pzero", F32(0.0)), ("nzero", F32(-0.0))):
            AtA, _, _ = LC.intended(by[f"b_lead_{tag}_l{l}"].rows)
            _, met = _np_qr32(AtA)
            assert _bits(met[l]) == _bits(lead), (tag, l)
            assert l == 5 or np.any(AtA[l + 1:, l] != 0)
    # the ground-only case: exactly rank 3, singular to the solve, X = 0 - which converges
    c = by["b_rank3_exact"]
    AtA, AtB, _ = LC.intended(c.rows)
    assert np.linalg.matrix_rank(AtA.astype(np.float64)) == 3
    conv, pose, _, _, tr = LC.oracle_close(O, c)
    assert conv == 1 and tr.stepped == 1 and not any(tr.delta) and np.array_equal(_bits(pose), _bits(c.pose0))
    for name in ("b_inf_entry", "b_neg_inf_offdiag", "b_nan_entry", "b_nan_rhs", "b_nan_row", "b_square_overflows", "b_zero_column"):
        _, pose, _, _, _ = LC.oracle_close(O, by[name])
        assert not LC.form1_ok(by[name], pose), name               # no registration pass ever sees these poses


def test_degeneracy_cases_against_fp64_eigenvalues():
    """The independent statement: numpy's fp64 eigenvalues of the same fp32 matrix agree with the oracle's decision wherever
    l_min is farther than 1e-4 l_max from the threshold; the nearer cases are the ones only bit-exact arithmetic gets right."""
    near = {True: 0, False: 0}
    shortcut = {True: 0, False: 0}
    n_deg = {}
    for c in LC.all_cases():
        if c.fam != "c":
            continue
        AtA, AtB, n = LC.intended(c.rows)
        th = float(F32(LC.params_of(c)["eig_thresh"]))
        conv, pose, dg, matP, tr = LC.oracle_close(O, c)
        if not np.all(np.isfinite(AtA)):
            continue
        w = np.linalg.eigvalsh(AtA.astype(np.float64))
        if abs(w[0] - th) > 1e-4 * abs(w[-1]):
            assert dg == (1 if w[0] < th else 0), (c.name, w[0])
            n_deg[int((w < th).sum())] = n_deg.get(int((w < th).sum()), 0) + 1
        else:
            near[bool(w[0] < th)] += 1
        tr_ = float(np.trace(AtA.astype(np.float64)))
        ok = 0.0 < tr_ < 1e30 and w[0] > th + 1e-5 * tr_           # the inequality of the device's Cholesky shortcut
        shortcut[bool(ok)] += 1
        if ok:
            assert dg == 0, c.name                                  # where the shortcut may answer, the full analysis agrees
        if dg:                                                      # the projector removes exactly the flagged directions
            k = int((w < th).sum()) if abs(w[0] - th) > 1e-4 * abs(w[-1]) else None
            if k is not None and k < 6 and w[k] - w[k - 1] > 1e-3 * w[-1]:
                assert np.linalg.matrix_rank(matP.astype(np.float64), tol=1e-3) == 6 - k, c.name
    assert near[True] >= 10 and near[False] >= 10, near
    assert shortcut[True] >= 8 and shortcut[False] >= 8, shortcut
    assert all(n_deg.get(k, 0) >= 3 for k in (0, 1, 2, 3, 5, 6)), n_deg
    by = {c.name: c for c in LC.all_cases()}
    _, _, dg, matP, tr = LC.oracle_close(O, by["c_eye_6_below"])
    assert dg == 1 and not matP.any() and not any(tr.delta)         # all six: matP = 0, X = 0
    assert LC.oracle_close(O, by["c_eye_100"])[2] == 0 and LC.oracle_close(O, by["c_eye_100-1ulp"])[2] == 1   # `<`, not `<=`


def test_later_iterations_project_exactly_when_flagged():
    for c in LC.all_cases():
        if c.fam != "d":
            continue
        AtA, AtB, n = LC.intended(c.rows)
        x, ok = O.solve6_qr(AtA, AtB)
        _, _, dg, matP, tr = LC.oracle_close(O, c)
        assert ok and dg == c.degen_in and np.array_equal(_bits(matP), _bits(c.matP_in))
        want = (c.matP_in.astype(np.float64) @ x.astype(np.float64)).astype(F32) if c.degen_in else x
        assert np.abs(np.array(tr.delta, np.float64) - want).max() <= 1e-6 * np.abs(want).max() + 1e-12
        if not c.degen_in:
            assert np.array_equal(_bits(tr.delta), _bits(x))


def test_convergence_cases_sit_on_their_edges():
    by = {c.name: c for c in LC.all_cases()}
    c05 = F32(0.05)
    assert float(c05) > 0.05 and float(LC.nxt(c05, -1)) < 0.05      # 0.05f itself does not converge
    for tag, k in (("prev", -1), ("at", 0), ("next", 1)):
        conv, _, _, _, tr = LC.oracle_close(O, by[f"e_deltaR_{tag}"])
        assert _bits(tr.deltaR) == _bits(LC.nxt(c05, k)) and _bits(tr.deltaT) == _bits(F32(0.01)) and conv == (k < 0)
        conv, _, _, _, tr = LC.oracle_close(O, by[f"e_deltaT_{tag}"])
        assert _bits(tr.deltaT) == _bits(LC.nxt(c05, k)) and _bits(tr.deltaR) == _bits(F32(0.01)) and conv == (k < 0)
    for a in ("in", "out"):
        for b in ("in", "out"):
            for ee in (1, 0):
                assert LC.oracle_close(O, by[f"e_R{a}_T{b}_early{ee}"])[0] == (a == "in" and b == "in")
    # a threshold whose float lies BELOW it: the float itself converges in double, and would not in float
    assert float(F32(0.7)) < 0.7
    for q in ("deg", "cm"):
        assert [LC.oracle_close(O, by[f"e_conv_{q}0.7_{t}"])[0] for t in ("prev", "at", "next")] == [1, 1, 0]
        assert [LC.oracle_close(O, by[f"e_conv_{q}0.1_{t}"])[0] for t in ("prev", "at", "next")] == [1, 0, 0]
        assert [LC.oracle_close(O, by[f"e_conv_{q}0.02_{t}"])[0] for t in ("prev", "at", "next")] == [1, 1, 0]
    assert float(F32(0.02)) < 0.02 and float(F32(0.1)) > 0.1


# ---- the scenes of the persistence and threshold tests ---------------------------------------------------------------
def test_persistence_sequence_on_the_oracle():
    """One Oracle object through the five registrations: the members give 1, 1, 1, 1, 0; then a single wall is degenerate
    in another subspace than the ground (matP has to be rebuilt, not carried)."""
    orc = O.Oracle(knn_backend=1, num_threads=8)
    flags, skipped = [], []
    for name, m, q, pose in LC.persistence_sequence():
        orc.set_map(m)
        orc.set_scan(q)
        r = orc.scan2MapOptimization(pose)
        flags.append(r.is_degenerate)
        skipped.append(r.skipped)
        if name == "ground only":
            P_ground, d = orc.matP()
            assert d == 1
        if name.startswith("fewer"):
            assert r.n_sel_last < 50 and r.iters_run == 30
    assert flags == [1, 1, 1, 1, 0] and skipped == [0, 0, 2, 1, 0]
    m, q = LC.scene_wall()
    orc.set_map(m)
    orc.set_scan(q)
    r = orc.scan2MapOptimization(LC.SCENE_POSE)
    P_wall, d = orc.matP()
    assert r.is_degenerate == 1 and d == 1 and r.skipped == 0
    assert np.abs(P_wall - P_ground).max() > 0.5                     # another subspace
    k = np.linalg.matrix_rank(P_wall.astype(np.float64), tol=1e-3)
    assert 1 <= k <= 5


def test_threshold_scenes_step_across_the_threshold():
    lmins, in_band, deg = [], 0, []
    for n in LC.PATCH_SIZES:
        m, q = LC.scene_threshold(n)
        AtA, AtB, cnt, lmin = LC.iteration0_lmin(O, m, q, LC.SCENE_POSE)
        lmins.append(lmin)
        in_band += abs(lmin - 100.0) <= 1e-3 * 100.0
        orc = O.Oracle(knn_backend=1, num_threads=8)
        orc.set_map(m)
        orc.set_scan(q)
        deg.append(orc.scan2MapOptimization(LC.SCENE_POSE).is_degenerate)
        if abs(lmin - 100.0) > 1e-3 * 100.0:
            assert deg[-1] == (1 if lmin < 100.0 else 0), n
    assert len(LC.PATCH_SIZES) >= 12 and in_band <= 2
    assert lmins == sorted(lmins) and lmins[0] < 20.0 and lmins[-1] > 150.0
    assert sum(deg) >= 4 and len(deg) - sum(deg) >= 4
    assert sum(1 for v in lmins if abs(v - 100.0) < 5.0) >= 3         # several scenes close to the threshold
