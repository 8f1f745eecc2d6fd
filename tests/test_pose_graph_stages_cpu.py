"""CPU tests of the pose graph's stage references (tests/ref/pose_graph_stages_ref.py) and of the observation hooks' host side
(include/liorf_s2m_debug.h, s2m_debug_pg_*): the fp64 reference against the 50-digit one where the rotation log and the SO(3)
Jacobians change branch, the longdouble substitutions against a dense solve, the numpy blocked scan's levels, the bounds file,
and the hooks' answers that need no GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_ref as P  # noqa: E402
import pose_graph_stages_ref as S  # noqa: E402
from liorf_amd import s2m  # noqa: E402

AXIS = S.SKEW_AXIS / np.linalg.norm(S.SKEW_AXIS)
NEAR_PI = (1e-2, 4.6e-3, 4.4e-3, 1e-3, 1e-6)
SMALL = (1e-11, 1e-6, 1e-4)


def _exact_rotation(theta, axis=AXIS):
    """exp(theta axis) in 50 digits, rounded to fp64 entry by entry, and theta axis itself."""
    w = [S.mpf(a) * S.M.mpf(theta) for a in axis]
    return np.array([[float(x) for x in row] for row in S.mp_exp(w)]), w


def _log_error(R, w):
    got = P.so3_log(R)
    return float(max(abs(S.mpf(g) - x) for g, x in zip(got, w)))


@pytest.mark.parametrize("theta", [math.pi - d for d in NEAR_PI] + list(SMALL) + [S.THRESH - 1e-7, S.THRESH + 1e-7])
def test_fp64_log_against_the_angle_and_axis_it_was_built_from(theta):
    """The log of exp(theta a), a the skew axis: theta a by construction, no formula of the log involved.  The entries of R
    are rounded to fp64 (1.1e-16); atan2(s, c) / s amplifies that by 1 / sin(theta) in the general branch, the near-pi branch
    (symmetric part, entries of size 1) does not: 16 roundings of 1.1e-16 each, through at most pi / sin(theta)."""
    R, w = _exact_rotation(theta)
    err = _log_error(R, w)
    near = 0.5 * (np.trace(R) - 1.0) < -0.99999
    bound = 16 * 1.1e-16 * (math.pi if near else max(1.0, math.pi / abs(math.sin(theta))))
    print("theta", theta, "pi - theta", math.pi - theta, "near-pi branch", near, "error", err, "bound", bound)
    assert err <= bound


def test_fp64_log_near_pi_for_random_axes():
    rng = np.random.default_rng(P.SEED)
    worst = 0.0
    for _ in range(200):
        a = rng.normal(0, 1, 3)
        a /= np.linalg.norm(a)
        theta = math.pi - 10.0 ** rng.uniform(-9, math.log10(4.4e-3))
        R, w = _exact_rotation(theta, a)
        assert 0.5 * (np.trace(R) - 1.0) < -0.99999
        worst = max(worst, _log_error(R, w))
    print("largest error of the near-pi branch over 200 axes", worst)
    assert worst <= 16 * 1.1e-16 * math.pi


def test_the_two_branches_of_the_log_agree_at_the_threshold():
    lo, wl = _exact_rotation(S.THRESH - 1e-9)
    hi, wh = _exact_rotation(S.THRESH + 1e-9)
    assert 0.5 * (np.trace(lo) - 1.0) > -0.99999 > 0.5 * (np.trace(hi) - 1.0)
    # both within the general branch's rounding (1 / sin = 224) of their own truth, 2e-9 apart: no jump
    for R, w in ((lo, wl), (hi, wh)):
        assert _log_error(R, w) <= 16 * 1.1e-16 * math.pi / math.sin(S.THRESH)
    assert np.abs(P.so3_log(hi) - P.so3_log(lo)).max() <= 2e-9 + 1e-12


@pytest.mark.parametrize("theta", [9e-6, 1.1e-5] + list(SMALL) + [0.3, 2.5] + [math.pi - d for d in NEAR_PI])
def test_fp64_so3_jacobians_against_central_differences_in_50_digits(theta):
    """so3_jr_inv and so3_jr on both sides of their switch at |phi|^2 = 1e-10 (|phi| = 1e-5) and near pi: Jr^-1(phi) is the
    derivative of Log(Exp(phi) Exp(d)) at d = 0, Jr its inverse.  Near pi the closed form's (1 + cos) / sin keeps
    1.1e-16 / (1 + cos) of its digits; elsewhere 1e-14 covers the handful of roundings on entries of size up to 1.6.
    Measured: so3_jr is off by 1.0e-11 at 1.1e-5 and 1.7e-13 at 1e-4 (its 1 - cos), 3e-16 below the switch."""
    w = [S.mpf(a) * S.M.mpf(theta) for a in AXIS]
    phi = np.array([float(x) for x in w])
    R = S.mp_exp([S.mpf(x) for x in phi])
    f = lambda X: S.mp_log(X[0])
    J = S.mp_jacobian(f, (R, [S.M.mpf(0)] * 3))
    want_inv = [[J[r][c] for c in range(3)] for r in range(3)]
    want = (S.M.matrix(want_inv) ** -1).tolist()
    gi = S.block_gap(P.so3_jr_inv(phi).tolist(), want_inv)
    gj = S.block_gap(P.so3_jr(phi).tolist(), want)
    bound = max(1e-14, 4 * 1.1e-16 / (1.0 + math.cos(theta)))
    # so3_jr above the switch: 1 - cos(th) is off by up to 1.1e-16, the K term (1 - cos) / th^2 K by 1.1e-16 / th per entry;
    # twice that for the rounding of cos itself (the form is the device's; 2 sin^2(th / 2) would not lose it)
    bound_jr = max(1e-14, 2.2e-16 / theta if theta * theta >= 1e-10 else 0.0)
    print("theta", theta, "jr_inv gap", gi, "bound", bound, "jr gap", gj, "bound", bound_jr)
    assert gi <= bound and gj <= bound_jr


def test_longdouble_substitutions_against_a_dense_solve():
    calls, X = S.chain_case(65)
    Binv, Aof = S.chain_blocks_fp64(S.graph_of(calls, X))
    n = 65
    Jc = np.zeros((6 * n, 6 * n))
    for i in range(n):
        Jc[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.linalg.inv(Binv[i])
        if i:
            Jc[6 * i:6 * i + 6, 6 * i - 6:6 * i] = Aof[i]
    V = np.concatenate(S.scan_vectors(n)).T
    f, b = S.fwd_ld(Binv, Aof, V), S.bwd_ld(Binv, Aof, V)
    # the dense fp64 check has the conditioning of J_c against it: residuals instead of solutions
    assert np.abs(Jc @ f.astype(np.float64) - V).max() <= 1e-9 * np.abs(V).max()
    assert np.abs(Jc.T @ b.astype(np.float64) - V).max() <= 1e-9 * np.abs(V).max()


@pytest.mark.parametrize("n", [1, 2, 32, 33, 1025])
def test_numpy_blocked_scan_is_the_sequential_recurrence(n):
    calls, X = S.chain_case(n)
    Binv, Aof = S.chain_blocks_fp64(S.graph_of(calls, X))
    V = np.concatenate(S.scan_vectors(n)).T
    assert S.col_gap(S.blocked_scan_f64(Binv, Aof, V, 0), S.fwd_ld(Binv, Aof, V)) <= 1e-12
    assert S.col_gap(S.blocked_scan_f64(Binv, Aof, V, 1), S.bwd_ld(Binv, Aof, V)) <= 1e-12


def test_graph40_holds_the_cases_the_stage_tests_name():
    g, names, calls = S.graph40()
    ex = S.extras_of(g)
    assert g.n == 40 and len(names) == len(ex) == len(calls) - 40
    assert ("between", 5, 6) in ex and any(k == "between" and j < i for k, i, j in ex)
    touching17 = [(k, i, j) for k, i, j in ex if 17 in (i, j)]
    assert len(touching17) == 3 and {17 == i for _k, i, _j in touching17} == {True, False}
    fac = S.fp64_factors(g, g.X)
    chain = set(P.split_chain(g))
    rot = {name: float(np.linalg.norm(f["r"][:3] / np.sqrt(1.0 / 0.5) / math.sqrt(f["w"]))) for name, f in
           zip(names, [f for k, f in enumerate(fac) if k not in chain]) if name.startswith(("near_pi", "rot_", "below", "above"))}
    for name, ang in (("near_pi_4.6e-3", math.pi - 4.6e-3), ("near_pi_4.4e-3_cauchy", math.pi - 4.4e-3), ("near_pi_1e-6", math.pi - 1e-6),
                      ("rot_1e-11", 1e-11), ("rot_1e-4", 1e-4), ("below_threshold", S.THRESH - 1e-7), ("above_threshold", S.THRESH + 1e-7)):
        assert abs(rot[name] - ang) <= 1e-14 + 1e-9 * min(ang, 1e-3), (name, rot[name], ang)
    w = {name: f["w"] for name, f in zip(names, [f for k, f in enumerate(fac) if k not in chain])}
    assert w["cauchy_satisfied_8_3"] > 0.999999 and w["cauchy_outlier_6m_25_14"] < 0.05


def test_stage_bounds_file_holds_every_case_and_ten_times_its_floor():
    b = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_stages_bounds.json")))
    _g, names, _calls = S.graph40()
    assert set(b["linearize"]) == set(names) | set(_g.chain_names) | {"total"}
    assert len(set(_g.chain_names)) == 9
    assert set(b["scan"]) == {str(n) for n in S.SCAN_N}
    assert set(b["products"]) == set(S.PRODUCT_CASES) and set(b["cg"]) == set(S.CG_CASES)
    for stage in b.values():
        for case in stage.values():
            assert set(case["bound"]) == set(case["floor"])
            for k, v in case["bound"].items():
                assert case["floor"][k] >= S.ULP
                assert v == pytest.approx(10 * case["floor"][k], rel=1e-12, abs=0.0)      # a hand-edited bound is caught


def test_hooks_answer_without_a_gpu():
    lib = s2m.load_library()
    chk = s2m.pg_apply_check_args
    assert chk(40, 14, s2m.S2M_DEBUG_PG_FWD, 0) == 0 and chk(1, 0, s2m.S2M_DEBUG_PG_BWD, s2m.S2M_PG_BLOCK_COLUMNS) == 0
    assert chk(40, 14, s2m.S2M_DEBUG_PG_K, 13) == 0 and chk(40, 1, s2m.S2M_DEBUG_PG_KT, 1) == 0
    bad = -1
    assert chk(0, 0, 0, 0) == bad and chk(40, -1, 0, 0) == bad
    assert chk(40, 14, -1, 0) == bad and chk(40, 14, 4, 0) == bad
    assert chk(40, 14, 0, -1) == bad and chk(40, 14, 0, s2m.S2M_PG_BLOCK_COLUMNS + 1) == bad
    assert chk(40, 0, s2m.S2M_DEBUG_PG_K, 0) == bad and chk(40, 0, s2m.S2M_DEBUG_PG_KT, 0) == bad
    assert chk(40, 14, 0, 0, has_in=False) == bad and chk(40, 14, 0, 0, has_out=False) == bad
    assert lib.s2m_debug_pg_set_estimate(None, 0, None) == bad
    assert lib.s2m_debug_pg_linearize(None, 0, 0, *([None] * 10)) == bad
    assert lib.s2m_debug_pg_apply(None, 0, 0, None, None) == bad
    assert lib.s2m_debug_pg_cg(None, None, 0, None, None, None) == bad
    assert lib.s2m_debug_pg_retract(None, 0, None, None) == bad
