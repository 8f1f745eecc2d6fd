"""CPU tests of the pose graph's host side (include/liorf_s2m.h, "Pose graph"): the exported symbols, the defaults
against the reference's literals (src/mapOptmization.cpp:1390, :1394, :712-719), s2m_pg_check_args, and the CPU
reference's own sanity (tests/ref/pose_graph_ref.py): analytic Jacobians against central differences, the gradient
at the converged estimate, and the agreement of its three linear solvers."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m  # noqa: E402

PG_SYMBOLS = ["s2m_pg_default_params", "s2m_pg_check_args", "s2m_pg_reset", "s2m_pg_size", "s2m_pg_add_prior", "s2m_pg_add_between",
              "s2m_pg_add_gps", "s2m_pg_set_initial", "s2m_pg_add_odometry", "s2m_pg_optimize", "s2m_pg_get_poses", "s2m_pg_marginal",
              "s2m_pg_apply_to_store"]
# the observation hooks of the stages: outside the drop-in boundary (include/liorf_s2m_debug.h)
PG_DEBUG_SYMBOLS = ["s2m_debug_pg_rebase", "s2m_debug_pg_set_estimate", "s2m_debug_pg_linearize", "s2m_debug_pg_apply",
                    "s2m_debug_pg_apply_check_args", "s2m_debug_pg_cg", "s2m_debug_pg_retract"]


def test_symbols_are_exported_and_declared():
    lib = s2m.load_library()
    header = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    debug = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    for names, text, other in ((PG_SYMBOLS, header, debug), (PG_DEBUG_SYMBOLS, debug, header)):
        for name in names:
            assert hasattr(lib, name), name
            assert name in s2m.ABI_SYMBOLS, name
            assert name + "(" in text and name + "(" not in other, name


def test_defaults_are_the_reference_literals():
    p = s2m.default_pg_params()
    assert list(p.prior_var) == [1e-2, 1e-2, math.pi * math.pi, 1e8, 1e8, 1e8]
    assert list(p.odom_var) == [1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]
    assert list(p.sc_loop_var) == [0.5] * 6 and p.sc_loop_robust_k == 1.0
    assert p.max_iterations == 100 and p.relative_error_tol == 1e-5 and p.absolute_error_tol == 1e-5
    assert list(p.prior_var) == list(P.PRIOR_VAR) and list(p.odom_var) == list(P.ODOM_VAR)


def test_check_args_verdicts():
    ok6, v6 = [0.1] * 6, [1.0] * 6
    chk = s2m.pg_check_args
    assert chk(s2m.S2M_PG_PRIOR, 0, 0, 0, ok6, v6) == 0
    assert chk(s2m.S2M_PG_BETWEEN, 5, 4, 5, ok6, v6, 0.0) == 0          # key 5 is new
    assert chk(s2m.S2M_PG_BETWEEN, 5, 4, 0, ok6, v6, 1.0) == 0          # a Cauchy loop
    assert chk(s2m.S2M_PG_GPS, 5, 2, 0, [1, 2, 3], [1, 1, 4]) == 0
    assert chk(s2m.S2M_PG_INITIAL, 5, 5, 0, ok6, None) == 0
    bad = -1
    assert chk(s2m.S2M_PG_BETWEEN, 5, 3, 3, ok6, v6) == bad             # self loop
    assert chk(s2m.S2M_PG_BETWEEN, 5, 4, 6, ok6, v6) == bad             # key gap
    assert chk(s2m.S2M_PG_PRIOR, 5, 6, 0, ok6, v6) == bad               # key gap
    assert chk(s2m.S2M_PG_INITIAL, 5, 7, 0, ok6, None) == bad
    assert chk(s2m.S2M_PG_PRIOR, 5, -1, 0, ok6, v6) == bad
    assert chk(s2m.S2M_PG_BETWEEN, 5, 1, -2, ok6, v6) == bad
    for k in range(6):
        for x in (np.nan, np.inf, -np.inf):
            p = list(ok6); p[k] = x
            assert chk(s2m.S2M_PG_PRIOR, 5, 1, 0, p, v6) == bad
        for x in (0.0, -1.0, np.nan, np.inf):
            v = list(v6); v[k] = x
            assert chk(s2m.S2M_PG_BETWEEN, 5, 1, 2, ok6, v) == bad
    assert chk(s2m.S2M_PG_GPS, 5, 1, 0, [0, np.nan, 0], [1, 1, 1]) == bad
    assert chk(s2m.S2M_PG_GPS, 5, 1, 0, [0, 0, 0], [1, 0, 1]) == bad
    assert chk(s2m.S2M_PG_BETWEEN, 5, 1, 2, ok6, v6, -1.0) == bad
    assert chk(s2m.S2M_PG_BETWEEN, 5, 1, 2, ok6, v6, np.nan) == bad
    assert chk(s2m.S2M_PG_PRIOR, 5, 1, 0, None, v6) == bad
    assert chk(s2m.S2M_PG_PRIOR, 5, 1, 0, ok6, None) == bad
    assert chk(7, 5, 1, 0, ok6, v6) == bad


def _rnd_pose(rng):
    return P.so3_exp(rng.normal(0, 0.8, 3)), rng.normal(0, 3, 3)


def _check_jacobians(Xi, Xj, Z, h, tol):
    _r, Ji, Jj = P.between_residual(Xi, Xj, *Z)
    _rp, Dp = P.prior_residual(Xj, *Z)
    worst = 0.0
    for a in range(6):
        d = np.zeros(6); d[a] = h
        ni = (P.between_residual(P.retract(*Xi, d), Xj, *Z, jac=False) - P.between_residual(P.retract(*Xi, -d), Xj, *Z, jac=False)) / (2 * h)
        nj = (P.between_residual(Xi, P.retract(*Xj, d), *Z, jac=False) - P.between_residual(Xi, P.retract(*Xj, -d), *Z, jac=False)) / (2 * h)
        npr = (P.prior_residual(P.retract(*Xj, d), *Z)[0] - P.prior_residual(P.retract(*Xj, -d), *Z)[0]) / (2 * h)
        worst = max(worst, np.abs(ni - Ji[:, a]).max(), np.abs(nj - Jj[:, a]).max(), np.abs(npr - Dp[:, a]).max())
    assert worst < tol, worst
    return worst


def test_reference_jacobians_against_central_differences():
    rng = np.random.default_rng(P.SEED)
    for _ in range(10):
        _check_jacobians(_rnd_pose(rng), _rnd_pose(rng), _rnd_pose(rng), 1e-6, 1e-7)
    # residual rotations of pi - d about a skew axis: Xj = Xi Z Exp(w) for the between factor, Xj = Z Exp(w) for the prior.
    # The step stays inside the distance to pi (the log's cut) and, at 4.6e-3 and 4.4e-3, on its side of the branch threshold
    # (4.472e-3): h = d / 100, at most 1e-6.  The differences' own rounding is 1e-16 / sin(theta) / h per entry in the general
    # branch (5e-9 at d = 4.6e-3 with h = 1e-6), 1e-16 / h in the near-pi one (1e-8 at d = 1e-6 with h = 1e-8); 1e-6 covers
    # both with the truncation h^2, and is a millionth of the 0.94 the log's former near-pi axis was off by.
    axis = np.array([0.6, 0.64, 0.48]) / np.linalg.norm([0.6, 0.64, 0.48])
    for d in (1e-2, 4.6e-3, 4.4e-3, 1e-3, 1e-6):
        Xi, Z = _rnd_pose(rng), _rnd_pose(rng)
        E = (P.so3_exp((math.pi - d) * axis), np.array([0.3, -0.2, 0.1]))
        # the prior residual is taken at Xj against Z: give it the same residual rotation
        Zp = (Z[0], Z[1])
        Xj_prior = (Zp[0] @ E[0], Zp[1] + Zp[0] @ E[1])
        h = min(1e-6, d / 100)
        ZE = (Z[0] @ E[0], Z[1] + Z[0] @ E[1])
        Xj = (Xi[0] @ ZE[0], Xi[1] + Xi[0] @ ZE[1])
        worst = _check_jacobians(Xi, Xj, Z, h, 1e-6)
        _rp, Dp = P.prior_residual(Xj_prior, *Zp)
        for a in range(6):
            dd = np.zeros(6); dd[a] = h
            npr = (P.prior_residual(P.retract(*Xj_prior, dd), *Zp)[0] - P.prior_residual(P.retract(*Xj_prior, -dd), *Zp)[0]) / (2 * h)
            worst = max(worst, np.abs(npr - Dp[:, a]).max())
        print("pi -", d, "largest gap to central differences", worst)
        assert worst < 1e-6
        assert abs(np.linalg.norm(P.between_residual(Xi, Xj, *Z, jac=False)[:3]) - (math.pi - d)) < 1e-12


def test_reference_converges_to_a_stationary_point_and_its_solvers_agree():
    out = {}
    for solver in ("dense_sqrt", "normal", "chain_sqrt"):
        g = CS.build("loops_200")
        res = P.optimize(g, solver, rel_tol=0.0, abs_tol=0.0, max_iterations=8)
        J, r = P.assemble(P.linearize(g, g.X)[0], g.n)
        grad = J.T @ r
        # gradient against the scale of its terms |J|^T |r|
        assert np.abs(grad).max() <= 1e-6 * (abs(J).T @ np.abs(r)).max(), solver
        out[solver] = (res.error_after, g.poses())
    for solver in ("normal", "chain_sqrt"):
        assert abs(out[solver][0] - out["dense_sqrt"][0]) <= 1e-9 * out["dense_sqrt"][0]
        rot, trans = P.pose_gap(out[solver][1], out["dense_sqrt"][1], relative=True)
        assert rot < 1e-7 and trans < 1e-6


def test_bounds_file_holds_every_case_and_keeps_key0_far_below_a_gauge_drift():
    b = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_bounds.json")))
    for name in CS.SMALL + CS.LARGE + (CS.INCREMENTAL,):
        assert name in b
        if name in CS.LARGE:
            assert b[name]["bound"]["key0_trans"] < 1e-3      # a naive solve drifts by 1 to 100 m
        assert set(b[name]["bound"]) == set(b[name]["floor"])
        for k, v in b[name]["bound"].items():
            assert v == pytest.approx(10 * b[name]["floor"][k], rel=1e-12, abs=0.0)      # a hand-edited bound is caught
