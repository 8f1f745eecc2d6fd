"""GPU tests of the pose graph stage by stage, through the observation hooks s2m_debug_pg_* (include/liorf_s2m_debug.h): the
linearisation against a 50-digit mpmath reference, the blocked scans and the extra factors' products against longdouble
substitutions built from the blocks the device returned, the CG against its true residual, the retraction, and the read-out at
the edges of the Euler angles.  References: tests/ref/pose_graph_stages_ref.py.  Bounds: tests/golden/pose_graph_stages_bounds.json,
written by tests/golden/make_golden_pose_graph_stages.py (10 x a floor measured on the CPU, never on the device).  Every test
prints the device's gaps beside their bounds.

Measured on an MI355X (gap / bound; no stage came within a factor 2 of its bound, the closest is ferr of the chain's prior at 0.45):
  linearize  near-pi cases with the parent's log (axis from R[:, k] + e_k), rx / Ji / Jj:
               near_pi_4.4e-3_cauchy 3.2e-3 / 9.2e-4 / 3.3e-3   against bounds 2.2e-15 / 4.9e-15 / 1.5e-14
               near_pi_1e-6          7.3e-7 / 2.6e-7 / 7.5e-7   against bounds 2.2e-15 / 1.4e-10 / 4.2e-10
               above_threshold       3.3e-3 / 1.2e-3 / 3.4e-3   against bounds 2.2e-15 / 1.2e-14 / 3.0e-14
             with the axis from the symmetric part: 1.0e-16 / 4.3e-16 / 1.4e-15, 2.1e-16 / 1.4e-11 / 4.2e-11, 2.7e-16 / 1.3e-15 /
             3.1e-15; below_threshold 1.7e-14 / 1.4e-14 / 1.8e-14 against 1.5e-13 / 1.6e-13 / 1.6e-13.  Binv of the chain:
             4.4e-13 / 4.4e-12 at |phi| = 1.1e-5, 2.4e-14 / 2.4e-13 at 1e-4, below 5e-16 / 2.2e-15 elsewhere.
  scan       n: fwd gap / bound, bwd gap / bound
             1: 2.3e-16 / 2.2e-15, 2.2e-16 / 2.2e-15          2: 4.4e-16 / 2.8e-15, 2.7e-16 / 3.6e-15
             31: 1.1e-15 / 9.9e-15, 1.7e-15 / 2.0e-14         32: 1.1e-15 / 8.8e-15, 1.1e-15 / 1.5e-14
             33: 1.3e-15 / 9.6e-15, 2.5e-15 / 5.2e-14         64: 1.5e-15 / 9.5e-15, 2.7e-15 / 2.4e-14
             65: 1.6e-15 / 1.4e-14, 1.4e-15 / 4.5e-14         1023: 6.5e-15 / 4.6e-14, 4.2e-15 / 6.6e-14
             1024: 6.4e-15 / 4.3e-14, 5.0e-15 / 7.1e-14       1025: 1.1e-14 / 5.6e-14, 8.1e-15 / 6.6e-14
             1057: 3.6e-15 / 7.4e-14, 1.0e-14 / 3.3e-14       32769: 2.3e-14 / 5.0e-13, 2.8e-14 / 4.4e-13
  products   graph40 K 1.3e-15 / 1.9e-14, K^T 3.1e-15 / 3.8e-14; loops_200 K 6.4e-11 / 9.6e-10, K^T 3.7e-10 / 3.1e-9
  cg         drift of the recurrence's residual from the true one: loops_200 2.2e-13 / 2.8e-12 (one iteration), 8.8e-13 / 1.3e-11
             (10 iterations, true residual 9.0e-13); gps_120 1.8e-14 / 1.8e-13, 5.5e-12 / 5.4e-11 (19 iterations, true 5.5e-12)
  retract    rotation at most 1.1e-16 / 1.8e-15, translation 2.5e-15 / 5.9e-14; ||R^T R - I|| of the results 2.8e-16 to 6.1e-16
  read-out   every float equal to the reference's; at pitch +-float(pi/2) with zero roll and yaw the device gives roll = yaw = -pi
             where the reference gives +pi (the sign of a zero entry)."""
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
import pose_graph_stages_ref as S  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
LD = S.LD
BOUNDS = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_stages_bounds.json")))
FWD, BWD, K_OP, KT_OP = s2m.S2M_DEBUG_PG_FWD, s2m.S2M_DEBUG_PG_BWD, s2m.S2M_DEBUG_PG_K, s2m.S2M_DEBUG_PG_KT


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _load(gpu, name):
    g, calls = S.case_graph(name)
    if calls is not None:
        S.load_calls(gpu, calls, g.X)
    else:
        CS.load_into(gpu, g)
    return g


# ---- the linearisation ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lin40(gpu):
    g, names, calls = S.graph40()
    S.load_calls(gpu, calls, g.X)
    dev = gpu.pgLinearize()
    want = S.stage_arrays(g, S.mp_factors(g, g.X), S.mp_inverse)
    return g, names, dev, want


def test_linearisation_of_the_40_key_graph_against_mpmath(lin40):
    """Every array of s2m_debug_pg_linearize against the 50-digit reference, case by case.  With the rotation log of the parent
    commit (axis from R[:, k] + e_k) the cases inside the near-pi branch miss their bounds: rx, Ji, Jj of
    near_pi_4.4e-3_cauchy and above_threshold by 1e-3 to 3e-3 against bounds of 6e-15 to 3e-14, of near_pi_1e-6 by 3e-7 to
    8e-7; with the axis from the symmetric part all pass.  Binv of the chain keeps 2.2e-16 / |phi| of its rotation block where
    the residual rotation lies above Jr's switch at 1e-5 (measured 4e-13 at 1.1e-5): that is the reference's closed form too,
    so those cases' floors hold it."""
    g, names, dev, want = lin40
    gaps = S.linearize_gaps(dev, want, names, g.chain_names)
    missed = []
    for case, arrays in gaps.items():
        for a, gap in arrays.items():
            bound = BOUNDS["linearize"][case]["bound"][a]
            print("linearize", case, a, "gap", gap, "bound", bound, "" if gap <= bound else "MISSED", "(within a factor 2)" if bound / 2 < gap <= bound else "")
            if not gap <= bound:
                missed.append((case, a, gap, bound))
    assert not missed, missed


def test_linearisation_error_sum_weights_and_branches(lin40):
    g, names, dev, want = lin40
    n = g.n
    robust = {n + x for x, name in enumerate(names) if "cauchy" in name}
    for f in range(n + len(names)):
        if f not in robust:
            assert dev["fw"][f] == 1.0, f                       # exactly 1 on every non-robust factor
        else:
            assert 0.0 < dev["fw"][f] < 1.0
    # err is the sum of the error terms: one per thread, then the 8 levels of the workgroup's tree, 2^-53 each
    total = float(sum(S.mpf(x) for x in dev["ferr"]))
    print("err", dev["err"], "sum of ferr", total, "reference", float(want["err"]), "wmin", dev["wmin"], "reference", float(want["wmin"]))
    assert abs(dev["err"] - total) <= 8 * 2.0 ** -53 * total
    assert dev["wmin"] == dev["fw"].min() and dev["wmin"] == dev["fw"][n + names.index("cauchy_outlier_6m_25_14")]
    # the two branches of the log agree to rounding at the threshold: the factors 1e-7 below and above it both match the
    # reference inside bounds that hold no jump (checked above), and their residual rotations are the placed angles
    for name, ang in (("below_threshold", S.THRESH - 1e-7), ("above_threshold", S.THRESH + 1e-7)):
        rot = float(np.linalg.norm(dev["rx"][names.index(name)][:3])) * math.sqrt(0.5)
        print(name, "residual rotation", rot, "placed", ang, "gap", abs(rot - ang))
        assert abs(rot - ang) <= 1e-12


# ---- the blocked scans --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", S.SCAN_N)
def test_scans_against_the_longdouble_substitution(gpu, n):
    """J_c^-1 v and J_c^-T v in the single form and in the block form with 1, 24 and 13 columns, every column another vector,
    plus unit vectors at the first, the last and a group-edge key; column c of a block is bit for bit the single form."""
    calls, X = S.chain_case(n)
    S.load_calls(gpu, calls, X)
    lin = gpu.pgLinearize()
    V, units = S.scan_vectors(n)
    for op, name, ref in ((FWD, "fwd", S.fwd_ld), (BWD, "bwd", S.bwd_ld)):
        want = ref(lin["Binv"], lin["Aof"], np.concatenate([V, units]).T)
        blocks = [gpu.pgApply(op, V[0:1], block=True), gpu.pgApply(op, V[1:25], block=True), gpu.pgApply(op, V[25:38], block=True),
                  gpu.pgApply(op, units, block=True)]
        got = np.concatenate(blocks)
        singles = np.array([gpu.pgApply(op, v) for v in np.concatenate([V, units])])
        assert np.array_equal(got.view(np.uint64), singles.view(np.uint64)), "a block column is not the single form bit for bit"
        gap, bound = S.col_gap(got.T, want), BOUNDS["scan"][str(n)]["bound"][name]
        print("scan n", n, name, "gap", gap, "bound", bound, "(within a factor 2)" if bound / 2 < gap <= bound else "")
        assert gap <= bound


# ---- K v and K^T u ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.PRODUCT_CASES)
def test_extra_factor_products_against_dense_longdouble(gpu, name):
    g = _load(gpu, name)
    lin = gpu.pgLinearize()
    ex = S.extras_of(g)
    Kd = S.dense_k_ld(lin["Binv"], lin["Aof"], lin["Ji"], lin["Jj"], ex)
    V, U = S.product_vectors(name, g.n, len(ex))
    kv = np.array([gpu.pgApply(K_OP, v) for v in V])
    ktu = np.array([gpu.pgApply(KT_OP, u) for u in U])
    assert np.array_equal(kv, gpu.pgApply(K_OP, V, block=True)) and np.array_equal(ktu, gpu.pgApply(KT_OP, U, block=True))
    b = BOUNDS["products"][name]["bound"]
    gk = S.col_gap(kv.T, Kd @ V.T.astype(LD))
    gt = S.col_gap(ktu.T, Kd.T @ U.T.astype(LD))
    print("products", name, "K gap", gk, "bound", b["K"], "K^T gap", gt, "bound", b["KT"],
          "(within a factor 2)" if gk > b["K"] / 2 or gt > b["KT"] / 2 else "")
    assert gk <= b["K"] and gt <= b["KT"]
    # <K v, u> = <v, K^T u>: each side is off by at most its product's bound times the largest entry, summed against the other vector
    for v, u, a, c in zip(V, U, kv, ktu):
        lhs, rhs = np.sum(a.astype(LD) * u.astype(LD)), np.sum(v.astype(LD) * c.astype(LD))
        tol = b["K"] * np.abs(a).max() * np.abs(u).sum() + b["KT"] * np.abs(c).max() * np.abs(v).sum()
        print("products", name, "<Kv,u>", float(lhs), "<v,K^T u>", float(rhs), "gap", float(abs(lhs - rhs)), "bound", float(tol))
        assert abs(lhs - rhs) <= tol


# ---- the CG ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", ["max_iters_1", "default"])
@pytest.mark.parametrize("name", S.CG_CASES)
def test_cg_true_residual_and_stop_rule(gpu, name, label):
    g = _load(gpu, name)
    lin = gpu.pgLinearize()
    ex = S.extras_of(g)
    Kd = S.dense_k_ld(lin["Binv"], lin["Aof"], lin["Ji"], lin["Jj"], ex)
    prm = s2m.default_pg_params(cg_max_iterations=1 if label == "max_iters_1" else 0)
    max_it = 1 if label == "max_iters_1" else S.default_max_cg(len(ex))
    assert prm.cg_rel_tol == S.CG_TOL
    B = np.concatenate([S.cg_rhs(name, g.n), np.zeros((1, 6 * g.n))])
    Y, outs = gpu.pgCg(B, prm, block=True)
    drift_bound = BOUNDS["cg"][name]["bound"][label]
    for c, b in enumerate(B):
        y, (o,) = gpu.pgCg(b, prm)
        assert np.array_equal(y, Y[c]) and (o.rr, o.bb, o.iters, o.stop) == (outs[c].rr, outs[c].bb, outs[c].iters, outs[c].stop)
        assert o.stop == 1
        if not b.any():                                     # b = 0 stops at once
            assert o.iters == 0 and o.bb == 0.0 and not y.any()
            continue
        # bb is the sum of 6n squares in fp64: n_terms * 2^-53 relative at the most
        bb = float(np.sum(b.astype(LD) ** 2))
        assert abs(o.bb - bb) <= 6 * g.n * 2.0 ** -53 * bb
        rec = math.sqrt(o.rr / o.bb)
        true = S.true_residual(Kd, y, b)
        print("cg", name, label, "column", c, "iters", o.iters, "recurrence", rec, "true", true, "drift", abs(true - rec), "bound", drift_bound,
              "(within a factor 2)" if abs(true - rec) > drift_bound / 2 else "")
        # the stop rule of k_pg_cg_beta: inside the tolerance, or out of iterations
        assert 1 <= o.iters <= max_it
        assert o.rr <= S.CG_TOL ** 2 * o.bb or o.iters == max_it
        assert abs(true - rec) <= drift_bound
        if o.iters < max_it:
            assert true <= S.CG_TOL + drift_bound


# ---- the retraction -------------------------------------------------------------------------------------------------

def test_retraction_against_mpmath(gpu):
    """X (+) delta for rotations of 0, 1e-11, 1e-9 (both sides of so3_exp's switch at |w|^2 = 1e-20), 1e-3, 1 and pi - 1e-6.
    Bound by the arithmetic: an entry of Exp(w) carries the rounding of sin / th, (1 - cos) / th^2 and of two products (4 x 2^-53
    on entries of size 1 at the most), an entry of R Exp(w) three such products and two additions: 16 x 2^-53 in all; a
    translation entry three products and three additions on numbers of size max |t|: 8 x 2^-53 max |t|."""
    rng = np.random.default_rng(P.SEED + 5)
    angles = [0.0, 1e-11, 1e-9, 1e-3, 1.0, math.pi - 1e-6]
    n = len(angles)
    X = [(P.so3_exp(rng.normal(0, 1.2, 3)), rng.normal(0, 20, 3)) for _ in range(n)]
    zero = np.zeros(6, F)
    calls = [("prior", 0, zero, P.PRIOR_VAR)] + [("between", k - 1, k, zero, P.ODOM_VAR, 0.0) for k in range(1, n)]
    S.load_calls(gpu, calls, X)
    axis = S.SKEW_AXIS / np.linalg.norm(S.SKEW_AXIS)
    delta = np.array([np.concatenate([a * axis, rng.normal(0, 1, 3)]) for a in angles])
    got = gpu.pgRetract(delta)
    for k in range(n):
        R, t = S.mp_retract(S.mp_state(X[k]), [S.mpf(x) for x in delta[k]])
        gr = float(max(abs(S.mpf(got[k, 3 * i + j]) - R[i][j]) for i in range(3) for j in range(3)))
        gt = float(max(abs(S.mpf(got[k, 9 + i]) - t[i]) for i in range(3)))
        Rn = got[k, :9].reshape(3, 3)
        tmax = float(np.abs(got[k, 9:]).max())
        print("retract |w|", angles[k], "rotation gap", gr, "bound", 16 * 2.0 ** -53, "translation gap", gt, "bound", 8 * 2.0 ** -53 * tmax,
              "||R^T R - I||", float(np.linalg.norm(Rn.T @ Rn - np.eye(3))))
        assert gr <= 16 * 2.0 ** -53 and gt <= 8 * 2.0 ** -53 * tmax
    # the estimates stay
    assert np.array_equal(gpu.pgRetract(np.zeros((n, 6)))[:, 9:], np.array([t for _R, t in X]))


# ---- the read-out ---------------------------------------------------------------------------------------------------

HALF_PI, PI = float(F(math.pi / 2)), float(F(math.pi))
EDGE_POSES = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 0, HALF_PI, 0], [-4, 5, 6, 0, -HALF_PI, 0], [7, -8, 9, 0, 0, PI], [1, 1, 1, 0, 0, -PI],
                       [2, 0, -2, PI, 0, 0], [0, 3, 0, -PI, 0, 0], [5, 5, 5, PI, HALF_PI, -PI], [-1, -2, -3, -PI, -HALF_PI, PI],
                       [10, 20, 30, 0.3, HALF_PI, -0.7], [3, 2, 1, 0.1, -0.2, 0.3]], F)


def _mp_readout(p):
    """The pose vector of Rz(yaw) Ry(pitch) Rx(roll), t in 50 digits from the float pose p, rounded to float."""
    r, pt, y = (S.mpf(x) for x in p[3:])
    cr, sr, cp, sp, cy, sy = S.M.cos(r), S.M.sin(r), S.M.cos(pt), S.M.sin(pt), S.M.cos(y), S.M.sin(y)
    R = [[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]]
    return np.array([p[0], p[1], p[2], float(S.M.atan2(R[2][1], R[2][2])), float(S.M.asin(-R[2][0])), float(S.M.atan2(R[1][0], R[0][0]))], F)


def _load_edge_poses(m):
    m.pgReset()
    zero = np.zeros(6, F)
    m.pgAddPrior(0, EDGE_POSES[0], P.PRIOR_VAR)
    for k in range(1, len(EDGE_POSES)):
        m.pgAddBetween(k - 1, k, zero, P.ODOM_VAR)
    for k, p in enumerate(EDGE_POSES):
        m.pgSetInitial(k, p)


def test_pose_readout_at_the_edges_of_the_angles(gpu):
    """s2m_pg_get_poses at pitch +-float(pi/2), yaw and roll +-float(pi) and the zero pose, within one float ulp of the 50-digit
    composition.  An angle of +-pi is one rotation: where the matrix entry that decides the sign is a zero - its sign exists in
    fp64 and not in mpmath - roll and yaw are compared modulo 2 pi."""
    _load_edge_poses(gpu)
    got = gpu.pgPoses()
    for k, p in enumerate(EDGE_POSES):
        want = _mp_readout(p)
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(got[k]))).astype(np.float64)
        d = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
        d[[3, 5]] = np.minimum(d[[3, 5]], np.abs(2 * math.pi - d[[3, 5]]))
        print("read-out", p.tolist(), "device", got[k].tolist(), "reference", want.tolist(), "gap in ulps", (d / ulp).tolist())
        assert (d <= ulp).all()


def _cloud(rng, n):
    c = synth.to_xyzi(rng.uniform(-20, 20, (n, 3)).astype(F))
    c[:, 4] = rng.uniform(0, 100, n).astype(F)
    return c


def _store_views(m, n):
    keys, local = m.extractSurroundingKeyFrames(float(n), s2m.default_kf_params(map_leaf=0.4), return_map=True)
    cloud, gkeys = m.publishGlobalMap(s2m.default_gmap_params(pose_density=2.0, leaf=0.5), return_keys=True)
    return [np.asarray(x) for x in (keys, local, cloud, gkeys, m.globalMapCloud(0, n, 0.0))]


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_apply_to_store_at_the_edges_and_with_a_not_finite_estimate():
    """The stored transforms at the edge poses are bit for bit those of s2m_kf_set_poses of the same float poses; with a NaN
    and an Inf among the estimates s2m_pg_apply_to_store returns an error and the store - the map of its transforms and what
    its positions select - is byte for byte what it was."""
    rng = np.random.default_rng(P.SEED + 6)
    n = len(EDGE_POSES)
    clouds = [_cloud(rng, int(rng.integers(200, 400))) for _ in range(n)]
    start = np.zeros((n, 6), F)
    start[:, 0] = np.arange(n)
    outs = []
    for direct in (True, False):
        m = s2m.MapOptimizationS2M()
        try:
            for k in range(n):
                m.saveKeyFrame(start[k], float(k), clouds[k])
            _load_edge_poses(m)
            poses = m.pgPoses()
            if direct:
                m.pgApplyToStore(0, n)
            else:
                m.correctPoses(poses, 0)
            views = _store_views(m, n)
            outs.append([poses] + views)
            if direct:
                R, t = P.pose_from_xyzrpy(EDGE_POSES[3])
                bad_R = R.copy()
                bad_R[1, 0] = np.nan
                m.pgSetEstimate(3, bad_R, t)
                m.pgSetEstimate(7, R, np.array([1.0, np.inf, 2.0]))
                with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
                    m.pgApplyToStore(0, n)
                for a, b in zip(views, _store_views(m, n)):
                    _same(a, b)
                # the finite keys alone still go through
                m.pgApplyToStore(0, 3)
                for a, b in zip(views, _store_views(m, n)):
                    _same(a, b)
        finally:
            m.close()
    for a, b in zip(outs[0], outs[1]):
        _same(np.asarray(a), np.asarray(b))


# ---- the hooks leave no trace ---------------------------------------------------------------------------------------

def test_hooks_leave_the_graph_as_a_handle_that_never_saw_them(gpu):
    g = CS.build("loops_200")
    CS.load_into(gpu, g)
    r0 = gpu.pgOptimize()
    want = (r0.iterations, r0.inner_iterations, r0.error_before, r0.error_after, gpu.pgPoses().tobytes(), gpu.pgMarginal(g.n - 1).tobytes())
    CS.load_into(gpu, g)
    rng = np.random.default_rng(3)
    n, m = g.n, len(S.extras_of(g))
    gpu.pgLinearize()
    gpu.pgApply(FWD, rng.normal(0, 1, 6 * n))
    gpu.pgApply(BWD, rng.normal(0, 1, (5, 6 * n)), block=True)
    gpu.pgApply(K_OP, rng.normal(0, 1, 6 * n))
    gpu.pgApply(KT_OP, rng.normal(0, 1, (24, 6 * m)), block=True)
    gpu.pgCg(rng.normal(0, 1, 6 * n))
    gpu.pgCg(rng.normal(0, 1, (7, 6 * n)), block=True)
    gpu.pgRetract(rng.normal(0, 0.1, (n, 6)))
    r1 = gpu.pgOptimize()
    gpu.pgLinearize()
    got = (r1.iterations, r1.inner_iterations, r1.error_before, r1.error_after, gpu.pgPoses().tobytes(), gpu.pgMarginal(g.n - 1).tobytes())
    assert got == want


def test_hooks_are_busy_while_a_launched_optimise_is_pending(gpu):
    g = CS.build("loops_200")
    CS.load_into(gpu, g)
    n = g.n
    code, _ = gpu.pgOptimizeLaunch()
    assert code == s2m.S2M_PG_PENDING
    try:
        R, t = g.X[0]
        for call in (lambda: gpu.pgSetEstimate(0, R, t), gpu.pgLinearize, lambda: gpu.pgApply(FWD, np.zeros(6 * n)),
                     lambda: gpu.pgCg(np.ones(6 * n)), lambda: gpu.pgRetract(np.zeros((n, 6)))):
            with pytest.raises(s2m.S2MError, match="BUSY"):
                call()
    finally:
        code, res = gpu.pgOptimizeCollect()
    assert code == s2m.S2M_OK and res.converged == 1
