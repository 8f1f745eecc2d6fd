"""CPU reference of the device pose graph (include/liorf_s2m.h, "Pose graph"): numpy / scipy, fp64.

Test infrastructure only - nothing in the product imports it.  Same state, retraction, residuals, whitening,
Cauchy reweighting and Gauss-Newton loop as liorf_amd/csrc/s2m_pose_graph.hip; three linear solvers:

  "dense_sqrt"  numpy.linalg.lstsq on the whitened Jacobian (graphs of up to 300 keys)
  "normal"      sparse normal equations J^T J, scipy.sparse.linalg.spsolve
  "chain_sqrt"  square-root form for large graphs: the odometry chain's whitened Jacobian J_c is square and
                block bidiagonal, so with y = J_c delta the problem is (I + K^T K) y = b, K = J_x J_c^-1 over
                the remaining factors; J_c is never squared, K K^T is a small dense matrix (Woodbury).
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SEED = 20250204
PRIOR_VAR = np.array([1e-2, 1e-2, math.pi * math.pi, 1e8, 1e8, 1e8])        # reference :1390 (rotation, translation)
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])                   # :1394
SC_LOOP_VAR = np.full(6, 0.5)                                               # :712-719
SC_LOOP_K = 1.0
MAX_ITERATIONS, REL_TOL, ABS_TOL = 100, 1e-5, 1e-5


# ---- SO(3) / SE(3) -----------------------------------------------------------------------------------------------
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rzryrx(roll, pitch, yaw):
    cr, sr, cp, sp_, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return np.array([[cy * cp, cy * sp_ * sr - sy * cr, sy * sr + cy * sp_ * cr],
                     [sy * cp, cy * cr + sy * sp_ * sr, sy * sp_ * cr - cy * sr],
                     [-sp_, cp * sr, cp * cr]])


def pose_from_xyzrpy(p):
    p = np.asarray(p, np.float64)
    return rzryrx(p[3], p[4], p[5]), p[:3].copy()


def xyzrpy_from_pose(R, t):
    s = min(1.0, max(-1.0, -R[2, 0]))
    return np.array([t[0], t[1], t[2], math.atan2(R[2, 1], R[2, 2]), math.asin(s), math.atan2(R[1, 0], R[0, 0])])


def so3_exp(w):
    th2 = float(w @ w)
    K = hat(w)
    if th2 < 1e-20:
        return np.eye(3) + K + 0.5 * (K @ K)
    th = math.sqrt(th2)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th2) * (K @ K)


def so3_log(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    s = math.sqrt(float(v @ v))
    if c < -0.99999:                       # near pi: the axis from the symmetric part, 0.5 (R + R^T) - c I = (1 - cos th) a a^T
        th = math.atan2(s, c)
        d = np.array([R[0, 0], R[1, 1], R[2, 2]])
        k = int(np.argmax(d))
        col = 0.5 * (R[:, k] + R[k, :]) - c * np.eye(3)[k]
        col /= math.sqrt(float(col @ col))
        if float(col @ v) < 0.0:
            col = -col
        return th * col
    if s < 1e-10:
        return v.copy()
    return (math.atan2(s, c) / s) * v


def so3_jr_inv(phi):
    th2 = float(phi @ phi)
    K = hat(phi)
    if th2 < 1e-10:
        return np.eye(3) + 0.5 * K + (K @ K) / 12.0
    th = math.sqrt(th2)
    return np.eye(3) + 0.5 * K + (1.0 / th2 - (1.0 + math.cos(th)) / (2.0 * th * math.sin(th))) * (K @ K)


def so3_jr(phi):
    th2 = float(phi @ phi)
    K = hat(phi)
    if th2 < 1e-10:
        return np.eye(3) - 0.5 * K + (K @ K) / 6.0
    th = math.sqrt(th2)
    # (1 - cos th keeps 1.1e-16 / (th^2 / 2) of its digits: the entries of the K term are off by up to 2.2e-16 / th, 2e-11 just
    # above the switch; the device's form, kept as it is - 2 sin^2(th / 2) would be exact)
    return np.eye(3) - ((1.0 - math.cos(th)) / th2) * K + ((th - math.sin(th)) / (th2 * th)) * (K @ K)


def retract(R, t, d):
    return R @ so3_exp(d[:3]), t + R @ d[3:]


# ---- graph -------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self):
        self.X = []                # [(R, t)] or None
        self.priors = []           # (key, R, t, var6)
        self.betweens = []         # (i, j, R, t, var6, k)
        self.gps = []              # (key, z, var3)

    @property
    def n(self):
        return len(self.X)

    def _touch(self, key):
        assert 0 <= key <= len(self.X), "key gap"
        if key == len(self.X):
            self.X.append(None)

    def add_prior(self, key, pose, var=PRIOR_VAR):
        self._touch(key)
        R, t = pose_from_xyzrpy(np.asarray(pose, np.float32))
        self.priors.append((key, R, t, np.asarray(var, np.float64)))

    def add_between(self, i, j, rel, var=ODOM_VAR, k=0.0):
        assert i != j
        for key in sorted((i, j)):
            self._touch(key)
        R, t = pose_from_xyzrpy(np.asarray(rel, np.float32))
        self.betweens.append((i, j, R, t, np.asarray(var, np.float64), float(k)))

    def add_between_pose(self, i, j, R, t, var=ODOM_VAR, k=0.0):
        for key in sorted((i, j)):
            self._touch(key)
        self.betweens.append((i, j, R.copy(), t.copy(), np.asarray(var, np.float64), float(k)))

    def add_gps(self, key, z, var):
        self._touch(key)
        self.gps.append((key, np.asarray(np.asarray(z, np.float32), np.float64), np.asarray(var, np.float64)))

    def set_initial(self, key, pose):
        self._touch(key)
        self.X[key] = pose_from_xyzrpy(np.asarray(pose, np.float32))

    def add_odometry(self, pose):
        """addOdomFactor() (:1386-1400)."""
        if self.n == 0:
            self.add_prior(0, pose)
            self.set_initial(0, pose)
            return
        Rl, tl = self.X[-1]
        Rn, tn = pose_from_xyzrpy(np.asarray(pose, np.float32))
        k = self.n
        self.add_between_pose(k - 1, k, Rl.T @ Rn, Rl.T @ (tn - tl))
        self.X[k] = (Rn, tn)

    def poses(self, X=None):
        X = self.X if X is None else X
        return np.array([xyzrpy_from_pose(R, t) for R, t in X])


def _local(Rr, tr, R, t):
    """[Log(R_E), t_E] of E = (Rr, tr)^-1 (R, t), and D = d local / d (right perturbation of E)."""
    RE = Rr.T @ R
    tE = Rr.T @ (t - tr)
    phi = so3_log(RE)
    D = np.zeros((6, 6))
    D[:3, :3] = so3_jr_inv(phi)
    D[3:, 3:] = RE
    return np.concatenate([phi, tE]), D


def between_residual(Xi, Xj, Rz, tz, jac=True):
    Ri, ti = Xi
    Rj, tj = Xj
    Rh = Ri.T @ Rj
    th = Ri.T @ (tj - ti)
    r, D = _local(Rz, tz, Rh, th)
    if not jac:
        return r
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Rh.T
    Ad[3:, :3] = -Rh.T @ hat(th)
    Ad[3:, 3:] = Rh.T
    return r, -D @ Ad, D


def prior_residual(X, Rp, tp):
    return _local(Rp, tp, X[0], X[1])


def _factor_rows(g, X):
    """Every factor as (keys, blocks, r, sw, k): raw residual and Jacobians, sqrt weights, robust scale."""
    out = []
    for key, Rp, tp, var in g.priors:
        r, D = prior_residual(X[key], Rp, tp)
        out.append(((key,), (D,), r, 1.0 / np.sqrt(var), 0.0))
    for i, j, Rz, tz, var, k in g.betweens:
        r, Ji, Jj = between_residual(X[i], X[j], Rz, tz)
        out.append(((i, j), (Ji, Jj), r, 1.0 / np.sqrt(var), k))
    for key, z, var in g.gps:
        R, t = X[key]
        J = np.zeros((3, 6))
        J[:, 3:] = R
        out.append(((key,), (J,), t - z, 1.0 / np.sqrt(var), 0.0))
    return out


def linearize_factors(g, X):
    """Every factor, whitened and robust-weighted: list of (keys, blocks, r, error term, robust weight)."""
    out = []
    for keys, blocks, r, sw, k in _factor_rows(g, X):
        rw = r * sw
        e2 = float(rw @ rw)
        if k > 0.0:
            w = k * k / (k * k + e2)
            e = 0.5 * k * k * math.log1p(e2 / (k * k))
            s = math.sqrt(w)
        else:
            w, e, s = 1.0, 0.5 * e2, 1.0
        out.append((keys, tuple((B * sw[:, None]) * s for B in blocks), rw * s, e, w))
    return out


def linearize(g, X):
    """Whitened, robust-weighted rows.  Returns (list of (keys, blocks, r), error, minimum robust weight)."""
    rows, err, wmin = [], 0.0, 1.0
    for keys, blocks, r, e, w in linearize_factors(g, X):
        err += e
        wmin = min(wmin, w)
        rows.append((keys, blocks, r))
    return rows, err, wmin


def error(g, X):
    return linearize(g, X)[1]


def assemble(rows, n):
    ri, ci, vv, rr = [], [], [], []
    at = 0
    for keys, blocks, r in rows:
        m = len(r)
        for key, B in zip(keys, blocks):
            a, b = np.meshgrid(np.arange(m) + at, np.arange(6) + 6 * key, indexing="ij")
            ri.append(a.ravel()); ci.append(b.ravel()); vv.append(B.ravel())
        rr.append(r)
        at += m
    J = sp.csr_matrix((np.concatenate(vv), (np.concatenate(ri), np.concatenate(ci))), shape=(at, 6 * n))
    return J, np.concatenate(rr)


def split_chain(g):
    """Factor indices (in _factor_rows order) of the chain: the first prior on key 0 and, per i, the first plain
    between factor i -> i+1.  Everything else is an extra factor."""
    n = g.n
    chain = [-1] * n
    for f, (key, *_rest) in enumerate(g.priors):
        if key == 0 and chain[0] < 0:
            chain[0] = f
    for f, (i, j, _R, _t, _v, k) in enumerate(g.betweens):
        if j == i + 1 and k == 0.0 and chain[j] < 0:
            chain[j] = len(g.priors) + f
    return chain


def solve_step(g, rows, solver):
    n = g.n
    if solver == "dense_sqrt":
        J, r = assemble(rows, n)
        return np.linalg.lstsq(J.toarray(), -r, rcond=None)[0]
    if solver == "normal":
        J, r = assemble(rows, n)
        H = (J.T @ J).tocsc()
        return spla.spsolve(H, -(J.T @ r))
    if solver == "chain_sqrt":
        chain = split_chain(g)
        assert min(chain) >= 0, "not a chain graph"
        cset = set(chain)
        Jc, rc = assemble([rows[f] for f in chain], n)
        extra = [rows[f] for f in range(len(rows)) if f not in cset]
        lu = spla.splu(Jc.tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=False))
        if not extra:
            return lu.solve(-rc)
        Jx, rx = assemble(extra, n)
        Kt = lu.solve(Jx.T.toarray(), trans="T")            # K^T = J_c^-T J_x^T, 6n x m
        b = -(rc + Kt @ rx)
        S = np.eye(Kt.shape[1]) + Kt.T @ Kt
        y = b - Kt @ np.linalg.solve(S, Kt.T @ b)
        return lu.solve(y)
    raise ValueError(solver)


class Result:
    pass


def optimize(g, solver="dense_sqrt", max_iterations=MAX_ITERATIONS, rel_tol=REL_TOL, abs_tol=ABS_TOL, update=True):
    """Gauss-Newton with an accepted-step check, as s2m_pg_optimize."""
    res = Result()
    res.iterations, res.converged = 0, 0
    X = list(g.X)
    assert all(x is not None for x in X), "missing initial value"
    rows, err, wmin = linearize(g, X) if X else ([], 0.0, 1.0)
    res.error_before = err
    for _ in range(max_iterations if X else 0):
        d = solve_step(g, rows, solver)
        Xn = [retract(R, t, d[6 * k:6 * k + 6]) for k, (R, t) in enumerate(X)]
        rows_n, err_n, wmin_n = linearize(g, Xn)
        if not err_n < err:
            res.converged = 1
            break
        dec, old = err - err_n, err
        X, rows, err, wmin = Xn, rows_n, err_n, wmin_n
        res.iterations += 1
        if dec < abs_tol or dec < rel_tol * old:
            res.converged = 1
            break
    res.error_after, res.robust_weight_min, res.X = err, wmin, X
    if update:
        g.X = X
    return res


def marginal(g, key, X=None):
    """Covariance of `key` in its tangent (rotation, translation): dense inverse of J^T J at X.  With the first prior's
    translation variance of 1e8, J^T J has a condition number of 1e16: the rotation block is good to 6e-8, the translation block
    to 0.5 % and the mixed blocks to 10-50 % of their norm.  Good for magnitudes and for graphs without that prior; the device
    is held to pose_graph_cov_ref's routes, which do not square J."""
    X = g.X if X is None else X
    J, _ = assemble(linearize(g, X)[0], g.n)
    H = (J.T @ J).toarray()
    return np.linalg.inv(H)[6 * key:6 * key + 6, 6 * key:6 * key + 6]


# ---- the synthetic trajectory ------------------------------------------------------------------------------------
def figure_eight(n_keys, n_loops, seed=SEED, loop_var=0.3, loop_k=0.0, truth_only=False):
    """A figure-of-eight driven twice, keys 1 m apart; odometry noise 2e-3 rad / 0.01 m per step; dead-reckoned
    initial estimate; loops from second-lap keys to the matching first-lap keys (noise 5e-3 rad / 0.03 m)."""
    rng = np.random.default_rng(seed)
    half = n_keys // 2                       # keys per lap
    s = np.arange(n_keys) % half
    u = 2.0 * math.pi * s / half
    # lemniscate-like curve whose arc length per key is about 1 m
    a = half / 6.1
    xy = np.stack([a * np.sin(u), a * np.sin(u) * np.cos(u)], 1)
    z = 0.5 * np.sin(2.0 * u)
    nxt = np.roll(xy, -1, 0) - xy
    nxt[-1] = nxt[-2]
    yaw = np.unwrap(np.arctan2(nxt[:, 1], nxt[:, 0]))
    truth = [(rzryrx(0.01 * math.sin(uu), 0.01 * math.cos(uu), yy), np.array([p[0], p[1], zz]))
             for uu, yy, p, zz in zip(u, yaw, xy, z)]
    if truth_only:
        return truth
    g = Graph()
    p0 = xyzrpy_from_pose(*truth[0]).astype(np.float32)
    g.add_prior(0, p0)
    g.set_initial(0, p0)
    for k in range(1, n_keys):
        Ra, ta = truth[k - 1]
        Rb, tb = truth[k]
        Rz = Ra.T @ Rb @ so3_exp(rng.normal(0.0, 2e-3, 3))
        tz = Ra.T @ (tb - ta) + rng.normal(0.0, 0.01, 3)
        rel = xyzrpy_from_pose(Rz, tz).astype(np.float32)
        g.add_between(k - 1, k, rel, ODOM_VAR)
        Rl, tl = g.X[k - 1]
        Rm, tm = pose_from_xyzrpy(rel)
        init = xyzrpy_from_pose(Rl @ Rm, tl + Rl @ tm).astype(np.float32)
        g.set_initial(k, init)
    loops = []
    if n_loops:
        for c in np.linspace(half + 5, n_keys - 5, n_loops).astype(int):
            i, j = int(c), int(c) - half
            Ra, ta = truth[i]
            Rb, tb = truth[j]
            Rz = Ra.T @ Rb @ so3_exp(rng.normal(0.0, 5e-3, 3))
            tz = Ra.T @ (tb - ta) + rng.normal(0.0, 0.03, 3)
            rel = xyzrpy_from_pose(Rz, tz).astype(np.float32)
            loops.append((i, j, rel, np.full(6, loop_var), loop_k))
            g.add_between(i, j, rel, np.full(6, loop_var), loop_k)
    g.loops = loops
    return g


def export(g):
    """The graph as plain calls for the device wrapper: list of (name, args)."""
    calls = []
    for key, R, t, var in g.priors:
        calls.append(("prior", key, xyzrpy_from_pose(R, t).astype(np.float32), var))
    for i, j, R, t, var, k in g.betweens:
        calls.append(("between", i, j, xyzrpy_from_pose(R, t).astype(np.float32), var, k))
    for key, z, var in g.gps:
        calls.append(("gps", key, z.astype(np.float32), var))
    return calls


def relative_poses(P):
    """X_0^-1 X_i of an (n, 6) xyzrpy array, as (rotation angle error basis) rotations and translations in fp64."""
    R0, t0 = pose_from_xyzrpy(P[0])
    Rs, ts = [], []
    for p in P:
        R, t = pose_from_xyzrpy(p)
        Rs.append(R0.T @ R)
        ts.append(R0.T @ (t - t0))
    return np.array(Rs), np.array(ts)


def pose_gap(Pa, Pb, relative=False):
    """(max rotation angle, max translation distance) between two (n, 6) pose arrays, absolute or gauge-free."""
    if relative:
        Ra, ta = relative_poses(Pa)
        Rb, tb = relative_poses(Pb)
    else:
        Ra = np.array([pose_from_xyzrpy(p)[0] for p in Pa]); ta = np.asarray(Pa, np.float64)[:, :3]
        Rb = np.array([pose_from_xyzrpy(p)[0] for p in Pb]); tb = np.asarray(Pb, np.float64)[:, :3]
    dR = np.einsum("nji,njk->nik", Ra, Rb)
    v = 0.5 * np.stack([dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]], 1)
    ang = np.arcsin(np.minimum(1.0, np.linalg.norm(v, axis=1)))
    return float(ang.max()), float(np.linalg.norm(ta - tb, axis=1).max())
