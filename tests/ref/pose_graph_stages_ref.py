"""Stage-by-stage references of the device pose graph (liorf_amd/csrc/s2m_pose_graph.hip), for the observation hooks
s2m_debug_pg_* of include/liorf_s2m_debug.h.  Test infrastructure only.

  mpmath, 50 digits   the linearisation: the rotation log from axis and angle of the exact rotation, the between / prior / GPS
                      residuals, Jacobians by central differences of the retraction (step 1e-16: truncation below 1e-30),
                      whitening, the Cauchy weight and the error term.  None of the device's closed forms appears here.
  numpy longdouble    sequential block substitution for J_c^-1 and J_c^-T, dense K and I + K^T K, built from the blocks the
                      device returned, so that a scan test cannot inherit an error of the linearisation.
  numpy fp64          the blocked scan with the device's group size and a CG of the device's recurrences: only to measure the
                      floors of tests/golden/pose_graph_stages_bounds.json (tests/golden/make_golden_pose_graph_stages.py).

The cases (graphs, estimates, vectors) of tests/test_pose_graph_stages_gpu.py are built here too, so that the generator of the
bounds and the GPU tests use the same ones.
"""
import math

import mpmath
import numpy as np

import pose_graph_ref as P

M = mpmath.mp.clone()
M.dps = 50
LD = np.longdouble
ULP = 2.0 ** -52                       # one fp64 ulp of a magnitude in [1, 2): no floor is taken below it
GROUP = 32                             # kPgGroup
SKEW_AXIS = np.array([0.6, 0.64, 0.48])
THRESH = math.acos(-0.99999)           # so3_log takes its near-pi branch above this angle


# ---- mpmath: SO(3), residuals, Jacobians ---------------------------------------------------------------------------
def mpf(x):
    return M.mpf(float(x))             # exact: every fp64 is a 50-digit number


def m3(A):
    return [[mpf(A[i][j]) for j in range(3)] for i in range(3)]


def v3(a):
    return [mpf(x) for x in a]


def mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def mt(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def mp_exp(w):
    """The exact rotation about w / |w| by |w| (Rodrigues in 50 digits; 1 - cos as 2 sin^2 so that tiny angles keep them)."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    I = [[M.mpf(int(i == j)) for j in range(3)] for i in range(3)]
    if th2 == 0:
        return I
    th = M.sqrt(th2)
    a, b = M.sin(th) / th, 2 * M.sin(th / 2) ** 2 / th2
    K = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    K2 = mm(K, K)
    return [[I[i][j] + a * K[i][j] + b * K2[i][j] for j in range(3)] for i in range(3)]


def mp_project(R):
    """The rotation nearest to a product of fp64 matrices (orthonormal to 1e-15): R <- R (3 I - R^T R) / 2, three times
    (the defect squares each time: 1e-15, 1e-30, 1e-60)."""
    for _ in range(3):
        G = mm(mt(R), R)
        H = [[(3 * int(i == j) - G[i][j]) / 2 for j in range(3)] for i in range(3)]
        R = mm(R, H)
    return R


def mp_log(R):
    """Axis times angle of an exact rotation: the axis from the antisymmetric part sin(th) a - in 50 digits that keeps 39 of
    them at pi - 1e-11 -, the angle from atan2(sin, cos).  Exactly pi (no antisymmetric part): the axis from a a^T."""
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    s = M.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if s == 0:
        if c > 0:
            return [M.mpf(0)] * 3
        k = max(range(3), key=lambda i: R[i][i])
        a = [(R[i][k] + int(i == k)) / 2 for i in range(3)]
        nrm = M.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        return [M.pi * x / nrm for x in a]
    th = M.atan2(s, c)
    return [th * x / s for x in v]


def mp_retract(X, d):
    R, t = X
    Rv = mv(R, d[3:])
    return mm(R, mp_exp(d[:3])), [t[i] + Rv[i] for i in range(3)]


def mp_between(Xi, Xj, Z):
    (Ri, ti), (Rj, tj), (Rz, tz) = Xi, Xj, Z
    RiT = mt(Ri)
    th = mv(RiT, [tj[k] - ti[k] for k in range(3)])
    RE = mm(mt(Rz), mm(RiT, Rj))
    tE = mv(mt(Rz), [th[k] - tz[k] for k in range(3)])
    return mp_log(mp_project(RE)) + tE


def mp_prior(X, Z):
    (R, t), (Rz, tz) = X, Z
    return mp_log(mp_project(mm(mt(Rz), R))) + mv(mt(Rz), [t[k] - tz[k] for k in range(3)])


H_STEP = M.mpf(10) ** -16


def mp_jacobian(f, X):
    """d f(X (+) d) / d d at d = 0 by central differences, 6 columns."""
    cols = []
    for a in range(6):
        d = [M.mpf(0)] * 6
        d[a] = H_STEP
        hi = f(mp_retract(X, d))
        d[a] = -H_STEP
        lo = f(mp_retract(X, d))
        cols.append([(x - y) / (2 * H_STEP) for x, y in zip(hi, lo)])
    return [[cols[a][r] for a in range(6)] for r in range(len(cols[0]))]


def mp_state(X):
    return m3(X[0]), v3(X[1])


def mp_factors(g, X):
    """Every factor of `g` (P._factor_rows order) at the fp64 estimates X, in 50 digits: dicts with keys, the whitened and
    robust-weighted residual r (6, zero rows beyond the factor's), blocks (6x6 each), err, w."""
    out = []
    Xm = [mp_state(x) for x in X]
    zero6 = [[M.mpf(0)] * 6 for _ in range(6)]

    def finish(keys, r, blocks, var, k):
        rows = len(r)
        sw = [1 / M.sqrt(mpf(v)) for v in var]
        rw = [r[a] * sw[a] for a in range(rows)]
        e2 = sum(x * x for x in rw)
        if k > 0.0:
            k2 = mpf(k) ** 2
            w = k2 / (k2 + e2)
            err = k2 * M.log(1 + e2 / k2) / 2
        else:
            w, err = M.mpf(1), e2 / 2
        s = M.sqrt(w)
        full = lambda B: [[B[a][b] * sw[a] * s for b in range(6)] for a in range(rows)] + zero6[rows:]
        out.append(dict(keys=keys, r=[x * s for x in rw] + [M.mpf(0)] * (6 - rows), blocks=[full(B) for B in blocks], err=err, w=w))

    for key, Rp, tp, var in g.priors:
        Z = (m3(Rp), v3(tp))
        finish((key,), mp_prior(Xm[key], Z), [mp_jacobian(lambda x: mp_prior(x, Z), Xm[key])], var, 0.0)
    for i, j, Rz, tz, var, k in g.betweens:
        Z = (m3(Rz), v3(tz))
        finish((i, j), mp_between(Xm[i], Xm[j], Z),
               [mp_jacobian(lambda x: mp_between(x, Xm[j], Z), Xm[i]), mp_jacobian(lambda x: mp_between(Xm[i], x, Z), Xm[j])], var, k)
    for key, z, var in g.gps:
        zz = v3(z)
        f = lambda x: [x[1][a] - zz[a] for a in range(3)]
        finish((key,), f(Xm[key]), [mp_jacobian(f, Xm[key])], var, 0.0)
    return out


def fp64_factors(g, X):
    """The same list from the fp64 reference (pose_graph_ref.py), rows padded to 6."""
    out = []
    for keys, blocks, r, e, w in P.linearize_factors(g, X):
        pad = lambda B: np.vstack([B, np.zeros((6 - B.shape[0], 6))])
        out.append(dict(keys=keys, r=np.concatenate([r, np.zeros(6 - len(r))]), blocks=[pad(B) for B in blocks], err=e, w=w))
    return out


def stage_arrays(g, factors, inverse, binv=None):
    """The factor list in the layout of s2m_debug_pg_linearize: chain entries by key, extra factors in P.split_chain's order.
    Entries keep their number type (mpf or float); `inverse` inverts a 6x6 block in it (`binv`: the inverses, given)."""
    chain = P.split_chain(g)
    assert min(chain) >= 0
    cset = set(chain)
    zero = [[0 * factors[0]["err"]] * 6 for _ in range(6)]
    rc, Binv, Aof = [], [], []
    for k, f in enumerate(chain):
        fa = factors[f]
        rc.append(list(fa["r"]))
        Binv.append(binv[k] if binv is not None else inverse(fa["blocks"][-1]))
        Aof.append([list(row) for row in fa["blocks"][0]] if k > 0 else zero)
    extra = [factors[f] for f in range(len(factors)) if f not in cset]
    return dict(rc=rc, Binv=Binv, Aof=Aof, rx=[list(f["r"]) for f in extra], Ji=[[list(r) for r in f["blocks"][0]] for f in extra],
                Jj=[[list(r) for r in f["blocks"][1]] if len(f["blocks"]) > 1 else zero for f in extra],
                ferr=[factors[f]["err"] for f in chain] + [f["err"] for f in extra], fw=[factors[f]["w"] for f in chain] + [f["w"] for f in extra],
                err=sum(f["err"] for f in factors), wmin=min(f["w"] for f in factors))


def mp_inverse(B):
    return (M.matrix(B) ** -1).tolist()


def fp64_binv(g):
    """(W D)^-1 of every chain factor in the closed form of the fp64 reference and of the device: blkdiag(Jr(phi), R_E^T) W^-1."""
    out = []
    for k, f in enumerate(P.split_chain(g)):
        if k == 0:
            _key, Rp, tp, var = g.priors[f]
            r, D = P.prior_residual(g.X[0], Rp, tp)
        else:
            i, j, Rz, tz, var, _k = g.betweens[f - len(g.priors)]
            r, _Ji, D = P.between_residual(g.X[i], g.X[j], Rz, tz)
        sw = 1.0 / np.sqrt(var)
        B = np.zeros((6, 6))
        B[:3, :3] = P.so3_jr(r[:3]) / sw[None, :3]
        B[3:, 3:] = D[3:, 3:].T / sw[None, 3:]
        out.append(B.tolist())
    return out


def block_gap(got, want):
    """max |got - want| / max |want| of one block (nested lists; `want` in 50 digits, `got` fp64), the difference taken in 50
    digits.  A block that is exactly zero in the reference must be exactly zero: 0.0 or inf."""
    a, b = np.asarray(got, object).ravel(), np.asarray(want, object).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    diff = max(abs(mpf(x) - y) for x, y in zip(a, b))
    scale = max(abs(y) for y in b)
    if scale == 0:
        return 0.0 if diff == 0 else math.inf
    return float(diff / scale)


def linearize_gaps(got, want, names, chain_names):
    """Per case and array the gap of `got` (arrays of s2m_debug_pg_linearize, or stage_arrays in fp64) to the 50-digit
    `want`: a chain case holds the largest gap over its keys (chain_names[k]: the case of key k), every extra factor is a
    case of its own."""
    n = len(want["rc"])
    out = {"total": {"err": block_gap([got["err"]], [want["err"]]), "wmin": block_gap([got["wmin"]], [want["wmin"]])}}
    for case in sorted(set(chain_names)):
        keys = [k for k in range(n) if chain_names[k] == case]
        out[case] = {a: max(block_gap(got[a][k], want[a][k]) for k in keys) for a in ("rc", "Binv", "Aof")}
        for a in ("ferr", "fw"):
            out[case][a] = max(block_gap([got[a][k]], [want[a][k]]) for k in keys)
    for x, name in enumerate(names):
        out[name] = {a: block_gap(got[a][x], want[a][x]) for a in ("rx", "Ji", "Jj")}
        for a in ("ferr", "fw"):
            out[name][a] = block_gap([got[a][n + x]], [want[a][n + x]])
    return out


# ---- the hand-built graph of 40 keys -------------------------------------------------------------------------------
def _f32(R, t):
    return P.xyzrpy_from_pose(R, t).astype(np.float32)


def _compose(A, B):
    return A[0] @ B[0], A[1] + A[0] @ B[1]


def _inv(A):
    return A[0].T, -(A[0].T @ A[1])


def _exp6(w, v):
    return P.so3_exp(np.asarray(w, np.float64)), np.asarray(v, np.float64)


def _orth(X):
    """The state with its rotation replaced by the nearest orthonormal one, rounded to fp64 entry by entry."""
    return np.array([[float(x) for x in row] for row in mp_project(m3(X[0]))]), X[1]


def graph40():
    """(graph, names of the extra factors, calls).  Measurements are float xyzrpy as the C ABI takes them (`calls` holds exactly
    what went into the graph, for the device); the estimates are fp64 and placed so that the named residuals come out: a key
    that closes a special between factor (i, j) is X_j = X_i Z Exp(w), which leaves the residual w to rounding.  Every estimate's
    rotation is orthonormal to fp64 rounding, as s2m_pg_set_initial makes them: the device takes (W D)^-1 with R^T for R^-1, so a
    product of forty rotations left as it comes (2e-15 off) shows in Binv by that much."""
    rng = np.random.default_rng(P.SEED + 40)
    n = 40
    axis = SKEW_AXIS / np.linalg.norm(SKEW_AXIS)
    loop_var = np.full(6, 0.5)
    # (i, j, residual rotation angle about the skew axis, robust k): j's estimate is placed by the factor
    special = {17: (15, math.pi - 4.6e-3, 0.0, "near_pi_4.6e-3"), 19: (17, math.pi - 4.4e-3, 1.0, "near_pi_4.4e-3_cauchy"),
               22: (19, math.pi - 1e-6, 0.0, "near_pi_1e-6"), 24: (22, 1e-11, 0.0, "rot_1e-11"), 27: (24, 1e-4, 0.0, "rot_1e-4"),
               29: (27, THRESH - 1e-7, 0.0, "below_threshold"), 31: (29, THRESH + 1e-7, 0.0, "above_threshold")}
    # residual rotations of the free chain links: both sides of so3_jr's switch at |phi|^2 = 1e-10, and plain ones
    chain_rot = [0.0, 1e-11, 9e-6, 1.1e-5, 1e-4, 3e-3, 0.05]
    X = [_orth((P.so3_exp(np.array([1.1, -1.3, 0.7])), np.array([4.0, -7.0, 2.5])))]
    zs = {}
    for k in range(1, n):
        if k in special:
            i, ang, _k, _name = special[k]
            rel = np.concatenate([rng.normal(0, 2.0, 3), rng.uniform(-1.5, 1.5, 3)]).astype(np.float32)
            zs[k] = rel
            Z = P.pose_from_xyzrpy(rel)
            X.append(_orth(_compose(_compose(X[i], Z), _exp6(ang * axis, [0.3, -0.2, 0.1]))))
        else:
            step = np.array([1.0, 0.05 * math.sin(k), 0.02, 0.01 * math.cos(k), 0.02 * math.sin(2 * k), 0.15], np.float32)
            zs[-k] = step
            d = rng.normal(0, 1, 3)
            X.append(_orth(_compose(_compose(X[k - 1], P.pose_from_xyzrpy(step)), _exp6(chain_rot[k % len(chain_rot)] * d / np.linalg.norm(d), rng.normal(0, 0.01, 3)))))
    calls, names = [], []
    rel_of = lambda i, j: _compose(_inv(X[i]), X[j])
    calls.append(("prior", 0, _f32(*_compose(X[0], _exp6([0.01, -0.02, 0.015], [0.1, 0.2, -0.1]))), P.PRIOR_VAR))
    calls.append(("prior", 0, _f32(*_compose(X[0], _exp6([-0.2, 0.1, 0.05], [0.5, -0.3, 0.2]))), np.array([0.1, 0.2, 0.3, 1.0, 2.0, 3.0])))
    names.append("second_prior_key0")
    for k in range(1, n):
        if k in special:                                    # the chain link into a placed key: measured as it lies, in float
            calls.append(("between", k - 1, k, _f32(*rel_of(k - 1, k)), P.ODOM_VAR, 0.0))
        else:
            calls.append(("between", k - 1, k, zs[-k], P.ODOM_VAR, 0.0))
    # (after the chain, so that key 17 exists; the extra factors still come in the order priors, betweens, GPS)
    calls.append(("prior", 17, _f32(*_compose(X[17], _exp6([0.3, 0.2, -0.4], [-1.0, 0.4, 0.3]))), np.array([0.05, 0.05, 0.08, 0.5, 0.5, 0.7])))
    names.append("prior_key17")
    calls.append(("between", 5, 6, _f32(*_compose(rel_of(5, 6), _exp6([0.02, 0.01, -0.03], [0.05, -0.02, 0.04]))), np.full(6, 1e-3), 0.0))
    names.append("second_between_5_6")
    calls.append(("between", 30, 12, _f32(*_compose(rel_of(30, 12), _exp6([0.2, -0.15, 0.1], [0.4, 0.3, -0.2]))), loop_var, 0.0))
    names.append("between_30_12")
    calls.append(("between", 8, 3, _f32(*rel_of(8, 3)), loop_var, 1.0))
    names.append("cauchy_satisfied_8_3")
    bad = _f32(*rel_of(25, 14))
    bad[:3] += np.array([6.0, 0.0, 0.0], np.float32)
    calls.append(("between", 25, 14, bad, loop_var, 1.0))
    names.append("cauchy_outlier_6m_25_14")
    for k in sorted(special):
        i, _ang, rk, name = special[k]
        calls.append(("between", i, k, zs[k], loop_var, rk))
        names.append(name)
    calls.append(("gps", 10, (X[10][1] + np.array([0.3, -0.2, 0.5])).astype(np.float32), np.array([0.25, 0.25, 1.0])))
    names.append("gps_key10")
    g = P.Graph()
    for c in calls:
        if c[0] == "prior":
            g.add_prior(c[1], c[2], c[3])
        elif c[0] == "between":
            g.add_between(c[1], c[2], c[3], c[4], c[5])
        else:
            g.add_gps(c[1], c[2], c[3])
    g.X = X
    assert g.n == n
    # the chain's cases: the prior, the links into placed keys (measured as they lie: a residual of float rounding, 1e-7), and
    # the free links by the size of their residual rotation - the device's Jr(phi) keeps 2.2e-16 / |phi| above its switch at 1e-5
    g.chain_names = ["chain_prior"] + ["chain_placed" if k in special else "chain_rot_%g" % chain_rot[k % len(chain_rot)] for k in range(1, n)]
    return g, names, calls


def load_calls(m, calls, X):
    """`calls` into the device graph of mapper `m`, the fp64 estimates X through s2m_debug_pg_set_estimate."""
    m.pgReset()
    for c in calls:
        if c[0] == "prior":
            m.pgAddPrior(c[1], c[2], c[3])
        elif c[0] == "between":
            m.pgAddBetween(c[1], c[2], c[3], c[4], c[5])
        else:
            m.pgAddGps(c[1], c[2], c[3])
    for k, (R, t) in enumerate(X):
        m.pgSetEstimate(k, R, t)


def extras_of(g):
    """(type, i, j) of every extra factor in the device's order: 'prior' / 'gps' have j = -1."""
    chain = set(P.split_chain(g))
    kinds = [("prior", f[0], -1) for f in g.priors] + [("between", f[0], f[1]) for f in g.betweens] + [("gps", f[0], -1) for f in g.gps]
    return [k for f, k in enumerate(kinds) if f not in chain]


# ---- the chains of the scan tests ---------------------------------------------------------------------------------
SCAN_N = (1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025, 1057, 32769)
SCAN_COLS = (1, 24, 13)


def _rzryrx_many(rpy):
    cr, sr, cp, sp, cy, sy = np.cos(rpy[:, 0]), np.sin(rpy[:, 0]), np.cos(rpy[:, 1]), np.sin(rpy[:, 1]), np.cos(rpy[:, 2]), np.sin(rpy[:, 2])
    return np.stack([np.stack([cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr], 1),
                     np.stack([sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr], 1),
                     np.stack([-sp, cp * sr, cp * cr], 1)], 1)


def chain_case(n):
    """A figure-of-eight-like drive of n keys 1 m apart (the yaw rate changes sign every half lap of 200 keys): the prior, the
    float odometry measurements, three loops where 64 <= n < 32769 (a plain chain at 32769: four scan levels), and fp64
    estimates 5e-3 rad / 0.02 m off the dead-reckoned ones, so that every right-hand side is non-zero.  (calls, X)."""
    rng = np.random.default_rng(P.SEED + n)
    k = np.arange(1, n)
    rel = np.zeros((n - 1, 6))
    rel[:, 0] = 1.0 + rng.normal(0, 0.01, n - 1)
    rel[:, 1:3] = rng.normal(0, 0.01, (n - 1, 2))
    rel[:, 3:5] = rng.normal(0, 2e-3, (n - 1, 2))
    rel[:, 5] = np.where((k // 200) % 2 == 0, 1.0, -1.0) * 2.0 * math.pi / 200 + rng.normal(0, 2e-3, n - 1)
    rel = rel.astype(np.float32)
    Rz = _rzryrx_many(rel[:, 3:].astype(np.float64))
    tz = rel[:, :3].astype(np.float64)
    noise_w, noise_t = rng.normal(0, 5e-3, (n, 3)), rng.normal(0, 0.02, (n, 3))
    p0 = np.array([1.0, -2.0, 0.5, 0.01, -0.02, 0.3], np.float32)
    R, t = P.pose_from_xyzrpy(p0)
    X = []
    for i in range(n):
        if i > 0:
            t = t + R @ tz[i - 1]
            R = R @ Rz[i - 1]
        X.append((R @ P.so3_exp(noise_w[i]), t + noise_t[i]))
    calls = [("prior", 0, p0, P.PRIOR_VAR)] + [("between", i - 1, i, rel[i - 1], P.ODOM_VAR, 0.0) for i in range(1, n)]
    if 64 <= n < 32769:
        for i, j in ((n - 1, 0), (n // 2, n // 4), (3 * n // 4, n // 3)):
            calls.append(("between", i, j, _f32(*_compose(_inv(X[i]), X[j])), np.full(6, 0.3), 0.0))
    return calls, X


def graph_of(calls, X):
    g = P.Graph()
    for c in calls:
        if c[0] == "prior":
            g.add_prior(c[1], c[2], c[3])
        elif c[0] == "between":
            g.add_between(c[1], c[2], c[3], c[4], c[5])
        else:
            g.add_gps(c[1], c[2], c[3])
    g.X = list(X)
    return g


def scan_vectors(n):
    """The right-hand sides of the scan tests, one per row: 1 + 24 + 13 random vectors (the single form takes the first, the
    block forms the next 24 and 13) and unit vectors at the first key, the last key and a group-edge key."""
    rng = np.random.default_rng(P.SEED + 7 * n)
    V = rng.normal(0, 1, (1 + 24 + 13, 6 * n))
    edge = min(n - 1, GROUP - 1 if n <= GROUP else GROUP * ((n - 1) // GROUP))   # last of the first group, or first of the last
    units = np.zeros((3, 6 * n))
    for r, (key, axis) in enumerate(((0, 1), (n - 1, 4), (edge, 2))):
        units[r, 6 * key + axis] = 1.0
    return V, units


def chain_blocks_fp64(g):
    """Binv and Aof (n x 6 x 6) of the chain from the fp64 reference: what the device's linearisation holds, for the floors."""
    fac = P.linearize_factors(g, g.X)
    chain = P.split_chain(g)
    Binv = np.array([np.linalg.inv(fac[f][1][-1]) for f in chain])
    Aof = np.array([fac[f][1][0] if k > 0 else np.zeros((6, 6)) for k, f in enumerate(chain)])
    return Binv, Aof


# ---- longdouble: sequential block substitution, dense K ------------------------------------------------------------
def fwd_ld(Binv, Aof, V):
    """x = J_c^-1 v for the columns of V (6n x C): row i of J_c is A_i x_(i-1) + B_i x_i."""
    B, A = np.asarray(Binv, LD), np.asarray(Aof, LD)
    n = B.shape[0]
    V = np.asarray(V, LD).reshape(n, 6, -1)
    out = np.zeros_like(V)
    x = np.zeros_like(V[0])
    for i in range(n):
        x = B[i] @ (V[i] - A[i] @ x) if i else B[0] @ V[0]
        out[i] = x
    return out.reshape(6 * n, -1)


def bwd_ld(Binv, Aof, V):
    """x = J_c^-T v: column i of J_c holds B_i (row i) and A_(i+1) (row i+1)."""
    B, A = np.asarray(Binv, LD), np.asarray(Aof, LD)
    n = B.shape[0]
    V = np.asarray(V, LD).reshape(n, 6, -1)
    out = np.zeros_like(V)
    x = np.zeros_like(V[0])
    for i in range(n - 1, -1, -1):
        x = B[i].T @ (V[i] - A[i + 1].T @ x) if i + 1 < n else B[i].T @ V[i]
        out[i] = x
    return out.reshape(6 * n, -1)


def dense_jx(n, Ji, Jj, extras, dtype=LD):
    Jx = np.zeros((6 * len(extras), 6 * n), dtype)
    for x, (kind, i, j) in enumerate(extras):
        Jx[6 * x:6 * x + 6, 6 * i:6 * i + 6] += np.asarray(Ji[x], dtype)
        if kind == "between":
            Jx[6 * x:6 * x + 6, 6 * j:6 * j + 6] += np.asarray(Jj[x], dtype)
    return Jx


def dense_k_ld(Binv, Aof, Ji, Jj, extras):
    """K = J_x J_c^-1 (6 n_extra x 6n) in longdouble: K^T = J_c^-T J_x^T by substitution."""
    n = len(Binv)
    return bwd_ld(Binv, Aof, dense_jx(n, Ji, Jj, extras).T).T


def col_gap(got, want):
    """Largest over the columns of max |got - want| / max |want| (arrays 6n x C; the difference in longdouble)."""
    got, want = np.asarray(got, LD).reshape(want.shape[0], -1), np.asarray(want, LD)
    return float((np.abs(got - want).max(0) / np.abs(want).max(0)).max())


def true_residual(K, y, b):
    """|| (I + K^T K) y - b || / || b || in longdouble."""
    y, b = np.asarray(y, LD), np.asarray(b, LD)
    r = y + K.T @ (K @ y) - b
    return float(np.sqrt(r @ r) / np.sqrt(b @ b))


# ---- fp64: the device's blocked scan and CG, for the floors ---------------------------------------------------------
def blocked_scan_f64(Binv, Aof, V, rev):
    """The device's scan in numpy fp64: x_e = M_e x_(e-1) + C0_e in_e in groups of 32 with prefix products, up-sweep and
    down-sweep over as many levels as the size needs.  V: 6n x C, in key order; rev: the transposed solve."""
    B, A = np.asarray(Binv, np.float64), np.asarray(Aof, np.float64)
    n = B.shape[0]
    V = np.asarray(V, np.float64).reshape(n, 6, -1)
    if not rev:
        M0, C0, inp = -(B @ A), B, V
    else:
        An = np.concatenate([A[1:], np.zeros((1, 6, 6))])
        M0 = -np.transpose(An @ B, (0, 2, 1))[::-1]
        C0, inp = np.transpose(B, (0, 2, 1))[::-1], V[::-1]
    Ms, Pres, sizes = [M0], [], [n]
    while True:                                           # prefix products per group; a group's product is the next level's matrix
        Mx, m = Ms[-1], sizes[-1]
        Pre = np.zeros_like(Mx)
        for s in range(GROUP):
            idx = np.arange(s, m, GROUP)
            Pre[idx] = Mx[idx] if s == 0 else Mx[idx] @ Pre[idx - 1]
        Pres.append(Pre)
        if m <= GROUP:
            break
        last = np.minimum(np.arange(0, m, GROUP) + GROUP, m) - 1
        Ms.append(Pre[last])
        sizes.append(len(last))
    locs = []
    for lvl, m in enumerate(sizes):                       # up-sweep: each group's recurrence from a zero input
        if lvl == 0:
            c = C0 @ inp
        else:
            c = locs[-1][np.minimum(np.arange(m) * GROUP + GROUP, sizes[lvl - 1]) - 1]
        loc = np.zeros_like(c)
        for s in range(GROUP):
            idx = np.arange(s, m, GROUP)
            loc[idx] = c[idx] if s == 0 else Ms[lvl][idx] @ loc[idx - 1] + c[idx]
        locs.append(loc)
    for lvl in range(len(sizes) - 2, -1, -1):             # down-sweep: add the carry that enters the element's group
        e = np.arange(GROUP, sizes[lvl])
        locs[lvl][e] = locs[lvl][e] + Pres[lvl][e] @ locs[lvl + 1][e // GROUP - 1]
    out = locs[0][::-1] if rev else locs[0]
    return out.reshape(6 * n, -1)


def cg_f64(apply_a, b, tol, max_iters):
    """The recurrences of k_pg_cg_* in numpy fp64 for the operator apply_a(p) = p + K^T K p: (y, rr, bb, iters)."""
    b = np.asarray(b, np.float64)
    y, r, p = np.zeros_like(b), b.copy(), b.copy()
    bb = rr = float(b @ b)
    iters = 0
    stop = bb == 0.0 or max_iters <= 0
    while not stop:
        q = apply_a(p)
        pq = float(p @ q)
        alpha = rr / pq if pq > 0.0 else 0.0
        y = y + alpha * p
        r = r - alpha * q
        rn = float(r @ r)
        beta = rn / rr if rr > 0.0 else 0.0
        rr = rn
        iters += 1
        if not rr > tol * tol * bb or iters >= max_iters or not pq > 0.0:
            break
        p = r + beta * p
    return y, rr, bb, iters


class Fp64Operators:
    """K v and K^T u in fp64 as the device forms them: the blocked scans around the extra factors' blocks."""

    def __init__(self, Binv, Aof, Ji, Jj, extras):
        self.B, self.A = np.asarray(Binv, np.float64), np.asarray(Aof, np.float64)
        self.Jx = dense_jx(len(self.B), Ji, Jj, extras, np.float64)

    def k(self, v):
        return self.Jx @ blocked_scan_f64(self.B, self.A, v, 0)[:, 0]

    def kt(self, u):
        return blocked_scan_f64(self.B, self.A, self.Jx.T @ u, 1)[:, 0]

    def a(self, p):
        return p + self.kt(self.k(p))


def extra_blocks_fp64(g):
    fac = P.linearize_factors(g, g.X)
    chain = set(P.split_chain(g))
    ex = [f for k, f in enumerate(fac) if k not in chain]
    pad = lambda B: np.vstack([B, np.zeros((6 - B.shape[0], 6))])
    return np.array([pad(f[1][0]) for f in ex]), np.array([pad(f[1][1]) if len(f[1]) > 1 else np.zeros((6, 6)) for f in ex])


PRODUCT_CASES = ("graph40", "loops_200")
CG_CASES = ("loops_200", "gps_120")
CG_TOL = 1e-13                           # s2m_pg_default_params: cg_rel_tol


def case_graph(name):
    """(graph with fp64 estimates, calls or None): graph40 is loaded by its calls, the others by pose_graph_cases.load_into."""
    import pose_graph_cases as CS
    if name == "graph40":
        g, _names, calls = graph40()
        return g, calls
    return CS.build(name), None


def default_max_cg(n_extra):
    return 6 * n_extra + 20 if n_extra else 1            # run_cg of s2m_abi_pose_graph.hip


def product_vectors(name, n, m):
    rng = np.random.default_rng(P.SEED + sum(map(ord, name)) + 1)
    return rng.normal(0, 1, (3, 6 * n)), rng.normal(0, 1, (3, 6 * m))


def cg_rhs(name, n):
    return np.random.default_rng(P.SEED + sum(map(ord, name))).normal(0, 1, (3, 6 * n))


def clamp(x):
    return max(float(x), ULP)
