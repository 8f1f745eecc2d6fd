"""Model of appending a saved session behind the stored keys and placing it (include/liorf_s2m.h, "Appending a saved session";
DESIGN.md section 21), on top of session_ref's model of the blob. Restated from the description and from nothing in the
library: math.* scalars and left-to-right sums, as session_ref.Graph.add_odometry, so that every bit the library computes on the
host is reproducible here. (The float read-out of a moved pose goes through atan2 / asin, which the device computes itself: those
six floats per key are the one place where the library may differ from this model, by one float step.)

A state is 12 doubles {R row-major, t}; A o X is R' = A_R R, t' = A_R t + A_t, every entry ((a0 b0 + a1 b1) + a2 b2), the
translation that sum plus A_t.
"""
import copy
import math

import numpy as np

import session_ref as M

JUNCTION_VAR = (1.0,) * 6


def compose(A, X):
    O = [0.0] * 12
    for i in range(3):
        for j in range(3):
            O[i * 3 + j] = (A[i * 3] * X[j] + A[i * 3 + 1] * X[3 + j]) + A[i * 3 + 2] * X[6 + j]
        O[9 + i] = ((A[i * 3] * X[9] + A[i * 3 + 1] * X[10]) + A[i * 3 + 2] * X[11]) + A[9 + i]
    return O


def inverse(X):
    O = [0.0] * 12
    for i in range(3):
        for j in range(3):
            O[i * 3 + j] = X[j * 3 + i]
        O[9 + i] = -((X[i] * X[9] + X[3 + i] * X[10]) + X[6 + i] * X[11])
    return O


def between(L, Xn):
    """L^-1 Xn, summed as Graph.add_odometry sums it."""
    Z = [0.0] * 12
    for a in range(3):
        for b in range(3):
            Z[a * 3 + b] = L[a] * Xn[b] + L[3 + a] * Xn[3 + b] + L[6 + a] * Xn[6 + b]
        Z[9 + a] = L[a] * (Xn[9] - L[9]) + L[3 + a] * (Xn[10] - L[10]) + L[6 + a] * (Xn[11] - L[11])
    return Z


def readout(P):
    """{x, y, z, roll, pitch, yaw} of Rot3::RzRyRx as float32 (the rule of s2m_pg_get_poses), with libm."""
    s = min(1.0, max(-1.0, -P[6]))
    return np.array([P[9], P[10], P[11], math.atan2(P[7], P[8]), math.asin(s), math.atan2(P[3], P[0])], np.float64).astype(np.float32)


def move_factor(A, f):
    """A prior's state becomes A o P; a GPS factor's position A_R z + A_t (its rotation block and variances stay); a between stays."""
    if f["type"] == M.BETWEEN:
        return f
    O = compose(A, list(f["R"]) + list(f["t"]))
    g = dict(f)
    if f["type"] == M.PRIOR:
        g["R"] = O[:9]
    g["t"] = O[9:12]
    return g


def junction_factor(n0, L, X0, var):
    return M.factor(M.BETWEEN, n0 - 1, n0, between(L, X0), var, 6, 0.0)


def merge(a, b, anchor=None, junction_var=None):
    """The Session a handle holds after s2m_session_append of b's blob behind a (anchor None: as stored). The result carries
    `first`, `count` and `junction` (the junction's index in the factor list, -1: b has no variables)."""
    var = JUNCTION_VAR if junction_var is None else junction_var
    n0, nk, nv = len(a.clouds), len(b.clouds), b.X.shape[0]
    assert n0 >= 1
    A = None if anchor is None else M.state_of(anchor)
    s = M.Session()
    poses_b = b.poses.copy() if A is None else np.array([readout(compose(A, M.state_of(p))) for p in b.poses], np.float32).reshape(nk, 6)
    s.poses = np.vstack([a.poses, poses_b]).astype(np.float32)
    s.times = np.concatenate([a.times, b.times])
    s.clouds = [c.copy() for c in a.clouds] + [c.copy() for c in b.clouds]
    if b.desc.shape[0]:
        assert a.desc.shape[0] == n0 and b.desc.shape[0] <= nk
    s.desc = np.vstack([a.desc, b.desc])
    s.n_search, s.counter = a.n_search, a.counter
    s.pairs = list(a.pairs) + [(c + n0, p + n0) for c, p in b.pairs]
    s.factors = [dict(f) for f in a.factors]
    s.X, s.has_init = a.X.copy(), a.has_init.copy()
    s.first, s.count, s.junction = n0, nk, -1
    if nv:
        assert a.X.shape[0] == n0 and nv <= nk and b.has_init[0] and a.has_init[n0 - 1]
        Xb = [list(x) for x in b.X]
        if A is not None:
            Xb = [compose(A, x) if b.has_init[k] else x for k, x in enumerate(Xb)]
        s.junction = len(s.factors)
        s.factors.append(junction_factor(n0, list(a.X[n0 - 1]), Xb[0], var))
        for f in b.factors:
            g = dict(f)
            g["i"] = f["i"] + n0
            if f["type"] == M.BETWEEN:
                g["j"] = f["j"] + n0
            s.factors.append(g if A is None else move_factor(A, g))
        s.X = np.vstack([a.X, np.array(Xb, np.float64).reshape(nv, 12)])
        s.has_init = np.concatenate([a.has_init, b.has_init]).astype(np.uint32)
    return s


def place(s, move):
    """s2m_session_place: the appended range of a merged Session moved by `move`; keys and variables behind it stay."""
    D = M.state_of(move)
    o = copy.copy(s)
    o.poses, o.X = s.poses.copy(), s.X.copy()
    lo, hi = s.first, s.first + s.count
    for k in range(lo, hi):
        o.poses[k] = readout(compose(D, M.state_of(s.poses[k])))
        if k < s.X.shape[0] and s.has_init[k]:
            o.X[k] = compose(D, list(s.X[k]))
    o.factors = [move_factor(D, f) if f["type"] != M.BETWEEN and lo <= f["i"] < hi else dict(f) for f in s.factors]
    if s.junction >= 0:
        Z = between(list(o.X[lo - 1]), list(o.X[lo]))
        o.factors[s.junction]["R"], o.factors[s.junction]["t"] = Z[:9], Z[9:12]
    return o


def anchor_from_pairs(pose_in_session, pose_in_map, tol_m, tol_rad):
    """(anchor as float32 x 6, supporters, index of the chosen pair): s2m_session_anchor_from_pairs."""
    A = [compose(M.state_of(m), inverse(M.state_of(s))) for s, m in zip(pose_in_session, pose_in_map)]
    best, best_n, best_sum = -1, 0, 0.0
    for i, a in enumerate(A):
        n, total = 0, 0.0
        for b in A:
            dx, dy, dz = a[9] - b[9], a[10] - b[10], a[11] - b[11]
            dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
            tr = 0.0
            for k in range(9):
                tr += a[k] * b[k]
            ang = math.acos(min(1.0, max(-1.0, (tr - 1.0) / 2.0)))
            if dist <= tol_m and ang <= tol_rad:
                n += 1
                total += dist
        if best < 0 or n > best_n or (n == best_n and total < best_sum):
            best, best_n, best_sum = i, n, total
    return readout(A[best]), best_n, best


def junction_residual(s):
    """The junction's residual at the estimates: the largest entry of Z^-1 o (X[first-1]^-1 o X[first]) - identity."""
    f = s.factors[s.junction]
    E = compose(inverse(list(f["R"]) + list(f["t"])), between(list(s.X[s.first - 1]), list(s.X[s.first])))
    return max(abs(x - y) for x, y in zip(E, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]))


def scripted(n_keys, n_desc, seed):
    """session_ref.scripted's recipe at any size: its loop pairs and extra factors name keys 20 .. 39 and its n_search assumes 30
    descriptors, so below 40 keys the same kinds of content are placed by proportion."""
    if n_keys >= 40 and n_desc >= 30:
        return M.scripted(n_keys, n_desc, seed)
    rng = np.random.default_rng(seed)
    s, g = M.Session(), M.Graph()
    for k in range(n_keys):
        pose = np.array([0.5 * k, 0.1 * k * k, 0.01 * k, 0.002 * k, -0.001 * k, 0.05 * k], np.float32)
        c = rng.normal(0, 5, (int(rng.integers(0, 300)), 8)).astype(np.float32)
        if k % 3 == 0:
            c[:, 3:] = 0
        s.add_key(pose, 100.0 + 0.5 * k, c)
        g.add_odometry(pose)
    next(c for c in s.clouds if c.shape[0])[0, 1] = 0x7fc00001
    d = rng.uniform(0, 3, (n_desc, 1200))
    d[rng.uniform(size=d.shape) < 0.4] = 0.0
    s.desc, s.n_search, s.counter = d, max(n_desc - 30, 0), 7
    last, mid = n_keys - 1, n_keys // 2
    s.pairs = [(mid, 1), (last, 0)]
    g.add_between(mid, 1, [0.1, 0.2, 0.0, 0.0, 0.0, 0.3], [0.04] * 6)
    g.add_between(last, 0, [0.5, -0.4, 0.0, 0.0, 0.02, 1.1], [0.5] * 6, 1.0)
    g.add_gps(mid + 1, [8.4, 29.0, 0.2], [1.0, 1.0, 4.0])
    g.add_prior(2, [1.0, 0.4, 0.02, 0.004, -0.002, 0.1], [0.3] * 6)
    s.set_graph(g)
    return s


# ---- the end-to-end fixture: a second drive through the scripted revisit's scene, stored in a frame of its own ------------------

B_DISPLACEMENT = (12.0, -7.0, 0.4, 0.0, 0.0, math.radians(25.0))    # the map frame seen from session B's: P_map = D o P_B
B_OFFSETS = [("Q1", None), ("Q2", None), ((0.4, -0.2, 0.0), math.radians(-45.0)), ((1.0, 0.3, 0.0), math.radians(60.0)),
             ((0.2, 0.6, 0.0), math.radians(100.0)), ((1.2, -0.8, 0.0), math.radians(-120.0))]
B_PROBES = (0, 1)                                                   # relocalize_ref's Q1 and Q2


def session_b():
    """(clouds, stored poses in B's frame (float32), times, true poses in the map frame (float64), descriptors) of six keys near
    relocalize_ref.TRUE_KEY: the two query poses of relocalize_ref first, then four more, with clouds by local_cloud."""
    import relocalize_ref as R
    from oracle import oracle as O
    from test_loop_closure_cpu import local_cloud, scene
    true0 = R.revisit()[3][R.TRUE_KEY]
    Dinv = inverse(M.state_of(B_DISPLACEMENT))
    clouds, stored, true = [], [], []
    for off, dyaw in B_OFFSETS:
        if isinstance(off, str):
            cloud, pose = R.query_scan(off)
        else:
            pose = true0.copy()
            pose[:3] += off
            pose[5] += dyaw
            cloud = local_cloud(scene(0), pose)
        clouds.append(cloud)
        true.append(np.asarray(pose, np.float64))
        stored.append(readout(compose(Dinv, state64(pose))))
    descs = [O.make_scancontext(c)[0] for c in clouds]
    return clouds, np.array(stored, np.float32), 1000.0 + np.arange(len(clouds)), np.array(true), descs


def state64(pose):
    """state_of for a float64 pose (no rounding to float32 first)."""
    p = [float(v) for v in pose]
    cr, sr, cp, sp, cy, sy = math.cos(p[3]), math.sin(p[3]), math.cos(p[4]), math.sin(p[4]), math.cos(p[5]), math.sin(p[5])
    return [cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr,
            sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr,
            -sp, cp * sr, cp * cr, p[0], p[1], p[2]]
