"""The model of s2m_pg_consistent_loops (include/liorf_s2m.h): NumPy fp64 with every product written out
in the association the header states, so that the device's bits are the model's.  Test infrastructure only.

  chain_length   step[k] = rint(1e6 * sqrt(((dx*dx + dy*dy) + dz*dz))) in int64 micrometres (a step of 2.5e11 or more, or one that
                 is not finite, counts as 2.5e11), s = inclusive prefix sum
  matrix         the pair measure for a < b, row chunk by row chunk, as a boolean matrix; pack() makes the uint64 bit rows
  select         (degree descending, index ascending) ranks, a greedy growth from every start on Python integers as bit sets,
                 the largest set, ties to the best-ranked start.  NOT the maximum clique (see heuristic_miss()).

and the scenes of tests/test_pg_consistency_cpu.py / _gpu.py.
"""
import math

import numpy as np

import pose_graph_ref as P

MAX = 4096
DEFAULTS = dict(tol_m=0.3, tol_chord=0.03, rate_m=0.02, rate_chord=0.0005)
STEP_CAP = 2.5e11
SEED = 20250611


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- inputs ----------------------------------------------------------------------------------------------------------
def rel_to_state(rel):
    """(m, 6) float32 {x, y, z, roll, pitch, yaw} -> (m, 12) fp64 (R row-major, t), as s2m_pg_add_between converts a measurement
    (libm sin / cos of the floats widened to double)."""
    rel = np.asarray(rel, np.float32).reshape(-1, 6)
    Z = np.empty((len(rel), 12))
    for i, p in enumerate(rel):
        Z[i, :9] = P.rzryrx(float(p[3]), float(p[4]), float(p[5])).reshape(9)
        Z[i, 9:] = [float(p[0]), float(p[1]), float(p[2])]
    return Z


def state(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def states_of(X):
    """[(R, t)] of pose_graph_ref -> (n, 12)."""
    return np.array([state(R, t) for R, t in X])


# ---- chain length ----------------------------------------------------------------------------------------------------
def chain_length(X):
    X = np.asarray(X, np.float64).reshape(-1, 12)
    d = X[1:, 9:12] - X[:-1, 9:12]
    with np.errstate(all="ignore"):
        v = 1e6 * np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
        v = np.where(v < STEP_CAP, v, STEP_CAP)
    step = np.concatenate([np.zeros(1, np.int64), np.rint(v).astype(np.int64)])
    return np.cumsum(step, dtype=np.int64)


# ---- the pair measure ------------------------------------------------------------------------------------------------
def _inv(A):                                       # (R^T, -(R^T t)) on lists of 12 broadcastable arrays
    return [A[0], A[3], A[6], A[1], A[4], A[7], A[2], A[5], A[8]] + [-((A[i] * A[9] + A[3 + i] * A[10]) + A[6 + i] * A[11]) for i in range(3)]


def _mul(A, B, diag_only=False):                   # (A_R B_R, (A_R B_t) + A_t); diag_only: only the entries rho2 and d2 read
    O = [None] * 12
    for i in range(3):
        for j in range(3):
            if diag_only and i != j:
                continue
            O[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j]
        O[9 + i] = ((A[i * 3] * B[9] + A[i * 3 + 1] * B[10]) + A[i * 3 + 2] * B[11]) + A[9 + i]
    return O


def measure(Xf_a, Xt_a, Z_a, sf_a, st_a, Xf_b, Xt_b, Z_b, sf_b, st_b, prm):
    """rho2, d2 and the two squared thresholds for candidates a (lower index) and b; every argument a list of 12 arrays (or an int64
    array for the chain lengths) that broadcast against each other."""
    with np.errstate(all="ignore"):
        Ot = _mul(_inv(Xt_a), Xt_b)
        Of = _mul(_inv(Xf_a), Xf_b)
        M1 = _mul(Z_a, Ot)
        M2 = _mul(Of, Z_b)
        D = _mul(_inv(M1), M2, diag_only=True)
        rho2 = ((3.0 - D[0]) - D[4]) - D[8]
        d2 = (D[9] * D[9] + D[10] * D[10]) + D[11] * D[11]
        L = (np.abs(sf_a - sf_b) + np.abs(st_a - st_b)).astype(np.float64) * 1e-6
        tc = prm["tol_chord"] + prm["rate_chord"] * L
        tm = prm["tol_m"] + prm["rate_m"] * L
        return rho2, d2, tc * tc, tm * tm


def matrix(X, key_from, key_to, Z, prm=None, chunk=64, with_margin=False, swap=False):
    """The (m, m) boolean consistency matrix: symmetric, zero diagonal.  with_margin: also the smallest relative distance of a
    finite measure from its threshold, min |v - thr| / max(thr, tiny) over all pairs and both tests.  swap: NOT the contract -
    every pair with its operands exchanged (higher index first), which conjugates D^-1 by O_t and so changes d2 by more than
    rounding; a test uses it to assert that no verdict of its scene hangs on the operand order."""
    prm = params() if prm is None else prm
    X = np.asarray(X, np.float64).reshape(-1, 12)
    kf, kt = np.asarray(key_from, np.int64), np.asarray(key_to, np.int64)
    Z = np.asarray(Z, np.float64).reshape(-1, 12)
    m = len(kf)
    s = chain_length(X)
    Xf, Xt, sf, st = X[kf], X[kt], s[kf], s[kt]
    M = np.zeros((m, m), bool)
    margin = np.inf
    for r0 in range(0, m, chunk):
        r1 = min(m, r0 + chunk)
        if r0 + 1 >= m:
            break
        c0 = r0 + 1                                 # columns b > a only
        a = lambda T: [T[r0:r1, k][:, None] for k in range(12)]
        b = lambda T: [T[c0:, k][None, :] for k in range(12)]
        lo = (a(Xf), a(Xt), a(Z), sf[r0:r1, None], st[r0:r1, None])
        hi = (b(Xf), b(Xt), b(Z), sf[None, c0:], st[None, c0:])
        rho2, d2, tc2, tm2 = measure(*(hi + lo if swap else lo + hi), prm)
        ok = np.isfinite(rho2) & np.isfinite(d2) & (rho2 <= tc2) & (d2 <= tm2)
        upper = np.arange(r0, r1)[:, None] < np.arange(c0, m)[None, :]
        ok &= upper
        M[r0:r1, c0:] = ok
        if with_margin:
            with np.errstate(all="ignore"):
                for v, t in ((rho2, tc2), (d2, tm2)):
                    rel = np.abs(v - t) / np.maximum(t, 1e-300)
                    rel = rel[upper & np.isfinite(rel)]
                    if rel.size:
                        margin = min(margin, float(rel.min()))
    M |= M.T
    return (M, margin) if with_margin else M


def pack(M):
    """(m, m) bool -> (m, (m + 63) // 64) uint64: bit q % 64 of word q // 64 of row p is the pair (p, q)."""
    m = M.shape[0]
    W = (m + 63) // 64
    padded = np.zeros((m, W * 64), np.uint8)
    padded[:, :m] = M
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(m, W)


def _row_ints(M):
    m = M.shape[0]
    by = np.packbits(M.astype(np.uint8), axis=1, bitorder="little")
    return [int.from_bytes(by[p].tobytes(), "little") for p in range(m)]


# ---- selection -------------------------------------------------------------------------------------------------------
def select(M):
    """The stated heuristic on a boolean matrix.  Returns a dict: selected (m,) bool, n_selected, start, degree (m,) int32,
    n_consistent_pairs, sizes (by start candidate) and tie_free: no pick of any growth had a second member of C with the picked
    one's degree, and no second start of the winning size has the winner's degree - the precondition under which the result does
    not depend on the order of the candidates."""
    M = np.asarray(M, bool)
    m = M.shape[0]
    deg = M.sum(1).astype(np.int32)
    if m == 0:
        return dict(selected=np.zeros(0, bool), n_selected=0, start=-1, degree=deg, n_consistent_pairs=0, sizes=[], tie_free=True)
    order = sorted(range(m), key=lambda p: (-int(deg[p]), p))
    o = np.array(order)
    rows = _row_ints(M[o][:, o])                    # the matrix in rank order
    dr = [int(deg[p]) for p in order]
    tie_free = True

    def grow(v, members=None):
        nonlocal tie_free
        C, size = rows[v], 1
        for _ in range(m):
            if not C:
                break
            u = (C & -C).bit_length() - 1
            rest = C & (C - 1)
            if rest and dr[(rest & -rest).bit_length() - 1] == dr[u]:
                tie_free = False
            size += 1
            if members is not None:
                members.append(u)
            C &= rows[u]
        return size

    sizes = [grow(v) for v in range(m)]
    best = max(sizes)
    v = sizes.index(best)
    if any(sizes[w] == best and dr[w] == dr[v] for w in range(v + 1, m)):
        tie_free = False
    members = [v]
    grow(v, members)
    sel = np.zeros(m, bool)
    sel[[order[u] for u in members]] = True
    by_candidate = np.zeros(m, np.int32)
    by_candidate[o] = sizes
    return dict(selected=sel, n_selected=best, start=order[v], degree=deg, n_consistent_pairs=int(deg.sum()) // 2, sizes=by_candidate,
                tie_free=tie_free)


def run(X, key_from, key_to, rel, prm=None, chunk=64):
    """The whole call on float32 measurements: select()'s dict plus matrix (bool) and words (uint64 bit rows)."""
    M = matrix(X, key_from, key_to, rel_to_state(rel), prm, chunk)
    out = select(M)
    out["matrix"], out["words"] = M, pack(M)
    return out


def is_clique(M, sel):
    idx = np.flatnonzero(sel)
    sub = M[np.ix_(idx, idx)]
    return bool((sub | np.eye(len(idx), dtype=bool)).all())


# ---- scenes ----------------------------------------------------------------------------------------------------------
def _rel_of(Ta, Tb, rng=None, rot=0.0, trans=0.0):
    """Ta^-1 Tb (+ noise) of two (R, t) as a float32 pose vector."""
    R, t = Ta[0].T @ Tb[0], Ta[0].T @ (Tb[1] - Ta[1])
    if rng is not None:
        R, t = R @ P.so3_exp(rng.normal(0.0, rot, 3)), t + rng.normal(0.0, trans, 3)
    return P.xyzrpy_from_pose(R, t).astype(np.float32)


def random_scene(m, n_keys=300, seed=SEED, offset=(0.0, 0.0, 0.0)):
    """n_keys random SE(3) estimates of moderate drift around a true random walk, and m candidates: about half true loops with
    noise, half random ones.  Returns X (n, 12), key_from, key_to (int32), rel (m, 6) float32."""
    rng = np.random.default_rng(seed + 7 * m + n_keys)
    truth, est = [], []
    R, t = np.eye(3), np.asarray(offset, np.float64).copy()
    Re, te = R.copy(), t.copy()
    for k in range(n_keys):
        if k:
            dR, dt = P.so3_exp(rng.normal(0.0, 0.15, 3)), np.array([1.0, 0.0, 0.0]) + rng.normal(0.0, 0.1, 3)
            R, t = R @ dR, t + R @ dt
            Re, te = Re @ dR @ P.so3_exp(rng.normal(0.0, 1e-3, 3)), te + Re @ (dt + rng.normal(0.0, 5e-3, 3))
        truth.append((R, t))
        est.append((Re, te))
    kf = rng.integers(0, n_keys, m)
    kt = (kf + rng.integers(1, n_keys, m)) % n_keys           # never key_from
    true = rng.random(m) < 0.5
    rel = np.empty((m, 6), np.float32)
    for i in range(m):
        if true[i]:
            rel[i] = _rel_of(truth[kf[i]], truth[kt[i]], rng, 2e-3, 0.02)
        else:
            rel[i] = np.concatenate([rng.normal(0.0, 20.0, 3), rng.uniform(-3.0, 3.0, 3) * [1.0, 0.45, 1.0]]).astype(np.float32)
    return states_of(est), kf.astype(np.int32), kt.astype(np.int32), rel


def structured_scene(m=MAX, n_keys=2000, groups=24, seed=SEED):
    """A large scene whose model stays quick: the estimates are the truth of a gentle walk; the candidates fall into `groups`
    families, family g measuring true loops through a world offset of its own, so a family is a clique and families do not mix;
    a sixth of the candidates is random."""
    rng = np.random.default_rng(seed + m)
    est = []
    R, t = np.eye(3), np.zeros(3)
    for k in range(n_keys):
        if k:
            R, t = R @ P.so3_exp(rng.normal(0.0, 0.05, 3)), t + R @ np.array([1.0, 0.0, 0.0])
        est.append((R, t))
    offs = [(P.so3_exp(rng.normal(0.0, 0.3, 3)), rng.normal(0.0, 30.0, 3)) for _ in range(groups)]
    offs[0] = (np.eye(3), np.zeros(3))
    kf = rng.integers(0, n_keys, m)
    kt = (kf + rng.integers(1, n_keys, m)) % n_keys
    fam = rng.integers(0, groups + groups // 5 + 1, m)        # >= groups: a random measurement
    rel = np.empty((m, 6), np.float32)
    for i in range(m):
        if fam[i] < groups:
            G = offs[fam[i]]
            Tb = est[kt[i]]
            rel[i] = _rel_of(est[kf[i]], (G[0] @ Tb[0], G[0] @ Tb[1] + G[1]), rng, 1e-3, 0.01)
        else:
            rel[i] = np.concatenate([rng.normal(0.0, 20.0, 3), rng.uniform(-3.0, 3.0, 3) * [1.0, 0.45, 1.0]]).astype(np.float32)
    return states_of(est), kf.astype(np.int32), kt.astype(np.int32), rel


def motivating_scene(n_keys=300, n_loops=10, seed=P.SEED):
    """The figure-of-eight of pose_graph_ref with its drifted dead-reckoned estimates and no loop factor in the graph; the
    candidates are its true loops (ground truth plus centimetre noise), one false loop that claims two places 40 m apart to be
    one (the mirror place across the crossing), and three false loops that agree with each other - the true relation seen
    through one common 15 m offset - but with no true one.  Returns dict(graph, truth, cand=[(i, j, rel)], true=[bool])."""
    with_loops = P.figure_eight(n_keys, n_loops, seed=seed)
    g = P.figure_eight(n_keys, 0, seed=seed)              # the same odometry and estimates (the loops are drawn after them)
    truth = P.figure_eight(n_keys, 0, truth_only=True)
    rng = np.random.default_rng(seed + 99)
    half = n_keys // 2
    cand = [(i, j, rel) for i, j, rel, _var, _k in with_loops.loops]
    true = [True] * len(cand)
    pos = np.array([t for _, t in truth])
    # the mirror place: a second-lap key 20 m from the crossing, and the first-lap key nearest the point opposite it
    i = half + int(np.argmin(np.abs(np.linalg.norm(pos[half:, :2] - pos[0, :2], axis=1) - 20.0)))
    j = int(np.argmin(np.linalg.norm(pos[:half, :2] - (2.0 * pos[0, :2] - pos[i, :2]), axis=1)))
    gap = float(np.linalg.norm(pos[i] - pos[j]))
    cand.append((i, j, np.concatenate([rng.normal(0.0, 0.03, 3), rng.normal(0.0, 5e-3, 3)]).astype(np.float32)))
    true.append(False)
    G = (P.so3_exp(np.array([0.0, 0.0, 0.2])), np.array([12.0, -9.0, 0.5]))
    for c in (half + 20, half + 23, half + 27):
        a, b = c, c - half + 3
        Tb = truth[b]
        cand.append((a, b, _rel_of(truth[a], (G[0] @ Tb[0], G[0] @ Tb[1] + G[1]), rng, 5e-3, 0.03)))
        true.append(False)
    return dict(graph=g, truth=truth, cand=cand, true=np.array(true), mirror_gap=gap)


def heuristic_miss():
    """A hand-made graph on which the heuristic is not optimal: the maximum clique is {0, 1, 2, 3}, but every one of its members
    has a hub of its own (4 .. 7) whose degree is higher, so every growth from a member picks the hub first and ends at two.
    Returns (M, the maximum clique)."""
    m = 4 + 4 + 4 * 5
    M = np.zeros((m, m), bool)

    def edge(a, b):
        M[a, b] = M[b, a] = True
    for a in range(4):
        for b in range(a + 1, 4):
            edge(a, b)
        hub = 4 + a
        edge(a, hub)
        for leaf in range(5):
            edge(hub, 8 + 5 * a + leaf)
    return M, [0, 1, 2, 3]


def tie_free_graph():
    """A hand-made graph whose selection does not depend on the order of the candidates: a clique of five whose members carry
    1, 2, .. 5 pendant neighbours, so their degrees differ, and a clique of three built alike."""
    edges, nxt = [], 8
    for clique, first in (((0, 1, 2, 3, 4), 1), ((5, 6, 7), 8)):
        for x in clique:
            for y in clique:
                if x < y:
                    edges.append((x, y))
        for k, x in enumerate(clique):
            for _ in range(first + k):
                edges.append((x, nxt))
                nxt += 1
    M = np.zeros((nxt, nxt), bool)
    for a, b in edges:
        M[a, b] = M[b, a] = True
    return M
