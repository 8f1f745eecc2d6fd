"""CPU references of the pose graph's covariances (s2m_pg_marginal, s2m_pg_marginals, s2m_pg_joint_marginal) that never
form J^T J in fp64, on tests/ref/pose_graph_ref.py.  Test infrastructure only.

The first prior's translation variance is 1e8, so the whitened Jacobian J has a singular value of 1.6e-5 beside 2e3 and
J^T J a condition number of about 1e16: its fp64 inverse (pose_graph_ref.marginal, pose_graph_marginals_ref.joint_dense)
carries 3e-3 of noise in the translation blocks and up to 0.5 in the mixed ones.  The routes here work on J itself:

  cov_svd    V diag(s^-2) V^T from the SVD of J
  cov_qr     J = Q R; Y = R^-T E by a triangular solve, Sigma = Y^T Y
  cov_chain  the product's own route in fp64 (solve_step's "chain_sqrt"): splu of the chain's J_c, Woodbury on the other
             factors, unit right-hand sides: Sigma E = J_c^-1 (I + K^T K)^-1 J_c^-T E
  cov_mp     mpmath at `dps` digits: one LU of J^T J, then only the wanted columns (small graphs; minutes)

Each returns the (6 k, 6 k) block of the covariance over the tangents of `keys`, in their order.  block_gaps compares two such
matrices 3x3 block by 3x3 block.
"""
import math

import numpy as np
import scipy.linalg as sla
import scipy.sparse.linalg as spla

import pose_graph_ref as P

TYPES = ("rr", "rt", "tr", "tt")
_R, _T = slice(0, 3), slice(3, 6)
_SL = {"rr": (_R, _R), "rt": (_R, _T), "tr": (_T, _R), "tt": (_T, _T)}
HELD_BELOW = 1e-6                   # a block whose reference norm is below this much of its scale is judged against the scale


SMALL = ("eight_40", "eight_65")                   # two and three scan groups, one level; reference cov_mp
SUITE = ("loops_200", "gps_120_at_45", "cauchy_outlier_300")       # reference cov_svd
GRAPHS = SMALL + SUITE


def build(name):
    """The graphs the covariances are held on, before the optimise.  gps_120_at_45 is pose_graph_cases' gps_120 with its GPS
    factor on key 45 instead of key 60: in gps_120 the factor sits on a listed key (n / 2) and pins its translation, so that
    every rotation's covariance with that translation falls below HELD_BELOW of its scale - scale-held blocks other than those
    of key 0's translation, which the golden script does not admit.  (gps_120 itself stays in tests/test_pose_graph_gpu.py and
    in the joint-marginal test, where those blocks are judged against their scale.)"""
    import pose_graph_cases as CS
    if name == "eight_40":
        return P.figure_eight(40, 2)
    if name == "eight_65":
        return P.figure_eight(65, 2)
    if name == "gps_120_at_45":
        g = P.figure_eight(120, 3)
        tr = P.figure_eight(120, 0, truth_only=True)
        g.add_gps(45, tr[45][1] + np.array([0.05, -0.04, 0.02]), np.array([0.25, 0.25, 1.0]))
        return g
    return CS.build(name)


def keys_of(name, n):
    if name in SMALL:
        return sorted({0, 1, 31, 32, 33, n // 2, n - 2, n - 1} | ({63, 64} if n == 65 else set()))
    return [0, 31, 32, 33, n // 2, n - 1]


def pairs_of(name, n):
    import pose_graph_marginals_ref as M
    if name in SMALL:
        return [(0, n - 1), (31, 32), (20, 33)]
    base = "gps_120" if name == "gps_120_at_45" else name
    return [(a, b) for nm, a, b in M.CASES if nm == base]


def all_keys_of(name, n):
    """The keys a reference matrix spans: the listed keys and those of the joint pairs, ascending."""
    return sorted(set(keys_of(name, n)) | {k for p in pairs_of(name, n) for k in p})


def sub(S, all_keys, keys):
    """The block over `keys` of a matrix over `all_keys`."""
    idx = rows_of([list(all_keys).index(k) for k in keys])
    return S[np.ix_(idx, idx)]


def load_golden():
    """(blocks, bounds) as tests/golden/make_golden_pose_graph_cov.py wrote them: {name: {"X", "keys", "cov", ...}} and the
    bounds file's dictionary."""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden")
    out = {}
    with np.load(os.path.join(here, "pose_graph_cov_golden.npz")) as z:
        for k in z.files:
            name, what = k.split("/")
            out.setdefault(name, {})[what] = z[k]
    for v in out.values():
        v["keys"] = [int(k) for k in v["keys"]]
    with open(os.path.join(here, "pose_graph_cov_bounds.json")) as f:
        return out, json.load(f)


def state_array(X):
    return np.array([np.concatenate([R.reshape(9), t]) for R, t in X])


def state_list(A):
    return [(a[:9].reshape(3, 3).copy(), a[9:].copy()) for a in np.asarray(A, np.float64)]


def rows_of(keys):
    return np.concatenate([np.arange(6 * int(k), 6 * int(k) + 6) for k in keys])


def jacobian(g, X=None):
    """The whitened, robust-weighted Jacobian at X, dense."""
    return P.assemble(P.linearize(g, g.X if X is None else X)[0], g.n)[0].toarray()


def cov_svd(g, keys, X=None):
    _u, s, vt = np.linalg.svd(jacobian(g, X), full_matrices=False)
    V = vt.T[rows_of(keys)]
    return (V / (s * s)) @ V.T


def cov_qr(g, keys, X=None):
    R = np.linalg.qr(jacobian(g, X), mode="r")
    E = np.zeros((R.shape[0], 6 * len(keys)))
    E[rows_of(keys), np.arange(E.shape[1])] = 1.0
    Y = sla.solve_triangular(R, E, trans="T", lower=False)
    return Y.T @ Y


def cov_chain(g, keys, X=None):
    rows = P.linearize(g, g.X if X is None else X)[0]
    n = g.n
    chain = P.split_chain(g)
    assert min(chain) >= 0, "not a chain graph"
    cset = set(chain)
    Jc, _ = P.assemble([rows[f] for f in chain], n)
    extra = [rows[f] for f in range(len(rows)) if f not in cset]
    lu = spla.splu(Jc.tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=False))
    idx = rows_of(keys)
    E = np.zeros((6 * n, len(idx)))
    E[idx, np.arange(len(idx))] = 1.0
    y = lu.solve(E, trans="T")                               # J_c^-T E
    if extra:
        Jx, _ = P.assemble(extra, n)
        Kt = lu.solve(Jx.T.toarray(), trans="T")             # K^T = J_c^-T J_x^T
        S = np.eye(Kt.shape[1]) + Kt.T @ Kt
        y = y - Kt @ np.linalg.solve(S, Kt.T @ y)
    return lu.solve(y)[idx]


def cov_dense(g, keys, X=None):
    """The old reference, kept to record why it was replaced: the fp64 inverse of J^T J."""
    J = jacobian(g, X)
    idx = rows_of(keys)
    return np.linalg.inv(J.T @ J)[np.ix_(idx, idx)]


# ---- mpmath ------------------------------------------------------------------------------------------------------
def normal_matrix_mp(g, X=None, dps=60):
    """J^T J as an mpmath matrix, summed factor by factor from the fp64 entries of J (which convert exactly)."""
    import mpmath as mp
    mp.mp.dps = dps
    n = g.n
    H = mp.zeros(6 * n, 6 * n)
    for keys, blocks, _r in P.linearize(g, g.X if X is None else X)[0]:
        cols = [6 * k + c for k in keys for c in range(6)]
        B = np.concatenate(blocks, axis=1)
        for row in B:
            v = [mp.mpf(float(x)) for x in row]
            for a, ca in enumerate(cols):
                if v[a] == 0:
                    continue
                for b, cb in enumerate(cols):
                    H[ca, cb] += v[a] * v[b]
    return H


def columns_mp(g, columns, X=None, dps=60):
    """Columns `columns` of (J^T J)^-1 in mpmath: a list of lists of mpf, one per column, each of length 6 n."""
    import mpmath as mp
    mp.mp.dps = dps
    H = normal_matrix_mp(g, X, dps)
    m = H.rows
    A, p = mp.mp.LU_decomp(H)
    out = []
    for c in columns:
        e = mp.zeros(m, 1)
        e[int(c)] = mp.mpf(1)
        x = mp.mp.U_solve(A, mp.mp.L_solve(A, e, p))
        out.append([x[i] for i in range(m)])
    return out


def cov_mp(g, keys, X=None, dps=60, full_columns=()):
    """The block over `keys` rounded to fp64; with `full_columns` (indices into rows_of(keys)) also those whole columns of
    the inverse as (hi, lo) pairs of fp64 arrays, hi + lo holding 106 bits."""
    idx = rows_of(keys)
    cols = columns_mp(g, idx, X, dps)
    S = np.array([[float(col[i]) for col in cols] for i in idx])
    if not len(full_columns):
        return S
    hi = np.array([[float(v) for v in cols[c]] for c in full_columns])
    lo = np.array([[float(v - float(v)) for v in cols[c]] for c in full_columns])
    return S, hi, lo


# ---- comparison --------------------------------------------------------------------------------------------------
def _norm(a):
    return float(np.linalg.norm(a))


def block_gaps(got, want, anchor=None):
    """Per key pair (a, b) of the (6 k, 6 k) matrices and per 3x3 block type: {(a, b, type): (gap, held)}, a and b positions in
    the key list.  gap = |got - want| / |want|; a block whose reference norm is below HELD_BELOW of
    scale = sqrt(|want_xx(a, a)| |want_yy(b, b)|), xx and yy the types of its rows and columns, is "scale-held": held is True
    and gap = |got - want| / scale.  (Key 0's translation is left free by the prior and a turn of the map about key 0 does not
    move it, so it shares nothing with any rotation: those blocks have norm 3e-11 against a scale of up to 4e4, and a relative
    gap of such a block measures rounding only.)
    With `anchor` the norms and scales are taken from it instead of `want` (symmetry_gaps)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ref = want if anchor is None else np.asarray(anchor, np.float64)
    assert got.shape == want.shape == ref.shape and got.shape[0] == got.shape[1] and got.shape[0] % 6 == 0
    k = got.shape[0] // 6
    out = {}
    for a in range(k):
        for b in range(k):
            sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
            D, W, Wa, Wb = got[sa, sb] - want[sa, sb], ref[sa, sb], ref[sa, sa], ref[sb, sb]
            for ty in TYPES:
                ra, rb = _SL[ty]
                scale = math.sqrt(_norm(Wa[ra, ra]) * _norm(Wb[rb, rb]))
                wn = _norm(W[ra, rb])
                held = wn < HELD_BELOW * scale
                out[(a, b, ty)] = (_norm(D[ra, rb]) / (scale if held else wn), held)
    return out


def symmetry_gaps(cov, want):
    """As block_gaps, of `cov` against its own transpose, every block relative to the reference's norm of it: the symmetry
    check and the value check share one yardstick."""
    cov = np.asarray(cov, np.float64)
    return block_gaps(cov.T, cov, anchor=want)


def tested_gaps(got, want, all_keys, keys, pairs):
    """What the device is held on, of two matrices over `all_keys`: every listed key's 6x6 and every listed pair's 12x12.
    Returns (worst per type, the scale-held blocks as (row key, column key, type))."""
    out, held = {}, set()
    for ks in [(k,) for k in keys] + [tuple(p) for p in pairs]:
        gaps = block_gaps(sub(got, all_keys, ks), sub(want, all_keys, ks))
        for k, v in worst(gaps).items():
            out[k] = max(out.get(k, 0.0), v)
        held |= {(ks[a], ks[b], ty) for (a, b, ty), (_g, h) in gaps.items() if h}
    return out, held


def within(gaps, bound):
    """The (block, gap, bound) of a block_gaps result that lie over `bound` ({type or type + "_held": value})."""
    bad = []
    for key, (gap, held) in sorted(gaps.items()):
        name = key[2] + "_held" if held else key[2]
        assert name in bound, "block %s is %s in this reference, but the bounds hold no '%s': the set of scale-held blocks " \
                              "differs from the one the bounds were written for" % (key, "scale-held" if held else "not scale-held", name)
        b = bound[name]
        if not gap <= b:
            bad.append((key, gap, b))
    return bad


MARGIN = 10.0                       # the project's margin for differing summation orders: bound = MARGIN x floor


def floors(per_route):
    """(floor, excluded) from {route: {type: gap to the reference}}.  The floor of a type is the largest gap of the routes,
    with one exception, decided here and never by hand: where the chain route lies more than MARGIN times farther from the
    reference than every other route does, its gap does not count and is returned under `excluded`.  The routes that agree
    confirm the reference to their own, smaller gap; a gap beyond what a change of summation order explains is then the chain
    route's own error.  It happens under a GPS factor: Woodbury forms y = b - K^T S^-1 K b as the difference of two vectors of
    the size of J_c^-T e (1e4, the free translation of the chain alone) that cancel almost wholly along the pinned direction - a
    variance of 1e8 becomes 0.25 - and delta = J_c^-1 y multiplies what rounding left by 1e4 again: 2e-7 of the pinned key's
    translation block, where the SVD, the QR and here even the inverse of J^T J agree to 3e-8 and better.  The device does not take that
    difference - its conjugate gradients build y up from zero - and lies 6e-14 to 9e-12 from the SVD there."""
    floor, excluded = {}, {}
    for ty in sorted({t for g in per_route.values() for t in g}):
        gaps = {r: g[ty] for r, g in per_route.items() if ty in g}
        others = [v for r, v in gaps.items() if r != "chain"]
        if "chain" in gaps and others and gaps["chain"] > MARGIN * max(others):
            excluded[ty] = gaps.pop("chain")
        floor[ty] = max(gaps.values())
    return floor, excluded


def worst(gaps):
    """{type or type + "_held": largest gap} of a block_gaps result."""
    out = {}
    for (_a, _b, ty), (gap, held) in gaps.items():
        k = ty + "_held" if held else ty
        out[k] = max(out.get(k, 0.0), gap)
    return out
