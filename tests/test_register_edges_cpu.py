"""CPU companions of tests/test_register_edges_gpu.py: the scenes those tests build for the registration path (k_register,
k_certify_lean, the map index of k_bin_count / k_scatter_map, plane_fit_5x3), and the statement they are checked against.

The statement (ref_knn) is a plain numpy brute force: d2 in fp32 from the fp32-transformed query in the reference's
association order, (dx*dx + dy*dy) + dz*dz without FMA, ordered by (d2, original index), gated in float64 with
d2[4] < gate_sq (reference src/mapOptmization.cpp:1087-1097).  Every companion checks that its builder produces the edge
it is named for, and that the oracle agrees with the statement bit for bit on that scene.  PARITY UNPINNED."""
import numpy as np
import pytest

from liorf_amd import synth
from oracle import oracle as O

F = np.float32
GATES = [1.0, 0.25, 0.7, 0.3, 4.0]


# ---------------------------------------------------------------------------------------------------------------------
# the statement

def d2_row(q, m):
    """fp32 squared distances of query q to every row of m, L2_Simple order, no FMA."""
    d = (np.asarray(q, F)[None, :] - np.asarray(m, F)).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def translate(scan, pose):
    """pointAssociateToMap (reference :302-308) in fp32, the reference's association order.  Without rotation T is the
    identity exactly, and sel = ((x + 0) + 0) + t."""
    T = O.getTransformation(pose)
    s = np.asarray(scan, F)[:, :3]
    out = np.empty_like(s)
    for r in range(3):
        out[:, r] = ((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3]
    return out


def ref_knn(map_xyz, queries, gate_sq, k=7):
    """The k nearest map points of every query by (d2, original index), their fp32 d2, and the float64 gate decision."""
    m = np.ascontiguousarray(np.asarray(map_xyz, F)[:, :3])
    q = np.asarray(queries, F)
    kk = min(k, m.shape[0])
    idx = np.full((q.shape[0], k), -1, np.int64)
    d2 = np.full((q.shape[0], k), np.inf, F)
    for i in range(q.shape[0]):
        d = d2_row(q[i], m)
        thr = np.partition(d, kk - 1)[kk - 1]
        c = np.nonzero(d <= thr)[0]
        o = c[np.lexsort((c, d[c]))][:kk]
        idx[i, :kk], d2[i, :kk] = o, d[o]
    gated = d2[:, 4].astype(np.float64) < gate_sq
    return idx, d2, gated


def oracle_surf(sc, pose=None):
    orc = O.Oracle(knn_backend=0, num_threads=8, gate_sq=sc["gate_sq"])
    orc.set_map(sc["map"])
    orc.set_scan(sc["scan"])
    out = orc.surfOptimization(sc["pose"] if pose is None else pose)
    orc.close()
    return out


def assert_oracle_is_the_statement(sc, pose=None):
    """Gate decision, indices (gated) and d2 bits (gated) of the oracle's brute force == ref_knn."""
    pose = sc["pose"] if pose is None else pose
    idx, d2, gated = ref_knn(sc["map"], translate(sc["scan"], pose), sc["gate_sq"])
    oidx, od2, _, _ = oracle_surf(sc, pose)
    assert np.array_equal(oidx[:, 0] >= 0, gated)
    assert np.array_equal(oidx[gated], idx[gated, :5])
    assert np.array_equal(od2[gated].view(np.uint32), d2[gated, :5].view(np.uint32))
    return idx, d2, gated


def ulps(a, b):
    """Distance in ulps of two positive fp32 arrays."""
    return np.abs(np.asarray(a, F).view(np.int32).astype(np.int64) - np.asarray(b, F).view(np.int32).astype(np.int64))


def step_ulps(x, k):
    """x moved by k ulps (k may be negative)."""
    b = np.asarray(x, F).view(np.int32).astype(np.int64)
    s = np.where(np.asarray(x) < 0, -1, 1)
    return (b + s * k).astype(np.int32).view(F)


def place(q, target, ax, sgn, perp, exact=True):
    """A map point whose fp32 d2 from q is exactly `target`: along axis `ax` (direction sgn), fine-tuned along `perp`.
    exact=False: just about there (small targets far from the origin cannot always be hit)."""
    q = np.asarray(q, F)
    t = F(target)
    base = F(np.float64(q[ax]) + sgn * np.sqrt(np.float64(t)))
    if not exact:
        m = q.copy()
        m[ax] = base
        return m
    for j in range(0, 8):
        c = step_ulps(base, -j if sgn > 0 else j) if q[ax] + sgn >= 0 else step_ulps(base, j if sgn > 0 else -j)
        dx = F(q[ax] - c)
        rest = np.float64(t) - np.float64(F(dx * dx))
        if rest < 0:
            continue
        b0 = F(np.float64(q[perp]) + np.sqrt(rest))
        cand = np.unique(np.concatenate([[q[perp]], step_ulps(np.full(161, b0), np.arange(-80, 81))]))
        m = np.repeat(q[None, :], cand.size, 0)
        m[:, ax] = c
        m[:, perp] = cand
        hit = np.nonzero(d2_row(q, m).view(np.uint32) == np.array(t, F).view(np.uint32))[0]
        if hit.size:
            return m[hit[0]]
    raise AssertionError(f"no point at d2 {t!r} from {q}")


AXES = [(0, 1.0, 1), (0, -1.0, 2), (1, 1.0, 2), (1, -1.0, 0), (2, 1.0, 0), (2, -1.0, 1)]


def lattice(lo, hi, step):
    v = np.arange(lo, hi, step)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)


def scene(map_pts, scan_pts, gate_sq, pose=None, perm_seed=None, **meta):
    m = np.asarray(map_pts, F)
    if perm_seed is not None:                      # original indices run against the order of construction
        m = m[np.random.default_rng(perm_seed).permutation(m.shape[0])]
    s = np.asarray(scan_pts, F)
    return dict(map=m, scan=s, gate_sq=float(gate_sq), pose=np.zeros(6, F) if pose is None else np.asarray(pose, F), **meta)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gate

def gate_scene(gate_sq, seed=0):
    """One query per cluster, clusters far apart.  Four near neighbours, the 5th at exactly prev(g), g or next(g) with
    g = float32(gate_sq) (along one of six axis directions), and a 6th: none, at the 5th's d2 (a tie across the 5th/6th
    boundary at the gate) or 3 ulps beyond.  Identity rotation and queries in [32, 64): every d2 is exact, and a pose
    translation of k * 2^-18 moves every query by exactly k ulps."""
    rng = np.random.default_rng(seed)
    g = F(gate_sq)
    R = float(np.sqrt(gate_sq))
    S = 4.0 * R + 1.0
    grid = lattice(33.0, 63.0, S)
    variants = [(t, a, six) for t in (-1, 0, 1) for a in range(6) for six in ("none", "tie", "beyond")]
    mp, qs, what = [], [], []
    for n, q in enumerate(grid.astype(F)):
        t, a, six = variants[n % len(variants)]
        ax, sgn, perp = AXES[a]
        tgt = step_ulps(g, t)
        for k in range(4):
            ang = 2 * np.pi * (k + rng.random() * 0.5) / 4
            off = np.zeros(3)
            off[perp], off[3 - ax - perp] = np.cos(ang), np.sin(ang)
            mp.append(q + (0.25 + 0.1 * k) * R * off)
        mp.append(place(q, tgt, ax, sgn, perp))
        ax2, sgn2, perp2 = AXES[(a + 3) % 6]
        if six == "tie":
            mp.append(place(q, tgt, ax2, sgn2, perp2))
        elif six == "beyond":
            mp.append(place(q, step_ulps(tgt, 3), ax2, sgn2, perp2))
        qs.append(q)
        what.append((t, six))
    return scene(mp, qs, gate_sq, perm_seed=seed + 1, target=np.array([w[0] for w in what]),
                 sixth=np.array([w[1] for w in what]))


@pytest.mark.parametrize("gate_sq", GATES)
def test_gate_scene_puts_the_fifth_neighbour_on_the_gate(gate_sq):
    sc = gate_scene(gate_sq)
    idx, d2, gated = assert_oracle_is_the_statement(sc)
    g = F(gate_sq)
    for t in (-1, 0, 1):
        sel = sc["target"] == t
        assert np.array_equal(d2[sel, 4].view(np.uint32), np.full(sel.sum(), step_ulps(g, t)).view(np.uint32))
    tie = sc["sixth"] == "tie"
    assert np.array_equal(d2[tie, 5].view(np.uint32), d2[tie, 4].view(np.uint32))
    # the float64 decision at g itself: gated iff float32(gate_sq) < gate_sq (0.7 rounds down, 0.3 up)
    assert np.all(gated[sc["target"] == -1]) and not np.any(gated[sc["target"] == 1])
    assert np.all(gated[sc["target"] == 0] == (np.float64(g) < gate_sq))
    # the pose walk: 1-ulp translations move every query by exactly one ulp (queries in [32, 64))
    q0 = translate(sc["scan"], sc["pose"])
    q1 = translate(sc["scan"], np.array([0, 0, 0, 2.0 ** -18, 0, 0], F))
    assert np.all(ulps(q1[:, 0], q0[:, 0]) == 1)


# ---------------------------------------------------------------------------------------------------------------------
# 2. non-default gates

NONDEFAULT_GATES = [0.01, 0.25, 4.0, 100.0]


def grid_of(map_xyz, gate_sq):
    """The search grid as set_map_build derives it: (E, origin, dims, doublings), or None (S2M_ERR_CAPACITY)."""
    m = np.asarray(map_xyz, F)[:, :3]
    mn, mx = m.min(0), m.max(0)
    E = np.sqrt(gate_sq) * 1.025
    for attempt in range(32):
        Ef = F(E)
        inv = F(F(1.0) / Ef)
        o = (mn - Ef).astype(F)
        n = np.floor((mx.astype(np.float64) - o.astype(np.float64)) * np.float64(inv)) + 2.0
        if np.prod(n) <= 2 ** 27 and np.all(n < 65536):
            return dict(E=Ef, inv_e=inv, origin=o, dims=n.astype(np.int64), doublings=attempt)
        E *= 2.0
    return None


def cell_of(p, g):
    """cell_coord (s2m_device.hpp) in fp32."""
    p = np.asarray(p, F)
    f = np.floor(((p - g["origin"]).astype(F) * g["inv_e"]).astype(F))
    return np.clip(f, 0, g["dims"] - 1).astype(np.int64)


def block_counts(map_xyz, queries, g):
    """Map points in the 3x3x3 cells around each query's cell: the candidates a search of that query may have to see."""
    dims = g["dims"]
    lin = lambda c: (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    ids, cnt = np.unique(lin(cell_of(map_xyz, g)), return_counts=True)
    qc = cell_of(queries, g)
    out = np.zeros(len(qc), np.int64)
    for d in lattice(-1, 2, 1):
        c = qc + d
        ok = np.all((c >= 0) & (c < dims), axis=1)
        j = np.clip(np.searchsorted(ids, lin(c)), 0, len(ids) - 1)
        out += np.where(ok & (ids[j] == lin(c)), cnt[j], 0)
    return out


def clump_scene(cfg, gate_sq):
    """The scene of test_dense_clump_and_scattered_queries_under_every_path (tests/test_tiers_gpu.py), smaller: queries
    around the densest 2 m slab of the map and scattered near map points, and 4 000 more map points in a 0.25 m clump."""
    rng = np.random.default_rng(11)
    m = cfg["map"]
    c = m[np.argmax(np.bincount((m[:, 0] // 2).astype(int) - int(m[:, 0].min() // 2)))]
    q = np.concatenate([c + rng.normal(0, 1.5, (1500, 3)),
                        m[rng.choice(len(m), 800, replace=False)] + rng.normal(0, 0.4, (800, 3))]).astype(F)
    dense = (c + rng.normal(0, 0.25, (4000, 3))).astype(F)
    return scene(np.concatenate([m, dense]), q, gate_sq, pose=np.array([0, 0, 0, 0.05, -0.03, 0.02], F))


@pytest.mark.parametrize("gate_sq", NONDEFAULT_GATES)
def test_non_default_gates_reach_their_paths(cfg_small, gate_sq):
    """0.01: 0.1 m cells, a handful of candidates and most queries not gated.  100: 10 m cells, hundreds to thousands
    of candidates per query - more than a tile (kTilePts = 512) and more than a served lane's area (kServeCap = 1 024),
    so searches overflow their tiles, lanes are served and the Top5k fallback sweeps."""
    sc = scene(cfg_small["map"], cfg_small["scan"][::40], gate_sq, pose=cfg_small["pose_init"])
    _, d2, gated = assert_oracle_is_the_statement(sc)
    assert (gated.sum() < len(gated)) if gate_sq < 1 else (gated.sum() > 0.9 * len(gated))
    g = grid_of(cfg_small["map"], gate_sq)
    assert g is not None and abs(float(g["E"]) - np.sqrt(gate_sq) * 1.025) < 1e-5 * max(1, np.sqrt(gate_sq))
    cl = clump_scene(cfg_small, gate_sq)
    assert_oracle_is_the_statement(dict(cl, scan=cl["scan"][::10]))
    for s in (sc, cl):
        n = block_counts(s["map"], translate(s["scan"], s["pose"]), grid_of(s["map"], gate_sq))
        if gate_sq == 0.01:
            assert g["E"] < F(0.103) and np.median(n) < 16, np.median(n)
        if gate_sq == 100.0:
            assert np.median(n) > 512 and np.mean(n > 1024) > 0.5, (np.median(n), np.mean(n > 1024))


# ---------------------------------------------------------------------------------------------------------------------
# 3. near-ties below the sweep key's resolution (2^9 ulps of d2)

NEAR_K = [1, 2, 4, 8, 16, 64, 256, 1024]


def near_tie_scene(k, seed=0):
    """Shells of map points along the six axis directions.  Half the clusters ('across'): ranks 1..4 well inside, ranks 5,
    6, 7 at t0, t0 + k ulps, t0 + 2k ulps.  The other half ('inside'): ranks 2..6 at t0 + j*k ulps, j = 0..4.  The
    points are listed farthest first, so original indices run against distance order."""
    rng = np.random.default_rng(seed + 1000 * k)
    mp, qs, mode = [], [], []
    for n, q in enumerate(lattice(33.0, 63.0, 4.0).astype(F)):
        t0 = F(rng.uniform(0.2, 0.7))
        pts = []
        if n % 2 == 0:
            near = [F(v) for v in (0.01, 0.02, 0.04, 0.06)] + [step_ulps(t0, j * k) for j in range(3)]
            exact = [False] * 4 + [True] * 3
            mode.append("across")
        else:
            near = [F(0.01)] + [step_ulps(t0, j * k) for j in range(5)] + [F(0.85)]
            exact = [False] + [True] * 5 + [False]
            mode.append("inside")
        dirs = rng.permutation(6)
        for j, t in enumerate(near):
            ax, sgn, perp = AXES[dirs[j % 6]]
            if j >= 6:                                 # a 7th direction: the first direction's axis, the other way
                sgn = -sgn
            pts.append(place(q, t, ax, sgn, perp, exact[j]))
        mp.extend(pts[::-1])
        qs.append(q)
    return scene(mp, qs, 1.0, mode=np.array(mode))


@pytest.mark.parametrize("k", NEAR_K)
def test_near_tie_scene_differs_below_the_key_resolution(k):
    sc = near_tie_scene(k)
    idx, d2, gated = assert_oracle_is_the_statement(sc)
    assert gated.all()
    a = sc["mode"] == "across"
    d56 = ulps(d2[a, 5], d2[a, 4])
    assert np.all(d56 == k) and np.all(ulps(d2[a, 6], d2[a, 5]) == k)
    if k < 256:
        assert np.all(d56 < 2 ** 9)
    i = ~a
    assert np.all(ulps(d2[i, 5], d2[i, 1]) == 4 * k)
    # indices run against distance order inside every cluster
    assert np.mean(idx[:, 4] < idx[:, 0]) > 0.9


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact ties and duplicates

DUP_COUNTS = [5, 6, 7, 8, 64, 511, 512, 513, 1025, 2000]


def tie_scene(seed=0):
    """Equidistant shells (6 axis points, 8 cube corners, 12 edge midpoints; with and without inner points), coincident
    duplicates in DUP_COUNTS copies (queries on them, d2 = 0, and 1 cm / 10 cm off), and clusters of points 1 ulp apart.
    The map order is shuffled."""
    rng = np.random.default_rng(seed)
    mp, qs, kind = [], [], []
    a = F(0.5)
    ax6 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    edge = np.array([v for v in (np.array([x, y, 0]) for x in (-1, 1) for y in (-1, 1))] +
                    [[x, 0, z] for x in (-1, 1) for z in (-1, 1)] + [[0, y, z] for y in (-1, 1) for z in (-1, 1)], F)
    cells = lattice(33.0, 63.0, 4.0).astype(F)
    rng.shuffle(cells)
    c = iter(cells)
    for shell, name in ((ax6, "axis"), (cube, "corner"), (edge, "edge")):
        for inner in (0, 2, 3, 4):
            for rep in range(2):
                q = next(c)
                mp.extend(q + a * shell)
                mp.extend(q + F(0.125) * ax6[rng.permutation(6)[:inner]] * F(0.5))
                qs.append(q)
                kind.append(f"{name}{inner}")
    for k in DUP_COUNTS:
        p = next(c)
        mp.extend(np.repeat(p[None], k, 0))
        for off in (0.0, 0.01, 0.1):
            qs.append((p + np.array([off, -off / 2, off / 4])).astype(F))
            kind.append(f"dup{k}")
    for n in (6, 20):
        for ax in range(3):
            p = next(c)
            pts = np.repeat(p[None], n, 0)
            pts[:, ax] = step_ulps(np.full(n, p[ax]), np.arange(n) - n // 2)
            mp.extend(pts)
            for off in (0.0, 0.003):
                qs.append((p + off).astype(F))
                kind.append(f"ulp{n}")
    return scene(mp, qs, 1.0, perm_seed=seed + 7, kind=np.array(kind))


def test_tie_scene_has_ties_across_the_fifth_and_sixth():
    sc = tie_scene()
    idx, d2, gated = assert_oracle_is_the_statement(sc)
    assert gated.all()
    tie56 = d2[:, 4].view(np.uint32) == d2[:, 5].view(np.uint32)
    for name in ("axis0", "corner0", "edge0", "axis2", "corner4", "edge3"):
        assert tie56[sc["kind"] == name].all(), name
    dup = np.char.startswith(sc["kind"], "dup")
    assert np.all(d2[dup][::3, :5] == 0) and tie56[dup & (sc["kind"] != "dup5")].all()
    assert sc["map"].shape[0] > sum(DUP_COUNTS)
    # the copies of a point are not contiguous in the map's original order
    k2000 = np.nonzero(sc["kind"] == "dup2000")[0][0]
    same = np.nonzero((sc["map"] == sc["scan"][k2000]).all(1))[0]
    assert same.size == 2000 and same[-1] - same[0] > 2000


# ---------------------------------------------------------------------------------------------------------------------
# 5. plane_fit_5x3 at its degeneracies

def plane_fit_mirror(A):
    """ColPivHouseholderQR<Matrix<float,5,3>>::solve(-1) as oracle/s2m_oracle.c states it, in numpy fp32, with what it
    did on the way: (x, nonzero_pivots, tailSq <= FLT_MIN taken, norm down-date recomputed, column-norm tie at a pivot)."""
    qr = np.array(A, F).copy()
    nd = np.array([np.sqrt(F(sum((qr[i, k] * qr[i, k] for i in range(5)), F(0)))) for k in range(3)], F)
    nu = nd.copy()
    perm = [0, 1, 2]
    eps = np.finfo(F).eps
    th = F(nu.max() * eps)
    helper = F(F(th * th) / F(5))
    down_th = np.sqrt(F(eps))
    rank, tail_small, recomputed, norm_tie = 3, False, False, False
    h = np.zeros(3, F)
    for k in range(3):
        big = k
        for j in range(k + 1, 3):
            if nu[j] > nu[big]:
                big = j
        norm_tie = norm_tie or any(nu[j] == nu[big] for j in range(k, 3) if j != big)
        if rank == 3 and F(nu[big] * nu[big]) < F(helper * F(5 - k)):
            rank = k
        if big != k:
            qr[:, [k, big]] = qr[:, [big, k]]
            nu[[k, big]] = nu[[big, k]]
            nd[[k, big]] = nd[[big, k]]
            perm[k], perm[big] = perm[big], perm[k]
        tail = F(0)
        for i in range(k + 1, 5):
            tail = F(tail + F(qr[i, k] * qr[i, k]))
        c0 = qr[k, k]
        if tail <= np.finfo(F).tiny:
            tau, beta = F(0), c0
            qr[k + 1:, k] = 0
            tail_small = True
        else:
            beta = np.sqrt(F(F(c0 * c0) + tail))
            beta = -beta if c0 >= 0 else beta
            den = F(c0 - beta)
            for i in range(k + 1, 5):
                qr[i, k] = F(qr[i, k] / den)
            tau = F(F(beta - c0) / beta)
        qr[k, k], h[k] = beta, tau
        if tau != 0:
            for j in range(k + 1, 3):
                tmp = F(0)
                for i in range(k + 1, 5):
                    tmp = F(tmp + F(qr[i, k] * qr[i, j]))
                tmp = F(tmp + qr[k, j])
                qr[k, j] = F(qr[k, j] - F(tau * tmp))
                for i in range(k + 1, 5):
                    qr[i, j] = F(qr[i, j] - F(F(tau * qr[i, k]) * tmp))
        for j in range(k + 1, 3):
            if nu[j] != 0:
                t = F(abs(qr[k, j]) / nu[j])
                t = F(F(F(1) + t) * F(F(1) - t))
                t = max(t, F(0))
                r = F(nu[j] / nd[j])
                t2 = F(t * F(r * r))
                if t2 <= down_th:
                    s = F(0)
                    for i in range(k + 1, 5):
                        s = F(s + F(qr[i, j] * qr[i, j]))
                    nd[j] = np.sqrt(s)
                    nu[j] = nd[j]
                    recomputed = True
                else:
                    nu[j] = F(nu[j] * np.sqrt(t))
    x = np.zeros(3, F)
    if rank == 0:
        return x, rank, tail_small, recomputed, norm_tie
    c = np.full(5, F(-1))
    for k in range(rank):
        if h[k] != 0:
            tmp = F(0)
            for i in range(k + 1, 5):
                tmp = F(tmp + F(qr[i, k] * c[i]))
            tmp = F(tmp + c[k])
            c[k] = F(c[k] - F(h[k] * tmp))
            for i in range(k + 1, 5):
                c[i] = F(c[i] - F(F(h[k] * qr[i, k]) * tmp))
    for i in range(rank - 1, -1, -1):
        if c[i] != 0:
            c[i] = F(c[i] / qr[i, i])
            for r in range(i):
                c[r] = F(c[r] - F(c[i] * qr[r, i]))
    for i in range(rank):
        x[perm[i]] = c[i]
    return x, rank, tail_small, recomputed, norm_tie


def plane_scene(seed=0):
    """Isolated 5-point clusters (4 m apart, gate 1), one query at each centre: the tuple is exactly the cluster.  Kinds:
    well-conditioned noisy planes; column-norm ties (x and y columns permutations of exactly summable values; all three);
    collinear tuples (axis-aligned and oblique); a collinear tuple with one point moved 2^-k off the line, k = 1..40;
    five identical points; planes through the origin (z = 0 and x = -y); a scale sweep of the cluster from 4 m down to
    2^-70 m about (X, 0, 0), where the squares of the small columns go subnormal.  Gate 16 (4 m cells), clusters 12 m
    apart, so that the 4 m clusters are inside the gate too."""
    rng = np.random.default_rng(seed)
    clusters, kind = [], []
    grid = iter(lattice(-60.0, 60.0, 12.0)[rng.permutation(10 ** 3)].astype(F))

    def add(c, pts, name):
        clusters.append((np.asarray(c, F), np.asarray(pts, F)))
        kind.append(name)

    for _ in range(20):
        c = next(grid) + F(8)
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = np.cross(n, [1.0, 0.3, 0.1])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        ab = rng.uniform(-0.3, 0.3, (5, 2))
        add(c, c + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0, 0.002, (5, 1)) * n, "plane")
    vals = np.array([0.0, 0.25, -0.25, 0.5, -0.5], F)
    for X in (34.0, 42.0, 50.0):
        c = np.array([X, X, 10.0], F)
        add(c, np.stack([X + vals, X + vals[[2, 0, 4, 1, 3]], 10.0 + vals[[1, 3, 0, 4, 2]] * F(0.125)], 1), "norm_tie2")
        c = np.array([X, X, X], F)
        add(c + F(4), np.stack([X + 4 + vals, X + 4 + vals[[3, 4, 0, 2, 1]], X + 4 + vals[[4, 2, 1, 0, 3]]], 1), "norm_tie3")
    ts = np.array([-0.3, -0.1, 0.0, 0.15, 0.3], F)
    for ax in range(3):
        c = next(grid)
        p = np.repeat(c[None], 5, 0)
        p[:, ax] += ts
        add(c, p, "collinear_axis")
    for _ in range(6):
        c = next(grid)
        d = rng.normal(size=3)
        add(c, c + ts[:, None] * (d / np.linalg.norm(d)), "collinear")
    for k in range(1, 41):
        c = next(grid)
        d = np.array([1.0, 2.0, 0.5]) / np.linalg.norm([1.0, 2.0, 0.5])
        e = np.cross(d, [0.0, 0.0, 1.0])
        e /= np.linalg.norm(e)
        p = (c + ts[:, None] * d).astype(F)
        p[3] = (p[3] + 2.0 ** -k * e).astype(F)
        add(c, p, f"rank{k}")
    for _ in range(3):
        c = next(grid)
        add(c, np.repeat(c[None], 5, 0), "identical")
    for X, Y in ((44.0, 44.0), (44.0, -44.0), (52.0, 48.0)):
        c = np.array([X, Y, 0.0], F)
        add(c, np.stack([X + vals, Y + vals[[1, 3, 0, 4, 2]], np.zeros(5)], 1), "origin_z0")
        c = np.array([X, -X, Y], F)
        add(c, np.stack([X + vals, -X - vals, Y + vals[[2, 0, 4, 1, 3]]], 1), "origin_xy")
    pat = np.array([[0.0, 0.0, 0.0], [0.3, 1.0, 0.2], [-0.2, -0.5, 1.0], [0.1, 0.7, -0.9], [-0.4, -0.8, -0.6]])
    pat *= 0.99 / np.linalg.norm(pat, axis=1).max()
    for n, k in enumerate(list(range(-2, 64, 2)) + [64, 66, 68, 70]):
        c = np.array([100.0 + 12.0 * n, 0.0, 0.0], F)
        add(c, (c + 2.0 ** -k * pat).astype(F), f"scale{k}")
    mp = np.concatenate([p for _, p in clusters])
    return scene(mp, np.stack([c for c, _ in clusters]), 16.0, kind=np.array(kind),
                 tuples=np.arange(mp.shape[0]).reshape(-1, 5))


def test_plane_scene_reaches_every_degeneracy_of_the_plane_fit():
    sc = plane_scene()
    idx, d2, gated = assert_oracle_is_the_statement(sc)
    assert gated.all()
    assert np.array_equal(np.sort(idx[:, :5], 1), sc["tuples"]), "a tuple is not exactly its cluster"
    m = sc["map"]
    kinds = sc["kind"]
    info = {}
    for i in range(len(kinds)):
        A = m[idx[i, :5]]
        x = np.zeros(3, F)
        O.lib().orc_plane_fit_5x3(O._fp(np.ascontiguousarray(A)), O._fp(x))
        xm, rank, tail, rec, tie = plane_fit_mirror(A)
        assert np.array_equal(xm.view(np.uint32), x.view(np.uint32)), (kinds[i], xm, x)
        info[i] = (rank, tail, rec, tie)
        if kinds[i] == "plane":                        # well-conditioned: the float64 least-squares normal
            xl = np.linalg.lstsq(A.astype(np.float64), -np.ones(5), rcond=None)[0]
            cos = abs(np.dot(xl, x)) / (np.linalg.norm(xl) * np.linalg.norm(x))
            assert cos > 1 - 1e-6, (i, cos)
    rank = np.array([info[i][0] for i in range(len(kinds))])
    tail = np.array([info[i][1] for i in range(len(kinds))])
    rec = np.array([info[i][2] for i in range(len(kinds))])
    tie = np.array([info[i][3] for i in range(len(kinds))])
    assert tie[np.char.startswith(kinds, "norm_tie")].all()
    assert np.all(rank[np.char.startswith(kinds, "collinear")] <= 2)
    assert np.all(rank[kinds == "identical"] == 1)
    rk = np.array([rank[kinds == f"rank{k}"][0] for k in range(1, 41)])
    assert rk[0] == 3 and rk[-1] == 2, rk                 # both sides of the rank threshold
    assert tail[kinds == "origin_z0"].all() and tail[kinds == "identical"].all()
    assert rec.sum() > 20
    sq = [i for i in range(len(kinds)) if kinds[i].startswith("scale")]
    small = m[idx[sq, :5]][:, :, 1:]
    assert np.any((np.abs(small * small) < np.finfo(F).tiny) & (small != 0)), "no subnormal squares"


# ---------------------------------------------------------------------------------------------------------------------
# 6. cell faces

FACE_OFFSETS = [(0.0, 0.0, 0.0), (20000.0, -20000.0, 20000.0)]


def face_scene(offset, seed=0):
    """The grid of set_map_build (E = float32(1.025), origin = bounding-box minimum - E, fixed by two anchors 50 m apart).
    Queries at a cell corner origin + k*E moved by -4..4 ulps per axis, four near neighbours around it (two of them on
    the faces, within ulps), the deciding 5th neighbour 0.45..0.9 m away in a direction that crosses one, two or three
    faces, and a 6th a little farther.  Queries outside the bounding box as well: by 0.5 m (neighbours inside the gate)
    and by 5 m and 100 m (none)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    anchors = (o + np.array([[0.0, 0.0, 0.0], [50.0, 50.0, 50.0]])).astype(F)
    g = grid_of(anchors, 1.0)
    E, org = np.float64(g["E"]), g["origin"].astype(np.float64)
    mp, qs = list(anchors), []
    ks = lattice(4, 46, 4).astype(np.int64)
    ks = ks[rng.permutation(len(ks))[:300]]
    for n, k in enumerate(ks):
        P = (org + k * E).astype(F)
        q = step_ulps(P, rng.integers(-4, 5, 3))
        for j in range(4):
            d = rng.normal(size=3)
            pt = (q + 0.12 * (j + 1) / 2 * d / np.linalg.norm(d)).astype(F)
            if j < 2:
                ax = rng.integers(3)
                pt[ax] = step_ulps(P[ax], rng.integers(-4, 5))
            mp.append(pt)
        cross = n % 3 + 1
        d = rng.uniform(0.3, 1.0, 3) * np.where(rng.random(3) < 0.5, -1, 1)
        axes = rng.permutation(3)[:cross]
        qc = cell_of(q[None], g)[0]
        for a in range(3):                              # toward the neighbouring cell on the axes to cross, inward elsewhere
            lo = org[a] + qc[a] * E
            if a in axes:
                d[a] = -abs(d[a]) if q[a] - lo < E / 2 else abs(d[a])
            else:
                d[a] = abs(d[a]) if q[a] - lo < E / 2 else -abs(d[a])
        d /= np.linalg.norm(d)
        r5 = rng.uniform(0.45, 0.9)
        mp.append((q + r5 * d).astype(F))
        mp.append((q + (r5 + 0.02) * -d[[1, 2, 0]]).astype(F))
        qs.append(q)
    hi = anchors[1].astype(np.float64)
    for j in range(6):
        mp.append((hi - rng.uniform(0.05, 0.6, 3)).astype(F))
    for out in (0.5, 5.0, 100.0):
        for a in range(3):
            q = hi - 0.3
            q[a] = hi[a] + out
            qs.append(q.astype(F))
    return scene(mp, qs, 1.0, perm_seed=seed + 3, grid=g, n_corner=len(ks))


@pytest.mark.parametrize("offset", FACE_OFFSETS)
def test_face_scene_decides_across_faces_edges_and_corners(offset):
    sc = face_scene(offset)
    idx, d2, gated = assert_oracle_is_the_statement(sc)
    g = grid_of(sc["map"], 1.0)
    assert g["doublings"] == 0 and np.array_equal(g["origin"], sc["grid"]["origin"])
    nc = sc["n_corner"]
    q = translate(sc["scan"], sc["pose"])
    qc = cell_of(q, g)
    c5 = cell_of(sc["map"][idx[:, 4]], g)
    across = (qc != c5).sum(1)[:nc][gated[:nc]]
    for k in (1, 2, 3):
        assert (across == k).sum() >= 20, (k, np.bincount(across))
    # the queries straddle the faces: the ulp offsets put them on both sides of a corner
    k = np.round((q[:nc].astype(np.float64) - g["origin"]) / np.float64(g["E"]))
    assert set(np.unique(qc[:nc] - k)) == {-1, 0}
    out = q[nc:]
    assert np.any(out > sc["map"].max(0), axis=1).all()
    assert gated[nc:nc + 3].all() and not gated[nc + 3:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. grid coarsening and capacity

OUTLIERS = [70000.0, 1.0e6, -1.6e7]


def coarse_scene(cfg, far):
    """A configuration's map with one finite outlier `far` metres out along x.  An outlier on the negative side becomes
    the grid origin: the map then lies 1.6e7 m from it, where fp32 rounds (v - origin) to a metre and only the slab
    margins (kSlabMargin + kSlabRound per metre) keep the row and cell bounds below the true distances.  It is moved so
    that a cell face of the coarsened grid runs through the middle of the map."""
    for _ in range(3 if far < 0 else 1):
        m = np.concatenate([cfg["map"], np.array([[far, 0.0, 0.0]], F)]).astype(F)
        if far < 0:
            g = grid_of(m, 1.0)
            E, o = np.float64(g["E"]), np.float64(g["origin"][0])
            far -= o + np.round(-o / E) * E
    return scene(m, cfg["scan"], 1.0, pose=cfg["pose_init"])


@pytest.mark.parametrize("far", OUTLIERS)
def test_outlier_forces_the_grid_to_coarsen(cfg_tiny, far):
    sc = coarse_scene(cfg_tiny, far)
    g = grid_of(sc["map"], 1.0)
    assert g["doublings"] == {70000.0: 1, 1.0e6: 4, -1.6e7: 8}[far], g
    if far < 0:                                   # a face through the map, and queries a metre of rounding from the origin
        q = translate(sc["scan"], sc["pose"])
        assert len(np.unique(cell_of(sc["map"][:-1], g)[:, 0])) == 2 and len(np.unique(cell_of(q, g)[:, 0])) == 2
        assert np.spacing((q[:, 0] - g["origin"][0]).astype(F)).min() >= 1.0
    assert grid_of(np.concatenate([sc["map"], [[1e30, 0, 0]]]), 1.0) is None
    sub = dict(sc, scan=sc["scan"][::10], pose=np.array([0, 0, 0, 0.5, -0.25, 0.125], F))
    assert_oracle_is_the_statement(sub)


# ---------------------------------------------------------------------------------------------------------------------
# 8. certificates under flip-flop

def flip_scene(seed=0):
    """Queries in (-16, 16) (ulps below 1 um, so 1 um translations move them).  'swap56': the 5th and 6th on the x axis
    at equal d2 (the query on their bisector), four nearer; 'gate': the 5th along +x at d2 = float32(1.0), no 6th inside
    the gate; 'swap23': the 2nd and 3rd on the x axis at equal d2.  Which of each pair has the lower index alternates."""
    rng = np.random.default_rng(seed)
    mp, qs, kind = [], [], []
    for n, q in enumerate(lattice(-14.0, 14.5, 3.5).astype(F)):
        name = ("swap56", "gate", "swap23")[n % 3]
        if name == "gate":
            a = F(0.6)
            near = [place(q, F(t), *AXES[j + 2], exact=False) for j, t in enumerate((0.04, 0.09, 0.16, 0.25))]
            pair = [place(q, F(1.0), 0, 1.0, 1)]
        else:
            a = F(0.625) if name == "swap56" else F(0.125)
            r = [0.05, 0.3, 0.35, 0.4]
            near = [place(q, F(t * t), *AXES[j + 2], exact=False) for j, t in enumerate(r)] if name == "swap56" else \
                [place(q, F(0.0025), 1, 1.0, 2, exact=False)] + \
                [place(q, F(t * t), *AXES[j + 2], exact=False) for j, t in enumerate(r[1:])]
            pair = [(q + np.array([a, 0, 0], F)).astype(F), (q - np.array([a, 0, 0], F)).astype(F)]
            if (n // 3) % 2:
                pair = pair[::-1]
        mp.extend(pair + near)
        qs.append(q)
        kind.append(name)
    return scene(mp, qs, 1.0, kind=np.array(kind))


FLIP_STEPS = [("ulps", 3), ("um", 1e-6), ("30um", 3e-5)]


def flip_poses(step):
    name, v = step
    d = F(v * 2.0 ** -20) if name == "ulps" else F(v)       # ulps: 3 ulps of a coordinate in [8, 16)
    return [np.array([0, 0, 0, d if k % 2 else 0, 0, 0], F) for k in range(6)]


@pytest.mark.parametrize("step", FLIP_STEPS)
def test_flip_scene_swaps_neighbours_every_step(step):
    sc = flip_scene()
    kind = sc["kind"]
    p0, p1 = flip_poses(step)[:2]
    i0, d0, g0 = assert_oracle_is_the_statement(sc, p0)
    i1, d1, g1 = assert_oracle_is_the_statement(sc, p1)
    s56 = kind == "swap56"
    assert np.all(d0[s56, 4] == d0[s56, 5])                    # the bisector: a tie at p
    moved = np.any(translate(sc["scan"], p1) != translate(sc["scan"], p0), axis=1)
    assert moved.mean() > 0.9
    sw = (i0[s56, 4] != i1[s56, 4])[moved[s56]]
    assert sw.mean() > 0.4                                  # half of the pairs have their nearer member second by index
    s23 = kind == "swap23"
    assert np.all(d0[s23, 1] == d0[s23, 2]) and ((i0[s23, 1] != i1[s23, 1])[moved[s23]]).mean() > 0.4
    gk = kind == "gate"
    assert not g0[gk].any() and g1[gk & moved].all()


def room_scene(spacing=0.25, size=8.0):
    """Three orthogonal walls (x = 10, y = 10, z = 2) sampled on a lattice; the scan is the same lattice seen from a lidar
    at (13, 13, 3.5) turned by a small rotation, so that at the true pose every query stands on a lattice point up to
    the fp32 rounding of the scan: equidistant lattice neighbours give near-ties below the sweep key's resolution
    almost everywhere, and some exact ties.  The loop starts 4 cm / 0.5 deg away."""
    v = np.arange(0.0, size + 1e-9, spacing)
    a, b = np.meshgrid(v, v, indexing="ij")
    a, b, z = a.ravel(), b.ravel(), np.zeros(a.size)
    walls = np.concatenate([np.stack([z, a, b], 1), np.stack([a, z, b], 1), np.stack([a, b, z], 1)])
    walls = np.unique(walls, axis=0) + np.array([10.0, 10.0, 2.0])      # (planes through the origin have no fit)
    pose_gt = np.array([0.004, -0.003, 0.012, 13.0, 13.0, 3.5])
    R = synth.rotation_rpy(*pose_gt[:3])
    pick = walls[np.random.default_rng(5).permutation(len(walls))[:2500]]
    scan = ((pick - pose_gt[3:]) @ R).astype(F)
    pose_init = (pose_gt + np.array([0.006, 0.004, -0.009, 0.04, -0.03, 0.02])).astype(F)
    return scene(walls, scan, 1.0, pose=pose_init, pose_gt=pose_gt.astype(F))


def test_room_scene_is_full_of_near_ties():
    sc = room_scene()
    T = O.getTransformation(sc["pose_gt"])
    s = sc["scan"]
    q = (((T[:, 0] * s[:, :1] + T[:, 1] * s[:, 1:2]) + T[:, 2] * s[:, 2:3]) + T[:, 3]).astype(F)
    _, d2, gated = ref_knn(sc["map"], q[::5], 1.0)
    assert gated.all()
    assert np.mean(ulps(d2[:, 4], d2[:, 3]) < 2 ** 9) > 0.8          # inside the six, below the key's resolution
    assert np.mean(ulps(d2[:, 5], d2[:, 4]) < 2 ** 9) > 0.05         # across the 5th / 6th boundary
    assert np.mean(ulps(d2[:, 5], d2[:, 4]) == 0) > 0.03             # exact ties among them
    orc = O.Oracle(knn_backend=0, num_threads=8)
    orc.set_map(sc["map"])
    orc.set_scan(s)
    r = orc.scan2MapOptimization(sc["pose"])
    assert r.iters_run < 30 and np.abs(np.array(r.pose)[3:] - sc["pose_gt"][3:]).max() < 5e-3
    orc.close()
