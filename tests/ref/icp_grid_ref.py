"""A numpy statement of the uniform grid the ICP device loop builds over a target (liorf_amd/csrc/s2m_icp.hip: k_icp_grid_bbox,
k_icp_grid_setup, cell_of, k_icp_grid_count / _scan / _scatter), and the scenes that hold it at the extents of real loop-closure
submaps, where the box needs more than kGridMaxCells cells at the edge asked for and the grid grows.

* `grid_shape`: the box of the finite targets and the growth loop of k_icp_grid_setup, operation by operation in float32 (the
  product of the counts in float64), with the list of tries.
* `cell_table`: every finite target's clamped cell, the cell counts, their exclusive sums and the targets ordered by cell.
* `big_scenes`: name -> (src, tgt, what is stated).
"""
import functools

import numpy as np

from test_icp_grid_cpu import CELL, _box_targets, _cloud, first_in_cell

F = np.float32
GRID_MAX_CELLS = 1 << 18                                   # kGridMaxCells
GRID_MAX_TRIES = 96
SHELL_CAP = 3                                              # kIcpShellCap


def grid_shape(tgt, cell_req):
    """dict(lo, hi, cell, inv, n, n_fin, usable, tries): the shape k_icp_grid_setup gives the box of the finite targets. tries:
    one (cell, inv, n as float32, prod as float64) per pass of the loop. Without a finite target lo is None and n_fin 0; without a
    grid (usable 0) the targets are not counted and n_fin is 1."""
    t = np.ascontiguousarray(tgt[:, :3], F)
    fin = np.isfinite(t).all(1)
    out = dict(lo=None, hi=None, cell=F(0), inv=F(0), n=(0, 0, 0), n_fin=0, usable=0, tries=[])
    if not fin.any():
        return out
    lo, hi = t[fin].min(0), t[fin].max(0)
    out.update(lo=lo, hi=hi, n_fin=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ext = hi - lo                                                     # fp32, as cell_coord subtracts
        ok = bool(np.isfinite(ext).all())
        cell = F(cell_req)
        for _ in range(GRID_MAX_TRIES):
            if not ok:
                break
            inv = F(1.0) / cell
            fn = np.floor(ext * inv) + F(1.0)
            prod = np.float64(fn[0]) * np.float64(fn[1]) * np.float64(fn[2])
            out["tries"].append((cell, inv, fn, prod))
            if np.isfinite(inv) and inv > 0 and prod <= np.float64(GRID_MAX_CELLS):
                out.update(cell=cell, inv=inv, n=tuple(int(v) for v in fn), usable=1, n_fin=int(fin.sum()))
                break
            if not np.isfinite(cell) or prod != prod:
                break
            cell = F(cell * max(F(1.1), F(np.cbrt(F(prod / np.float64(GRID_MAX_CELLS))) * F(1.02))))
    return out


def shape_counts(lo, hi, cell):
    """n = floor((hi - lo) * fl(1 / cell)) + 1 per axis in float32: the counts k_icp_grid_setup derives from an edge."""
    inv = F(1.0) / F(cell)
    return tuple(int(v) for v in np.floor((np.asarray(hi, F) - np.asarray(lo, F)) * inv) + F(1.0))


def cell_table(tgt, lo, inv, n):
    """(cell, counts, starts, order): the flat clamped cell of every target as cell_of computes it (-1 for a non-finite target),
    the targets per cell, their exclusive cumulative sum, and the finite targets' original indices ordered by (cell, index), so
    that order[starts[c] : starts[c] + counts[c]] is the set of cell c."""
    t = np.ascontiguousarray(tgt[:, :3], F)
    fin = np.isfinite(t).all(1)
    lo, inv = np.asarray(lo, F), F(inv)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((t - lo) * inv)
    c = np.where(fin[:, None], c, 0).astype(np.int64)
    for a in range(3):
        c[:, a] = np.clip(c[:, a], 0, n[a] - 1)
    flat = (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]
    flat[~fin] = -1
    ncells = n[0] * n[1] * n[2]
    counts = np.bincount(flat[fin], minlength=ncells).astype(np.int64)
    starts = np.cumsum(counts) - counts
    idx = np.flatnonzero(fin)
    order = idx[np.argsort(flat[fin], kind="stable")]
    return flat, counts, starts, order


def sorted_within_cells(order, counts):
    """A device `order` array with the entries of every cell put in ascending order: comparable with cell_table's."""
    cell_of_pos = np.repeat(np.arange(counts.shape[0]), counts)
    return np.asarray(order)[np.lexsort((order, cell_of_pos))]


def face_points(lo, cell, k):
    """sliver_scene's three points on a grid of origin `lo` and edge `cell`, the query in cell k = (kx, ky, kz): the query one
    fp32 step below the face to cell kx + 1, B two steps beyond the face to cell kx + 2 (outside the 27 cells around the query),
    A inside them at the query's x and z, two steps farther from the query than B. Returns (query, A, B) as float32 triples."""
    lo = np.asarray(lo, F)
    kx, ky, kz = k
    xq = np.nextafter(first_in_cell(kx + 1, lo[0], cell), F(-np.inf))
    yq = F(np.float64(lo[1]) + (ky + 0.5) * np.float64(cell))
    zq = F(np.float64(lo[2]) + (kz + 0.5) * np.float64(cell))
    xf = first_in_cell(kx + 2, lo[0], cell)
    xb = np.nextafter(np.nextafter(xf, F(np.inf)), F(np.inf))
    d_b = np.float64(xb) - np.float64(xq)
    ya = F(np.float64(yq) - d_b)                                          # then to the second fp32 y that is farther than B
    while np.float64(yq) - np.float64(ya) <= d_b:
        ya = np.nextafter(ya, F(-np.inf))
    while np.float64(yq) - np.float64(np.nextafter(ya, F(np.inf))) > d_b:
        ya = np.nextafter(ya, F(np.inf))
    ya = np.nextafter(ya, F(-np.inf))
    return np.array([xq, yq, zq], F), np.array([xq, ya, zq], F), np.array([xb, yq, zq], F)


def sharpest_face_cell(lo, cell, n, z):
    """The cell (kx, ky, kz) for face_points where a stopping rule without slack on the faces is most too generous: kx such that
    the fp32 face to cell kx + 2 lies farthest below the exact one, ky the cell whose centre is nearest to y = 0 (A's steps are
    finest there), kz the cell of height z. Returns (k, fp32 steps the face lies below the exact one)."""
    from test_icp_grid_cpu import cell_index
    below = [steps_below_exact_face(lo[0], cell, k + 2) for k in range(20, n[0] - 20)]
    yc = np.float64(lo[1]) + (np.arange(10, n[1] - 10) + 0.5) * np.float64(cell)
    k = (20 + int(np.argmax(below)), 10 + int(np.argmin(np.abs(yc))), int(cell_index(F(z), lo[2], cell)))
    return k, float(max(below))


def steps_below_exact_face(lo, cell, k):
    """How many fp32 steps the first x of cell k lies below the face lo + k * cell taken in float64 (negative: above it)."""
    x = first_in_cell(k, lo, cell)
    return (np.float64(lo) + k * np.float64(cell) - np.float64(x)) / abs(np.float64(np.spacing(x)))


# ---- the scenes -------------------------------------------------------------------------------------------------------------

STREET_LO, STREET_HI = (-105.0, -80.0, -2.0), (105.0, 80.0, 28.0)      # 210 x 160 x 30 m
AIR_Z = (18.0, 24.0)                                                    # no target between the facade tops (12 m) and the corner


def _street(rng, n_tgt, n_near=1400, n_air=100):
    """Two corner points fixing the box, a ground plane and two facades (y = -12 and y = 12, 12 m high); sources beside targets
    and in the empty air."""
    n_face = n_tgt // 5
    n_ground = n_tgt - 2 - 2 * n_face
    ground = np.c_[rng.uniform(-100, 100, n_ground), rng.uniform(-75, 75, n_ground), rng.normal(0, 0.03, n_ground)]
    fac = [np.c_[rng.uniform(-100, 100, n_face), np.full(n_face, y) + rng.normal(0, 0.03, n_face), rng.uniform(0, 12, n_face)]
           for y in (-12.0, 12.0)]
    body = np.concatenate([ground] + fac)[rng.permutation(n_tgt - 2)]
    tgt = np.concatenate([[STREET_LO], body[:n_tgt // 2], [STREET_HI], body[n_tgt // 2:]]).astype(F)
    near = tgt[rng.integers(0, n_tgt, n_near)] + rng.normal(0, 0.05, (n_near, 3)).astype(F)
    air = np.c_[rng.uniform(-90, 90, n_air), rng.uniform(-70, 70, n_air), rng.uniform(*AIR_Z, n_air)].astype(F)
    src = np.concatenate([near[:n_near // 2], air, near[n_near // 2:]]).astype(F)
    return _cloud(src), _cloud(tgt)


def _near(rng, tgt, n, sigma=0.05):
    return (tgt[rng.integers(0, tgt.shape[0], n)] + rng.normal(0, sigma, (n, 3))).astype(F)


def last_in_cell(k, lo, cell=CELL):
    return np.nextafter(first_in_cell(k + 1, lo, cell), F(-np.inf))


@functools.lru_cache(maxsize=None)
def big_scenes():
    """name -> (src, tgt, stated) with stated = dict(grows=, usable=, fallback=): whether the edge asked for (CELL) has to grow
    (None: no grid), whether a grid is built (None: not stated) and the fallback count ('zero', 'some', 'all' = every finite
    source, None = not stated). The arrays are shared: do not write to them."""
    rng = np.random.default_rng(2024)
    out = {}
    out["street"] = _street(rng, 20000) + (dict(grows=True, usable=1, fallback="some"),)
    out["street_60k"] = _street(rng, 60000) + (dict(grows=True, usable=1, fallback="some"),)
    # a corridor: floor, two walls and the two corner points; its grid keeps nearly all of the kGridMaxCells cells
    n = 8000 - 2
    k = rng.integers(0, 3, n)
    x, u = rng.uniform(0, 2000, n), rng.uniform(0, 1, n)
    p = np.where((k == 0)[:, None], np.c_[x, u * 10 - 5, np.zeros(n)],
                 np.where((k == 1)[:, None], np.c_[x, np.full(n, -5.0), u * 5], np.c_[x, np.full(n, 5.0), u * 5]))
    p = np.clip(p + rng.normal(0, 0.01, p.shape), [0, -5, 0], [2000, 5, 5])
    tgt = np.concatenate([[[0.0, -5.0, 0.0]], p, [[2000.0, 5.0, 5.0]]]).astype(F)
    out["corridor"] = (_cloud(_near(rng, tgt, 500)), _cloud(tgt), dict(grows=True, usable=1, fallback="zero"))
    # the 12 m box with one finite target 50 km away in x and one 3 km below: the whole box in one or two cells
    base = _box_targets(rng)
    near = _near(rng, base, 300)
    tgt = np.concatenate([base[:700], [[50000.0, 0.0, 0.0]], base[700:], [[0.0, 0.0, -3000.0]]]).astype(F)
    out["outlier"] = (_cloud(near), _cloud(tgt), dict(grows=True, usable=1, fallback=None))
    # 64 x 64 x 64 = kGridMaxCells at the edge asked for: the upper corner is the last fp32 of cell 63 on every axis; one step
    # more along x and the box needs 65 x 64 x 64
    lo = np.array([-19.0, -18.5, -20.25], F)
    hi = np.array([last_in_cell(63, lo[a]) for a in range(3)], F)
    inner = (lo + F(0.5) + rng.uniform(0, 1, (1000, 3)) * (hi - lo - F(1.0))).astype(F)
    for name, top, grows in (("fits_exactly", hi, False), ("one_over", np.array([first_in_cell(64, lo[0]), hi[1], hi[2]], F), True)):
        tgt = np.concatenate([[lo], inner, [top]]).astype(F)
        out[name] = (_cloud(_near(rng, inner, 300, 0.02)), _cloud(tgt), dict(grows=grows, usable=1, fallback="zero" if not grows else None))
    # an extent that overflows fp32: no grid, every finite source goes to the brute force (two sources are not finite)
    tgt = np.concatenate([[[3e38, 0.0, 0.0]], base, [[-3e38, 1.0, 0.0]]]).astype(F)
    s = near.copy()
    s[7, 1] = np.nan
    s[200] = (np.inf, 0.0, 0.0)
    out["overflow"] = (_cloud(s), _cloud(tgt), dict(grows=None, usable=0, fallback="all"))
    tgt = np.concatenate([base, [[1e20, 1e20, 1e20]]]).astype(F)
    out["huge_cube"] = (_cloud(near), _cloud(tgt), dict(grows=None, usable=None, fallback=None))
    for s, t, _ in out.values():
        s.setflags(write=False)
        t.setflags(write=False)
    return out


# ---- the second trip of the sums --------------------------------------------------------------------------------------------

SUM_THREADS = 256 * 256                                    # kSumBlocks workgroups of 256 lanes: sources beyond take a second trip


def reach_scene_big(n_within, n_far=SUM_THREADS):
    """reach_scene with n_far sources out of reach first and the n_within (2 or 3) sources within max_correspondence_distance
    = 0.75 m last, the last of them at exactly 0.75 m; 300 targets, the 294 added ones far from every source."""
    tgt6 = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10], [50, 50, 50], [-50, 20, 5]], F)
    near = np.array([[0.5, 0, 0], [10, 0.25, 0], [0.75, 10, 0]], F)[3 - n_within:]
    rng = np.random.default_rng(100 + n_within)
    extra = rng.uniform([200, 200, 200], [300, 300, 300], (294, 3)).astype(F)
    far = rng.uniform([20, 20, -5], [40, 40, 5], (n_far, 3)).astype(F)
    return _cloud(np.concatenate([far, near])), _cloud(np.concatenate([tgt6[:3], extra[:150], tgt6[3:], extra[150:]]))


def fitness_scene(n_src=SUM_THREADS + 1):
    """300 targets on a 3 m lattice; every source 0.1 m from a target of its own, the last one 1 m (ten times farther): its squared
    distance is 100 times the others', so a mean that drops it is lower by about 1.5e-3 of its value."""
    rng = np.random.default_rng(77)
    g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), -1).reshape(-1, 3)[:300]
    tgt = ((g - 3.0) * 3.0).astype(F)
    d = rng.normal(0, 1, (n_src, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.full(n_src, 0.1)
    r[-1] = 1.0
    src = (tgt[rng.integers(0, 300, n_src)] + d * r[:, None]).astype(F)
    return _cloud(src), _cloud(tgt)


def fitness_in_blocks(src, tgt, T, block=8192):
    """numpy_fitness (tests/test_icp_edges_cpu.py) of a large finite source, 8 192 points at a time."""
    from test_icp_edges_cpu import numpy_fitness
    assert np.isfinite(src[:, :3]).all()
    tot = 0.0
    for a in range(0, src.shape[0], block):
        part = src[a:a + block]
        tot += numpy_fitness(part, tgt, T) * part.shape[0]
    return tot / src.shape[0]
