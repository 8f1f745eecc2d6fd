"""CPU companions of tests/test_icp_grid_gpu.py and tests/test_icp_device_loop_gpu.py.

* `numpy_keys`: the nearest-neighbour key of every source point restated in numpy - fp32 d2 = (dx*dx + dy*dy) + dz*dz, the
  minimum over all finite targets, equal distances to the lower index, (d2 bits << 32) | index, ~0 for no match - checked here
  against the oracle's correspondences through what they produce (the first transformation of oracle.icp_align).
* `grid_scenes`: the scenes the grid search is held to (ties across cells, equal points, non-finite points, degenerate grids,
  sources outside the box, sources on cell faces, far nearest neighbours, a dense cell, the sliver at 20 km, forced fallbacks).
* the close of an ICP iteration (liorf_amd/csrc/s2m_icp_close.hpp, the source the host loop and the device loop share) built
  stand-alone by the host compiler (tests/ref/icp_close_main.cpp) against oracle.icp_umeyama bit for bit, and a whole
  alignment driven by it against oracle.icp_align.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O
from test_icp_cpu import icp_scene
from test_icp_edges_cpu import tie_scene

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_MATCH = np.uint64(0xFFFFFFFFFFFFFFFF)
# the grid's cell edge in the debug calls: kIcpCellLeaves (s2m_icp.hpp) times the default icp_leaf, in fp32
CELL = F(2.0) * F(0.3)
DENSE_CELL = (12, 12, 3)                                  # the cell grid_scenes()['dense_cell'] fills


def numpy_keys(src, tgt, chunk=512):
    """keys[i] = (fp32 d2 bits << 32) | j of the finite target j nearest to source i (ties: the lowest j); ~0 where the source
    is not finite, no target is, or every distance overflows to inf (k_icp_nn's `d < best` never fires from best = inf)."""
    s = np.ascontiguousarray(src[:, :3], F)
    t = np.ascontiguousarray(tgt[:, :3], F)
    keys = np.full(s.shape[0], NO_MATCH, np.uint64)
    tfin = np.isfinite(t).all(1)
    sfin = np.isfinite(s).all(1)
    if not tfin.any():
        return keys
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, s.shape[0], chunk):
            p = s[a:a + chunk]
            dx = p[:, None, 0] - t[None, :, 0]
            dy = p[:, None, 1] - t[None, :, 1]
            dz = p[:, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz                    # float32 ufuncs: one rounding per operation, no contraction
            d2 = np.where(tfin[None, :], d2, F(np.inf))
            j = np.argmin(d2, 1)                                  # the first (lowest) index among equals
            m = d2[np.arange(p.shape[0]), j]
            ok = sfin[a:a + chunk] & np.isfinite(m)
            k = (m.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
            keys[a:a + chunk] = np.where(ok, k, NO_MATCH)
    return keys


def shifted(src, tgt, offset):
    """Both clouds moved by `offset` in float64 and rounded to fp32 there (as the key frames are in the map frame)."""
    if offset is None:
        return src, tgt
    o = np.asarray(offset, np.float64)
    a, b = src.copy(), tgt.copy()
    a[:, :3] = (src[:, :3].astype(np.float64) + o).astype(F)
    b[:, :3] = (tgt[:, :3].astype(np.float64) + o).astype(F)
    return a, b


def cell_index(x, lo, cell=CELL):
    """The grid's cell coordinate along one axis as the device computes it: floor((x - lo) * (1 / cell)) in fp32."""
    inv = F(1.0) / F(cell)
    return np.floor((np.asarray(x, F) - F(lo)) * inv)


def first_in_cell(k, lo, cell=CELL):
    """The least fp32 x whose cell index is >= k."""
    x = F(np.float64(lo) + np.float64(k) * np.float64(cell))
    while cell_index(x, lo, cell) >= k:
        x = np.nextafter(x, F(-np.inf))
    while cell_index(x, lo, cell) < k:
        x = np.nextafter(x, F(np.inf))
    return x


def _cloud(xyz):
    return synth.to_xyzi(np.asarray(xyz, F).reshape(-1, 3))


def _box_targets(rng, n=1500, half=6.0):
    """A structured target: points on three planes of a 12 m box, 0.25 m apart with 1 cm of noise."""
    u = rng.uniform(-half, half, (n, 2))
    k = rng.integers(0, 3, n)
    p = np.zeros((n, 3))
    p[k == 0] = np.c_[u[k == 0], np.full((k == 0).sum(), -1.0)]
    p[k == 1] = np.c_[u[k == 1, 0], np.full((k == 1).sum(), half), u[k == 1, 1] * 0.3]
    p[k == 2] = np.c_[np.full((k == 2).sum(), -half), u[k == 2, 0], u[k == 2, 1] * 0.3]
    return (p + rng.normal(0, 0.01, p.shape)).astype(F)


def sliver_scene():
    """20 km out, where fp32 coordinates are 1.95 mm apart. The query sits in cell 5 along x, one step below the face to cell 6.
    Target B lies two steps beyond the face to cell 7 - outside the 3 x 3 x 3 cells around the query - at distance gap + 3 steps.
    Target A, inside those cells, is 2 steps farther than B. B is the answer; a bound on the unvisited cells that is even two
    steps too generous stops at A."""
    lo = np.array([20000.0, 8000.0, -50.0], F)
    ulp = np.spacing(lo[0])
    xq = np.nextafter(first_in_cell(6, lo[0]), F(-np.inf))
    yq = F(lo[1] + F(5.5) * CELL)
    zq = F(lo[2] + F(5.5) * CELL)
    xb = F(first_in_cell(7, lo[0]) + 2 * ulp)
    d_b = np.float64(xb) - np.float64(xq)
    ya = F(np.float64(yq) - (d_b + 2 * np.spacing(lo[1])))
    tgt = np.array([lo, lo + F(12 * CELL), [xq, ya, zq], [xb, yq, zq]], F)
    src = np.array([[xq, yq, zq]], F)
    assert cell_index(xq, lo[0]) == 5 and cell_index(xb, lo[0]) == 7 and abs(cell_index(ya, lo[1]) - 5) <= 1
    return _cloud(src), _cloud(tgt)


def grid_scenes():
    """name -> (src, tgt, fallback) with fallback 'zero' (every source is settled by the grid), 'some' (the scene forces the
    brute-force fallback) or None (not stated)."""
    rng = np.random.default_rng(12)
    out = {}
    base = _box_targets(rng)
    near = (base[rng.integers(0, base.shape[0], 300)] + rng.normal(0, 0.05, (300, 3))).astype(F)
    out["box"] = (_cloud(near), _cloud(base), "zero")
    # exact ties between distinct targets in different cells (1 m lattice, cells of 0.6 m), lower index = the x = 2k+1 point
    s, t = tie_scene(n_src=257)
    out["ties_across_cells"] = (s, t, "zero")
    # equal points in one cell: five copies of each of 40 points, scattered through the target; the lowest copy wins
    pts = rng.uniform(-3, 3, (40, 3)).astype(F)
    dup = np.concatenate([pts[rng.permutation(40)] for _ in range(5)], 0)
    out["equal_points"] = (_cloud(pts + F(0.01)), _cloud(dup), "zero")
    # non-finite targets never win and never stretch the grid; non-finite sources give ~0
    t = base.copy()
    for k, j in enumerate(range(0, t.shape[0], 7)):
        t[j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    t[1] = (np.inf, 1e6, -1e6)
    t[3] = (1e7, np.nan, 0)
    s = near.copy()
    s[5, 0] = np.nan; s[9, 2] = np.inf; s[11] = (-np.inf, np.nan, 0)
    out["non_finite"] = (_cloud(s), _cloud(t), "zero")
    out["no_finite_target"] = (_cloud(near[:70]), _cloud(np.full((5, 3), np.nan, F)), "zero")
    # degenerate grids: every target in one cell; every target on a line (one cell thick in y and z)
    out["one_cell"] = (_cloud(rng.uniform(-0.5, 0.5, (130, 3))), _cloud(F(0.1) + rng.uniform(0, 0.1, (90, 3)).astype(F)), "zero")
    line = np.c_[np.arange(500) * 0.05, np.full(500, 2.0), np.full(500, -1.0)].astype(F)
    out["line"] = (_cloud(line[rng.integers(0, 500, 200)] + rng.normal(0, 0.1, (200, 3)).astype(F)), _cloud(line), "zero")
    # sources outside the target box: 1 m (the clamped cell), 100 m and 10 km (the fallback)
    lo, hi = base.min(0), base.max(0)
    mid = (lo + hi) / 2
    # (1 m outside a hollow box the nearest target can be more than the shell cap away: its fallback count is not stated)
    for name, d, fb in (("outside_1m", 1.0, None), ("outside_100m", 100.0, "some"), ("outside_10km", 10000.0, "some")):
        o = []
        for a in range(3):
            for sgn in (-1, 1):
                p = mid + rng.uniform(-2, 2, 3)
                p[a] = (hi[a] + d) if sgn > 0 else (lo[a] - d)
                o.append(p)
        o.append(hi + d); o.append(lo - d)
        out[name] = (_cloud(np.array(o)), _cloud(base), fb)
    # a source exactly on a cell face, on an edge and on a corner of the grid's cells (fp32 faces as the device computes them):
    # target points with one, two and three coordinates moved onto the lower faces of their own cell, so that each source stays
    # within a cell diagonal of its target and the grid settles it
    faces = []
    for j in (3, 500, 1200):
        b = base[j]
        fx, fy, fz = (first_in_cell(cell_index(b[a], lo[a]), lo[a]) for a in range(3))
        faces += [[fx, b[1], b[2]], [b[0], fy, b[2]], [fx, fy, b[2]], [fx, fy, fz],
                  [np.nextafter(fx, F(-np.inf)), fy, np.nextafter(fz, F(-np.inf))]]
    out["on_faces"] = (_cloud(faces), _cloud(base), "zero")
    # a source inside the box whose nearest target is 40 m away (beyond max_correspondence_distance, beyond any shell cap)
    two = np.concatenate([rng.uniform(-2, 2, (600, 3)), rng.uniform(-2, 2, (600, 3)) + [100.0, 0, 0]]).astype(F)
    out["nearest_40m"] = (_cloud([[42.0, 0, 0], [58.0, 0.5, 0], [1.0, 1.0, 1.0]]), _cloud(two), "some")
    # more points in one cell than a wave has lanes: 300 targets in a 0.2 m cube that starts 0.2 m inside cell (12, 12, 3) of the
    # box's grid (tests below count them), queried from inside the cube, from the cells around it and from elsewhere
    corner = np.array([first_in_cell(k, lo[a]) for a, k in enumerate(DENSE_CELL)], F) + F(0.2)
    cube = (corner + rng.uniform(0, 0.2, (300, 3))).astype(F)
    dense = np.concatenate([base[:700], cube, base[700:]])
    around = (corner + rng.uniform(-0.9, 1.1, (120, 3))).astype(F)
    out["dense_cell"] = (_cloud(np.concatenate([near[:64], cube[:40] + F(0.003), around])), _cloud(dense), "zero")
    out["sliver_20km"] = sliver_scene() + ("zero",)
    return out


# ---- the restatement against the oracle ---------------------------------------------------------------------------------

def _first_transform(src, tgt, keys, max_corr_dist):
    """Umeyama of the correspondences `keys` names, sums in float64 (the device's), through the oracle's icp_umeyama."""
    ok = keys != NO_MATCH
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(F).astype(np.float64)
    ok &= d2 <= max_corr_dist * max_corr_dist
    j = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    s = src[ok, :3].astype(np.float64)
    t = tgt[j[ok], :3].astype(np.float64)
    ms, mt = s.mean(0), t.mean(0)
    sigma = (t - mt).T @ (s - ms) / s.shape[0]
    return O.icp_umeyama(ms.astype(F), mt.astype(F), sigma.astype(F)), int(ok.sum())


def test_numpy_keys_are_the_oracles_correspondences():
    src, tgt, _ = icp_scene(3000, 800, 7)
    keys = numpy_keys(src, tgt)
    T, n = _first_transform(src, tgt, keys, 30.0)
    To, conv, _, its = O.icp_align(src, tgt, max_corr_dist=30.0, max_iter=1)
    assert its == 1 and n == 800 and np.abs(T - To).max() <= 1e-5
    # one wrong correspondence is visible at this bar: send source 0 to the target farthest from it
    bad = keys.copy()
    far = int(np.argmax(((tgt[:, :3] - src[0, :3]) ** 2).sum(1)))
    d = F(((tgt[far, :3] - src[0, :3]) ** 2).sum())
    bad[0] = (np.uint64(d.view(np.uint32)) << np.uint64(32)) | np.uint64(far)
    Tb, _ = _first_transform(src, tgt, bad, 1e3)
    assert np.abs(Tb - To).max() > 1e-4


def test_numpy_keys_send_ties_to_the_lower_index():
    src, tgt = tie_scene()
    keys = numpy_keys(src, tgt)
    assert np.all((keys >> np.uint64(32)).astype(np.uint32).view(F) == F(0.25))
    j = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.all(tgt[j, 0] == src[:, 0] + F(0.5))               # the x = 2k + 1 partner, the lower index of each pair
    T, _ = _first_transform(src, tgt, keys, 30.0)
    To, _, _, _ = O.icp_align(src, tgt, max_corr_dist=30.0, max_iter=1)
    assert np.abs(T - To).max() <= 1e-5 and abs(T[0, 3] - 0.5) < 1e-5


def test_numpy_keys_on_non_finite_points():
    src, tgt, _ = grid_scenes()["non_finite"]
    keys = numpy_keys(src, tgt)
    bad_src = ~np.isfinite(src[:, :3]).all(1)
    assert bad_src.sum() == 3 and np.all(keys[bad_src] == NO_MATCH) and np.all(keys[~bad_src] != NO_MATCH)
    j = (keys[~bad_src] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.isfinite(tgt[j, :3]).all()
    assert np.all(numpy_keys(*grid_scenes()["no_finite_target"][:2]) == NO_MATCH)


def test_sliver_scene_is_what_it_says():
    src, tgt = sliver_scene()
    keys = numpy_keys(src, tgt)
    assert int(keys[0] & np.uint64(0xFFFFFFFF)) == 3              # B, two cells away along x
    d = np.sqrt(((tgt[:, :3].astype(np.float64) - src[0, :3].astype(np.float64)) ** 2).sum(1))
    assert 0 < d[2] - d[3] < 3 * np.spacing(F(20000.0))           # A is at most three coordinate steps farther


def test_dense_cell_scene_is_what_it_says():
    """One cell of a many-cell grid holds more targets than a wave has lanes, and sources lie in it and in the cells around it."""
    src, tgt, _ = grid_scenes()["dense_cell"]
    lo = tgt[:, :3].min(0)
    ct = np.stack([cell_index(tgt[:, a], lo[a]) for a in range(3)], 1).astype(int)
    cells, counts = np.unique(ct, axis=0, return_counts=True)
    full = cells[np.argmax(counts)]
    assert counts.max() >= 300 and tuple(full) == DENSE_CELL and len(cells) > 300 and np.sort(counts)[-2] < 64
    cs = np.stack([cell_index(src[:, a], lo[a]) for a in range(3)], 1).astype(int)
    cheb = np.abs(cs - full).max(1)
    assert (cheb == 0).sum() >= 40 and (cheb == 1).sum() >= 20 and (cheb >= 2).sum() >= 20


def test_scene_fallback_labels_cover_both_paths():
    labels = [v[2] for v in grid_scenes().values()]
    assert "zero" in labels and "some" in labels


# ---- the shared close of an iteration, built by the host compiler ---------------------------------------------------------

@pytest.fixture(scope="module")
def close_exe():
    d = tempfile.mkdtemp(prefix="icp_close_")
    exe = os.path.join(d, "icp_close_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "liorf_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ref", "icp_close_main.cpp")])
    yield exe
    for f in os.listdir(d):
        os.unlink(os.path.join(d, f))
    os.rmdir(d)


def _umeyama_cases():
    rng = np.random.default_rng(3)
    cases = []
    for k in range(40):
        A = rng.normal(0, 1, (3, 3)) * 10.0 ** rng.integers(-3, 3)
        cases.append(A)
    u, v = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    cases += [np.outer(u, v), np.zeros((3, 3)), np.outer(u, v) + np.outer(v, u) * 0.5,         # rank 1, 0, 2
              np.diag([1.0, 1.0, 0.0]), np.diag([2.0, 0.0, 0.0]), -np.eye(3), np.eye(3) * 1e-30,
              np.diag([1.0, 1.0, -1.0]), np.diag([3.0, 2.0, -1e-20])]
    out = []
    for A in cases:
        out.append((rng.normal(0, 5, 3).astype(F), rng.normal(0, 5, 3).astype(F), A.astype(F)))
    return out


def test_shared_umeyama_has_the_oracles_bits(close_exe):
    cases = _umeyama_cases()
    text = "\n".join(" ".join(float(x).hex() for x in np.concatenate([ms, mt, sg.reshape(-1)])) for ms, mt, sg in cases)
    got = subprocess.run([close_exe, "umeyama"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [line for line in got if line]
    assert len(got) == len(cases)
    for (ms, mt, sg), line in zip(cases, got):
        T = np.array([int(w, 16) for w in line.split()], np.uint32)
        To = O.icp_umeyama(ms, mt, sg).reshape(-1).view(np.uint32)
        assert np.array_equal(T, To), (sg, T.view(F), To.view(F))


@pytest.mark.parametrize("max_iter,max_corr", [(100, 30.0), (1, 30.0), (3, 30.0), (100, 0.5)])
def test_shared_close_drives_an_alignment_like_the_oracle(close_exe, tmp_path, max_iter, max_corr):
    """A brute-force ICP whose every iteration is closed by icp_close_step (the state machine the device runs): iterations and
    `converged` equal to the oracle's, T within 1e-5 (the bars of tests/test_icp_gpu.py: fp64 sums here, fp32 in the oracle)."""
    src, tgt, _ = icp_scene(1500, 400, 2)
    src[:, :3].astype(F).tofile(tmp_path / "src.bin")
    tgt[:, :3].astype(F).tofile(tmp_path / "tgt.bin")
    out = subprocess.run([close_exe, "align", str(tmp_path / "src.bin"), str(src.shape[0]), str(tmp_path / "tgt.bin"), str(tgt.shape[0]),
                          repr(max_corr), str(max_iter)], capture_output=True, text=True, check=True).stdout.split()
    conv, its = int(out[0]), int(out[1])
    T = np.array([int(w, 16) for w in out[2:18]], np.uint32).view(F).reshape(4, 4)
    To, convo, _, itso = O.icp_align(src, tgt, max_corr_dist=max_corr, max_iter=max_iter)
    assert (conv, its) == (int(convo), itso) and np.abs(T - To).max() <= 1e-5


def test_too_few_correspondences_end_the_shared_state_machine(close_exe, tmp_path):
    src, tgt, _ = icp_scene(1500, 400, 2)
    far = src.copy(); far[:, 0] += 500.0
    far[:, :3].astype(F).tofile(tmp_path / "src.bin")
    tgt[:, :3].astype(F).tofile(tmp_path / "tgt.bin")
    out = subprocess.run([close_exe, "align", str(tmp_path / "src.bin"), "400", str(tmp_path / "tgt.bin"), "1500", "1.0", "100"],
                         capture_output=True, text=True, check=True).stdout.split()
    T = np.array([int(w, 16) for w in out[2:18]], np.uint32).view(F).reshape(4, 4)
    assert (int(out[0]), int(out[1])) == (0, 0) and np.array_equal(T, np.eye(4, dtype=F))


# ---- the boundary -----------------------------------------------------------------------------------------------------

NEW = ["s2m_loop_align_launch", "s2m_loop_closure_rs_launch", "s2m_loop_poll", "s2m_loop_collect", "s2m_debug_icp_nearest",
       "s2m_debug_icp_time_nearest", "s2m_debug_icp_align_device", "s2m_debug_icp_tuning", "s2m_debug_icp_grid",
       "s2m_debug_icp_grid_check_args"]


def test_new_symbols_and_constants_declared_bound_and_exported():
    import ctypes as C
    lib = C.CDLL(s2m.LIB_PATH)
    main = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    dbg = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    for n in NEW:
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n)
        assert (n in dbg) if n.startswith("s2m_debug_") else (n in main)
    assert int(re.search(r"#define S2M_ERR_BUSY\s+(-?\d+)", main).group(1)) == s2m.S2M_ERR_BUSY == -6
    assert int(re.search(r"#define S2M_LOOP_PENDING\s+(\d+)", main).group(1)) == s2m.S2M_LOOP_PENDING == 5
    assert int(re.search(r"#define S2M_ICP_RANGE\s+(\d+)", dbg).group(1)) == s2m.S2M_ICP_RANGE
    assert s2m.ERRORS[s2m.S2M_ERR_BUSY] == "S2M_ERR_BUSY"


def test_null_handle_calls_are_rejected():
    import ctypes as C
    lib = s2m.load_library()
    r = s2m.LoopResult()
    assert lib.s2m_loop_align_launch(None, 0, 0, -1, None, C.byref(r)) == -1
    assert lib.s2m_loop_closure_rs_launch(None, 0.0, None, C.byref(r)) == -1
    assert lib.s2m_loop_poll(None, C.byref(r)) == -1 and lib.s2m_loop_collect(None, C.byref(r)) == -1
    assert lib.s2m_debug_icp_tuning(None, 0.0, 0, -1) == -1
    assert lib.s2m_debug_icp_align_device(None, None, 0, None, 0, 32, None, None) == -1
