"""CPU companions of tests/test_icp_big_grid_gpu.py: the scenes of tests/ref/icp_grid_ref.py are what they say, by the numpy
model of the grid alone - which of them make k_icp_grid_setup enlarge the cell edge, by how many tries and to how many cells,
that the cell counts do not depend on the last bits of a grown edge (the device's edge passes through its own cbrtf), which
sources the grid can settle - and the argument checks of s2m_debug_icp_grid."""
import os
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))

import icp_grid_ref as R  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402
from test_icp_edges_cpu import MAP_OFFSETS, numpy_fitness  # noqa: E402
from test_icp_grid_cpu import CELL, NO_MATCH, cell_index, first_in_cell, numpy_keys, shifted  # noqa: E402

F = np.float32
OFFSETS = [None] + MAP_OFFSETS
SCENES = R.big_scenes()
EDGE_BAR = 1e-5                 # the device's grown edge against the model's, relative (tests/test_icp_big_grid_gpu.py)
# tries of k_icp_grid_setup at the origin, the first included
TRIES = {"street": 2, "street_60k": 2, "corridor": 2, "outlier": 4, "fits_exactly": 1, "one_over": 2, "overflow": 0, "huge_cube": 2}


def _floats_around(x, rel):
    """every float32 within rel (relative) of x"""
    x = F(x)
    k = int(np.ceil(abs(float(x)) * rel / float(np.spacing(x)))) + 1
    return (x.view(np.uint32).astype(np.int64) + np.arange(-k, k + 1)).astype(np.uint32).view(F)


def test_scene_sizes():
    want = {"street": (1500, 20000), "street_60k": (1500, 60000), "corridor": (500, 8000), "outlier": (300, 1502),
            "fits_exactly": (300, 1002), "one_over": (300, 1002), "overflow": (300, 1502), "huge_cube": (300, 1501)}
    assert {k: (v[0].shape[0], v[1].shape[0]) for k, v in SCENES.items()} == want
    lo, hi = SCENES["street"][1][:, :3].min(0), SCENES["street"][1][:, :3].max(0)
    assert np.array_equal(hi - lo, F([210, 160, 30])) and np.array_equal(lo, SCENES["street_60k"][1][:, :3].min(0))
    t = SCENES["corridor"][1][:, :3]
    assert np.array_equal(t.max(0) - t.min(0), F([2000, 10, 5]))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_grow_as_stated(name):
    src, tgt, st = SCENES[name]
    g = R.grid_shape(tgt, CELL)
    prods = [t[3] for t in g["tries"]]
    print(name, "tries", len(g["tries"]), "cell", g["cell"], "n", g["n"], "products", prods)
    assert len(g["tries"]) == TRIES[name]
    if st["usable"] is not None:
        assert g["usable"] == st["usable"]
    if not g["usable"]:
        assert g["n_fin"] == 1 and g["n"] == (0, 0, 0)
        return
    assert np.prod(g["n"]) <= R.GRID_MAX_CELLS and g["n_fin"] == np.isfinite(tgt[:, :3]).all(1).sum()
    assert all(p > R.GRID_MAX_CELLS for p in prods[:-1]) and prods[-1] == np.prod(g["n"])
    if st["grows"]:
        assert len(g["tries"]) > 1 and g["cell"] > CELL
        cells = [t[0] for t in g["tries"]]
        assert all(b >= F(1.1) * a for a, b in zip(cells, cells[1:]))
    else:
        assert len(g["tries"]) == 1 and g["cell"] == CELL and g["cell"].view(np.uint32) == CELL.view(np.uint32)


def test_the_indicative_shapes():
    g = R.grid_shape(SCENES["street"][1], CELL)
    assert g["tries"][0][3] == 4779567 and g["n"] == (131, 100, 19) and abs(g["cell"] - 1.6108) < 1e-4
    assert R.grid_shape(SCENES["street_60k"][1], CELL)["n"] == g["n"]
    g = R.grid_shape(SCENES["corridor"][1], CELL)
    assert g["n"][1:] == (14, 7) and abs(g["cell"] - 0.764) < 1e-3 and np.prod(g["n"]) > 0.97 * R.GRID_MAX_CELLS   # nearly full cell arrays
    g = R.grid_shape(SCENES["outlier"][1], CELL)
    assert 20 < g["cell"] < 30
    flat, counts, _, _ = R.cell_table(SCENES["outlier"][1], g["lo"], g["inv"], g["n"])
    assert (counts > 0).sum() <= 4 and counts.max() >= 700                # the whole box in one or two cells, and the two outliers
    g = R.grid_shape(SCENES["one_over"][1], CELL)
    assert g["n"] == (59, 59, 59) and abs(g["cell"] - 0.66) < 1e-6


def test_fits_exactly_and_one_over_differ_by_one_step():
    a, b = SCENES["fits_exactly"][1][:, :3], SCENES["one_over"][1][:, :3]
    ga, gb = R.grid_shape(a, CELL), R.grid_shape(b, CELL)
    assert len(ga["tries"]) == 1 and ga["tries"][0][3] == R.GRID_MAX_CELLS == 64 ** 3 and ga["n"] == (64, 64, 64)
    assert len(gb["tries"]) > 1 and gb["tries"][0][3] == 65 * 64 * 64
    assert np.array_equal(ga["lo"], gb["lo"]) and np.array_equal(ga["hi"][1:], gb["hi"][1:])
    assert gb["hi"][0] == np.nextafter(ga["hi"][0], F(np.inf))
    assert cell_index(ga["hi"][0], ga["lo"][0]) == 63 and cell_index(gb["hi"][0], gb["lo"][0]) == 64


def test_overflow_has_no_grid_and_huge_cube_ends_on_an_infinite_edge():
    g = R.grid_shape(SCENES["overflow"][1], CELL)
    with np.errstate(over="ignore"):
        assert g["usable"] == 0 and g["tries"] == [] and not np.isfinite(g["hi"][0] - g["lo"][0])
    assert np.isfinite(g["hi"]).all() and np.isfinite(g["lo"]).all()      # finite targets, an extent that is not
    src = SCENES["overflow"][0]
    assert (~np.isfinite(src[:, :3]).all(1)).sum() == 2
    # 1e20 m: the first product of counts is finite in fp64, its quotient by 2^18 is not in fp32: the edge becomes inf and the loop ends
    g = R.grid_shape(SCENES["huge_cube"][1], CELL)
    assert g["usable"] == 0 and len(g["tries"]) == 2 and np.isfinite(g["tries"][0][3]) and np.isinf(g["tries"][1][0])


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_counts_do_not_depend_on_the_last_bits_of_a_grown_edge(name, offset):
    """The GPU test compares n with the model's although the device's edge differs from the model's in its last bits (its cbrtf
    is the device library's): every float32 edge within the bar of the model's gives the model's counts."""
    _, tgt = shifted(*SCENES[name][:2], offset)
    g = R.grid_shape(tgt, CELL)
    if not g["usable"] or len(g["tries"]) == 1:
        return
    around = _floats_around(g["cell"], EDGE_BAR)
    assert around.shape[0] > 160 and around[0] < g["cell"] * (1 - EDGE_BAR) and around[-1] > g["cell"] * (1 + EDGE_BAR)
    for c in around:
        assert R.shape_counts(g["lo"], g["hi"], c) == g["n"], (c, g["cell"])
    # and the same through every grown try before the last (the first is the edge asked for, bit for bit): an edge that differs
    # by the bar still fails where the model's fails
    for cell, _, fn, prod in g["tries"][1:-1]:
        for c in _floats_around(cell, EDGE_BAR)[::8]:
            assert np.prod(np.array(R.shape_counts(g["lo"], g["hi"], c), np.float64)) > R.GRID_MAX_CELLS


@pytest.mark.parametrize("leaves", [1.0, 3.0])
def test_street_at_other_edges_grows_to_robust_counts(leaves):
    """The tuned runs of the GPU test: 0.3 m and 0.9 m asked for, edges beyond 1.5 m given."""
    tgt = SCENES["street"][1]
    g = R.grid_shape(tgt, F(leaves) * F(0.3))
    assert g["usable"] and len(g["tries"]) > 1 and g["cell"] > 1.5 and g["cell"] not in (F(0.6), F(1.0))
    for c in _floats_around(g["cell"], EDGE_BAR):
        assert R.shape_counts(g["lo"], g["hi"], c) == g["n"], (c, g["cell"])
    for cell, _, fn, prod in g["tries"][1:-1]:
        for c in _floats_around(cell, EDGE_BAR)[::8]:
            assert np.prod(np.array(R.shape_counts(g["lo"], g["hi"], c), np.float64)) > R.GRID_MAX_CELLS


def test_street_has_settled_and_fallback_sources():
    src, tgt, _ = SCENES["street"]
    g = R.grid_shape(tgt, CELL)
    keys = numpy_keys(src, tgt)
    assert np.all(keys != NO_MATCH)
    d = np.sqrt((keys >> np.uint64(32)).astype(np.uint32).view(F).astype(np.float64))
    assert (d > R.SHELL_CAP * float(g["cell"])).sum() >= 1 and (d < float(g["cell"])).sum() >= 1000
    air = src[:, 2] > 15.0
    assert air.sum() == 100 and np.all(d[air] > R.SHELL_CAP * float(g["cell"])) and np.all(d[~air] < 1.0)
    # the air the face test builds its three points in holds no target
    assert not ((tgt[:, 2] > 13.0) & (tgt[:, 2] < 27.0)).any()


def test_cell_table_of_a_hand_made_cloud():
    """50 points on a 4 x 3 x 2 grid of 1 m cells from (10, 20, 30): point i in cell (i % 4, (i // 4) % 3, (i // 12) % 2), three
    of them moved outside the box (clamped to the border cells) and two not finite."""
    lo = np.array([10.0, 20.0, 30.0], F)
    n = (4, 3, 2)
    i = np.arange(50)
    c = np.stack([i % 4, (i // 4) % 3, (i // 12) % 2], 1)
    pts = (lo + c + F(0.25) + F(0.5) * ((i * 7) % 10 / 10.0)[:, None]).astype(F)
    pts[5, 0] = 9.0          # below the box in x: cell x 0 (was x = 1)
    pts[6, 1] = 99.0         # above in y: cell y 2 (was y = 1)
    pts[30, 2] = -4.0        # below in z: cell z 0 (was z = 0 already)
    pts[8, 0] = np.nan
    pts[49] = (np.inf, 0, 0)
    c[5, 0] = 0; c[6, 1] = 2; c[30, 2] = 0
    flat_want = (c[:, 2] * 3 + c[:, 1]) * 4 + c[:, 0]
    members = {}
    for j in range(50):
        if j not in (8, 49):
            members.setdefault(int(flat_want[j]), []).append(j)
    flat, counts, starts, order = R.cell_table(synth.to_xyzi(pts), lo, F(1.0), n)
    assert flat[8] == -1 and flat[49] == -1 and np.array_equal(np.delete(flat, [8, 49]), np.delete(flat_want, [8, 49]))
    assert counts.shape == (24,) and counts.sum() == 48 and order.shape == (48,)
    run = 0
    for cell in range(24):
        assert starts[cell] == run and counts[cell] == len(members.get(cell, []))
        assert list(order[run:run + counts[cell]]) == members.get(cell, [])
        run += counts[cell]
    # by hand: cell (0, 0, 0) holds 0, 24, 48; (1, 0, 0) holds 1, 25 (49 is not finite); point 5 joined 4 and 28 in (0, 1, 0) =
    # cell 4, point 6 joined 10 and 34 in (2, 2, 0) = cell 10, and their old cells (1, 1, 0) = 5 and (2, 1, 0) = 6 keep 29 and 30
    assert list(order[:3]) == [0, 24, 48] and list(order[3:5]) == [1, 25] and list(starts[:3]) == [0, 3, 5]
    assert list(order[starts[4]:starts[4] + counts[4]]) == [4, 5, 28] and list(order[starts[10]:starts[10] + counts[10]]) == [6, 10, 34]
    assert list(order[starts[5]:starts[5] + counts[5]]) == [29] and list(order[starts[6]:starts[6] + counts[6]]) == [30]
    # a device order with the cells' entries in any order compares after sorting within cells
    rng = np.random.default_rng(0)
    dev = order.copy()
    for cell in range(24):
        seg = dev[starts[cell]:starts[cell] + counts[cell]]
        dev[starts[cell]:starts[cell] + counts[cell]] = seg[rng.permutation(seg.shape[0])]
    assert np.array_equal(R.sorted_within_cells(dev, counts), order)


def test_face_points_at_a_grown_edge():
    """The three points of the face test on the model's street grid, at the origin and 20 km out: the query's nearest target is B,
    two cells away along x; A, inside the 27 cells around the query, is two coordinate steps farther."""
    for offset in (None, MAP_OFFSETS[1]):
        _, tgt = shifted(*SCENES["street"][:2], offset)
        g = R.grid_shape(tgt, CELL)
        k, below = R.sharpest_face_cell(g["lo"], g["cell"], g["n"], F(20.0) + (g["lo"][2] + F(2.0)))
        q, a, b = R.face_points(g["lo"], g["cell"], k)
        print("cell", k, "fp32 face below the exact one by", below, "steps; q", q, "A", a, "B", b)
        if offset is None:
            # a bound taken from the exact face, lo + (kx + 2) * cell, lies beyond A: only the slack on the face keeps B in play
            face = np.float64(g["lo"][0]) + (k[0] + 2) * np.float64(g["cell"])
            # (even after the 1e-6 that kBoundSlack takes off the squared bound)
            assert (face - np.float64(q[0])) * (1 - 1e-6) > np.float64(q[1]) - np.float64(a[1])
        cq = [int(cell_index(q[i], g["lo"][i], g["cell"])) for i in range(3)]
        ca = [int(cell_index(a[i], g["lo"][i], g["cell"])) for i in range(3)]
        cb = [int(cell_index(b[i], g["lo"][i], g["cell"])) for i in range(3)]
        assert tuple(cq) == k and cb == [k[0] + 2, k[1], k[2]] and ca == [k[0], k[1] - 1, k[2]]
        assert cell_index(np.nextafter(q[0], F(np.inf)), g["lo"][0], g["cell"]) == k[0] + 1       # one step below the face
        down = [b[0]]
        for _ in range(3):
            down.append(np.nextafter(down[-1], F(-np.inf)))
        assert [int(cell_index(x, g["lo"][0], g["cell"])) - k[0] for x in down] == [2, 2, 2, 1]   # two steps beyond the next face
        t2 = np.concatenate([tgt, synth.to_xyzi(np.array([a, b]))])
        key = numpy_keys(synth.to_xyzi(q[None]), t2)[0]
        assert int(key & np.uint64(0xFFFFFFFF)) == t2.shape[0] - 1
        d = np.sqrt(((np.array([a, b], np.float64) - q.astype(np.float64)) ** 2).sum(1))
        assert 0 < d[0] - d[1] <= 2 * np.spacing(np.abs(a[1]))             # A is two of its own coordinate steps farther, at most
        g2 = R.grid_shape(t2, CELL)
        assert np.array_equal(g2["lo"], g["lo"]) and g2["cell"] == g["cell"] and g2["n"] == g["n"]


def test_numpy_keys_of_the_largest_scene_is_quick():
    src, tgt, _ = SCENES["street_60k"]
    t0 = time.perf_counter()
    keys = numpy_keys(src, tgt)
    dt = time.perf_counter() - t0
    print(f"numpy_keys {src.shape[0]} x {tgt.shape[0]}: {dt:.2f} s")
    assert np.all(keys != NO_MATCH) and dt < 20.0


# ---- the second trip of the sums --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_within", [2, 3])
def test_reach_scene_big_is_what_it_says(n_within):
    src, tgt = R.reach_scene_big(n_within)
    assert src.shape[0] == R.SUM_THREADS + n_within and tgt.shape[0] == 300
    keys = numpy_keys(src, tgt)
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(F).astype(np.float64)
    within = d2 <= 0.75 * 0.75
    assert not within[:R.SUM_THREADS].any() and within[R.SUM_THREADS:].all()            # only sources of the second trip
    assert d2[-1] == 0.5625 and (d2[:R.SUM_THREADS] > 4.0).all()


def test_fitness_scene_shows_a_dropped_last_point():
    src, tgt = R.fitness_scene()
    assert src.shape[0] == R.SUM_THREADS + 1
    keys = numpy_keys(src, tgt)
    d = np.sqrt((keys >> np.uint64(32)).astype(np.uint32).view(F).astype(np.float64))
    assert np.all(np.abs(d[:-1] - 0.1) < 1e-5) and abs(d[-1] - 1.0) < 1e-5
    full = R.fitness_in_blocks(src, tgt, np.eye(4))
    dropped = R.fitness_in_blocks(src[:-1], tgt, np.eye(4))
    assert abs(full - numpy_fitness(src[-9000:], tgt, np.eye(4))) < 2e-2 * full      # (the blocks are numpy_fitness's)
    assert abs(full - dropped) > 100 * 1e-5 * full                       # the GPU test's bar is 1e-5 relative


# ---- the boundary -----------------------------------------------------------------------------------------------------------

NEW = ["s2m_debug_icp_grid", "s2m_debug_icp_grid_check_args"]


def test_new_symbols_declared_bound_and_exported():
    lib = s2m.load_library()
    dbg = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    main = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    for n in NEW:
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n) and n + "(" in dbg and n not in main
    assert int(re.search(r"#define S2M_DEBUG_ICP_GRID_MAX_CELLS\s+(\d+)", dbg).group(1)) == s2m.S2M_DEBUG_ICP_GRID_MAX_CELLS == R.GRID_MAX_CELLS
    assert int(re.search(r"#define S2M_LOOP_MAX_CANDIDATES\s+(\d+)", main).group(1)) == s2m.S2M_LOOP_MAX_CANDIDATES
    src = open(os.path.join(ROOT, "liorf_amd", "csrc", "s2m_icp.hip")).read()
    assert re.search(r"kGridMaxCells = 1 << 18;", src) and f"kIcpShellCap = {R.SHELL_CAP};" in open(
        os.path.join(ROOT, "liorf_amd", "csrc", "s2m_icp.hpp")).read()


def test_grid_hook_argument_checks():
    import ctypes as C
    lib = s2m.load_library()
    t = SCENES["fits_exactly"][1]
    ok = s2m.debug_icp_grid_check_args
    assert ok([t]) == 0 and ok([t] * s2m.S2M_LOOP_MAX_CANDIDATES) == 0
    bad = -1                                                              # S2M_ERR_INVALID_ARG
    assert ok([t] * (s2m.S2M_LOOP_MAX_CANDIDATES + 1)) == bad and ok([t], n_cand=0) == bad and ok([t], n_cand=-1) == bad
    assert ok([t], has_out=False) == bad and ok([t], has_list=False) == bad and ok([t], has_counts=False) == bad
    assert ok([t, None]) == bad and ok([t, t[:0]]) == bad                 # a null target, an empty one
    assert ok([t], stride=8) == bad and ok([t], stride=18) == bad and ok([t], stride=12) == 0
    odd = np.zeros(64, np.uint8)[1:33].view(np.uint8)                     # a buffer that is not 4-byte aligned
    ptrs = (C.c_void_p * 1)(odd.ctypes.data | 1)
    ns = (C.c_size_t * 1)(1)
    out = (s2m.IcpGridOut * 1)()
    assert lib.s2m_debug_icp_grid_check_args(ptrs, ns, 1, 16, out) == bad
    ns[0] = 0x40000000
    ptrs[0] = t.ctypes.data
    assert lib.s2m_debug_icp_grid_check_args(ptrs, ns, 1, 16, out) == s2m.S2M_ERR_CAPACITY
    # the null handle, before anything else is looked at
    assert lib.s2m_debug_icp_grid(None, None, None, 0, 0, None, None, None, None) == bad
    assert lib.s2m_debug_icp_grid(None, ptrs, ns, 1, 16, out, None, None, None) == bad
