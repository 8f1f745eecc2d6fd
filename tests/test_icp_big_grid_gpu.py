"""The uniform grid of the ICP device loop at the extents of real loop-closure submaps (tests/ref/icp_grid_ref.py): boxes that
need more than kGridMaxCells cells at the edge asked for, so that k_icp_grid_setup enlarges the edge, k_icp_grid_scan serves
hundreds of cells per lane and grid_settled works on an edge that is neither 0.6 nor 1.0 m; a box whose extent overflows fp32
(no grid: every source to the brute force); and more sources than the sums kernel has lanes.

* shape and table: what s2m_debug_icp_grid hands back of the product's own launches against the numpy model, alone and in the
  slots of an eight-target call;
* keys: s2m_debug_icp_nearest mode 1 = mode 0 = numpy_keys bit for bit, at the origin and up to 100 km out;
* a target a few fp32 steps beyond a cell face of a grown grid that is nearer than everything in the 27 cells;
* whole alignments by the device loop, bit for bit s2m_icp_align;
* the second trip of the sums' grid-stride loop (n_src > 65 536) through all three forms of the alignment.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))

import icp_grid_ref as R  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_icp_device_loop_gpu import _same  # noqa: E402
from test_icp_edges_cpu import MAP_OFFSETS  # noqa: E402
from test_icp_grid_cpu import CELL, cell_index, numpy_keys, shifted  # noqa: E402
from test_icp_grid_gpu import _check  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
OFFSETS = [None] + MAP_OFFSETS
SCENES = R.big_scenes()
NAMES = sorted(SCENES)
# The device's grown edge against the model's, relative. The edge asked for is exact; every further try multiplies it by
# max(1.1, cbrtf(..) * 1.02), where only cbrtf - the device library's there, the host's here, a few fp32 steps apart at most -
# is not correctly rounded on both sides. With at most 17 tries here that stays within 1e-5, about 80 fp32 steps, and the cell
# counts are the same for every edge within that bar (tests/test_icp_big_grid_cpu.py checks each of them).
EDGE_BAR = 1e-5


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _scene(name, oi):
    src, tgt, stated = SCENES[name]
    return shifted(src, tgt, OFFSETS[oi]) + (stated,)


def _check_shape(g, tgt, cell_req=CELL):
    """One grid of the hook against the model; returns the relative difference of the edges (0 where it did not grow, None
    without a grid)."""
    m = R.grid_shape(tgt, cell_req)
    assert np.array_equal(g["lo"].view(np.uint32), m["lo"].view(np.uint32)), (g["lo"], m["lo"])
    assert g["n_fin"] == m["n_fin"] and g["usable"] == m["usable"], (g, m["n_fin"], m["usable"])
    if not m["usable"]:
        return None
    if len(m["tries"]) == 1:
        assert g["cell"].view(np.uint32) == F(cell_req).view(np.uint32) and g["inv"].view(np.uint32) == m["inv"].view(np.uint32)
        assert g["n"] == m["n"]
        return 0.0
    assert g["cell"] > F(cell_req)
    assert g["inv"].view(np.uint32) == (F(1.0) / g["cell"]).view(np.uint32)
    assert g["n"] == R.shape_counts(m["lo"], m["hi"], g["cell"]) == m["n"], (g["n"], m["n"])
    assert g["n"][0] * g["n"][1] * g["n"][2] <= R.GRID_MAX_CELLS
    rel = abs(float(g["cell"]) - float(m["cell"])) / float(m["cell"])
    assert rel <= EDGE_BAR, (g["cell"], m["cell"], rel)
    return rel


def _check_table(g, tgt):
    """The cell starts, ends and sorted order of one grid of the hook against cell_table on the device's own shape."""
    flat, counts, starts, order = R.cell_table(tgt, g["lo"], g["inv"], g["n"])
    assert g["start"].shape == counts.shape and np.array_equal(g["start"], starts), np.flatnonzero(g["start"] != starts)[:8]
    assert np.array_equal(g["end"], starts + counts), np.flatnonzero(g["end"] != starts + counts)[:8]
    assert g["order"].shape == order.shape
    assert np.array_equal(np.sort(g["order"]), np.flatnonzero(flat >= 0))                    # every finite target once
    assert np.array_equal(R.sorted_within_cells(g["order"], counts), order)                 # and in its own cell


@pytest.mark.parametrize("oi", range(len(OFFSETS)))
@pytest.mark.parametrize("name", NAMES)
def test_shape_against_the_model(gpu, name, oi):
    src, tgt, _ = _scene(name, oi)
    g = gpu.debugIcpGrid([tgt], tables=False)[0]
    rel = _check_shape(g, tgt)
    print(f"EDGE {name} offset {OFFSETS[oi]}: cell {g['cell']!r} n {g['n']} usable {g['usable']} relative edge difference {rel}")


@pytest.mark.parametrize("name", [n for n in NAMES if SCENES[n][2]["usable"] == 1])
def test_table_against_the_model(gpu, name):
    src, tgt, _ = SCENES[name]
    g = gpu.debugIcpGrid([tgt])[0]
    _check_shape(g, tgt)
    _check_table(g, tgt)


def test_tables_in_the_slots_of_an_eight_target_call(gpu):
    """street in slots 1 and 7, corridor (a cell array filled to 98 %) and outlier around them: every slot's shape and table are
    those of the single call, so the slot offsets of the cell arrays and of the sorted targets hold."""
    names = ["corridor", "street", "outlier", "corridor", "outlier", "corridor", "outlier", "street"]
    single = {n: gpu.debugIcpGrid([SCENES[n][1]])[0] for n in set(names)}
    many = gpu.debugIcpGrid([SCENES[n][1] for n in names])
    assert len(many) == s2m.S2M_LOOP_MAX_CANDIDATES
    for k, (n, g) in enumerate(zip(names, many)):
        one = single[n]
        for f in ("lo", "cell", "inv"):
            assert np.array_equal(np.asarray(g[f]).view(np.uint32), np.asarray(one[f]).view(np.uint32)), (k, n, f)
        assert (g["n"], g["n_fin"], g["usable"]) == (one["n"], one["n_fin"], one["usable"]), (k, n)
        assert np.array_equal(g["start"], one["start"]) and np.array_equal(g["end"], one["end"]), (k, n)
        _check_table(g, SCENES[n][1])


def test_the_hook_is_busy_while_a_closure_is_pending():
    """Like its neighbours the hook uses the closure's target buffers and the ICP workspace: S2M_ERR_BUSY, nothing written and
    the pending closure untouched; after the collect it works again."""
    import ctypes as C
    from test_loop_closure_cpu import scripted_revisit
    clouds, poses, times, _ = scripted_revisit()
    tgt = SCENES["one_over"][1]
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for g in (a, b):
            for k in range(len(clouds)):
                g.saveKeyFrame(poses[k], times[k], clouds[k])
        prm = s2m.default_loop_params(search_radius=15.0, search_num=2, icp_leaf=0.5)
        want = b.loopAlign(len(clouds) - 1, 0, -1, prm)
        assert a.loopAlignLaunch(len(clouds) - 1, 0, -1, prm).status == s2m.S2M_LOOP_PENDING
        ptrs = (C.c_void_p * 1)(tgt.ctypes.data)
        ns = (C.c_size_t * 1)(tgt.shape[0])
        out = (s2m.IcpGridOut * 1)()
        out[0].n_fin, out[0].usable = 77, 78
        rc = a.lib.s2m_debug_icp_grid(a.h, ptrs, ns, 1, tgt.shape[1] * 4, out, None, None, None)
        assert rc == s2m.S2M_ERR_BUSY and (out[0].n_fin, out[0].usable) == (77, 78)
        with pytest.raises(s2m.S2MError, match="BUSY"):
            a.debugIcpGrid([tgt])
        got = a.loopCollect()
        assert C.string_at(C.addressof(got), C.sizeof(got)) == C.string_at(C.addressof(want), C.sizeof(want))
        assert got.status == s2m.S2M_LOOP_ACCEPTED
        _check_shape(a.debugIcpGrid([tgt], tables=False)[0], tgt)
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):                # and the argument check behind the handle
            a.debugIcpGrid([tgt, tgt[:0]])
    finally:
        a.close()
        b.close()


def _fallbacks(gpu, src, tgt):
    return gpu.debugIcpNearest(src, tgt, 1)[1]


@pytest.mark.parametrize("oi", range(len(OFFSETS)))
@pytest.mark.parametrize("name", NAMES)
def test_keys_on_the_big_scenes(gpu, name, oi):
    src, tgt, stated = _scene(name, oi)
    fb = stated["fallback"]
    _check(gpu, src, tgt, "some" if fb == "all" else fb)
    n_fin_src = int(np.isfinite(src[:, :3]).all(1).sum())
    if name == "street":
        assert 0 < _fallbacks(gpu, src, tgt) < src.shape[0]
    if fb == "all":
        assert n_fin_src < src.shape[0] and _fallbacks(gpu, src, tgt) == n_fin_src
    if name == "fits_exactly":
        assert _fallbacks(gpu, src, tgt) == 0


@pytest.mark.parametrize("leaves,cap", [(1.0, 0), (3.0, 0), (0.0, 1)])
def test_street_keys_with_other_edges_and_a_small_shell_cap(gpu, leaves, cap):
    """Cells asked for at 0.3 m and 0.9 m grow to edges that are neither 0.6 nor 1.0 m; shell cap 1 sends every source its 27
    cells do not settle to the brute force. The route changes, the keys do not."""
    src, tgt, _ = SCENES["street"]
    want = numpy_keys(src, tgt)
    try:
        gpu.debugIcpTuning(leaves, cap, -1)
        if leaves:
            g = gpu.debugIcpGrid([tgt], tables=False)[0]
            rel = _check_shape(g, tgt, F(leaves) * F(0.3))
            print(f"EDGE street at {leaves} leaves: cell {g['cell']!r} n {g['n']} relative edge difference {rel}")
            assert g["cell"] > 1.5
        k, f = gpu.debugIcpNearest(src, tgt, 1)
        print("n_fallback", f)
        assert np.array_equal(k, want) and 0 < f < src.shape[0]
    finally:
        gpu.debugIcpTuning()


@pytest.mark.parametrize("oi", [0, 2])
def test_a_target_beyond_a_face_of_a_grown_grid(gpu, oi):
    """sliver_scene on street's grown grid, in the empty air at z = 20 m: the query one fp32 step below a cell face, B two steps
    beyond the next face (outside the 27 cells), A inside them and two steps farther. The x cell is the one whose fp32 face lies
    farthest below the exact one and the y cell the one nearest to y = 0, where A's steps are finest: there a bound without
    kFaceSlack is most too generous (at the origin by more than A's two steps). The key must be B."""
    src, tgt, _ = _scene("street", oi)
    g = gpu.debugIcpGrid([tgt], tables=False)[0]
    _check_shape(g, tgt)
    k, below = R.sharpest_face_cell(g["lo"], g["cell"], g["n"], F(20.0) + (g["lo"][2] + F(2.0)))
    q, a, b = R.face_points(g["lo"], g["cell"], k)
    print(f"cell {k}: the fp32 face to cell {k[0] + 2} lies {below:.2f} steps below the exact one; q {q} A {a} B {b}")
    t2 = np.concatenate([tgt, synth.to_xyzi(np.array([a, b]))])
    s2 = np.concatenate([src, synth.to_xyzi(q[None])])
    g2 = gpu.debugIcpGrid([t2], tables=False)[0]
    assert np.array_equal(g2["lo"], g["lo"]) and g2["cell"] == g["cell"] and g2["n"] == g["n"]   # the box has not changed
    cq = tuple(int(cell_index(q[i], g["lo"][i], g["cell"])) for i in range(3))
    cb = tuple(int(cell_index(b[i], g["lo"][i], g["cell"])) for i in range(3))
    ca = tuple(int(cell_index(a[i], g["lo"][i], g["cell"])) for i in range(3))
    assert cq == k and cb == (k[0] + 2, k[1], k[2]) and ca == (k[0], k[1] - 1, k[2])
    want = numpy_keys(s2, t2)
    assert int(want[-1] & np.uint64(0xFFFFFFFF)) == t2.shape[0] - 1                             # B
    k0, _ = gpu.debugIcpNearest(s2, t2, 0)
    k1, f1 = gpu.debugIcpNearest(s2, t2, 1)
    assert np.array_equal(k0, want) and np.array_equal(k1, want), (k1[-1], want[-1])
    assert f1 == _fallbacks(gpu, src, t2)                                                       # and the grid settled it


def test_whole_alignments_on_grown_grids(gpu):
    src, tgt, _ = SCENES["street"]
    want = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    _same(gpu.debugIcpAlignDevice(src, tgt, max_correspondence_distance=30.0), want)
    assert want[1] and want[3] >= 1
    src, tgt, _ = SCENES["corridor"]
    want = gpu.icpAlign(src, tgt)
    _same(gpu.debugIcpAlignDevice(src, tgt), want)
    assert want[1]


def test_four_grids_of_one_source_in_lockstep(gpu):
    """street, corridor, outlier and overflow (no grid at all) as the targets of street's source: every record is the single
    alignment's."""
    src = SCENES["street"][0]
    tgts = [SCENES[n][1] for n in ("street", "corridor", "outlier", "overflow")]
    got = gpu.debugIcpAlignManyDevice(src, tgts, max_correspondence_distance=30.0)
    for t, r in zip(tgts, got):
        _same(r, gpu.icpAlign(src, t, max_correspondence_distance=30.0))


# ---- the second trip of the sums --------------------------------------------------------------------------------------------

def _three_forms(gpu, src, tgt, **kw):
    want = gpu.icpAlign(src, tgt, **kw)
    _same(gpu.debugIcpAlignDevice(src, tgt, **kw), want)
    for r in gpu.debugIcpAlignManyDevice(src, [tgt, tgt], **kw):
        _same(r, want)
    return want


def test_correspondences_beyond_the_sums_lanes_are_counted(gpu):
    """65 539 sources, of which only the last three - beyond the 65 536 lanes of the sums kernel - have a target within reach,
    one of them exactly on the boundary: three correspondences are what the alignment needs."""
    src, tgt = R.reach_scene_big(3)
    assert src.shape[0] == 65539 and tgt.shape[0] == 300
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=0.75)
    T, conv, fit, its = _three_forms(gpu, src, tgt, max_correspondence_distance=0.75)
    print("iterations", its, "oracle", itso, "max |T - oracle|", np.abs(T - To).max())
    assert convo and conv and its == itso and np.abs(T - To).max() <= 1e-5


def test_two_correspondences_beyond_the_sums_lanes_are_too_few(gpu):
    src, tgt = R.reach_scene_big(2)
    assert src.shape[0] == 65538
    T, conv, fit, its = _three_forms(gpu, src, tgt, max_correspondence_distance=0.75)
    assert not conv and its == 0 and np.array_equal(T, np.eye(4, dtype=F))
    assert not O.icp_align(src, tgt, max_corr_dist=0.75)[1]


def test_fitness_counts_the_source_beyond_the_sums_lanes(gpu):
    """65 537 sources in reach, the last one ten times farther than the rest: a fitness that drops it is 1.5e-3 lower
    (tests/test_icp_big_grid_cpu.py), the bar is 1e-5."""
    src, tgt = R.fitness_scene()
    T, conv, fit, its = _three_forms(gpu, src, tgt, max_iterations=1)
    want = R.fitness_in_blocks(src, tgt, T)
    print("fitness", fit, "numpy", want, "relative", abs(fit - want) / want)
    assert its == 1 and abs(fit - want) <= 1e-5 * want
