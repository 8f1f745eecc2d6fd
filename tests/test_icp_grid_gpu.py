"""The indexed exact 1-NN of the ICP device loop (s2m_icp.hip: the uniform grid over the target, k_icp_nn_grid, the brute-force
fallback k_icp_nn_list) through s2m_debug_icp_nearest: the keys of mode 1 (grid) equal those of mode 0 (k_icp_nn), and both
equal the numpy restatement of tests/test_icp_grid_cpu.py, bit for bit - at the tiling edges of both kernels, on ties, non-finite
points, degenerate grids, sources outside the box and on cell faces, far nearest neighbours, a dense cell, 5-100 km from the
origin and on the sliver case the bound's margin exists for.  n_fallback tells that both paths have run."""
import functools

import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_edges_cpu import MAP_OFFSETS, edge_scene
from test_icp_grid_cpu import NO_MATCH, grid_scenes, numpy_keys, shifted

pytestmark = pytest.mark.gpu

OFFSETS = [None] + MAP_OFFSETS
SCENES = grid_scenes()


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _edge(n_tgt, n_src):
    return edge_scene(n_tgt, n_src, seed=n_tgt + n_src)


def _check(gpu, src, tgt, fallback):
    want = numpy_keys(src, tgt)
    k0, f0 = gpu.debugIcpNearest(src, tgt, 0)
    k1, f1 = gpu.debugIcpNearest(src, tgt, 1)
    print(f"n_src {src.shape[0]} n_tgt {tgt.shape[0]} n_fallback {f1} no-match {(want == NO_MATCH).sum()}")
    assert np.array_equal(k0, want), np.flatnonzero(k0 != want)[:8]
    assert np.array_equal(k1, want), np.flatnonzero(k1 != want)[:8]
    assert np.array_equal(k1, k0) and f0 == 0
    if fallback == "zero":
        assert f1 == 0
    elif fallback == "some":
        assert 0 < f1 <= src.shape[0]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n_src", [1, 3, 255, 256, 257])
@pytest.mark.parametrize("n_tgt", [1, 2, 3, 1023, 1024, 1025, 4097])
def test_grid_keys_on_edge_scenes(gpu, n_tgt, n_src, offset):
    """k_icp_nn_grid serves 64 sources per workgroup, k_icp_nn / k_icp_nn_list 256 against 1 024-target tiles; one to three
    targets are a grid of one to a few cells. Every source lies beside the target it was drawn from: no fallback."""
    src, tgt = shifted(*_edge(n_tgt, n_src), offset)
    _check(gpu, src, tgt, "zero")


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_grid_keys_on_the_grid_scenes(gpu, name, offset):
    src, tgt, fallback = SCENES[name]
    if name == "sliver_20km" and offset is not None:
        fallback = None                                          # moved again, the scene is no longer at its face: keys only
    src, tgt = shifted(src, tgt, offset)
    _check(gpu, src, tgt, fallback)


def test_brute_force_only_and_a_small_shell_cap_give_the_same_keys(gpu):
    """The search's experiment switches change the route, never the keys: shell cap 1 sends every source not settled by its 27
    cells to the fallback; cells of 2.4 m settle the box scene at once; use_grid off makes mode 1 the list kernel over every
    source (k_icp_nn_list without a list: the device loop's brute-force search), which reports no fallback."""
    src, tgt, _ = SCENES["nearest_40m"]
    want = numpy_keys(src, tgt)
    try:
        gpu.debugIcpTuning(0.0, 1, -1)
        k, f = gpu.debugIcpNearest(src, tgt, 1)
        assert np.array_equal(k, want) and f > 0
        gpu.debugIcpTuning(8.0, 0, -1)                           # cells of 2.4 m
        k, f = gpu.debugIcpNearest(*SCENES["box"][:2], 1)
        assert np.array_equal(k, numpy_keys(*SCENES["box"][:2])) and f == 0
        gpu.debugIcpTuning(0.0, 0, 0)                            # no grid
        for name in ("nearest_40m", "non_finite", "ties_across_cells", "dense_cell"):
            s, t, _ = SCENES[name]
            k, f = gpu.debugIcpNearest(s, t, 1)
            assert np.array_equal(k, numpy_keys(s, t)) and f == 0, name
        s, t = _edge(4097, 257)
        k, f = gpu.debugIcpNearest(s, t, 1)
        assert np.array_equal(k, numpy_keys(s, t)) and f == 0
    finally:
        gpu.debugIcpTuning()


def test_no_source_and_no_target(gpu):
    src, tgt, _ = SCENES["box"]
    k, f = gpu.debugIcpNearest(src[:0], tgt, 1)
    assert k.shape == (0,) and f == 0
    k, f = gpu.debugIcpNearest(src, tgt[:0], 1)
    assert np.all(k == NO_MATCH) and f == 0
