"""The ICP loop on the device (s2m_icp.hip: the grid search, k_icp_close, ranges of S2M_ICP_RANGE iterations, the fitness pass)
through s2m_debug_icp_align_device, against s2m_icp_align (k_icp_nn, the host-driven loop) on the same inputs: T as 32-bit
patterns, `converged`, `iterations`, and the fitness score as a 64-bit pattern - all equal.  Both loops close an iteration with
one source (s2m_icp_close.hpp), the searches return the same keys (tests/test_icp_grid_gpu.py), and the sums are folded in
workgroup order, so nothing is left to differ."""
import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_cpu import icp_scene
from test_icp_edges_cpu import MAP_OFFSETS, edge_scene, moved_scene, reach_scene, tie_scene

pytestmark = pytest.mark.gpu

R = s2m.S2M_ICP_RANGE


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _same(a, b):
    Ta, ca, fa, ia = a
    Tb, cb, fb, ib = b
    assert (ca, ia) == (cb, ib), (ca, ia, cb, ib)
    assert np.array_equal(Ta.view(np.uint32), Tb.view(np.uint32)), np.abs(Ta - Tb).max()
    assert np.float64(fa).view(np.uint64) == np.float64(fb).view(np.uint64), (fa, fb)


def _both(gpu, src, tgt, **kw):
    want = gpu.icpAlign(src, tgt, **kw)
    got = gpu.debugIcpAlignDevice(src, tgt, **kw)
    _same(got, want)
    return want


@pytest.mark.parametrize("n_tgt,n_src,seed", [(6000, 1500, 5), (20000, 3000, 9), (1500, 700, 2)])
def test_device_loop_on_the_icp_scenes(gpu, n_tgt, n_src, seed):
    src, tgt, _ = icp_scene(n_tgt, n_src, seed)
    T, conv, fit, its = _both(gpu, src, tgt, max_correspondence_distance=30.0)
    assert conv and its > 1
    _both(gpu, src, tgt, max_correspondence_distance=0.5)


@pytest.mark.parametrize("n_src", [3, 255, 256, 257])
@pytest.mark.parametrize("n_tgt", [1023, 1024, 1025, 4097])
def test_device_loop_on_tile_and_block_edges(gpu, n_tgt, n_src):
    src, tgt = edge_scene(n_tgt, n_src, seed=n_tgt + n_src)
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


@pytest.mark.parametrize("n_src", [3, 255, 256, 257])
def test_device_loop_on_three_targets(gpu, n_src):
    src, tgt = edge_scene(3, n_src, seed=3 + n_src)
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


@pytest.mark.parametrize("n_tgt", [1, 2])
@pytest.mark.parametrize("n_src", [3, 257])
def test_device_loop_on_one_or_two_targets(gpu, n_tgt, n_src):
    """Rank 0 or 1 cross-covariances up to rounding noise: the rotation is fixed by that noise, the same noise in both loops, and
    it is a rotation all the same - R R^T = I and det R = 1 to 4e-7, the bar of tests/test_icp_close_cpu.py for one Umeyama step
    (so it is asked of the alignment that ends after one iteration)."""
    src, tgt = edge_scene(n_tgt, n_src, seed=7 + n_tgt)
    T, _, _, _ = _both(gpu, src, tgt, max_correspondence_distance=30.0, max_iterations=1)
    Rm = T[:3, :3].astype(np.float64)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 4e-7 and abs(np.linalg.det(Rm) - 1.0) <= 4e-7, T
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


@pytest.mark.parametrize("n_within", [2, 3, 4])
def test_device_loop_min_correspondences_and_reach(gpu, n_within):
    if n_within == 4:                                            # reach_scene(3) and one more source within 0.75 m
        src, tgt = reach_scene(3)
        src = np.concatenate([src, src[:1]])
        src[-1, :3] = (0.0, 0.3, 10.0)
    else:
        src, tgt = reach_scene(n_within)
    T, conv, fit, its = _both(gpu, src, tgt, max_correspondence_distance=0.75)
    assert conv == (n_within >= 3)
    if n_within == 2:                                            # ends by cnt < 3 in the first iteration
        assert its == 0 and np.array_equal(T, np.eye(4, dtype=np.float32))
    _both(gpu, src, tgt, max_correspondence_distance=float(np.nextafter(0.75, 0.0)))


def test_device_loop_with_non_finite_points(gpu):
    src, tgt = edge_scene(4097, 700, seed=11)
    for k, j in enumerate(range(0, tgt.shape[0], 7)):
        tgt[j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    tgt[1023, :3] = np.nan; tgt[1024, 0] = np.inf; tgt[4096, 2] = -np.inf
    T, conv, fit, its = _both(gpu, src, tgt, max_correspondence_distance=30.0)
    assert conv and np.isfinite(fit)
    src[5, 0] = np.nan; src[9, 2] = np.inf
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


@pytest.mark.parametrize("n_src", [256, 257])
def test_device_loop_on_exact_ties(gpu, n_src):
    src, tgt = tie_scene(n_src=n_src)
    T, _, _, its = _both(gpu, src, tgt, max_correspondence_distance=30.0, max_iterations=1)
    assert its == 1 and abs(T[0, 3] - 0.5) < 1e-5
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


@pytest.mark.parametrize("offset", MAP_OFFSETS)
def test_device_loop_in_the_map_frame(gpu, offset):
    src, tgt, _ = moved_scene(6000, 1500, 5, offset)
    _both(gpu, src, tgt, max_correspondence_distance=30.0)


def _moved(src0, scale):
    """icp_scene's source under a further rigid motion, `scale` times (0.05 rad of yaw, (0.6, -0.45, 0.15) m)."""
    c, s_ = np.cos(0.05 * scale), np.sin(0.05 * scale)
    m = src0.copy()
    m[:, :3] = (src0[:, :3].astype(np.float64) @ np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]]).T
                + np.array([0.6, -0.45, 0.15]) * scale).astype(np.float32)
    return m


def test_iteration_limit_around_a_range(gpu):
    """max_iterations of 1, R - 1, R, R + 1, 2R, 2R + 1 on a scene that needs more: the alignment ends by the iteration limit at
    and beside a range boundary."""
    src0, tgt, _ = icp_scene(6000, 1500, 5)
    src = _moved(src0, 2.0)
    kw = dict(max_correspondence_distance=30.0, transformation_epsilon=1e-12, euclidean_fitness_epsilon=1e-14)
    full = gpu.icpAlign(src, tgt, **kw)
    assert full[3] > R + 1, full[3]
    for m in (1, R - 1, R, R + 1, 2 * R, 2 * R + 1):
        T, conv, fit, its = _both(gpu, src, tgt, max_iterations=m, **kw)
        assert conv and its == min(m, full[3])


def test_convergence_at_a_range_edge(gpu):
    """Alignments that end by PCL's own criteria on the iteration before the last of a range, on the last, and on the first of the
    next range (R - 1, R, R + 1): found by running the synchronous call first, over initial motions of growing size and a few
    epsilon pairs; every one of the three must be found, and the device loop must give its bits."""
    src0, tgt, _ = icp_scene(6000, 1500, 5)
    want = (R - 1, R, R + 1)
    seen = {}
    for scale in np.arange(0.5, 8.01, 0.25):
        src = _moved(src0, float(scale))
        for eps in (1e-6, 1e-4, 1e-3, 1e-5, 1e-7, 1e-8, 1e-9):
            kw = dict(max_correspondence_distance=30.0, transformation_epsilon=eps, euclidean_fitness_epsilon=eps)
            run = gpu.icpAlign(src, tgt, **kw)
            if run[3] in want and run[3] not in seen and run[1]:
                seen[run[3]] = (src, kw, run)
        if len(seen) == len(want):
            break
    print("converged by its criteria at iterations", sorted(seen))
    assert sorted(seen) == list(want), sorted(seen)
    for its, (src, kw, run) in seen.items():
        assert its < 100                                         # (ended by a criterion, not by max_iterations)
        _same(gpu.debugIcpAlignDevice(src, tgt, **kw), run)


def test_device_loop_is_bitwise_reproducible(gpu):
    src, tgt, _ = moved_scene(20000, 8000, 9, MAP_OFFSETS[1])
    a = gpu.debugIcpAlignDevice(src, tgt, max_correspondence_distance=30.0)
    b = gpu.debugIcpAlignDevice(src, tgt, max_correspondence_distance=30.0)
    _same(a, b)
    g2 = s2m.MapOptimizationS2M()
    try:
        _same(g2.debugIcpAlignDevice(src, tgt, max_correspondence_distance=30.0), a)
    finally:
        g2.close()
    _same(a, gpu.icpAlign(src, tgt, max_correspondence_distance=30.0))


def test_brute_force_search_in_the_device_loop(gpu):
    """The one constant that selects the search (here through the experiment switch): the same bits with the grid off."""
    src, tgt, _ = icp_scene(1500, 700, 2)
    try:
        gpu.debugIcpTuning(0.0, 0, 0)
        _both(gpu, src, tgt, max_correspondence_distance=30.0)
    finally:
        gpu.debugIcpTuning()


def test_empty_clouds_and_bad_arguments(gpu):
    src, tgt, _ = icp_scene(1500, 700, 2)
    T, conv, fit, its = gpu.debugIcpAlignDevice(src[:0], tgt)
    assert not conv and its == 0 and np.array_equal(T, np.eye(4, dtype=np.float32))
    _same(gpu.debugIcpAlignDevice(src, tgt[:0]), gpu.icpAlign(src, tgt[:0]))
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignDevice(src, tgt, max_iterations=0)
