"""ICP (s2m_icp.hip: k_icp_nn, k_icp_sums) at the edges of its tiling and far from the origin, against the oracle and
against float64 numpy statements (tests/test_icp_edges_cpu.py).  Bars at the origin are those of tests/test_icp_gpu.py:
T within 1e-5, equal iterations, equal `converged`.  PARITY UNPINNED."""
import numpy as np
import pytest

from liorf_amd import s2m
from oracle import oracle as O
from test_icp_edges_cpu import MAP_OFFSETS, aligned, edge_scene, moved_scene, numpy_fitness, reach_scene, tie_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@pytest.mark.parametrize("n_src", [3, 255, 256, 257])
@pytest.mark.parametrize("n_tgt", [1023, 1024, 1025, 4097])
def test_icp_tile_and_block_edges(gpu, n_tgt, n_src):
    """k_icp_nn: 256 source points per workgroup (n_src 255 / 256 / 257 = one block full, one lane over), targets
    staged in 1 024-point LDS tiles (n_tgt 1023 / 1024 / 1025: a last tile of 1023, 1 024 or 1 point) and split into
    up to ceil(1024 / source blocks) slices (n_tgt 4097: 5 slices of 1 024, the last holding 1 point); n_src = 3 is
    min_number_correspondences_."""
    src, tgt = edge_scene(n_tgt, n_src, seed=n_tgt + n_src)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv == convo and its == itso, (its, itso)
    assert np.abs(T - To).max() <= 1e-5
    assert abs(fit - numpy_fitness(src, tgt, T)) <= 1e-5 * max(fit, 1e-2)


@pytest.mark.parametrize("n_src", [3, 255, 256, 257])
def test_icp_three_targets(gpu, n_src):
    """Three target points (a plane: the fewest for which the rotation is determined), the source drawn from them
    with 1 cm of noise.  The residual goes to the noise floor (to zero for 3 source points), where REL_MSE compares
    two differences of nearly equal numbers: the iteration at which it fires is decided by the rounding of the sums
    (device fp64, oracle fp32; measured 3 vs 4 iterations at n_src = 3 and |T - T_oracle| = 1.2e-5 at n_src = 255).
    With n_src = 3 every target is drawn once: three sources on two targets are a line, and the rotation about it is
    rounding noise (measured |T - T_oracle| = 18 when two of the three draws hit one target).
    Bars: equal `converged`, iterations within one, T within 1e-4, fitness equal to the float64 recomputation."""
    src, tgt = edge_scene(3, n_src, seed=3 + n_src)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv == convo and abs(its - itso) <= 1, (its, itso)
    assert np.abs(T - To).max() <= 1e-4
    assert abs(fit - numpy_fitness(src, tgt, T)) <= 1e-5 * max(fit, 1e-2)


@pytest.mark.parametrize("n_tgt", [1, 2])
@pytest.mark.parametrize("n_src", [3, 257])
def test_icp_one_or_two_targets(gpu, n_tgt, n_src):
    """One or two target points: the cross-covariance has rank 0 or 1 up to the rounding noise of its sums, so which
    rotation Umeyama returns is fixed by that noise (in PCL as in the oracle and the device) and T is not comparable
    entry by entry.  What is determined: R is a rotation (R R^T = I and det R = 1 to 4e-7, the bar of
    tests/test_icp_close_cpu.py, where the exact ranks 0 and 1 - zero rows, no noise - are held to it too), the
    translation brings the source centroid onto the target centroid of its correspondences, and the fitness (mean
    squared distance of the aligned source to the nearest target) does not depend on the rotation for one target.
    With three sources on one target the sums cancel exactly on the device and in the oracle: sigma = 0, R = I, fitness
    3.018e-4 on both sides.  (Before host_svd3 completed U for rank 0 both sides returned R = 0 there, the source
    collapsed onto the target and the two fitness values compared were both 0.)"""
    src, tgt = edge_scene(n_tgt, n_src, seed=7 + n_tgt)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0, max_iterations=1)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0, max_iter=1)
    assert conv and convo and its == itso == 1
    Rm = T[:3, :3].astype(np.float64)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 4e-7 and abs(np.linalg.det(Rm) - 1.0) <= 4e-7, T
    a = aligned(src, T)
    if n_tgt == 1:
        assert np.abs(a.mean(0) - tgt[0, :3]).max() < 1e-4
        assert abs(fit - fito) <= 1e-5 * fito and abs(fit - numpy_fitness(src, tgt, T)) <= 1e-5 * fit
    else:
        assert abs(fit - numpy_fitness(src, tgt, T)) <= 1e-5 * max(fit, 1e-2)


@pytest.mark.parametrize("n_within", [2, 3])
def test_icp_min_correspondences_and_reach_boundary(gpu, n_within):
    """Exactly 2 or 3 source points within max_correspondence_distance = 0.75 m, one of them at exactly 0.75 m
    (d2 = 0.5625 = max^2 in fp32 and in double: `<=` keeps it).  2 -> fewer than min_number_correspondences_ (3):
    not converged, identity, no iteration; 3 -> converged.  One ulp less distance drops the boundary pair."""
    src, tgt = reach_scene(n_within)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=0.75)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=0.75)
    assert conv == convo == (n_within == 3) and its == itso
    assert np.abs(T - To).max() <= 1e-5
    if n_within == 2:
        assert its == 0 and np.array_equal(T, np.eye(4, dtype=np.float32))
    T2, conv2, _, its2 = gpu.icpAlign(src, tgt, max_correspondence_distance=float(np.nextafter(0.75, 0.0)))
    assert not conv2 and its2 == 0


def test_icp_non_finite_targets(gpu):
    """NaN / +-inf in target points (every 7th point, one coordinate each, in every tile): their distances are NaN or
    inf and never win `d2 < best`; the fitness ignores them too."""
    src, tgt = edge_scene(4097, 700, seed=11)
    for k, j in enumerate(range(0, tgt.shape[0], 7)):
        tgt[j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    tgt[1023, :3] = np.nan; tgt[1024, 0] = np.inf; tgt[4096, 2] = -np.inf
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv == convo and conv and its == itso and np.abs(T - To).max() <= 1e-5
    assert np.isfinite(fit) and abs(fit - numpy_fitness(src, tgt, T)) <= 1e-5 * max(fit, 1e-2)


@pytest.mark.parametrize("n_src", [256, 257])
def test_icp_exact_ties_across_tiles_and_slices(gpu, n_src):
    """Every source point is equidistant (d2 = 0.25 exactly) from two distinct targets whose indices differ by 2 048:
    two LDS tiles apart, and with n_src = 256 (1 source block, 5 target slices of 1 024) in different slices, so the
    winner is settled by the 64-bit atomicMin key (d2 bits << 32 | index): ties go to the lower index, the x = 2k+1
    point, as in the oracle.  After one iteration the first transform is +0.5 m in x; a wrong tie-break moves it."""
    src, tgt = tie_scene(n_src=n_src)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0, max_iterations=1)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0, max_iter=1)
    assert its == itso == 1 and np.abs(T - To).max() <= 1e-5 and abs(T[0, 3] - 0.5) < 1e-5
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv == convo and its == itso and np.abs(T - To).max() <= 1e-5


@pytest.mark.parametrize("offset", MAP_OFFSETS)
def test_icp_in_the_map_frame(gpu, offset):
    """icp_scene moved to 5 km, 20 km and 100 km from the origin (loopFindNearKeyframes, reference :821-843, moves the
    key frames there).  T entries are not comparable there (a rotation difference d moves t by d * |mean|), so the
    bars are on the aligned source in metres.  The oracle restates PCL's fp32 centroid and covariance sums, whose
    rounding grows with the offset (at 20 km a sum of 1 500 coordinates is ~3e7, one fp32 ulp 2 m, so the mean is off
    by ~1e-3 m per add): it ran 7 / 100 / 14 iterations and reached fitness 3.2e-4 / 2.7e-3 / 9.1e-4, against the
    device's 8 / 9 / 9 and 3.1e-4 / 3.4e-4 / 1.3e-3 (fp64 sums, folded in workgroup order).  So the device is held to
    the known motion and to a float64 recomputation: aligned source within 0.06 m of the truth (measured 1.4 / 7.2 /
    35 mm; fp32 coordinates are 0.49 / 1.95 / 7.8 mm apart at these offsets, the noise is 10 mm, and at 100 km the
    fp32 composition of T moves the result by several grid steps: 14 mm with the earlier arrival-order sums),
    fitness within 5 % of the float64 value for the returned T (measured 0.08 / 0.8 / 0.14 %), converged in fewer than
    30 iterations; and to the oracle's aligned source within 0.1 m (measured 2.7 / 46 / 17 mm)."""
    src, tgt, true_pos = moved_scene(6000, 1500, 5, offset)
    T, conv, fit, its = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    To, convo, fito, itso = O.icp_align(src, tgt, max_corr_dist=30.0)
    a, ao = aligned(src, T), aligned(src, To)
    d_oracle, d_true = np.abs(a - ao).max(), np.abs(a - true_pos).max()
    fit64 = numpy_fitness(src, tgt, T)
    print(f"offset {offset}: |aligned - oracle| {d_oracle:.3g} m, |aligned - truth| {d_true:.3g} m, iterations {its} / {itso}, "
          f"fitness {fit:.6g} / oracle {fito:.6g} / float64 {fit64:.6g}")
    assert conv and convo and its < 30
    assert d_true < 0.06 and d_oracle < 0.1
    assert abs(fit - fit64) <= 0.05 * fit64


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), MAP_OFFSETS[1]])
def test_icp_is_bitwise_reproducible(gpu, offset):
    """The same icpAlign call twice on one handle and once on a second handle: bit-identical T, fitness, iterations
    and `converged`.  20 000 x 8 000 points: k_icp_sums runs 32 workgroups, whose partial sums must be folded in an
    order that does not depend on when each workgroup finishes (at 20 km the raw moments are ~4e8 m^2, where one
    fp64 rounding of a different summation order is ~6e-8 m^2, the size of one fp32 ulp of the covariance)."""
    src, tgt, _ = moved_scene(20000, 8000, 9, offset)
    runs = [gpu.icpAlign(src, tgt, max_correspondence_distance=30.0) for _ in range(2)]
    g2 = s2m.MapOptimizationS2M()
    try:
        runs.append(g2.icpAlign(src, tgt, max_correspondence_distance=30.0))
    finally:
        g2.close()
    T0, c0, f0, i0 = runs[0]
    for T, c, f, i in runs[1:]:
        assert np.array_equal(T.view(np.uint32), T0.view(np.uint32)) and c == c0 and i == i0
        assert np.float64(f).view(np.uint64) == np.float64(f0).view(np.uint64)
