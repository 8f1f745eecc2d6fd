"""CPU companions of tests/test_icp_edges_gpu.py: the scenes those tests build, and the float64 numpy statements they
compare the device with, checked against the oracle (reference src/mapOptmization.cpp:571-586 ->
pcl::IterativeClosestPoint, PCL 1.10 [ext]) on the same inputs.  PARITY UNPINNED."""
import numpy as np
import pytest

from liorf_amd import synth
from oracle import oracle as O
from test_icp_cpu import icp_scene

# loopFindNearKeyframes (reference :821-843) moves key frames into the map frame before ICP sees them
MAP_OFFSETS = [(5000.0, -3000.0, 20.0), (20000.0, 8000.0, -50.0), (100000.0, 60000.0, 30.0)]


def numpy_fitness(src, tgt, T):
    """Registration::getFitnessScore in float64: the source under T (applied in float64), mean squared distance to its
    nearest finite target point, every source point counted (max range = DBL_MAX)."""
    s = src[:, :3].astype(np.float64)
    s = s[np.isfinite(s).all(1)]
    t = tgt[:, :3].astype(np.float64)
    t = t[np.isfinite(t).all(1)]
    a = s @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]
    best = np.full(a.shape[0], np.inf)
    for k in range(0, t.shape[0], 2048):                # brute force, chunked
        c = t[k:k + 2048] - t[0]
        d2 = (((a - t[0])[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        best = np.minimum(best, d2.min(1))
    return float(best.mean())


def aligned(src, T):
    """The source under T, T applied in float64 (metres, in the frame of the clouds)."""
    T = np.asarray(T, np.float64)
    return src[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def moved_scene(n_tgt, n_src, seed, offset):
    """icp_scene in the map frame: both clouds shifted by `offset` (rounded to fp32 there, as the key frames are)
    and the source's true position, R src + t + offset, in float64."""
    src, tgt, T_true = icp_scene(n_tgt, n_src, seed)
    o = np.asarray(offset, np.float64)
    true_pos = src[:, :3].astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3] + o
    src_m, tgt_m = src.copy(), tgt.copy()
    src_m[:, :3] = (src[:, :3].astype(np.float64) + o).astype(np.float32)
    tgt_m[:, :3] = (tgt[:, :3].astype(np.float64) + o).astype(np.float32)
    return src_m, tgt_m, true_pos


def edge_scene(n_tgt, n_src, seed):
    """A structured target of exactly n_tgt points and a source of n_src points drawn from it (with replacement, except
    for n_src == n_tgt: each target once), 1 cm of noise, moved by a small known rigid motion."""
    scene = synth.make_scene(seed=31, half=25.0, n_boxes=10)
    base = synth.make_map(scene, max(n_tgt, 64), leaf=0.4, seed=seed)
    rng = np.random.default_rng(seed)
    tgt = base[:n_tgt]
    pick = rng.permutation(n_tgt) if n_src == n_tgt else rng.integers(0, n_tgt, n_src)    # n_src == n_tgt: every target once
    sub = tgt[pick] + rng.normal(0, 0.01, (n_src, 3)).astype(np.float32)
    R = synth.rotation_rpy(0.01, -0.015, 0.04)
    t = np.array([0.25, -0.18, 0.06])
    src = ((sub.astype(np.float64) - t) @ R).astype(np.float32)
    return synth.to_xyzi(src), synth.to_xyzi(tgt)


def tie_scene(nx=17, ny=16, nz=16, n_src=257, seed=4):
    """Exact nearest-neighbour ties between DISTINCT targets.  Target: the integer lattice [0,nx) x [0,ny) x [0,nz)
    (spacing 1 m, exact in fp32); sources at (2k + 0.5, y, z): the two targets (2k, y, z) and (2k + 1, y, z) are both
    at d2 = 0.25 exactly.  The target is permuted so that every odd-x point comes first (indices < n/2) and every even-x
    point after it, each half in lattice order: the lower index of each tied pair is the point at x = 2k + 1, and its
    partner at x = 2k lies exactly (nx // 2) * ny * nz = 2 048 indices later - two 1 024-point LDS tiles later in
    k_icp_nn, and in another target slice whenever the slice length is 1 024 or 2 048 (n_src <= 256: 5 slices of 1 024)."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    odd = g[:, 0] % 2 == 1
    rng = np.random.default_rng(seed)
    tgt = np.concatenate([g[odd], g[~odd]], 0)
    k = rng.integers(0, (nx - 1) // 2, n_src)
    src = np.stack([2 * k + 0.5, rng.integers(0, ny, n_src), rng.integers(0, nz, n_src)], 1).astype(np.float32)
    return synth.to_xyzi(src), synth.to_xyzi(tgt)


def reach_scene(n_within):
    """n_within (2 or 3) source points with a target within 0.75 m - the last of them at EXACTLY 0.75 m (dx = 0.75:
    d2 = 0.5625 in fp32 and max_corr_dist^2 = 0.5625 in double, so it is kept only by determineCorrespondences'
    `d2 > max_dist_sqr -> skip`) - and 40 source points farther than 2 m from every target."""
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10], [50, 50, 50], [-50, 20, 5]], np.float32)
    near = np.array([[0.5, 0, 0], [10, 0.25, 0], [0.75, 10, 0]], np.float32)[3 - n_within:]
    rng = np.random.default_rng(n_within)
    far = rng.uniform([20, 20, -5], [40, 40, 5], (40, 3)).astype(np.float32)
    return synth.to_xyzi(np.concatenate([far[:20], near, far[20:]], 0)), synth.to_xyzi(tgt)


def test_numpy_fitness_matches_oracle():
    src, tgt, _ = icp_scene(3000, 800, 7)
    T, conv, fit, its = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv and abs(numpy_fitness(src, tgt, T) - fit) <= 1e-6 * max(fit, 1e-3)


@pytest.mark.parametrize("offset", MAP_OFFSETS)
def test_oracle_in_the_map_frame_recovers_the_motion(offset):
    src, tgt, true_pos = moved_scene(3000, 800, 7, offset)
    T, conv, fit, its = O.icp_align(src, tgt, max_corr_dist=30.0)
    assert conv
    err = np.abs(aligned(src, T) - true_pos).max()
    assert err < 0.08, err                   # fp32 coordinates at 1e5 m are 7.8 mm apart
    assert abs(numpy_fitness(src, tgt, T) - fit) <= 0.05 * fit + 1e-4


def test_tie_scene_has_exact_ties_across_tiles():
    src, tgt = tie_scene()
    s, t = src[:, :3], tgt[:, :3]
    d2 = ((s[:, None, 0] - t[None, :, 0]) ** 2 + (s[:, None, 1] - t[None, :, 1]) ** 2) + (s[:, None, 2] - t[None, :, 2]) ** 2
    m = d2.min(1)
    assert np.all(m == np.float32(0.25))
    for i in range(s.shape[0]):
        j = np.flatnonzero(d2[i] == m[i])
        assert len(j) == 2 and j[1] - j[0] == 2048 and t[j[0], 0] == t[j[1], 0] + 1   # the lower index is the x = 2k+1 point
    T, conv, fit, its = O.icp_align(src, tgt, max_corr_dist=30.0, max_iter=1)
    # every source point went to its x = 2k + 1 partner: the first transform moves the centroid by +0.5 m in x
    assert its == 1 and abs(T[0, 3] - 0.5) < 1e-5 and abs(T[1, 3]) < 1e-5


@pytest.mark.parametrize("n_within,conv_expected", [(2, False), (3, True)])
def test_reach_scene_counts_and_boundary(n_within, conv_expected):
    src, tgt = reach_scene(n_within)
    d = np.sqrt(((src[:, None, :3].astype(np.float64) - tgt[None, :, :3]) ** 2).sum(-1)).min(1)
    assert (d <= 0.75).sum() == n_within and (d == 0.75).sum() == 1 and ((d > 0.75) & (d < 2.0)).sum() == 0
    assert np.float32(0.75) * np.float32(0.75) == np.float32(0.5625) and 0.75 * 0.75 == 0.5625
    T, conv, fit, its = O.icp_align(src, tgt, max_corr_dist=0.75)
    assert conv == conv_expected and (its > 0) == conv_expected
    T2, conv2, _, _ = O.icp_align(src, tgt, max_corr_dist=np.nextafter(0.75, 0.0))
    assert not conv2                                              # one ulp less and the boundary pair is gone
