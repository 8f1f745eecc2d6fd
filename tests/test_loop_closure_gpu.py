"""GPU tests of the loop closure against the key-frame store (s2m_loop_*, reference src/mapOptmization.cpp:542-844): the
detection equals the numpy restatement (test_loop_closure_cpu.detect_loop), the submaps are bit for bit the host composition
and the oracle's, the ICP is bit for bit s2m_icp_align on the same submaps, the gates sit where the reference puts them, and
a loop call leaves the registration alone.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O
from test_loop_closure_cpu import (BOUNDARY, detect_loop, expected_loop, near_frames, near_submap, pose_from64,
                                   scripted_revisit)

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KITTI = dict(search_radius=15.0, search_num=25, icp_leaf=0.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    assert a.shape == b.shape
    assert np.array_equal(_bits(a), _bits(b))


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _trajectory(n, seed, loop=False):
    rng = np.random.default_rng(seed)
    if loop:                              # a circle of radius 20 m driven round and round
        a = np.arange(n) * 0.05
        xyz = np.c_[20 * np.cos(a), 20 * np.sin(a), 0.2 * np.sin(3 * a)] + rng.normal(0, 0.3, (n, 3))
    else:
        xyz = np.cumsum(rng.normal(0, 1.2, (n, 3)) * [1, 1, 0.2], 0)
    rpy = rng.normal(0, 0.05, (n, 3))
    return np.c_[xyz, rpy].astype(F), np.arange(n, dtype=np.float64) * 0.7


def _small_cloud(rng, n=16):
    return synth.to_xyzi(rng.uniform(-5, 5, (n, 3)).astype(F))


def _fill(g, poses, times, clouds):
    g.kfReset()
    for k in range(poses.shape[0]):
        g.saveKeyFrame(poses[k], times[k], clouds[k % len(clouds)])


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@pytest.fixture(scope="module")
def revisit():
    return scripted_revisit()


# ---- 1. detection ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,loop", [(1, False), (2, False), (37, False), (37, True), (3000, False), (3000, True), (50000, True)])
def test_detection_equals_the_restatement(gpu, n, loop):
    poses, times = _trajectory(n, seed=n, loop=loop)
    rng = np.random.default_rng(1)
    _fill(gpu, poses, times, [_small_cloud(rng) for _ in range(4)])
    found = 0
    for R in (10.0, 15.0):
        for tc in (times[-1], times[-1] + 12.5, times[0] - 5.0, times[n // 2]):
            r = gpu.performRSLoopClosure(tc, s2m.default_loop_params(search_radius=R))
            want = detect_loop(poses[:, :3], times, tc, R=R, W=30.0)
            assert (r.key_cur, r.key_pre) == want, (n, R, tc)
            assert r.status == (s2m.S2M_LOOP_NONE if want[1] == -1 else s2m.S2M_LOOP_TOO_FEW_POINTS)
            found += want[1] != -1
    if loop and n > 37:
        assert found > 0


@pytest.mark.parametrize("case", range(len(BOUNDARY)))
def test_boundary_stores(gpu, case):
    P, t, tcs = BOUNDARY[case]
    P = np.asarray(P, F)
    cloud = _small_cloud(np.random.default_rng(case))
    gpu.kfReset()
    for k in range(P.shape[0]):
        gpu.saveKeyFrame(np.r_[P[k], 0, 0, 0].astype(F), t[k], cloud)
    for tc in tcs:
        r = gpu.performRSLoopClosure(tc, s2m.default_loop_params())
        assert (r.key_cur, r.key_pre) == detect_loop(P, t, tc), tc


def test_time_window_is_the_double_abs(gpu):
    P = np.asarray([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 0]], F)
    t = [69.5, 99.0, 100.0]                                     # |dt| = W + 0.5 for key 0
    cloud = _small_cloud(np.random.default_rng(3))
    gpu.kfReset()
    for k in range(3):
        gpu.saveKeyFrame(np.r_[P[k], 0, 0, 0].astype(F), t[k], cloud)
    r = gpu.performRSLoopClosure(100.0)
    assert (r.key_cur, r.key_pre) == (2, 0)


# ---- 2. submaps ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,num,loop_index", [(0, 3, -1), (5, 2, -1), (9, 4, -1), (9, 0, -1), (4, 25, -1), (6, 2, 0), (0, 0, 0)])
def test_near_keyframes_bits(gpu, key, num, loop_index):
    rng = np.random.default_rng(key * 7 + num)
    n = 10
    poses = np.c_[rng.normal(0, 3, (n, 3)), rng.normal(0, 0.1, (n, 3))].astype(F)
    clouds = [synth.to_xyzi(rng.uniform(-8, 8, (int(rng.integers(0, 400)), 3)).astype(F)) for _ in range(n)]
    clouds[3] = clouds[3][:0]                                   # an empty key frame
    _fill(gpu, poses, np.arange(n, dtype=np.float64), clouds)
    got = gpu.loopFindNearKeyframes(key, num, loop_index, 0.5)
    # host composition: per-frame s2m_transform_cloud, concatenated, s2m_voxel_downsample
    parts = [gpu.transformPointCloud(clouds[k], poses[p]) for k, p in near_frames(key, num, n, loop_index) if len(clouds[k])]
    host = gpu.voxelGrid(np.concatenate(parts), 0.5) if parts else np.zeros((0, 8), F)
    _same(got, host)
    _same(got, near_submap(clouds, poses, key, num, loop_index, 0.5))


# ---- 3. alignment ---------------------------------------------------------------------------------------

def _fill_revisit(g, rv):
    clouds, poses, times, _ = rv
    g.kfReset()
    for k in range(len(clouds)):
        g.saveKeyFrame(poses[k], times[k], clouds[k])


def _check_against_host_icp(g, r, key_cur, key_pre, base_key, num, R=15.0):
    cur = g.loopFindNearKeyframes(key_cur, 0, base_key, 0.5)
    prev = g.loopFindNearKeyframes(key_pre, num, base_key, 0.5)
    assert (r.n_cur, r.n_prev) == (cur.shape[0], prev.shape[0])
    T, conv, fit, its = g.icpAlign(cur, prev, max_correspondence_distance=float(F(R) * F(2)))
    assert np.array_equal(_bits(np.array(r.icp.T, F)), _bits(T.reshape(-1)))
    assert (bool(r.icp.converged), r.icp.iterations, r.icp.fitness_score) == (conv, its, fit)
    To, convo, fito, itso = O.icp_align(cur, prev, max_corr_dist=float(F(R) * F(2)))
    assert convo == conv and itso == its and np.abs(T - To).max() <= 1e-5 and abs(fit - fito) <= 1e-6
    return T


@pytest.mark.parametrize("num", [2, 25])
def test_rs_alignment_on_a_revisit(gpu, revisit, num):
    clouds, poses, times, true = revisit
    _fill_revisit(gpu, revisit)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=num))
    r = gpu.performRSLoopClosure(times[-1], prm)
    e = expected_loop(clouds, poses, times, times[-1], search_num=num)
    assert (r.status, r.key_cur, r.key_pre, r.n_cur, r.n_prev) == (s2m.S2M_LOOP_ACCEPTED, e["key_cur"], e["key_pre"],
                                                                    e["n_cur"], e["n_prev"])
    T = _check_against_host_icp(gpu, r, r.key_cur, r.key_pre, -1, num)
    assert np.abs(np.array(r.pose_from) - pose_from64(T, poses[r.key_cur])).max() <= 1e-5
    assert np.abs(np.array(r.pose_from) - e["pose_from"]).max() <= 1e-4
    assert np.array_equal(_bits(np.array(r.pose_to, F)), _bits(poses[r.key_pre]))
    assert np.abs(np.array(r.pose_from)[:3] - true[-1, :3]).max() < 0.05
    # the same key again: closed; a reset store forgets it
    r2 = gpu.performRSLoopClosure(times[-1], prm)
    assert (r2.status, r2.key_cur, r2.key_pre) == (s2m.S2M_LOOP_ALREADY_CLOSED, len(clouds) - 1, -1)
    assert gpu.loopAlign(len(clouds) - 1, 0, -1, prm).status == s2m.S2M_LOOP_ALREADY_CLOSED
    _fill_revisit(gpu, revisit)
    assert _bytes(gpu.performRSLoopClosure(times[-1], prm)) == _bytes(r)


def test_sc_alignment_on_a_revisit(gpu, revisit):
    clouds, poses, times, _ = revisit
    n = len(clouds)
    _fill_revisit(gpu, revisit)
    rng = np.random.default_rng(4)
    descs = [rng.uniform(0, 3, (20, 60)) for _ in range(n)]
    descs[-1] = descs[0].copy()                                 # the revisit: key n-1 looks like key 0
    sc = O.SCManager()
    gpu.scReset()
    for d in descs:
        gpu.scAddDescriptor(d)
        sc.add_descriptor(d)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=0))
    r = gpu.performSCLoopClosure(prm)
    pre, _, _ = sc.detectLoopClosureID()
    assert (r.key_cur, r.key_pre) == (n - 1, pre) and pre == 0
    assert r.status == s2m.S2M_LOOP_ACCEPTED
    T = _check_against_host_icp(gpu, r, n - 1, pre, 0, 0)
    assert np.abs(np.array(r.pose_from) - pose_from64(T)).max() <= 1e-5
    assert list(r.pose_to) == [0.0] * 6
    e = expected_loop(clouds, poses, times, times[-1], search_num=0, base_key=0)
    assert (e["n_cur"], e["n_prev"]) == (r.n_cur, r.n_prev)
    assert np.abs(e["T"] - T).max() <= 1e-5 and e["iterations"] == r.icp.iterations


# ---- 4. gates -------------------------------------------------------------------------------------------

def _grid_cloud(m, offset=0.0):
    """m points, one per 0.5 m voxel (spacing 1 m): m voxels after the filter at leaf 0.5."""
    i = np.arange(m)
    xyz = np.c_[i % 40 + 0.25 + offset, (i // 40) % 40 + 0.25, i // 1600 + 0.25].astype(F)
    return synth.to_xyzi(xyz)


@pytest.mark.parametrize("n_cur,n_prev,ok", [(299, 1000, False), (300, 999, False), (300, 1000, True), (299, 999, False)])
def test_size_gate(gpu, n_cur, n_prev, ok):
    gpu.kfReset()
    zero = np.zeros(6, F)
    gpu.saveKeyFrame(zero, 0.0, _grid_cloud(n_prev))
    gpu.saveKeyFrame(zero, 100.0, _grid_cloud(n_cur))
    r = gpu.loopAlign(1, 0, -1, s2m.default_loop_params(search_num=0, icp_leaf=0.5))
    assert (r.n_cur, r.n_prev) == (n_cur, n_prev)
    if ok:
        assert r.status == s2m.S2M_LOOP_ACCEPTED and r.icp.converged and r.icp.fitness_score < 1e-8
    else:
        assert r.status == s2m.S2M_LOOP_TOO_FEW_POINTS and r.icp.iterations == 0


def test_fitness_gate(gpu, revisit):
    clouds, poses, times, _ = revisit
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2, fitness_score=np.inf))
    _fill_revisit(gpu, revisit)
    f = gpu.performRSLoopClosure(times[-1], prm).icp.fitness_score
    assert 0 < f < 0.3
    t = F(f)
    if float(t) < f:
        t = np.nextafter(t, F(np.inf))                          # the least float threshold that the fitness does not exceed
    for thr, status in ((t, s2m.S2M_LOOP_ACCEPTED), (np.nextafter(t, F(0)), s2m.S2M_LOOP_REJECTED)):
        _fill_revisit(gpu, revisit)
        r = gpu.performRSLoopClosure(times[-1], s2m.default_loop_params(**dict(KITTI, search_num=2, fitness_score=float(thr))))
        assert r.icp.fitness_score == f and r.status == status, (thr, f)
    # a rejected pair is not recorded: the next call runs again
    r = gpu.performRSLoopClosure(times[-1], s2m.default_loop_params(**dict(KITTI, search_num=2, fitness_score=float(t))))
    assert r.status == s2m.S2M_LOOP_ACCEPTED


# ---- 5. no interference --------------------------------------------------------------------------------

def test_loop_call_leaves_the_registration_alone(cfg_tiny, revisit):
    clouds, poses, times, _ = revisit
    scan = synth.to_xyzi(cfg_tiny["scan"])
    kf = s2m.default_kf_params(map_leaf=0.4)
    out = []
    for with_loop in (False, True):
        g = s2m.MapOptimizationS2M()
        try:
            _fill_revisit(g, revisit)
            g.extractSurroundingKeyFrames(times[-1] + 1.0, kf)
            ds = g.downsampleCurrentScan(scan, 0.3)
            if with_loop:
                r = g.performRSLoopClosure(times[-1], s2m.default_loop_params(**KITTI))
                assert r.status == s2m.S2M_LOOP_ACCEPTED
                g.loopFindNearKeyframes(3, 4, -1, 0.5)
            g.transformTobeMapped = poses[-1][[3, 4, 5, 0, 1, 2]].copy()
            res = g.scan2MapOptimization()
            tr = b"".join(_bytes(x) for x in g.trace())
            g.saveKeyFrame(poses[-1], times[-1] + 1.0)          # S2M_KF_FROM_LAST_DOWNSAMPLE: the scan downsampled last
            n = g.kfSize()
            sub = g.loopFindNearKeyframes(n - 1, 0, -1, 0.5)
            _same(sub, g.voxelGrid(g.transformPointCloud(ds, poses[-1]), 0.5))
            out.append((_bytes(res), tr, g.transformTobeMapped.tobytes(), _bits(sub).tobytes()))
        finally:
            g.close()
    assert out[0] == out[1]


# ---- 6. the C++ mirror ---------------------------------------------------------------------------------

def test_harness_loop_mode_matches_the_python_mirror(tmp_path):
    clouds, poses, times, _ = scripted_revisit(n=32)
    harness = os.path.join(ROOT, "liorf_amd", "host", "s2m_harness")
    np.concatenate(clouds).astype(F).tofile(tmp_path / "keys.bin")
    with open(tmp_path / "keys.txt", "w") as f:
        for k in range(len(clouds)):
            f.write("%d %.17g %s\n" % (len(clouds[k]), times[k], " ".join("%.9g" % v for v in poses[k])))
    txt = subprocess.run([harness, "--loop", str(tmp_path / "keys.bin"), str(tmp_path / "keys.txt"), "0.3", "15", "2", "0.5", "0.3"],
                         capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
    g = s2m.MapOptimizationS2M()
    want = []
    try:
        prm = s2m.default_loop_params(search_radius=15.0, search_num=2, icp_leaf=0.5)
        for k in range(len(clouds)):
            ds = g.downsampleCurrentScan(clouds[k], 0.3)
            g.saveKeyFrame(poses[k], times[k])
            g.makeAndSaveScancontextAndKeys(ds)
            for what, r in (("rs", g.performRSLoopClosure(times[k], prm)), ("sc", g.performSCLoopClosure(prm))):
                want.append("%s %d status %d keys %d %d n %d %d iters %d converged %d fitness %.17g pose_from %s pose_to %s" % (
                    what, k, r.status, r.key_cur, r.key_pre, r.n_cur, r.n_prev, r.icp.iterations, r.icp.converged,
                    r.icp.fitness_score, " ".join("%.9g" % v for v in r.pose_from), " ".join("%.9g" % v for v in r.pose_to)))
        want.append("near %d" % g.loopFindNearKeyframes(len(clouds) - 1, 2, -1, 0.5).shape[0])
    finally:
        g.close()
    assert [s for s in txt if s] == want
    assert any(s.startswith("rs 31 status 4") for s in want)


# ---- 7. errors -----------------------------------------------------------------------------------------

def test_errors_and_empty_store(gpu):
    gpu.kfReset()
    r = gpu.performRSLoopClosure(5.0)
    assert (r.status, r.key_cur, r.key_pre) == (s2m.S2M_LOOP_NONE, -1, -1)
    assert gpu.loopAlign(0, 0).status == s2m.S2M_LOOP_NONE
    assert gpu.loopFindNearKeyframes(0, 3).shape == (0, 8)
    cloud = _small_cloud(np.random.default_rng(0), 50)
    for k in range(4):
        gpu.saveKeyFrame(np.array([k, 0, 0, 0, 0, 0], F), float(k), cloud)
    bad = [lambda: gpu.loopAlign(4, 0), lambda: gpu.loopAlign(0, -1), lambda: gpu.loopAlign(1, 0, 4),
           lambda: gpu.loopAlign(1, 0, -2), lambda: gpu.loopFindNearKeyframes(4, 1), lambda: gpu.loopFindNearKeyframes(1, -1),
           lambda: gpu.loopFindNearKeyframes(1, 1, 7), lambda: gpu.loopFindNearKeyframes(1, 1, -1, 0.0),
           lambda: gpu.loopFindNearKeyframes(1, 1, -1, float("nan")),
           lambda: gpu.performRSLoopClosure(1.0, s2m.default_loop_params(search_num=-1)),
           lambda: gpu.performRSLoopClosure(1.0, s2m.default_loop_params(search_radius=0.0)),
           lambda: gpu.performRSLoopClosure(1.0, s2m.default_loop_params(icp_leaf=-1.0)),
           lambda: gpu.performRSLoopClosure(float("inf"))]
    for f in bad:
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
            f()
    # a short output buffer: cap records written, S2M_ERR_CAPACITY, the full count reported
    full = gpu.loopFindNearKeyframes(1, 2, -1, 0.5)
    assert full.shape[0] > 3
    out = np.full((3, 8), -7.0, F)
    m = C.c_size_t(0)
    rc = gpu.lib.s2m_loop_near_keyframes(gpu.h, 1, 2, -1, 0.5, out.ctypes.data, 32, 2, C.byref(m))
    assert rc == s2m.S2M_ERR_CAPACITY and m.value == full.shape[0]
    _same(out[:2], full[:2])
    assert (out[2] == -7.0).all()
