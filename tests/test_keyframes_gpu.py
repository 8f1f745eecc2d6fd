"""GPU tests of the resident key-frame store and s2m_extract_surrounding (extractSurroundingKeyFrames(), reference
src/mapOptmization.cpp:1046-1059): the key list equals the numpy restatement (test_keyframes_cpu.select_surrounding), and
the map - with everything registered against it - is bit for bit that of s2m_extract_cloud on the same frames from host memory.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O
from test_keyframes_cpu import BOUNDARY_D, boundary_store, select_surrounding

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    assert a.shape == b.shape
    assert np.array_equal(_bits(a), _bits(b))


def _result_bytes(r):
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
    for k in range(poses.shape[0]):
        g.saveKeyFrame(poses[k], times[k], clouds[k % len(clouds)])


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


# ---- 1. the key list ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,loop", [(1, False), (2, False), (37, False), (3000, False), (20000, True)])
def test_key_list_equals_the_restatement(gpu, n, loop):
    poses, times = _trajectory(n, seed=n, loop=loop)
    rng = np.random.default_rng(1)
    clouds = [_small_cloud(rng) for _ in range(4)]
    gpu.kfReset()
    _fill(gpu, poses, times, clouds)
    assert gpu.kfSize() == n
    if loop:                              # far more candidates than the selection's LDS tile (4 096)
        d = np.linalg.norm(poses[:, :3] - poses[-1, :3], axis=1)
        assert (d < 50).sum() > 4096
    for D in (1.0, 2.0):
        for tc in (times[-1], times[-1] + 3.0, times[-1] + 10.0, times[-1] + 100.0):
            prm = s2m.default_kf_params(density=D, map_leaf=0.5)
            keys = gpu.extractSurroundingKeyFrames(tc, prm)
            want = select_surrounding(poses[:, :3], times, tc, R=50.0, D=D, W=10.0)
            assert keys.tolist() == want, (n, D, tc)


def test_key_list_leaf_too_small_and_small_radius(gpu):
    poses, times = _trajectory(500, seed=9)
    gpu.kfReset()
    _fill(gpu, poses, times, [_small_cloud(np.random.default_rng(2))])
    for R, D in ((50.0, 1e-6), (3.0, 0.5), (1e-3, 1.0)):
        keys = gpu.extractSurroundingKeyFrames(times[-1], s2m.default_kf_params(search_radius=R, density=D, map_leaf=0.5))
        assert keys.tolist() == select_surrounding(poses[:, :3], times, times[-1], R=R, D=D)


# ---- 1b. the rules that set the selection apart, on hand-built stores and one checked to need them ---------------

_NN_FAR = [[9.9, 0.0, 0], [9.9, 0.6, 0], [10.05, 0.3, 0], [0.0, 0, 0]]
HAND = [  # (positions, times, time_cur, R, D, expected key list)
    ([[50.0, 0, 0], [0, 0, 0]], [0, 0], 100.0, 50.0, 1.0, [1]),                        # d2 == R*R exactly: excluded
    ([[float(np.nextafter(F(50), F(0))), 0, 0], [0, 0, 0]], [0, 0], 100.0, 50.0, 1.0, [1, 0]),
    ([[4.0, 5, 5], [6.0, 5, 5], [5.0, 5, 8]], [0, 0, 0], 100.0, 50.0, 10.0, [0]),       # equidistant keys: the lower id
    ([[6.0, 5, 5], [4.0, 5, 5], [5.0, 5, 8]], [0, 0, 0], 100.0, 50.0, 10.0, [0]),
    ([[1.0, 2, 3]], [5.0], 6.0, 50.0, 1.0, [0, 0]),                                      # a recent key chosen twice
    ([[0.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0]], [15.0, 10.0, 12.0], 20.0, 50.0, 1.0, [0, 1, 2, 2]),   # exactly 10.0 s: stop
    (_NN_FAR, [0, 0, 0, 0], 100.0, 10.0, 1.0, [3, 2]),        # nearest key of a centroid is no candidate; (f) at the centroid
    (_NN_FAR, [0, 0, 99.0, 99.0], 100.0, 10.0, 1.0, [3, 2, 3]),   # a recent key beyond R is dropped (tested at its pose)
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_built_stores(gpu, case):
    P, t, tc, R, D, want = HAND[case]
    P = np.asarray(P, F)
    gpu.kfReset()
    cloud = _small_cloud(np.random.default_rng(case))
    for k in range(P.shape[0]):
        gpu.saveKeyFrame(np.r_[P[k], 0, 0, 0].astype(F), t[k], cloud)
    keys = gpu.extractSurroundingKeyFrames(tc, s2m.default_kf_params(search_radius=R, density=D, map_leaf=0.5))
    assert select_surrounding(P, t, tc, R=R, D=D) == want
    assert keys.tolist() == want


def test_boundary_store_needs_the_centroid_filter_and_the_full_nearest_search(gpu):
    P, t = boundary_store()
    right = select_surrounding(P, t, 100.0, D=BOUNDARY_D)
    for v in ("filter_at_key", "nn_among_candidates"):             # the input tells both wrong selections apart
        assert select_surrounding(P, t, 100.0, D=BOUNDARY_D, variant=v) != right
    gpu.kfReset()
    cloud = _small_cloud(np.random.default_rng(3))
    for k in range(P.shape[0]):
        gpu.saveKeyFrame(np.r_[P[k], 0, 0, 0].astype(F), t[k], cloud)
    keys = gpu.extractSurroundingKeyFrames(100.0, s2m.default_kf_params(density=BOUNDARY_D, map_leaf=0.5))
    assert keys.tolist() == right
    far = [k for k in keys.tolist() if np.linalg.norm(P[k]) > 50.0]
    assert far                                                     # keys beyond R reached the map through their centroid


# ---- 2. the map and what is registered against it --------------------------------------------------------

def _map_frames(cfg, n_frames, seed):
    """Key frames cut from the tiny configuration's map: frame k holds every n_frames-th point minus its key position."""
    rng = np.random.default_rng(seed)
    m = synth.to_xyzi(cfg["map"])
    m[:, 4] = rng.uniform(0, 100, m.shape[0]).astype(F)
    pos = (rng.normal(0, 3.0, (n_frames, 3))).astype(F)
    poses = np.c_[pos, np.zeros((n_frames, 3), F)].astype(F)
    frames = []
    for k in range(n_frames):
        f = m[k::n_frames].copy()
        f[:, :3] = (f[:, :3] - pos[k]).astype(F)
        frames.append(f)
    return frames, poses, np.arange(n_frames, dtype=np.float64)


def test_map_bits_and_registration_equal_extract_cloud(cfg_tiny):
    frames, poses, times = _map_frames(cfg_tiny, 12, seed=4)
    prm = s2m.default_kf_params(density=2.0, map_leaf=0.4)
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for k in range(len(frames)):
            a.saveKeyFrame(poses[k], times[k], frames[k])
        tc = times[-1] + 4.0
        keys, m_a = a.extractSurroundingKeyFrames(tc, prm, return_map=True)
        want = select_surrounding(poses[:, :3], times, tc, D=2.0)
        assert keys.tolist() == want and len(want) > 3
        m_b = b.extractCloud([frames[k] for k in keys], poses[keys], 0.4)
        _same(m_a, m_b)
        # the oracle directly: transformPointCloud of every frame, concatenated, VoxelGrid
        cat = np.concatenate([O.transform_point_cloud(frames[k], poses[k]) for k in keys])
        m_o, _ = O.voxel_grid(cat, 0.4)
        _same(m_a, m_o)
        scan = synth.to_xyzi(cfg_tiny["scan"])
        for g in (a, b):
            g.setScan(scan)
        for x, y in zip(a.surfOptimization(cfg_tiny["pose_init"]), b.surfOptimization(cfg_tiny["pose_init"])):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
        ra, rb = [], []
        for g, out in ((a, ra), (b, rb)):
            g.transformTobeMapped = cfg_tiny["pose_init"].copy()
            out.append(g.scan2MapOptimization())
        assert ra[0].skipped == 0 and ra[0].iters_run > 0
        assert _result_bytes(ra[0]) == _result_bytes(rb[0])
    finally:
        a.close(); b.close()


# ---- 3. the add sources ------------------------------------------------------------------------------------

def test_last_downsample_host_and_device_sources_give_the_same_map(cfg_tiny):
    import torch
    rng = np.random.default_rng(6)
    raws = [synth.to_xyzi((synth.to_xyzi(cfg_tiny["map"])[k::5, :3] + rng.normal(0, 0.01, 3)).astype(F)) for k in range(5)]
    poses = np.c_[rng.normal(0, 2, (5, 3)), rng.normal(0, 0.05, (5, 3))].astype(F)
    prm = s2m.default_kf_params(map_leaf=0.4)
    g = [s2m.MapOptimizationS2M() for _ in range(4)]
    try:
        keep = []
        for k in range(5):
            g[0].downsampleCurrentScan(raws[k], 0.3, readback=False)
            g[0].saveKeyFrame(poses[k], float(k))                                  # S2M_KF_FROM_LAST_DOWNSAMPLE
            ds = g[1].downsampleCurrentScan(raws[k], 0.3)
            g[1].saveKeyFrame(poses[k], float(k), ds)                              # S2M_KF_FROM_HOST, the returned copy
            t12 = torch.from_numpy(np.ascontiguousarray(raws[k][:, :3])).cuda()    # stride 12
            t32 = torch.from_numpy(raws[k]).cuda()                                  # stride 32
            keep += [t12, t32]
            torch.cuda.synchronize()
            g[2].saveKeyFrame(poses[k], float(k), device_ptr=(t12.data_ptr(), t12.shape[0], 12))
            g[3].saveKeyFrame(poses[k], float(k), device_ptr=(t32.data_ptr(), t32.shape[0], 32))
        k0, m0 = g[0].extractSurroundingKeyFrames(4.5, prm, return_map=True)
        k1, m1 = g[1].extractSurroundingKeyFrames(4.5, prm, return_map=True)
        assert np.array_equal(k0, k1) and m0.shape[0] > 0
        _same(m0, m1)
        # the device sources against the same records from host memory (stride 12: intensity reads as 0)
        h = s2m.MapOptimizationS2M()
        try:
            for gi, st in ((2, 12), (3, 32)):
                kd, md = g[gi].extractSurroundingKeyFrames(4.5, prm, return_map=True)
                src = [np.ascontiguousarray(raws[k][:, :3]) if st == 12 else raws[k] for k in kd]
                _same(md, h.extractCloud(src, poses[kd], 0.4))
        finally:
            h.close()
    finally:
        for x in g:
            x.close()


# ---- 4. pose updates ---------------------------------------------------------------------------------------

def test_correct_poses_leaves_no_stale_transform(cfg_tiny):
    frames, poses, times = _map_frames(cfg_tiny, 8, seed=8)
    prm = s2m.default_kf_params(map_leaf=0.4)
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for k in range(8):
            a.saveKeyFrame(poses[k], times[k], frames[k])
        a.extractSurroundingKeyFrames(times[-1], prm)
        new = poses.copy()
        rng = np.random.default_rng(3)
        new[2:7, :3] += rng.normal(0, 0.3, (5, 3)).astype(F)
        new[2:7, 3:] += rng.normal(0, 0.02, (5, 3)).astype(F)
        a.correctPoses(new[2:7], first=2)
        keys, m_a = a.extractSurroundingKeyFrames(times[-1], prm, return_map=True)
        assert keys.tolist() == select_surrounding(new[:, :3], times, times[-1])
        _same(m_a, b.extractCloud([frames[k] for k in keys], new[keys], 0.4))
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
            a.correctPoses(new[:3], first=6)                       # 6 .. 8 is outside [0, 8)
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
            a.correctPoses(new[:1], first=-1)
        bad = new[:1].copy(); bad[0, 4] = np.nan
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
            a.correctPoses(bad, first=0)
    finally:
        a.close(); b.close()


# ---- 5. edges ----------------------------------------------------------------------------------------------

def test_empty_store_leaves_the_map_alone(cfg_tiny):
    g = s2m.MapOptimizationS2M()
    try:
        assert g.kfSize() == 0
        assert g.extractSurroundingKeyFrames(10.0).tolist() == []
        assert g.laserCloudSurfFromMapDSNum == 0
        g.setScan(synth.to_xyzi(cfg_tiny["scan"]))
        g.transformTobeMapped = cfg_tiny["pose_init"].copy()
        assert g.scan2MapOptimization().skipped == 1             # a fresh handle: still no map
        g.setInputCloud(synth.to_xyzi(cfg_tiny["map"]))
        before = g.surfOptimization(cfg_tiny["pose_init"])
        assert g.extractSurroundingKeyFrames(10.0).tolist() == []
        after = g.surfOptimization(cfg_tiny["pose_init"])
        gated = before[0][:, 0] >= 0                              # (d2_5 is defined for gated queries only)
        assert gated.any() and np.array_equal(before[0], after[0])
        assert np.array_equal(before[1][gated], after[1][gated])
        assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    finally:
        g.close()


def test_capacity_rejections_and_sources(cfg_tiny):
    frames, poses, times = _map_frames(cfg_tiny, 6, seed=2)
    g = s2m.MapOptimizationS2M()
    L = g.lib
    try:
        pose = np.zeros(6, F)
        assert L.s2m_kf_add(g.h, s2m._fp(pose), 0.0, None, 0, 32, s2m.S2M_KF_FROM_LAST_DOWNSAMPLE) == -4   # S2M_ERR_NO_SCAN
        assert L.s2m_kf_add(g.h, s2m._fp(pose), 0.0, None, 0, 32, 7) == -1
        bad = pose.copy(); bad[5] = np.inf
        a = frames[0]
        assert L.s2m_kf_add(g.h, s2m._fp(bad), 0.0, a.ctypes.data, a.shape[0], 32, 0) == -1
        assert L.s2m_kf_add(g.h, s2m._fp(pose), float("nan"), a.ctypes.data, a.shape[0], 32, 0) == -1
        assert L.s2m_kf_add(g.h, s2m._fp(pose), 0.0, a.ctypes.data, a.shape[0], 10, 0) == -1
        assert g.kfSize() == 0                                    # failed adds leave the store as it was
        for k in range(6):
            g.saveKeyFrame(poses[k], times[k], frames[k])
        prm = s2m.default_kf_params(map_leaf=0.4)
        keys = g.extractSurroundingKeyFrames(times[-1], prm)
        n_map = g.laserCloudSurfFromMapDSNum
        n_out, n_keys = C.c_size_t(0), C.c_size_t(0)
        kbuf = np.zeros(1, np.int32)
        out = np.zeros((4, 8), F)
        rc = L.s2m_extract_surrounding(g.h, float(times[-1]), C.byref(prm), out.ctypes.data, 32, 4, C.byref(n_out),
                                       kbuf.ctypes.data_as(C.POINTER(C.c_int32)), 1, C.byref(n_keys))
        assert rc == -5 and n_out.value == n_map and n_keys.value == len(keys) > 1 and kbuf[0] == keys[0]
        rc = L.s2m_extract_surrounding(g.h, float(times[-1]), C.byref(prm), None, 32, 0, C.byref(n_out),
                                       kbuf.ctypes.data_as(C.POINTER(C.c_int32)), 1, C.byref(n_keys))
        assert rc == -5 and n_keys.value == len(keys)
        bad_prm = s2m.default_kf_params(search_radius=-1.0)
        assert L.s2m_extract_surrounding(g.h, 0.0, C.byref(bad_prm), None, 32, 0, C.byref(n_out), None, 0, None) == -1
    finally:
        g.close()


def test_store_spanning_several_arena_blocks():
    # 5 key frames of 900 000 records: 144 MB, three 64 MiB blocks; the early frames must still read correctly
    rng = np.random.default_rng(12)
    frames = [synth.to_xyzi(rng.uniform(-40, 40, (900_000, 3)).astype(F)) for _ in range(5)]
    poses = np.c_[rng.normal(0, 1, (5, 3)), rng.normal(0, 0.02, (5, 3))].astype(F)
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for k in range(5):
            a.saveKeyFrame(poses[k], float(k), frames[k])
        prm = s2m.default_kf_params(map_leaf=1.0)
        keys, m_a = a.extractSurroundingKeyFrames(4.0, prm, return_map=True)
        assert sorted(set(keys.tolist())) == [0, 1, 2, 3, 4]
        _same(m_a, b.extractCloud([frames[k] for k in keys], poses[keys], 1.0))
    finally:
        a.close(); b.close()


# ---- 6. the handler loop -----------------------------------------------------------------------------------

def _scans(n=20, pts=6000):
    scene = synth.make_scene(seed=11, half=70.0, n_boxes=92)
    out = []
    for i in range(n):
        gt = np.array([0.0, 0.0, 0.03 * i, 1.5 * i - 15.0, 0.4 * np.sin(0.3 * i), 0.0])
        out.append((synth.to_xyzi(synth.make_scan(scene, gt, "velodyne64", pts, seed=200 + i)), synth.pose_init_from(gt.astype(F)),
                    1.5 * i))
    return out


def _xyzrpy(rpyxyz):
    p = np.asarray(rpyxyz, F)
    return np.r_[p[3:], p[:3]].astype(F)


def test_handler_loop_matches_host_frames_with_the_restated_selection(tmp_path):
    prm = s2m.default_kf_params(density=2.0, map_leaf=0.5)
    scans = _scans()
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    frames, kposes, ktimes, poses_a = [], [], [], []
    try:
        for raw, guess, t in scans:
            keys = a.extractSurroundingKeyFrames(t, prm)
            a.downsampleCurrentScan(raw, 0.4, readback=False)
            a.transformTobeMapped = guess.copy()
            ra = a.scan2MapOptimization()
            a.saveKeyFrame(_xyzrpy(ra.pose), t)
            poses_a.append(np.array(ra.pose, F))

            if kposes:
                P = np.stack(kposes)
                want = select_surrounding(P[:, :3], ktimes, t, D=2.0)
                assert keys.tolist() == want
                b.extractCloud([frames[k] for k in want], P[want], 0.5)
            ds = b.downsampleCurrentScan(raw, 0.4)
            b.transformTobeMapped = guess.copy()
            rb = b.scan2MapOptimization()
            assert _result_bytes(ra) == _result_bytes(rb)
            frames.append(ds); kposes.append(_xyzrpy(rb.pose)); ktimes.append(t)
        assert sum(1 for p in poses_a[1:] if np.any(p != 0)) == len(scans) - 1
    finally:
        a.close(); b.close()
    # the C++ mirror through the harness prints the same poses
    harness = os.path.join(ROOT, "liorf_amd", "host", "s2m_harness")
    np.concatenate([r for r, _, _ in scans]).astype(F).tofile(tmp_path / "scans.bin")
    with open(tmp_path / "scans.txt", "w") as f:
        for raw, guess, t in scans:
            f.write(f"{raw.shape[0]} {t!r} " + " ".join("%.9g" % float(v) for v in np.asarray(guess, F)) + "\n")
    txt = subprocess.run([harness, "--keyframes", str(tmp_path / "scans.bin"), str(tmp_path / "scans.txt"), "0.5", "0.4", "2.0"],
                         capture_output=True, text=True, timeout=300, check=True).stdout
    got = [np.array([float(v) for v in ln.split()[2:8]], F) for ln in txt.splitlines() if ln.startswith("pose ")]
    assert len(got) == len(scans)
    for p, q in zip(got, poses_a):
        assert np.array_equal(_bits(p), _bits(q))


# ---- 7. reproducibility ------------------------------------------------------------------------------------

def test_two_handles_give_identical_bits(cfg_tiny):
    frames, poses, times = _map_frames(cfg_tiny, 10, seed=21)
    out = []
    for _ in range(2):
        g = s2m.MapOptimizationS2M()
        try:
            for k in range(10):
                g.saveKeyFrame(poses[k], times[k], frames[k])
            out.append(g.extractSurroundingKeyFrames(times[-1] + 2.0, s2m.default_kf_params(map_leaf=0.3), return_map=True))
        finally:
            g.close()
    assert np.array_equal(out[0][0], out[1][0])
    _same(out[0][1], out[1][1])
