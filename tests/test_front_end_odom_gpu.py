"""GPU tests of positional deskew (s2m_project_scan_motion: findPosition() with its commented lines live) and of the chain it
completes: raw bytes, IMU and odometry samples in; cloud_deskewed, scan_ds, the initial guess and the registered pose out.
Every cloud is compared bit for bit with the C restatement of the reference (tests/ref/front_end_odom_ref.c, pinned against
an independent numpy statement by tests/test_front_end_odom_cpu.py on these same cases); a NaN coordinate matches any NaN
(tests/ref/project_ref.py::same_cloud). One process, no retries: a GPU step that faults ends the run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import front_end_odom_ref as FR  # noqa: E402
import project_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def project(g, case, motion="case", device_ptr=None, cap=None, plain=False):
    """s2m_project_scan_motion on a case (plain: s2m_project_scan): (rc, n_out, out as (cap, 8) float32). motion: "case" takes
    case["motion"], None passes a null pointer, anything else is an s2m.MotionInfo."""
    lay = s2m.ScanLayout(*case["layout"])
    prm = s2m.ProjectParams(**case["params"])
    dk = case["deskew"]
    d = s2m.make_deskew_info(dk["time_scan_cur"], dk["deskew"], dk["imu_pointer_cur"], *dk["tables"])
    if motion == "case":
        mo = case["motion"]
        motion = s2m.make_motion_info(mo["enabled"], mo["time_scan_end"], mo["odom_incre"])
    n = case["raw"].size // lay.stride
    if cap is None:
        cap = (n + prm.point_filter_num - 1) // prm.point_filter_num
    out = np.full((max(cap, 1), 8), 7.0, np.float32)
    m = C.c_size_t(0)
    src = C.c_void_p(device_ptr) if device_ptr is not None else case["raw"].ctypes.data
    on_dev = 1 if device_ptr is not None else 0
    if plain:
        rc = g.lib.s2m_project_scan(g.h, src, n, C.byref(lay), on_dev, C.byref(prm), C.byref(d), out.ctypes.data if cap else None, 32, cap, C.byref(m))
    else:
        rc = g.lib.s2m_project_scan_motion(g.h, src, n, C.byref(lay), on_dev, C.byref(prm), C.byref(d),
                                           C.byref(motion) if motion is not None else None, out.ctypes.data if cap else None, 32, cap, C.byref(m))
    g.cloudDeskewedNum = m.value
    return rc, m.value, out


@pytest.mark.parametrize("name", list(FR.MOTION_CASES))
def test_project_scan_motion_is_the_c_restatement(gpu, name):
    import torch
    case = FR.get_motion_case(name)
    want = FR.c_project_motion(case)
    rc, m, out = project(gpu, case)
    assert rc == 0, gpu.lib.s2m_last_error(gpu.h)
    assert m == want.shape[0]
    assert PR.same_cloud(out[:m], want), name
    # device input: the same bytes
    d_raw = torch.from_numpy(case["raw"]).cuda()
    rc2, m2, out2 = project(gpu, case, device_ptr=d_raw.data_ptr())
    assert rc2 == 0 and m2 == m and PR.same_cloud(out2[:m2], want)
    assert np.array_equal(_bits(out[:m]), _bits(out2[:m2]))
    if name not in ("nothing_survives",):
        assert m > 1000
    # the resident cloud_deskewed and its count are those of the call: the filter of it is the filter of the checker's cloud
    if m > 0 and not np.isnan(want).any():
        ds = gpu.downsampleCurrentScanProjected(0.4)
        ds_want = gpu.downsampleCurrentScan(want, 0.4)
        assert ds.shape == ds_want.shape and np.array_equal(_bits(ds), _bits(ds_want))


def test_without_motion_the_call_is_project_scan(gpu):
    """motion == NULL and enabled == 0 give the bytes and the count of s2m_project_scan on the same input, the resident cloud
    included; zero increments with enabled != 0 are the checker's (signs of zero may differ from the rotation-only path)."""
    for name in ("velodyne_pfn3_car", "ouster_pfn1_car", "first_survivor_late", "no_deskew_copies", "size_4097_walk"):
        case = FR.get_motion_case(name)
        rc0, m0, out0 = project(gpu, case, plain=True)
        ds0 = gpu.downsampleCurrentScanProjected(0.4)
        assert rc0 == 0 and PR.same_cloud(out0[:m0], PR.c_project(case))
        off = case["motion"]
        for motion in (None, s2m.make_motion_info(False, off["time_scan_end"], off["odom_incre"]),
                       s2m.make_motion_info(False, float("nan"), (float("inf"), 0.0, 0.0))):
            rc, m, out = project(gpu, case, motion=motion)
            assert rc == 0 and m == m0 and np.array_equal(_bits(out), _bits(out0)), name
            ds = gpu.downsampleCurrentScanProjected(0.4)
            assert np.array_equal(_bits(ds), _bits(ds0))
    case = FR.get_motion_case("zero_increments")
    rc, m, out = project(gpu, case)
    rc0, m0, out0 = project(gpu, case, plain=True)
    assert rc == 0 and rc0 == 0 and m == m0
    assert PR.same_cloud(out[:m], FR.c_project_motion(case)) and np.array_equal(out[:m], out0[:m0])       # equal as numbers


def test_refused_motion_and_short_buffer(gpu):
    case = FR.get_motion_case("velodyne_pfn3_car")
    for bad in (s2m.make_motion_info(True, float("nan"), (1.0, 0.0, 0.0)), s2m.make_motion_info(True, 1000.1, (1.0, float("inf"), 0.0)),
                s2m.make_motion_info(True, 1000.1, (1.0, 0.0, float("nan")))):
        rc, m, _ = project(gpu, case, motion=bad)
        assert rc == -1 and m == 0
    want = FR.c_project_motion(case)
    cap = want.shape[0] // 3
    lay, prm, dk, mo = s2m.ScanLayout(*case["layout"]), s2m.ProjectParams(**case["params"]), case["deskew"], case["motion"]
    d = s2m.make_deskew_info(dk["time_scan_cur"], dk["deskew"], dk["imu_pointer_cur"], *dk["tables"])
    motion = s2m.make_motion_info(mo["enabled"], mo["time_scan_end"], mo["odom_incre"])
    out = np.full((cap + 64, 8), 7.0, np.float32)
    m = C.c_size_t(0)
    rc = gpu.lib.s2m_project_scan_motion(gpu.h, case["raw"].ctypes.data, case["raw"].size // lay.stride, C.byref(lay), 0, C.byref(prm), C.byref(d),
                                         C.byref(motion), out.ctypes.data, 32, cap, C.byref(m))
    assert rc == s2m.S2M_ERR_CAPACITY and m.value == want.shape[0] and PR.same_cloud(out[:cap], want[:cap]) and np.all(out[cap:] == 7.0)


def _lm_trace(g):
    r = g.scan2MapOptimization()
    tr = g.trace()
    return (C.string_at(C.addressof(r), C.sizeof(r)), [C.string_at(C.addressof(t), C.sizeof(t)) for t in tr], g.transformTobeMapped.tobytes())


def _raw_from_scan(xyz, n_scan=64, seed=3):
    """A registration-sized lidar-frame scan as raw records with rings, times over a 0.09 s sweep and a mild rotation table."""
    rng = np.random.default_rng(seed)
    n = xyz.shape[0]
    lay = PR.LAYOUTS["velodyne"]
    tabs = PR.make_table(50, rng, rate=0.05)
    time = np.round(np.sort(rng.uniform(0.0, 0.09, n)) * 4096.0) / 4096.0
    raw = PR.make_records(lay, xyz, rng.uniform(0, 100, n).astype(np.float32), rng.integers(0, n_scan, n), time, rng)
    return dict(raw=raw, layout=lay, params=PR.default_params(n_scan=n_scan, point_filter_num=1),
                deskew=dict(deskew=True, time_scan_cur=PR.TIME_SCAN_CUR, imu_pointer_cur=49, tables=tabs))


def test_the_chain_equals_the_host_route_on_the_checkers_cloud_and_guess(cfg_small):
    """raw bytes -> s2m_project_scan_motion -> s2m_downsample_projected -> s2m_update_initial_guess -> s2m_optimize_resident
    against: the checker's cloud through s2m_downsample_scan, the checker's guess, s2m_optimize_resident."""
    m_rec = synth.to_xyzi(cfg_small["map"])
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    ref = FR.GuessRun("c")
    for g in (a, b):
        g.setInputCloud(m_rec)
        g.transformTobeMapped = np.array(cfg_small["pose_init"], np.float32)
    ref.pose = np.array(cfg_small["pose_init"], np.float32)
    grid = FR.CUR - 0.15 + 0.01 * np.arange(60)
    queue = FR.make_queue(grid, seed=11, speed=0.3)
    imu = (0.004, -0.003, 0.02)
    for k in range(3):                                   # scan k: the sweep [cur, cur + 0.1); scan 0 arms lastImuPreTransformation
        cur, end = FR.CUR + 0.1 * k, FR.CUR + 0.1 * k + 0.09
        od = s2m.odom_deskew_info(queue, cur, end, 200.0)
        od_ref = FR.c_odom_deskew_info(queue, cur, end, 200.0)
        assert od.odom_available == 1 and od.odom_deskew_flag == 1
        assert np.array(od.odom_incre, np.float32).tobytes() == od_ref["odom_incre"].tobytes()
        info = s2m.make_guess_info(1, od.odom_available, imu, list(od.initial_guess))
        a.updateInitialGuess(info, key_poses_empty=False)
        front_ref = ref.step(dict(key_poses_empty=0, imuAvailable=1, odomAvailable=od_ref["odom_available"], imu=imu,
                                  guess=od_ref["initial_guess"], heading=0, imu_type=0))
        assert a.transformTobeMapped.tobytes() == ref.pose.tobytes() and a.incrementalOdometryAffineFront.tobytes() == front_ref.tobytes()
    assert not np.array_equal(ref.pose, np.array(cfg_small["pose_init"], np.float32))                    # the guess moved
    case = _raw_from_scan(cfg_small["scan"])
    case["deskew"]["time_scan_cur"] = PR.TIME_SCAN_CUR
    case["motion"] = dict(enabled=1, time_scan_end=PR.TIME_SCAN_CUR + 0.09, odom_incre=tuple(od_ref["odom_incre"]))
    rc, m, _ = project(a, case, cap=0)
    assert rc == 0 and m > 10000
    ds_a = a.downsampleCurrentScanProjected(0.4)
    cloud = FR.c_project_motion(case)
    assert cloud.shape[0] == m and not np.array_equal(_bits(cloud), _bits(PR.c_project(case)))           # the position took part
    ds_b = b.downsampleCurrentScan(cloud, 0.4)
    assert ds_a.shape == ds_b.shape and np.array_equal(_bits(ds_a), _bits(ds_b))
    b.transformTobeMapped = ref.pose.copy()
    ra, rb = _lm_trace(a), _lm_trace(b)
    assert ra == rb
    assert a.last_result.skipped == 0 and a.last_result.iters_run > 0
    a.close(); b.close()


def test_a_motion_call_leaves_the_rest_of_the_handle_alone(cfg_small):
    """The next registration after s2m_project_scan_motion calls is bitwise the one without them."""
    case = FR.get_motion_case("size_131072_car")

    def run(with_motion):
        g = s2m.MapOptimizationS2M()
        g.setInputCloud(synth.to_xyzi(cfg_small["map"]))
        g.setScan(synth.to_xyzi(cfg_small["scan"]))
        out = []
        for _ in range(2):
            if with_motion:
                assert project(g, case, cap=0)[0] == 0
                assert project(g, case)[0] == 0
            g.transformTobeMapped = np.array(cfg_small["pose_init"], np.float32)
            out.append(_lm_trace(g))
        g.close()
        return out
    assert run(False) == run(True)


def test_harness_front_end_mode_matches_the_python_mirror(tmp_path):
    stamp = FR.CUR
    scene = synth.make_scene(half=30.0, n_boxes=10)
    scan = synth.make_raw_scan(scene, synth.POSE_GT, "ouster", n_rings=32, n_az=512,
                               angular_velocity=lambda t: np.array([0.1, -0.2, 0.8]), imu_rate=400.0, stamp=stamp, keep_misses=True)
    queue = FR.make_queue(stamp - 0.3 + 0.01 * np.arange(60), seed=21, speed=25.0)
    g = s2m.MapOptimizationS2M(imu_type=1)
    proj = s2m.ImageProjectionS2M(g, s2m.S2M_SENSOR_OUSTER, n_scan=32, downsample_rate=1, point_filter_num=2)
    proj.positionalDeskew = True
    proj.imuRate = 400.0
    proj.cachePointCloud(scan["raw"], stamp)
    assert proj.imuDeskewInfo(scan["imu"])
    assert proj.odomDeskewInfo(queue) and proj.odomDeskewFlag
    full = proj.projectPointCloud()
    ds = g.downsampleCurrentScanProjected(0.4)
    # the Python mirror against the checker
    want_od = FR.c_odom_deskew_info(queue, proj.timeScanCur, proj.timeScanEnd, 400.0)
    assert proj.odomIncre.tobytes() == want_od["odom_incre"].tobytes() and proj.initialGuess.tobytes() == want_od["initial_guess"].tobytes()
    assert proj.odomQueue.shape[0] == queue.shape[0] - want_od["n_popped"] and want_od["n_popped"] > 0
    case = dict(raw=scan["raw"], layout=PR.LAYOUTS["ouster"], params=PR.default_params(n_scan=32, point_filter_num=2),
                deskew=dict(deskew=True, time_scan_cur=stamp, imu_pointer_cur=proj.imuPointerCur,
                            tables=[proj.imuTime, proj.imuRotX, proj.imuRotY, proj.imuRotZ]),
                motion=dict(enabled=1, time_scan_end=proj.timeScanEnd, odom_incre=tuple(want_od["odom_incre"])))
    assert full.shape[0] > 4000 and PR.same_cloud(full, FR.c_project_motion(case))
    assert not PR.same_cloud(full, PR.c_project(case))
    # the harness against the Python mirror
    scan["raw"].tofile(tmp_path / "raw.bin")
    np.ascontiguousarray(scan["imu"], np.float64).tofile(tmp_path / "imu.bin")
    np.ascontiguousarray(queue, np.float64).tofile(tmp_path / "odom.bin")
    txt = subprocess.run([os.path.join(ROOT, "liorf_amd", "host", "s2m_harness"), "--front-end", str(tmp_path / "raw.bin"), "2", repr(stamp),
                          str(tmp_path / "imu.bin"), str(tmp_path / "odom.bin"), "32", "1", "2", "0.4", "1", "400", str(tmp_path / "out.bin")],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    vals = {ln.split()[0]: ln.split()[1:] for ln in txt.splitlines()}
    line = dict(zip(txt.split()[::1], txt.split()[1::1]))                                # "key value" pairs, keys are unique words
    assert float(line["timeScanEnd"]) == proj.timeScanEnd and int(line["imuPointerCur"]) == proj.imuPointerCur
    assert int(line["odomAvailable"]) == 1 and int(line["odomDeskewFlag"]) == 1 and int(line["queue"]) == proj.odomQueue.shape[0]
    assert [np.float32(v) for v in vals["odomIncre"]] == list(proj.odomIncre)
    assert [np.float32(v) for v in vals["initialGuess"]] == list(proj.initialGuess)
    assert int(line["fullCloud"]) == full.shape[0] and int(line["laserCloudSurfLastDSNum"]) == ds.shape[0]
    assert int(line["checksum"]) == int(_bits(full).astype(np.uint64).sum())
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 8)
    assert np.array_equal(_bits(got), _bits(full))
    # updateInitialGuess(): the harness's three steps on the Python mirror
    imu_init = [np.float32(0.01), np.float32(-0.02), proj.initialGuess[5]]
    guess = proj.initialGuess.copy()
    for step in range(3):
        if step == 2:
            guess[:3] = guess[:3] + proj.odomIncre
            imu_init[2] = imu_init[2] + np.float32(0.005)
        info = s2m.make_guess_info(1, 1, imu_init, guess)
        g.updateInitialGuess(info, key_poses_empty=(step == 0), useImuHeadingInitialization=True)
        assert [np.float32(v) for v in vals["guess%d" % step]] == list(g.transformTobeMapped), step
        assert [np.float32(v) for v in vals["front%d" % step]] == list(g.incrementalOdometryAffineFront.reshape(-1)), step
    assert np.linalg.norm(g.transformTobeMapped[3:]) > 1.0                                  # the third step moved by the odometry increment
    g.close()
