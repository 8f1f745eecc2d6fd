"""GPU tests of imageProjection's point filter and IMU deskew (s2m_project_scan and the two calls that read its resident
result). Everything is compared bit for bit with the C restatement of the reference (tests/ref/project_ref.c, pinned against
an independent numpy statement by tests/test_project_cpu.py on these same cases); a NaN coordinate matches any NaN, because
an x86 host and the device propagate different NaN payloads (tests/ref/project_ref.py::same_cloud)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
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


def project(g, case, out_stride=32, cap=None, device_ptr=None):
    """s2m_project_scan on a case: (rc, n_out, out as (cap, out_stride / 4) float32)."""
    lay = s2m.ScanLayout(*case["layout"])
    prm = s2m.ProjectParams(**case["params"])
    dk = case["deskew"]
    d = s2m.make_deskew_info(dk["time_scan_cur"], dk["deskew"], dk["imu_pointer_cur"], *dk["tables"])
    n = case["raw"].size // lay.stride
    if cap is None:
        cap = (n + prm.point_filter_num - 1) // prm.point_filter_num
    out = np.full((max(cap, 1), out_stride // 4), 7.0, np.float32)
    m = C.c_size_t(0)
    src = C.c_void_p(device_ptr) if device_ptr is not None else case["raw"].ctypes.data
    rc = g.lib.s2m_project_scan(g.h, src, n, C.byref(lay), 1 if device_ptr is not None else 0, C.byref(prm), C.byref(d),
                                out.ctypes.data if cap else None, out_stride, cap, C.byref(m))
    g.cloudDeskewedNum = m.value                      # what ImageProjectionS2M.projectPointCloud() records on the mapper
    return rc, m.value, out


@pytest.mark.parametrize("name", list(PR.CASES))
def test_project_scan_is_the_c_restatement(gpu, name):
    case = PR.get_case(name)
    want = PR.c_project(case)
    rc, m, out = project(gpu, case)
    assert rc == 0, gpu.lib.s2m_last_error(gpu.h)
    assert m == want.shape[0]
    assert PR.same_cloud(out[:m], want), name
    if name.startswith("filter_") or name == "first_record_filtered":
        n = case["raw"].size // case["layout"][0]
        assert m < (n + case["params"]["point_filter_num"] - 1) // case["params"]["point_filter_num"] or name == "filter_point_num"


def test_before_any_projection_there_is_no_scan():
    g = s2m.MapOptimizationS2M()
    m = C.c_size_t(0)
    assert g.lib.s2m_downsample_projected(g.h, 0.4, None, 32, 0, C.byref(m)) == -4
    assert g.lib.s2m_sc_add_projected(g.h) == -4
    g.close()


def test_device_input_strides_short_buffer_and_repeat(gpu):
    import torch
    for name in ("layout_ouster", "layout_custom40", "size_4097"):
        case = PR.get_case(name)
        want = PR.c_project(case)
        rc, m, out = project(gpu, case)
        assert rc == 0 and PR.same_cloud(out[:m], want)
        # two runs give identical bytes
        rc2, m2, out2 = project(gpu, case)
        assert rc2 == 0 and m2 == m and np.array_equal(_bits(out[:m]), _bits(out2[:m2]))
        # device input
        d_raw = torch.from_numpy(case["raw"]).cuda()
        rc3, m3, out3 = project(gpu, case, device_ptr=d_raw.data_ptr())
        assert rc3 == 0 and m3 == m and np.array_equal(_bits(out[:m]), _bits(out3[:m3]))
        # 12-byte output records
        rc4, m4, out4 = project(gpu, case, out_stride=12)
        assert rc4 == 0 and m4 == m and np.array_equal(_bits(out4[:m]), _bits(out[:m, :3]))
        # a short buffer: the count is full, the first records are right, nothing is written behind them
        cap = m // 3
        lay = s2m.ScanLayout(*case["layout"])
        prm = s2m.ProjectParams(**case["params"])
        dk = case["deskew"]
        d = s2m.make_deskew_info(dk["time_scan_cur"], dk["deskew"], dk["imu_pointer_cur"], *dk["tables"])
        out5 = np.full((cap + 64, 8), 7.0, np.float32)            # 64 records of room the call is not told about
        m5 = C.c_size_t(0)
        rc5 = gpu.lib.s2m_project_scan(gpu.h, case["raw"].ctypes.data, case["raw"].size // lay.stride, C.byref(lay), 0, C.byref(prm),
                                       C.byref(d), out5.ctypes.data, 32, cap, C.byref(m5))
        assert rc5 == s2m.S2M_ERR_CAPACITY and m5.value == m and np.array_equal(_bits(out5[:cap]), _bits(out[:cap]))
        assert np.all(out5[cap:] == 7.0)
        # cap == 0: count only, the cloud stays resident
        rc6, m6, _ = project(gpu, case, cap=0)
        assert rc6 == 0 and m6 == m
        got = gpu.downsampleCurrentScanProjected(0.4)
        assert got.shape[0] > 0
    # a misaligned device pointer is refused
    case = PR.get_case("layout_velodyne")
    d_raw = torch.from_numpy(np.concatenate([np.zeros(4, np.uint8), case["raw"]])).cuda()
    rc, _, _ = project(gpu, case, device_ptr=d_raw.data_ptr() + 4)
    assert rc == -1


def _lm_trace(g, pose):
    g.transformTobeMapped = np.array(pose, np.float32)
    r = g.scan2MapOptimization()
    tr = g.trace()
    return (C.string_at(C.addressof(r), C.sizeof(r)), [C.string_at(C.addressof(t), C.sizeof(t)) for t in tr])


def _raw_from_scan(xyz, layout_name="velodyne", n_scan=64, seed=3):
    """A registration-sized lidar-frame scan as raw records with rings, times and a mild rotation table."""
    rng = np.random.default_rng(seed)
    n = xyz.shape[0]
    lay = PR.LAYOUTS[layout_name]
    tabs = PR.make_table(50, rng, rate=0.05)
    time = np.round(np.sort(rng.uniform(0.0, 0.09, n)) * 4096.0) / 4096.0
    raw = PR.make_records(lay, xyz, rng.uniform(0, 100, n).astype(np.float32), rng.integers(0, n_scan, n), time, rng)
    return dict(raw=raw, layout=lay, params=PR.default_params(n_scan=n_scan, point_filter_num=1),
                deskew=dict(deskew=True, time_scan_cur=PR.TIME_SCAN_CUR, imu_pointer_cur=49, tables=tabs))


def test_downsample_projected_is_downsample_scan_of_the_downloaded_cloud(cfg_small):
    case = _raw_from_scan(cfg_small["scan"])
    m_rec = synth.to_xyzi(cfg_small["map"])
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    for g in (a, b):
        g.setInputCloud(m_rec)
    rc, m, cloud = project(a, case)
    assert rc == 0 and m > 10000 and PR.same_cloud(cloud[:m], PR.c_project(case))
    ds_a = a.downsampleCurrentScanProjected(0.4)
    ds_b = b.downsampleCurrentScan(cloud[:m], 0.4)
    assert ds_a.shape == ds_b.shape and np.array_equal(_bits(ds_a), _bits(ds_b))
    assert a.laserCloudSurfLastDSNum == b.laserCloudSurfLastDSNum
    assert _lm_trace(a, cfg_small["pose_init"]) == _lm_trace(b, cfg_small["pose_init"])        # the installed scan and the LM trace
    # scan_ds feeds the key-frame store the same way
    for g in (a, b):
        g.saveKeyFrame(np.zeros(6, np.float32), 1.0)
    assert np.array_equal(_bits(a.globalMapCloud()), _bits(b.globalMapCloud()))
    # the leaf-too-small warning is passed on
    a.downsampleCurrentScanProjected(1e-7, readback=False)
    b.downsampleCurrentScan(cloud[:m], 1e-7, readback=False)
    assert a.leaf_too_small and b.leaf_too_small and a.laserCloudSurfLastDSNum == b.laserCloudSurfLastDSNum == m
    a.close(); b.close()


def test_sc_add_projected_is_sc_add_scan_of_the_downloaded_cloud():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    rng = np.random.default_rng(5)
    for k in range(34):                                       # more than NUM_EXCLUDE_RECENT + 1 keys: the detector searches
        xyz = rng.normal(0, 15.0, (3000, 3)).astype(np.float32) if k not in (0, 33) else \
            np.random.default_rng(99).normal(0, 15.0, (3000, 3)).astype(np.float32)          # key 33 revisits key 0
        case = _raw_from_scan(xyz, "ouster", n_scan=128, seed=k)
        rc, m, cloud = project(a, case)
        assert rc == 0 and m > 2000
        a.makeAndSaveScancontextAndKeysProjected()
        b.makeAndSaveScancontextAndKeys(cloud[:m])
    assert a.scSize() == b.scSize() == 34
    idx = np.arange(34, dtype=np.int32)
    da, sa = a.distanceBtnScanContext(33, idx)
    db, sb = b.distanceBtnScanContext(33, idx)
    assert np.array_equal(da.view(np.uint64), db.view(np.uint64)) and np.array_equal(sa, sb)       # descriptors and sector keys
    la, ya, ma = a.detectLoopClosureID()
    lb, yb, mb = b.detectLoopClosureID()
    assert (la, ya) == (lb, yb) and C.string_at(C.addressof(ma), C.sizeof(ma)) == C.string_at(C.addressof(mb), C.sizeof(mb))   # ring keys
    a.close(); b.close()


def test_projection_leaves_the_rest_of_the_handle_alone(cfg_small):
    """A registration, an s2m_extract_surrounding and an s2m_loop_closure_rs give the same bytes with and without an
    s2m_project_scan in between."""
    from test_loop_closure_cpu import scripted_revisit
    clouds, stored, times, _ = scripted_revisit()
    keys = [(stored[k], float(times[k]), clouds[k]) for k in range(len(clouds))]
    case = PR.get_case("size_131072")

    def run(with_projection):
        g = s2m.MapOptimizationS2M()
        out = []
        g.setInputCloud(synth.to_xyzi(cfg_small["map"]))
        g.setScan(synth.to_xyzi(cfg_small["scan"]))
        if with_projection:
            assert project(g, case)[0] == 0
        out.append(_lm_trace(g, cfg_small["pose_init"]))
        g.kfReset()
        for k, (pose, t, cloud) in enumerate(keys):
            g.saveKeyFrame(pose, t, cloud)
            if with_projection and k % 7 == 3:
                assert project(g, case, cap=0)[0] == 0
        if with_projection:
            assert project(g, case)[0] == 0
        ks, mp = g.extractSurroundingKeyFrames(keys[-1][1], return_map=True)
        out.append((ks.tobytes(), mp.tobytes()))
        if with_projection:
            assert project(g, case, cap=0)[0] == 0
        r = g.performRSLoopClosure(keys[-1][1], s2m.default_loop_params(search_radius=15.0, icp_leaf=0.5))
        assert r.status != s2m.S2M_LOOP_NONE                                                       # a candidate was found
        out.append(C.string_at(C.addressof(r), C.sizeof(r)))
        if with_projection:
            assert project(g, case, cap=0)[0] == 0
        out.append(_lm_trace(g, cfg_small["pose_init"]))
        g.close()
        return out
    assert run(False) == run(True)


def test_harness_project_mode_matches_the_python_mirror(tmp_path):
    scene = synth.make_scene(half=30.0, n_boxes=10)
    scan = synth.make_raw_scan(scene, synth.POSE_GT, "ouster", n_rings=32, n_az=512,
                               angular_velocity=lambda t: np.array([0.1, -0.2, 0.8]), imu_rate=400.0, stamp=12.5, keep_misses=True)
    g = s2m.MapOptimizationS2M()
    proj = s2m.ImageProjectionS2M(g, s2m.S2M_SENSOR_OUSTER, n_scan=32, downsample_rate=1, point_filter_num=2)
    proj.cachePointCloud(scan["raw"], 12.5)
    assert proj.imuDeskewInfo(scan["imu"])
    full = proj.projectPointCloud()
    ds = g.downsampleCurrentScanProjected(0.4)
    g.makeAndSaveScancontextAndKeysProjected()
    # the Python mirror against the C restatement, then the harness against the Python mirror
    case = dict(raw=scan["raw"], layout=PR.LAYOUTS["ouster"], params=PR.default_params(n_scan=32, point_filter_num=2),
                deskew=dict(deskew=True, time_scan_cur=12.5, imu_pointer_cur=proj.imuPointerCur,
                            tables=[proj.imuTime, proj.imuRotX, proj.imuRotY, proj.imuRotZ]))
    assert full.shape[0] > 4000 and PR.same_cloud(full, PR.c_project(case))
    scan["raw"].tofile(tmp_path / "raw.bin")
    np.ascontiguousarray(scan["imu"], np.float64).tofile(tmp_path / "imu.bin")
    txt = subprocess.run([os.path.join(ROOT, "liorf_amd", "host", "s2m_harness"), "--project", str(tmp_path / "raw.bin"), "2", "12.5",
                          str(tmp_path / "imu.bin"), "32", "1", "2", "0.4", str(tmp_path / "out.bin"), str(tmp_path / "ds.bin")],
                         check=True, capture_output=True, text=True).stdout.split()
    vals = dict(zip(txt[::2], txt[1::2]))
    assert float(vals["timeScanEnd"]) == proj.timeScanEnd and int(vals["imuPointerCur"]) == proj.imuPointerCur
    assert int(vals["imuAvailable"]) == 1 and int(vals["fullCloud"]) == full.shape[0]
    assert int(vals["laserCloudSurfLastDSNum"]) == ds.shape[0] and int(vals["sc_size"]) == g.scSize() == 1
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 8)
    assert np.array_equal(_bits(got), _bits(full))
    # laserCloudSurfLastDS of a fresh node (an empty vector before the call) holds the filtered points, not zeros
    got_ds = np.fromfile(tmp_path / "ds.bin", np.float32).reshape(-1, 8)
    assert got_ds.shape[0] == ds.shape[0] > 1000 and np.array_equal(_bits(got_ds), _bits(ds)) and np.any(got_ds[:, :3] != 0)
    g.close()
