"""CPU checks of imageProjection's point filter and IMU deskew (include/liorf_s2m.h, the s2m_project_* block): the boundary,
the host half (s2m_imu_deskew_info) against the C restatement of the reference, the C restatement against an independent
numpy statement on every case the GPU file runs, and what deskewing means on a synthetic sweep."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import project_ref as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["s2m_scan_layout_preset", "s2m_project_default_params", "s2m_imu_deskew_info", "s2m_project_check_args", "s2m_project_scan",
       "s2m_downsample_projected", "s2m_sc_add_projected"]


def test_header_binding_and_library_agree_on_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liorf_s2m.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(s2m_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(s2m.LIB_PATH)
    for name in NEW:
        assert name in declared and name in s2m.ABI_SYMBOLS and hasattr(lib, name), name


def test_defaults_and_presets_are_the_references():
    p = s2m.default_project_params()                  # include/utility.h:204-209
    assert (p.n_scan, p.downsample_rate, p.point_filter_num, p.lidar_min_range, p.lidar_max_range) == (16, 1, 3, 1.0, 1000.0)
    for name, sensor in PR.SENSOR_ID.items():         # src/imageProjection.cpp:4-57
        lay = s2m.scan_layout_preset(sensor)
        got = (lay.stride, lay.off_x, lay.off_intensity, lay.off_ring, lay.off_time, lay.ring_type, lay.time_type)
        assert got == PR.LAYOUTS[name], name
    with pytest.raises(ValueError):
        s2m.scan_layout_preset(5)
    assert s2m.S2M_IMU_QUEUE_LENGTH == 2000           # queueLength, src/imageProjection.cpp:62


def _check(layout, params=None, deskew=None):
    return s2m.load_library().s2m_project_check_args(C.byref(layout) if layout is not None else None,
                                                     C.byref(params) if params is not None else None,
                                                     C.byref(deskew) if deskew is not None else None)


def test_invalid_arguments_are_rejected_without_a_gpu():
    ok = s2m.scan_layout_preset(s2m.S2M_SENSOR_OUSTER)
    assert _check(ok) == 0 and _check(None) == -1
    for lay in PR.LAYOUTS.values():
        assert _check(s2m.ScanLayout(*lay)) == 0
    bad = [dict(stride=0), dict(off_x=40), dict(off_x=2), dict(off_intensity=46), dict(off_ring=48), dict(off_time=46),
           dict(off_time=22), dict(ring_type=3), dict(time_type=4), dict(time_type=s2m.S2M_TIME_F64_REL, off_time=44),
           dict(time_type=s2m.S2M_TIME_F64_REL, off_time=20), dict(ring_type=s2m.S2M_RING_U16, off_ring=25), dict(stride=46)]
    for kw in bad:
        lay = s2m.scan_layout_preset(s2m.S2M_SENSOR_OUSTER)
        for k, v in kw.items():
            setattr(lay, k, v)
        assert _check(lay) == -1, kw
    for kw in (dict(n_scan=0), dict(downsample_rate=0), dict(point_filter_num=0), dict(point_filter_num=-3),
               dict(lidar_min_range=float("nan")), dict(lidar_max_range=float("inf"))):
        assert _check(ok, s2m.default_project_params(**kw)) == -1, kw
    assert _check(ok, s2m.default_project_params(n_scan=128, downsample_rate=2, point_filter_num=1)) == 0
    t = np.arange(10, dtype=np.float64)
    z = np.zeros(10)
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 9, t, z, z, z)) == 0
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 1, t, z, z, z)) == 0
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 0, t, z, z, z)) == -1
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 2000, np.arange(2001.0), np.zeros(2001), np.zeros(2001), np.zeros(2001))) == -1
    assert _check(ok, None, s2m.make_deskew_info(0.0, False, 0, t, z, z, z)) == 0          # no deskew: the tables are not read
    dec = t.copy(); dec[5] = 3.5
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 9, dec, z, z, z)) == -1
    eq = t.copy(); eq[5] = eq[4]
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 9, eq, z, z, z)) == 0          # non-decreasing is enough
    nan = t.copy(); nan[7] = np.nan
    assert _check(ok, None, s2m.make_deskew_info(0.0, True, 9, nan, z, z, z)) == -1
    # the projection itself refuses them before it looks at the handle
    m = C.c_size_t(7)
    lay = s2m.scan_layout_preset(s2m.S2M_SENSOR_OUSTER); lay.off_time = 46
    assert s2m.load_library().s2m_project_scan(None, None, 0, C.byref(lay), 0, None, None, None, 32, 0, C.byref(m)) == -1
    assert s2m.load_library().s2m_downsample_projected(None, 0.4, None, 32, 0, C.byref(m)) == -1
    assert s2m.load_library().s2m_sc_add_projected(None) == -1


def _imu_stream(rate, t_first, t_last, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(t_first, t_last, 1.0 / rate)
    return np.concatenate([t[:, None], rng.normal(0, 0.5, (t.size, 3))], 1)


IMU_CASES = {
    "500hz": lambda: (_imu_stream(500.0, 99.9905, 100.3, 1), 100.0, 100.1),
    "100hz": lambda: (_imu_stream(100.0, 99.992, 100.3, 2), 100.0, 100.1),
    "starts_after_scan_cur": lambda: (_imu_stream(200.0, 100.03, 100.3, 3), 100.0, 100.1),
    "ends_inside_scan_end": lambda: (_imu_stream(200.0, 99.995, 100.105, 4), 100.0, 100.1),
    "one_sample": lambda: (_imu_stream(200.0, 100.0, 100.004, 5), 100.0, 100.1),
    "all_after_scan_end": lambda: (_imu_stream(200.0, 100.5, 100.6, 6), 100.0, 100.1),
    "no_samples": lambda: (np.zeros((0, 4)), 100.0, 100.1),
    "2000_samples": lambda: (_imu_stream(20000.0, 99.995, 99.995 + 2000 / 20000.0 - 1e-9, 7), 100.0, 100.1),
    "2001_samples": lambda: (_imu_stream(20000.0, 99.995, 99.995 + 2001 / 20000.0 - 1e-9, 8), 100.0, 100.1),
}


@pytest.mark.parametrize("name", list(IMU_CASES))
def test_imu_deskew_info_is_the_c_restatement(name):
    imu, cur, end = IMU_CASES[name]()
    got = s2m.imu_deskew_info(imu, cur, end)
    ref = PR.c_imu_deskew_info(imu, cur, end)
    assert got[0] == ref[0] and got[5:] == ref[5:], (got[0], ref[0], got[5:], ref[5:])
    used = max(ref[5] + 1, 0)
    for a, b in zip(got[1:5], ref[1:5]):
        assert np.array_equal(a[:used].view(np.uint64), b[:used].view(np.uint64))
    if name == "one_sample":
        assert imu.shape[0] == 1 and got[5:] == (0, False)
    if name == "2000_samples":
        assert imu.shape[0] == 2000 and got[0] == 0 and got[5:] == (1999, True)
    if name == "2001_samples":
        assert imu.shape[0] == 2001 and got[0] == s2m.S2M_ERR_CAPACITY
    if name in ("500hz", "100hz"):
        assert got[6] and got[1][got[5]] > end and got[1][0] < cur      # the table brackets the sweep


@pytest.mark.parametrize("name", list(PR.CASES))
def test_c_restatement_is_the_numpy_statement(name):
    case = PR.get_case(name)
    a, b = PR.c_project(case), PR.np_project(case)
    assert a.shape == b.shape and PR.same_cloud(a, b), (a.shape, b.shape)
    lay = case["layout"]
    n = case["raw"].size // lay[0]
    if name == "filter_nothing_survives":
        assert a.shape[0] == 0
    elif n:
        assert 0 < a.shape[0] <= (n + case["params"]["point_filter_num"] - 1) // case["params"]["point_filter_num"]


def test_zero_angular_velocity_returns_the_filtered_input():
    case = PR.get_case("layout_ouster")
    for k in (1, 2, 3):
        case["deskew"]["tables"][k][:] = 0.0
    off = dict(case, deskew=dict(case["deskew"], deskew=False))
    a, b = PR.c_project(case), PR.c_project(off)
    assert a.shape[0] > 1000 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_deskewed_sweep_is_the_scene_from_the_first_pose():
    """A static scene swept by a sensor that only turns about its z axis, seen through the whole chain (synth.make_raw_scan
    -> s2m_imu_deskew_info -> the C restatement) and compared with the scene as seen from the pose of the first survivor.

    Bound, constant rate w = 1 rad/s. The IMU samples are exact, imuDeskewInfo's sums give imuRot(t_k) = w * (t_k - t_0) up
    to double rounding, and findRotation's linear interpolation between samples is exact for a constant rate: the angle it
    returns at a point time is right up to its fp32 rounding (2^-24 * 0.12 rad) and the fp32 rounding of the record's time
    (2^-24 * 0.1 s * w). The transform chain adds about 16 fp32 roundings of entries <= 1 applied to coordinates <= r, and
    the generator's fp32 point has 2 more: |deskewed - truth| < 20 * 2^-24 * r, i.e. 1.2e-4 m at r <= 100 m. The test
    allows 2e-4 m. The IMU sample spacing does not enter for a constant rate.
    Stepped rate (1 rad/s, then 0.4 rad/s from t = 0.05 s on), spacing dt = 1 / imu_rate. imuDeskewInfo integrates with
    the rate of the sample that ENDS an interval (:395-398), so the one interval that straddles the step is integrated with
    the wrong rate for at most dt: an angle error of at most |dw| * dt = 0.6 * dt that stays for the rest of the sweep, and
    a position error of at most r * 0.6 * dt on top of the bound above (0.12 m at 100 m and 500 Hz).
    Without deskew the end of the sweep is off by about w * 0.1 s * r, which the test shows to be > 100 times larger."""
    scene = synth.make_scene(half=30.0, n_boxes=10)
    for rate, profile, slack in ((200.0, lambda t: np.array([0.0, 0.0, 1.0]), 0.0),
                                 (500.0, lambda t: np.array([0.0, 0.0, 1.0 if t < 0.05 else 0.4]), 0.6 / 500.0)):
        scan = synth.make_raw_scan(scene, synth.POSE_GT, "velodyne", n_rings=16, n_az=600, angular_velocity=profile, imu_rate=rate,
                                   stamp=50.0)
        rc, T, RX, RY, RZ, cur, avail = s2m.imu_deskew_info(scan["imu"], scan["time_scan_cur"], scan["time_scan_end"])
        assert rc == 0 and avail
        case = dict(raw=scan["raw"], layout=PR.LAYOUTS["velodyne"], params=PR.default_params(point_filter_num=1),
                    deskew=dict(deskew=True, time_scan_cur=scan["time_scan_cur"], imu_pointer_cur=cur, tables=[T, RX, RY, RZ]))
        p = scan["points"]
        rng_ = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        keep = ~((rng_ < np.float32(1.0)) | (rng_ > np.float32(1000.0)))
        first = int(np.flatnonzero(keep)[0])
        truth = ((scan["world"] - scan["origin"]) @ scan["R_cols"][scan["col"][first]])[keep]
        got = PR.c_project(case)[:, :3].astype(np.float64)
        assert got.shape[0] == int(keep.sum()) > 3000
        r = np.linalg.norm(truth, axis=1)
        err = np.linalg.norm(got - truth, axis=1)
        assert r.max() <= 100.0 and np.all(err <= 2e-4 + r * slack), (float(err.max()), rate)
        raw_err = np.linalg.norm(p[keep].astype(np.float64) - truth, axis=1)
        if slack == 0.0:
            assert raw_err.max() > 100 * err.max()
