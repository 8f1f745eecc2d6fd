"""CPU tests of odomDeskewInfo(), the positional-deskew argument check and updateInitialGuess() (s2m_odom_deskew_info,
s2m_project_check_args_motion, s2m_guess_state_init, s2m_update_initial_guess: host code of the library, no handle, no GPU),
every output bit against the C restatement of the reference (tests/ref/front_end_odom_ref.c), and of the two checkers
against each other - the C restatement and the independent numpy statement - on the cases the GPU tests run."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import front_end_odom_ref as FR  # noqa: E402
import project_ref as PR  # noqa: E402


def _lib_odom(q, cur, end, rate):
    r = s2m.odom_deskew_info(q, cur, end, rate)
    return dict(odom_available=r.odom_available, odom_deskew_flag=r.odom_deskew_flag, initial_guess=np.array(r.initial_guess, np.float32),
                odom_incre=np.array(r.odom_incre, np.float32), n_popped=r.n_popped)


def test_the_library_exports_the_new_symbols_and_the_structs_have_the_c_sizes():
    lib = s2m.load_library()
    for name in ("s2m_odom_deskew_info", "s2m_project_scan_motion", "s2m_update_initial_guess", "s2m_project_check_args_motion",
                 "s2m_guess_state_init"):
        assert hasattr(lib, name) and name in s2m.ABI_SYMBOLS
    # the C sizes: 9 doubles; 2 + 6 + 3 + 1 four-byte members; int32, padding, double, 3 floats, padding; 25 four-byte
    # members; 2 int64 + 9 floats, padded to 8
    assert C.sizeof(s2m.OdomSample) == 72 and C.sizeof(s2m.OdomDeskew) == 48 and C.sizeof(s2m.MotionInfo) == 32
    assert C.sizeof(s2m.GuessState) == 100 and C.sizeof(s2m.GuessInfo) == 56
    assert s2m.MotionInfo.time_scan_end.offset == 8 and s2m.MotionInfo.odom_incre.offset == 16
    assert s2m.GuessInfo.imuRollInit.offset == 16 and s2m.GuessInfo.initialGuess.offset == 28
    # the state init writes exactly the struct: a guard behind it stays
    buf = (C.c_ubyte * 104)(*([0xAB] * 104))
    assert lib.s2m_guess_state_init(C.cast(buf, C.POINTER(s2m.GuessState))) == 0
    assert bytes(buf[:100]) == bytes(100) and bytes(buf[100:]) == b"\xab" * 4
    out = (C.c_ubyte * 52)(*([0xCD] * 52))
    assert lib.s2m_odom_deskew_info(None, 0, 1.0, 2.0, 500.0, C.cast(out, C.POINTER(s2m.OdomDeskew))) == 0
    assert bytes(out[:48]) == bytes(48) and bytes(out[48:]) == b"\xcd" * 4


@pytest.mark.parametrize("name", list(FR.ODOM_CASES))
def test_odom_deskew_info_is_the_c_restatement(name):
    q, cur, end, rate = FR.ODOM_CASES[name]
    want = FR.c_odom_deskew_info(q, cur, end, rate)
    got = _lib_odom(q, cur, end, rate)
    assert FR.same_odom(got, want), (name, got, want)
    assert FR.same_odom(FR.np_odom_deskew_info(q, cur, end, rate), want), name          # the two checkers agree


def test_the_named_odom_cases_take_the_branches_they_are_named_for():
    r = {k: FR.c_odom_deskew_info(*v) for k, v in FR.ODOM_CASES.items() if not k.startswith("random_")}
    assert (r["empty_queue"]["odom_available"], r["empty_queue"]["n_popped"]) == (0, 0)
    assert (r["all_older_than_the_pop_limit"]["odom_available"], r["all_older_than_the_pop_limit"]["n_popped"]) == (0, 20)
    assert (r["front_later_than_cur"]["odom_available"], r["front_later_than_cur"]["n_popped"]) == (0, 0)
    q = FR.ODOM_CASES["none_at_or_after_cur_takes_the_last"][0]
    a = r["none_at_or_after_cur_takes_the_last"]
    assert a["odom_available"] == 1 and a["odom_deskew_flag"] == 0 and a["initial_guess"][0] == np.float32(q[-1, 1])
    assert (r["queue_ends_before_end"]["odom_available"], r["queue_ends_before_end"]["odom_deskew_flag"]) == (1, 0)
    assert (r["cov0_rounding_mismatch"]["odom_available"], r["cov0_rounding_mismatch"]["odom_deskew_flag"]) == (1, 0)
    assert r["cov0_same_after_rounding"]["odom_deskew_flag"] == 1
    assert r["cov0_negative_half"]["odom_deskew_flag"] == 0                            # round(-0.5) = -1, round(-0.49) = 0
    q = FR.ODOM_CASES["stamps_equal_cur_and_end"][0]
    a = r["stamps_equal_cur_and_end"]
    assert a["odom_deskew_flag"] == 1 and a["n_popped"] == 0 and a["initial_guess"][0] == np.float32(q[1, 1])
    # imuRate 299: samples down to cur - 0.20f stay; 300: only those from cur - 0.01f on. The sample stamped cur - 0.01 goes too:
    # the limit is cur - (double)0.01f = cur - 0.00999999977..., which is later than it (samples cur - 0.15 .. cur - 0.01: 15)
    assert r["imu_rate_299"]["n_popped"] == 0 and r["imu_rate_300"]["n_popped"] == 15
    assert r["imu_rate_299"]["odom_deskew_flag"] == r["imu_rate_300"]["odom_deskew_flag"] == 1
    assert r["not_unit_quaternion"]["odom_deskew_flag"] == 1
    unit = FR.c_odom_deskew_info(FR.make_queue(FR.ODOM_CASES["not_unit_quaternion"][0][:, 0], seed=4), FR.CUR, FR.END, 200.0)
    assert np.allclose(r["not_unit_quaternion"]["initial_guess"], unit["initial_guess"], atol=1e-6)        # scaled by 2 / length2, not refused
    g = r["gimbal_branch"]["initial_guess"]
    assert abs(abs(float(g[4])) - math.pi / 2) < 1e-6 and g[5] == 0 and r["gimbal_branch"]["odom_deskew_flag"] == 1
    g = r["gimbal_branch_start_only"]["initial_guess"]
    assert g[4] == np.float32(-math.pi / 2) and g[5] == 0
    inc = r["fast_vehicle"]["odom_incre"]
    assert 2.5 < float(np.linalg.norm(inc)) < 3.6                                      # 30 m/s over the 0.1 s between the two samples
    n_flag = sum(FR.c_odom_deskew_info(*v)["odom_deskew_flag"] for k, v in FR.ODOM_CASES.items() if k.startswith("random_"))
    n_av = sum(FR.c_odom_deskew_info(*v)["odom_available"] for k, v in FR.ODOM_CASES.items() if k.startswith("random_"))
    assert n_flag > 30 and n_av - n_flag > 30 and 300 - n_av > 30                      # the random queues reach every outcome


def test_odom_deskew_info_refuses_bad_arguments():
    lib = s2m.load_library()
    out = s2m.OdomDeskew()
    q = np.ascontiguousarray(FR.make_queue(FR.CUR + 0.01 * np.arange(-3, 20)))
    qp = q.ctypes.data_as(C.POINTER(s2m.OdomSample))
    assert lib.s2m_odom_deskew_info(qp, q.shape[0], FR.CUR, FR.END, 500.0, C.byref(out)) == 0
    assert lib.s2m_odom_deskew_info(None, 3, FR.CUR, FR.END, 500.0, C.byref(out)) == -1
    assert lib.s2m_odom_deskew_info(qp, q.shape[0], FR.CUR, FR.END, 500.0, None) == -1
    assert lib.s2m_odom_deskew_info(qp, q.shape[0], float("nan"), FR.END, 500.0, C.byref(out)) == -1
    assert lib.s2m_odom_deskew_info(qp, q.shape[0], FR.CUR, float("inf"), 500.0, C.byref(out)) == -1


class _LibGuess:
    """The library's updateInitialGuess() with the state the caller owns."""

    def __init__(self):
        self.lib = s2m.load_library()
        self.st = s2m.GuessState()
        assert self.lib.s2m_guess_state_init(C.byref(self.st)) == 0
        self.pose = np.zeros(6, np.float32)

    def step(self, s):
        info = s2m.make_guess_info(s["imuAvailable"], s["odomAvailable"], [float(np.float32(v)) for v in s["imu"]],
                                   [float(np.float32(v)) for v in s["guess"]])
        front = np.zeros(12, np.float32)
        fp = C.POINTER(C.c_float)
        assert self.lib.s2m_update_initial_guess(C.byref(self.st), self.pose.ctypes.data_as(fp), int(s["key_poses_empty"]), C.byref(info),
                                                 int(s["heading"]), int(s["imu_type"]), front.ctypes.data_as(fp)) == 0
        return front

    def state(self):
        return (np.array(self.st.last_imu_transformation, np.float32), np.array(self.st.last_imu_pre_transformation, np.float32),
                int(self.st.last_imu_pre_trans_available))


def _same_state(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


@pytest.mark.parametrize("name", list(FR.guess_sequences()))
def test_update_initial_guess_is_the_c_restatement_step_by_step(name):
    seq = FR.guess_sequences()[name]
    got, want, other = _LibGuess(), FR.GuessRun("c"), FR.GuessRun("np")
    moved = 0
    for k, s in enumerate(seq):
        before = want.pose.copy()
        f_got, f_want, f_other = got.step(s), want.step(s), other.step(s)
        assert f_got.tobytes() == f_want.tobytes() == f_other.astype(np.float32).tobytes(), (name, k)
        assert got.pose.tobytes() == want.pose.tobytes() == other.pose.tobytes(), (name, k, got.pose, want.pose, other.pose)
        assert _same_state(got.state(), want.state()) and _same_state(other.state(), want.state()), (name, k)
        moved += int(before.tobytes() != want.pose.tobytes())
    assert np.all(np.isfinite(want.pose))
    if name == "imu_type_0_falls_through_to_no_change":
        # scan 0 sets the pose from the IMU; scan 1 is the first odometry sample: it only arms lastImuPreTransformation, and
        # with imuType 0 the IMU branch it falls through to does nothing; every later scan moves by odometry
        assert moved == len(seq) - 1
    elif name == "first_odometry_falls_through_to_imu":
        assert moved == len(seq)


def test_update_initial_guess_branches():
    seqs = FR.guess_sequences()
    # the heading switch: yaw 0 without it, imuYawInit with it
    for name, yaw_is_zero in (("first_scan_with_heading", False), ("first_scan_without_heading", True)):
        g = _LibGuess()
        s = seqs[name][0]
        g.step(s)
        assert (g.pose[2] == 0) == yaw_is_zero and g.pose[0] == np.float32(s["imu"][0]) and np.all(g.pose[3:] == 0)
        assert g.state()[2] == 0 and np.any(g.state()[0] != 0)
    # the first odometry sample falls through to the IMU branch: the pose moves by the IMU increment, translation stays
    g = _LibGuess()
    seq = seqs["first_odometry_falls_through_to_imu"]
    g.step(seq[0])
    p0 = g.pose.copy()
    g.step(seq[1])
    assert g.state()[2] == 1 and np.all(g.pose[3:] == p0[3:]) and np.any(g.pose[:3] != p0[:3])
    g.step(seq[2])
    assert abs(float(g.pose[3]) - 1.5) < 0.2                                           # then odometry increments: 15 m/s * 0.1 s along x
    # imuAvailable values other than 1 are not `== true`: nothing moves, lastImuTransformation is not refreshed
    g = _LibGuess()
    seq = seqs["imu_available_other_than_1"]
    g.step(seq[0])
    st0, p0 = g.state(), g.pose.copy()
    for s in seq[1:4]:
        g.step(s)
        assert g.pose.tobytes() == p0.tobytes() and _same_state(g.state(), st0)
    g.step(seq[4])
    assert g.pose.tobytes() != p0.tobytes()
    # affine_front is the transform of the pose on entry
    g = _LibGuess()
    g.pose[:] = [0.1, -0.2, 0.3, 1.0, 2.0, 3.0]
    front = g.step(seqs["imu_only"][1]).reshape(3, 4)
    assert front[:, 3].tolist() == [1.0, 2.0, 3.0] and front[2, 0] == -np.float32(math.sin(np.float32(-0.2)))
    # null arguments
    lib = s2m.load_library()
    assert lib.s2m_guess_state_init(None) == -1
    fp = C.POINTER(C.c_float)
    info = s2m.make_guess_info()
    assert lib.s2m_update_initial_guess(None, g.pose.ctypes.data_as(fp), 0, C.byref(info), 0, 0, front.ctypes.data_as(fp)) == -1
    assert lib.s2m_update_initial_guess(C.byref(g.st), None, 0, C.byref(info), 0, 0, front.ctypes.data_as(fp)) == -1
    assert lib.s2m_update_initial_guess(C.byref(g.st), g.pose.ctypes.data_as(fp), 0, None, 0, 0, front.ctypes.data_as(fp)) == -1
    assert lib.s2m_update_initial_guess(C.byref(g.st), g.pose.ctypes.data_as(fp), 0, C.byref(info), 0, 0, None) == -1


def test_project_check_args_motion():
    lib = s2m.load_library()
    case = PR.get_case("layout_velodyne")
    lay, prm = s2m.ScanLayout(*case["layout"]), s2m.ProjectParams(**case["params"])
    dk = case["deskew"]
    d = s2m.make_deskew_info(dk["time_scan_cur"], dk["deskew"], dk["imu_pointer_cur"], *dk["tables"])

    def check(mo, layout=lay, deskew=d):
        return lib.s2m_project_check_args_motion(C.byref(layout), C.byref(prm), C.byref(deskew) if deskew is not None else None,
                                                 C.byref(mo) if mo is not None else None)
    nan, inf = float("nan"), float("inf")
    assert check(None) == 0
    assert check(s2m.make_motion_info(True, 1000.1, (2.9, -0.3, 0.0))) == 0
    assert check(s2m.make_motion_info(True, 1000.1, (0.0, -0.0, 0.0))) == 0
    assert check(s2m.make_motion_info(True, dk["time_scan_cur"], (1.0, 1.0, 1.0))) == 0          # end == cur is not refused
    assert check(s2m.make_motion_info(True, 1000.1, (1.0, 1.0, 1.0)), deskew=None) == 0
    for k in range(3):
        for bad in (nan, inf, -inf):
            inc = [0.5, 0.5, 0.5]
            inc[k] = bad
            assert check(s2m.make_motion_info(True, 1000.1, inc)) == -1
            assert check(s2m.make_motion_info(False, 1000.1, inc)) == 0                            # a disabled motion is not read
    for bad in (nan, inf, -inf):
        assert check(s2m.make_motion_info(True, bad, (1.0, 1.0, 1.0))) == -1
        assert check(s2m.make_motion_info(False, bad, (1.0, 1.0, 1.0))) == 0
    # everything s2m_project_check_args refuses is refused here too, and the two agree without motion
    bad_lay = s2m.ScanLayout(*case["layout"])
    bad_lay.off_time = 30
    assert check(s2m.make_motion_info(True, 1000.1, (1.0, 1.0, 1.0)), layout=bad_lay) == -1
    assert lib.s2m_project_check_args(C.byref(bad_lay), C.byref(prm), C.byref(d)) == -1
    tabs = [np.array(t, np.float64) for t in dk["tables"]]
    tabs[0][3] = tabs[0][2] - 1.0
    bad_d = s2m.make_deskew_info(dk["time_scan_cur"], True, dk["imu_pointer_cur"], *tabs)
    assert check(None, deskew=bad_d) == -1 and check(s2m.make_motion_info(True, 1000.1, (1.0, 1.0, 1.0)), deskew=bad_d) == -1
    assert lib.s2m_project_check_args_motion(None, C.byref(prm), C.byref(d), None) == -1
    # a refused motion is refused by the call itself before the handle is looked at (no GPU needed for that)
    m = C.c_size_t(0)
    bad = s2m.make_motion_info(True, nan, (1.0, 1.0, 1.0))
    assert lib.s2m_project_scan_motion(None, case["raw"].ctypes.data, 10, C.byref(lay), 0, C.byref(prm), C.byref(d), C.byref(bad), None, 32, 0,
                                       C.byref(m)) == -1


@pytest.mark.parametrize("name", list(FR.MOTION_CASES))
def test_the_two_motion_checkers_agree(name):
    case = FR.get_motion_case(name)
    a, b = FR.c_project_motion(case), FR.np_project_motion(case)
    assert a.shape == b.shape and PR.same_cloud(a, b), name
    mo, dk = case["motion"], case["deskew"]
    plain = PR.c_project(case)
    assert plain.shape == a.shape
    if name == "nothing_survives":
        assert a.shape[0] == 0
    elif not mo["enabled"] or not dk["deskew"]:
        assert np.array_equal(a.view(np.uint32), plain.view(np.uint32))                # motion off, or deskew off: projectPointCloud() as shipped
    elif name == "zero_increments":
        assert np.array_equal(a, plain)                                                # equal as numbers (signs of zero may differ)
    elif name.startswith("end_equals_cur"):
        assert np.isnan(a[:, :3]).any()
    else:
        assert a.shape[0] > 1000 and np.isfinite(a).all()
        d = np.linalg.norm(a[:, :3] - plain[:, :3], axis=1)
        scale = float(np.linalg.norm(mo["odom_incre"]))
        assert 0.3 * scale < d.max() < 1.5 * scale                                     # the sweep is unsmeared by about one increment


def test_motion_first_survivor_has_a_position_of_its_own():
    case = FR.get_motion_case("first_survivor_late")
    raw, stride = case["raw"], case["layout"][0]
    t = np.ascontiguousarray(raw.reshape(-1, stride)[:, 24:28]).view(np.float32).reshape(-1)
    assert t[9] >= np.float32(3 * 2.0 ** -9)                                           # record 9 is the first survivor (rings 0-6 out, i % 3 == 0)
    a = FR.c_project_motion(case)
    x = np.ascontiguousarray(raw.reshape(-1, stride)[9, 0:12]).view(np.float32)
    assert np.allclose(a[0, :3], x, atol=2e-4) and not np.array_equal(a[0, :3], x)     # S * T of the first survivor is the identity up to rounding
