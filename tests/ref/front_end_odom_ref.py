"""Checkers of odomDeskewInfo(), positional deskew and the initial pose guess, and the cases the two test files run.

* `lib()` compiles tests/ref/front_end_odom_ref.c (the C restatement of the reference's odomDeskewInfo(), findPosition() with
  its commented lines live inside deskewPoint() / projectPointCloud(), and updateInitialGuess()) with
  `gcc -O2 -ffp-contract=off` into a temporary directory and loads it with ctypes; the `c_*` functions call it.
* the `np_*` functions are an independent statement of the same arithmetic: numpy float32 / float64 scalars and ufuncs (one
  rounding per operation), the host libm through ctypes for the float functions and through `math` for the double ones.
* `ODOM_CASES`, `guess_sequences()` and `MOTION_CASES` are the inputs of tests/test_front_end_odom_cpu.py and
  tests/test_front_end_odom_gpu.py.
"""
import atexit
import ctypes as C
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import project_ref as PR  # noqa: E402

_LIBS = {}
f32 = np.float32


class RefOdomOut(C.Structure):
    _fields_ = [("odomAvailable", C.c_int32), ("odomDeskewFlag", C.c_int32), ("initialGuess", C.c_float * 6),
                ("odomIncre", C.c_float * 3), ("popped", C.c_int32)]


class RefGuessState(C.Structure):
    _fields_ = [("lastImuTransformation", C.c_float * 16), ("lastImuPreTransformation", C.c_float * 16),
                ("lastImuPreTransAvailable", C.c_int)]


class RefCloudInfo(C.Structure):
    _fields_ = [("imuAvailable", C.c_int64), ("odomAvailable", C.c_int64), ("imuRollInit", C.c_float), ("imuPitchInit", C.c_float),
                ("imuYawInit", C.c_float), ("initialGuess", C.c_float * 6)]


def lib(opt: str = "-O2"):
    if opt in _LIBS:
        return _LIBS[opt]
    d = tempfile.mkdtemp(prefix="front_end_odom_ref_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libfront_end_odom_ref.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "front_end_odom_ref.c"), "-lm"])
    L = C.CDLL(so)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.ref_odom_deskew_info.restype = None
    L.ref_odom_deskew_info.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, C.c_float, C.POINTER(RefOdomOut)]
    L.ref_project_motion.restype = C.c_size_t
    L.ref_project_motion.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(PR.RefLayout), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_int, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, C.c_double, fp, C.c_void_p]
    L.ref_guess_state_init.restype = None
    L.ref_guess_state_init.argtypes = [C.POINTER(RefGuessState)]
    L.ref_update_initial_guess.restype = None
    L.ref_update_initial_guess.argtypes = [C.POINTER(RefGuessState), fp, C.c_int, C.POINTER(RefCloudInfo), C.c_int, C.c_int, fp]
    _LIBS[opt] = L
    return L


# ---- libm ------------------------------------------------------------------------------------------------------------
_LIBM = None


def _m():
    global _LIBM
    if _LIBM is None:
        _LIBM = C.CDLL("libm.so.6")
        for n in ("sinf", "cosf", "asinf"):
            f = getattr(_LIBM, n)
            f.restype, f.argtypes = C.c_float, [C.c_float]
        _LIBM.atan2f.restype, _LIBM.atan2f.argtypes = C.c_float, [C.c_float, C.c_float]
    return _LIBM


def _transformation(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation in float: (3, 4) float32."""
    m = _m()
    x, y, z, roll, pitch, yaw = [f32(v) for v in (x, y, z, roll, pitch, yaw)]
    A, B = f32(m.cosf(yaw)), f32(m.sinf(yaw))
    Cc, D = f32(m.cosf(pitch)), f32(m.sinf(pitch))
    E, F = f32(m.cosf(roll)), f32(m.sinf(roll))
    DE, DF = D * E, D * F
    with np.errstate(all="ignore"):
        return np.array([[A * Cc, A * DF - B * E, B * F + A * DE, x],
                         [B * Cc, A * E + B * DF, B * DE - A * F, y],
                         [-D, Cc * F, Cc * E, z]], f32)


def _inverse(T):
    """Eigen's Affine3f::inverse() as the checker assumes it: cofactors, 1 / det from column 0, -(Linv * t)."""
    with np.errstate(all="ignore"):
        def cof(i, j):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            return T[i1, j1] * T[i2, j2] - T[i1, j2] * T[i2, j1]
        det = (cof(0, 0) * T[0, 0] + cof(1, 0) * T[1, 0]) + cof(2, 0) * T[2, 0]
        inv = f32(1.0) / det
        S = np.zeros((3, 4), f32)
        for r in range(3):
            for c in range(3):
                S[r, c] = cof(c, r) * inv
            S[r, 3] = -((S[r, 0] * T[0, 3] + S[r, 1] * T[1, 3]) + S[r, 2] * T[2, 3])
    return S


def _mul_affine(A, B):
    """linear = L * L (three terms), translation = L * t + t."""
    R = np.zeros((3, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                R[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
            R[i, 3] = ((A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3]) + A[i, 2] * B[2, 3]) + A[i, 3]
    return R


def _rpy_of_quaternion(x, y, z, w):
    """tf::Matrix3x3(q).getRPY in double."""
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    m00, m01, m02 = 1.0 - (yy + zz), xy - wz, xz + wy
    m10, m20, m21, m22 = xy + wz, xz - wy, yz + wx, 1.0 - (xx + yy)
    if abs(m20) >= 1:
        if m20 < 0:
            return math.atan2(m01, m02), math.pi / 2.0, 0.0
        return math.atan2(-m01, -m02), -math.pi / 2.0, 0.0
    pitch = -math.asin(m20)
    cp = math.cos(pitch)
    return math.atan2(m21 / cp, m22 / cp), pitch, math.atan2(m10 / cp, m00 / cp)


def _c_round(v):
    """C's round(): half away from zero."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


# ---- odomDeskewInfo() ------------------------------------------------------------------------------------------------
def c_odom_deskew_info(queue, time_scan_cur, time_scan_end, imu_rate, opt="-O2"):
    """queue: (n, 9) float64 {time, px, py, pz, qx, qy, qz, qw, cov0}. Returns the result as a dict of exact values."""
    q = np.ascontiguousarray(queue, np.float64).reshape(-1, 9)
    o = RefOdomOut()
    lib(opt).ref_odom_deskew_info(q.ctypes.data_as(C.POINTER(C.c_double)), q.shape[0], time_scan_cur, time_scan_end, imu_rate, C.byref(o))
    return dict(odom_available=o.odomAvailable, odom_deskew_flag=o.odomDeskewFlag, initial_guess=np.array(o.initialGuess, f32),
                odom_incre=np.array(o.odomIncre, f32), n_popped=o.popped)


def np_odom_deskew_info(queue, time_scan_cur, time_scan_end, imu_rate):
    q = np.asarray(queue, np.float64).reshape(-1, 9)
    out = dict(odom_available=0, odom_deskew_flag=0, initial_guess=np.zeros(6, f32), odom_incre=np.zeros(3, f32), n_popped=0)
    sync = float(f32(0.01) if f32(imu_rate) >= 300 else f32(0.20))
    limit = time_scan_cur - sync
    old = q[:, 0] < limit
    popped = int(np.argmin(old)) if (old.size and not old.all()) else int(old.size)      # the leading run of old samples
    out["n_popped"] = popped
    q = q[popped:]
    if q.shape[0] == 0 or q[0, 0] > time_scan_cur:
        return out

    def pick(t):
        late = np.nonzero(~(q[:, 0] < t))[0]
        return q[late[0]] if late.size else q[-1]
    s = pick(time_scan_cur)
    rpy = _rpy_of_quaternion(*s[4:8])
    out["initial_guess"] = np.array([s[1], s[2], s[3], *rpy]).astype(f32)
    out["odom_available"] = 1
    if q[-1, 0] < time_scan_end:
        return out
    e = pick(time_scan_end)
    if _c_round(s[8]) != _c_round(e[8]):
        return out
    tb = _transformation(s[1], s[2], s[3], *rpy)
    te = _transformation(e[1], e[2], e[3], *_rpy_of_quaternion(*e[4:8]))
    S = _inverse(tb)
    with np.errstate(all="ignore"):
        out["odom_incre"] = np.array([((S[a, 0] * te[0, 3] + S[a, 1] * te[1, 3]) + S[a, 2] * te[2, 3]) + S[a, 3] * f32(1) for a in range(3)], f32)
    out["odom_deskew_flag"] = 1
    return out


def same_odom(a, b):
    return (a["odom_available"], a["odom_deskew_flag"], a["n_popped"]) == (b["odom_available"], b["odom_deskew_flag"], b["n_popped"]) and \
        a["initial_guess"].tobytes() == b["initial_guess"].tobytes() and a["odom_incre"].tobytes() == b["odom_incre"].tobytes()


def quat(roll, pitch, yaw):
    """tf's setRPY, for building inputs."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(roll / 2), math.sin(roll / 2)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def make_queue(times, seed=0, speed=12.0, cov=0.0, scale=1.0):
    """A vehicle driving a gentle curve: one sample per time."""
    rng = np.random.default_rng(seed)
    t = np.asarray(times, np.float64)
    q = np.zeros((t.size, 9))
    q[:, 0] = t
    yaw0, rate = rng.uniform(-3, 3), rng.uniform(-0.5, 0.5)
    for k, tk in enumerate(t):
        d = tk - 1000.0
        yaw = yaw0 + rate * d
        q[k, 1:4] = [5.0 + speed * d * math.cos(yaw0), -3.0 + speed * d * math.sin(yaw0), 0.3 + 0.2 * d]
        q[k, 4:8] = np.array(quat(0.03 * math.sin(d), -0.02 + 0.05 * d, yaw)) * scale
        q[k, 8] = cov
    return q


CUR, END = 1000.0, 1000.1


def _odom_cases():
    c = {}
    grid = CUR - 0.15 + 0.01 * np.arange(40)                     # 100 Hz from cur - 0.15 to cur + 0.24
    c["empty_queue"] = (np.zeros((0, 9)), CUR, END, 500.0)
    c["all_older_than_the_pop_limit"] = (make_queue(CUR - 1.0 + 0.01 * np.arange(20)), CUR, END, 500.0)
    c["front_later_than_cur"] = (make_queue(CUR + 0.005 + 0.01 * np.arange(30)), CUR, END, 500.0)
    c["none_at_or_after_cur_takes_the_last"] = (make_queue(CUR - 0.009 + 0.002 * np.arange(4)), CUR, END, 500.0)
    c["queue_ends_before_end"] = (make_queue(CUR - 0.005 + 0.01 * np.arange(8)), CUR, END, 500.0)
    q = make_queue(grid, cov=0.49)
    q[q[:, 0] > CUR + 0.05, 8] = 0.51
    c["cov0_rounding_mismatch"] = (q, CUR, END, 200.0)
    q = make_queue(grid, cov=0.49)
    q[q[:, 0] > CUR + 0.05, 8] = 0.2
    c["cov0_same_after_rounding"] = (q, CUR, END, 200.0)
    q = make_queue(grid, cov=-0.5)
    q[q[:, 0] > CUR + 0.05, 8] = -0.49
    c["cov0_negative_half"] = (q, CUR, END, 200.0)
    c["stamps_equal_cur_and_end"] = (make_queue(np.array([CUR - 0.005, CUR, CUR + 0.05, END, END + 0.01])), CUR, END, 500.0)
    c["imu_rate_299"] = (make_queue(grid, seed=3), CUR, END, 299.0)
    c["imu_rate_300"] = (make_queue(grid, seed=3), CUR, END, 300.0)
    c["not_unit_quaternion"] = (make_queue(grid, seed=4, scale=1.7), CUR, END, 200.0)
    q = make_queue(grid, seed=5)
    q[:, 4:8] = [0.0, 1.0, 0.0, 1.0]                             # length2 2, s = 1: m20 = -1 exactly, pitch +pi/2
    q[::2, 4:8] = [0.0, -1.0, 0.0, 1.0]                          # m20 = +1 exactly, pitch -pi/2
    c["gimbal_branch"] = (q, CUR, END, 200.0)
    q = make_queue(np.array([CUR - 0.005, CUR + 0.2]), seed=8)
    q[0, 4:8] = [0.0, -1.0, 0.0, 1.0]                            # the last sample before cur is the front; the start sample is
    q[1, 4:8] = [0.0, -1.0, 0.0, 1.0]                            # the first at or after cur
    c["gimbal_branch_start_only"] = (q, CUR, END, 200.0)
    c["fast_vehicle"] = (make_queue(grid, seed=6, speed=30.0), CUR, END, 200.0)
    rng = np.random.default_rng(77)
    for k in range(300):
        n = int(rng.integers(0, 40))
        t = np.sort(CUR + rng.uniform(-0.4, 0.4, n))
        if n and k % 5 == 0:
            t[rng.integers(0, n)] = CUR
        if n and k % 7 == 0:
            t[rng.integers(0, n)] = END
            t = np.sort(t)
        q = make_queue(t, seed=1000 + k, speed=float(rng.uniform(0, 30)), scale=float(rng.uniform(0.5, 2.0)))
        q[:, 8] = np.round(rng.uniform(-1, 2, n), 2) if k % 3 == 0 else float(rng.integers(0, 3))
        c["random_%03d" % k] = (q, CUR, END if k % 11 else CUR, float(rng.choice([100.0, 299.0, 300.0, 500.0])))
    return c


ODOM_CASES = _odom_cases()


# ---- updateInitialGuess() ----------------------------------------------------------------------------------------------
class GuessRun:
    """One node's state, on the C restatement (`backend="c"`) or the numpy statement (`backend="np"`)."""

    def __init__(self, backend="c"):
        self.backend = backend
        self.pose = np.zeros(6, f32)
        if backend == "c":
            self.st = RefGuessState()
            lib().ref_guess_state_init(C.byref(self.st))
        else:
            self.last_imu = np.zeros((3, 4), f32)
            self.last_pre = np.zeros((3, 4), f32)
            self.pre_available = 0

    def state(self):
        if self.backend == "c":
            return (np.array(self.st.lastImuTransformation, f32)[:12].copy(), np.array(self.st.lastImuPreTransformation, f32)[:12].copy(),
                    int(self.st.lastImuPreTransAvailable))
        return self.last_imu.reshape(-1).copy(), self.last_pre.reshape(-1).copy(), self.pre_available

    def step(self, s):
        """s: dict(key_poses_empty, imuAvailable, odomAvailable, imu=(r, p, y), guess=(x, y, z, r, p, y), heading, imu_type).
        Returns affine_front (12 floats)."""
        if self.backend == "c":
            ci = RefCloudInfo(s["imuAvailable"], s["odomAvailable"], *[float(f32(v)) for v in s["imu"]], (C.c_float * 6)(*[float(f32(v)) for v in s["guess"]]))
            front = np.zeros(16, f32)
            fp = C.POINTER(C.c_float)
            lib().ref_update_initial_guess(C.byref(self.st), self.pose.ctypes.data_as(fp), int(s["key_poses_empty"]), C.byref(ci),
                                           int(s["heading"]), int(s["imu_type"]), front.ctypes.data_as(fp))
            return front[:12].copy()
        return self._np_step(s)

    def _tobe(self):
        t = self.pose
        return _transformation(t[3], t[4], t[5], t[0], t[1], t[2])

    def _apply(self, last, back):
        m = _m()
        fin = _mul_affine(self._tobe(), _mul_affine(_inverse(last), back))
        self.pose = np.array([m.atan2f(fin[2, 1], fin[2, 2]), m.asinf(-fin[2, 0]), m.atan2f(fin[1, 0], fin[0, 0]), fin[0, 3], fin[1, 3], fin[2, 3]], f32)

    def _np_step(self, s):
        front = self._tobe().reshape(-1)
        imu = [f32(v) for v in s["imu"]]
        imu_t = _transformation(0, 0, 0, *imu)
        if s["key_poses_empty"]:
            self.pose[0:3] = imu
            if not s["heading"]:
                self.pose[2] = 0
            self.last_imu = imu_t
            return front
        if s["odomAvailable"] == 1:
            back = _transformation(*[f32(v) for v in s["guess"]])
            if not self.pre_available:
                self.last_pre, self.pre_available = back, 1
            else:
                self._apply(self.last_pre, back)
                self.last_pre, self.last_imu = back, imu_t
                return front
        if s["imuAvailable"] == 1 and s["imu_type"]:
            self._apply(self.last_imu, imu_t)
            self.last_imu = imu_t
        return front


def guess_sequences():
    """name -> list of steps (see GuessRun.step)."""
    def steps(heading, imu_type, plan, seed):
        rng = np.random.default_rng(seed)
        out = []
        for k, (empty, imu_av, odom_av) in enumerate(plan):
            d = 0.1 * k
            imu = (0.02 * math.sin(d) + rng.normal(0, 1e-3), -0.03 + 0.01 * d, 0.8 + 0.05 * d + rng.normal(0, 1e-3))
            guess = (2.0 + 15.0 * d + rng.normal(0, 1e-2), -1.0 + 3.0 * d, 0.1 * d, imu[0] + 0.001, imu[1] - 0.002, imu[2] + 0.003)
            out.append(dict(key_poses_empty=empty, imuAvailable=imu_av, odomAvailable=odom_av, imu=imu, guess=guess, heading=heading,
                            imu_type=imu_type))
        return out
    steady = [(1, 1, 0), (0, 1, 1)] + [(0, 1, 1)] * 6
    return {
        "first_scan_with_heading": steps(1, 1, [(1, 1, 1), (0, 1, 1), (0, 1, 1)], 1),
        "first_scan_without_heading": steps(0, 1, [(1, 1, 1), (0, 1, 1), (0, 1, 1)], 2),
        "first_odometry_falls_through_to_imu": steps(1, 1, steady, 3),
        "imu_type_0_falls_through_to_no_change": steps(1, 0, steady, 4),
        "odometry_drops_out_and_returns": steps(1, 1, steady + [(0, 1, 0)] * 3 + [(0, 1, 1)] * 3 + [(0, 0, 0)] * 2 + [(0, 1, 1)] * 2, 5),
        "imu_available_other_than_1": steps(1, 1, [(1, 1, 0), (0, 2, 0), (0, -1, 0), (0, 256, 0), (0, 1, 0), (0, 0, 2), (0, 1, 2), (0, 1, 1), (0, 2, 1),
                                                   (0, 2, 1)], 6),
        "imu_only": steps(0, 1, [(1, 1, 0)] + [(0, 1, 0)] * 6, 7),
        "second_scan_still_without_key_poses": steps(1, 1, [(1, 1, 0), (1, 1, 1), (0, 1, 1), (0, 1, 1)], 8),
    }


# ---- projectPointCloud() with findPosition() live ------------------------------------------------------------------------
def c_project_motion(case, opt="-O2"):
    """(m, 8) float32: the C restatement's fullCloud. case = a project_ref case plus case["motion"] =
    dict(enabled, time_scan_end, odom_incre) (absent or None: findPosition() returns zeros)."""
    raw, lay, prm, dk = case["raw"], PR.RefLayout(*case["layout"]), case["params"], case["deskew"]
    mo = case.get("motion") or dict(enabled=0, time_scan_end=0.0, odom_incre=(0, 0, 0))
    n = raw.size // lay.stride
    out = np.zeros((max(n, 1), 8), f32)
    dp = C.POINTER(C.c_double)
    tabs = [np.ascontiguousarray(t, np.float64) for t in dk["tables"]]
    inc = np.ascontiguousarray(mo["odom_incre"], f32)
    m = lib(opt).ref_project_motion(raw.ctypes.data, n, C.byref(lay), prm["n_scan"], prm["downsample_rate"], prm["point_filter_num"],
                                    prm["lidar_min_range"], prm["lidar_max_range"], 1 if dk["deskew"] else 0, dk["time_scan_cur"],
                                    dk["imu_pointer_cur"], *[t.ctypes.data_as(dp) for t in tabs], 1 if mo["enabled"] else 0,
                                    float(mo["time_scan_end"]), inc.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data)
    return out[:m]


def np_project_motion(case):
    """The vectorised numpy statement; without motion it is project_ref.np_project."""
    mo = case.get("motion")
    raw, layout, prm, dk = case["raw"], case["layout"], case["params"], case["deskew"]
    if not mo or not mo["enabled"] or not dk["deskew"]:
        return PR.np_project(case)
    x, y, z, inten, ring, t = PR._fields(raw, layout)
    n = x.size
    with np.errstate(all="ignore"):
        rng_ = np.sqrt((x * x + y * y) + z * z)
        keep = ~((rng_ < f32(prm["lidar_min_range"])) | (rng_ > f32(prm["lidar_max_range"])))
        keep &= (ring >= 0) & (ring < prm["n_scan"])
        keep &= (np.where(ring >= 0, ring, 0) % prm["downsample_rate"]) == 0
        keep &= (np.arange(n) % prm["point_filter_num"]) == 0
        x, y, z, inten, t = x[keep], y[keep], z[keep], inten[keep], t[keep]
        m = x.size
        out = np.zeros((m, 8), f32)
        out[:, 4] = inten
        if m == 0:
            return out
        cur = dk["imu_pointer_cur"]
        T, RX, RY, RZ = [np.asarray(a, np.float64) for a in dk["tables"]]
        rel = t.astype(np.float64)
        pt = dk["time_scan_cur"] + rel
        front = np.searchsorted(T[:cur], pt, side="right")
        back = np.maximum(front - 1, 0)
        copy = (pt > T[front]) | (front == 0)
        rf = (pt - T[back]) / (T[front] - T[back])
        rb = (T[front] - pt) / (T[front] - T[back])
        rot = [np.where(copy, A[front], A[front] * rf + A[back] * rb).astype(f32) for A in (RX, RY, RZ)]
        R = PR._rotation(*rot)
        ratio = (rel / np.float64(mo["time_scan_end"] - dk["time_scan_cur"])).astype(f32)
        pos = [ratio * f32(v) for v in mo["odom_incre"]]
        m0 = {k: v[0] for k, v in R.items()}
        t0 = [p[0] for p in pos]

        def cof(i, j):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            return m0[(i1, j1)] * m0[(i2, j2)] - m0[(i1, j2)] * m0[(i2, j1)]
        c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
        det = (c0 * m0[(0, 0)] + c1 * m0[(1, 0)]) + c2 * m0[(2, 0)]
        inv = f32(1.0) / det
        S = np.zeros((3, 4), f32)
        for r in range(3):
            for c in range(3):
                S[r, c] = cof(c, r) * inv
            S[r, 3] = -((S[r, 0] * t0[0] + S[r, 1] * t0[1]) + S[r, 2] * t0[2])
        zero, one = f32(0), f32(1)
        p = (x, y, z)
        for a in range(3):
            Bm = [((S[a, 0] * R[(0, b)] + S[a, 1] * R[(1, b)]) + S[a, 2] * R[(2, b)]) + S[a, 3] * zero for b in range(3)]
            B3 = ((S[a, 0] * pos[0] + S[a, 1] * pos[1]) + S[a, 2] * pos[2]) + S[a, 3] * one
            out[:, a] = ((Bm[0] * p[0] + Bm[1] * p[1]) + Bm[2] * p[2]) + B3
    return out


def _e_first_survivor_late(f):
    """The first survivor is not record 0 and its time is not zero."""
    f["ring"][:7] = 99
    f["time"][:] = np.maximum(f["time"], 3 * 2.0 ** -9)


WALK = (0.11, -0.02, 0.004)              # about 1.1 m/s over a 0.1 s sweep
CAR = (2.9, -0.35, 0.06)                 # about 30 m/s
SPAN = 52 * 2.0 ** -9                    # make_case's default record times span (entries + 2) * 2^-9 s

MOTION_CASES = {}
for _s in ("velodyne", "livox", "ouster", "mulran", "robosense"):
    for _pfn in (1, 3):
        MOTION_CASES["%s_pfn%d_car" % (_s, _pfn)] = dict(base=dict(n=6000, layout=_s, seed=20 + _pfn, params=dict(point_filter_num=_pfn)), incre=CAR)
MOTION_CASES.update({
    "walking": dict(base=dict(n=6000, layout="velodyne", seed=31), incre=WALK),
    "negative_and_zero_components": dict(base=dict(n=6000, layout="ouster", seed=32), incre=(-2.5, 0.0, -0.0)),
    "zero_increments": dict(base=dict(n=6000, layout="velodyne", seed=33), incre=(0.0, 0.0, 0.0)),
    "first_survivor_late": dict(base=dict(n=6000, layout="velodyne", seed=34, edit=_e_first_survivor_late), incre=CAR),
    "no_deskew_copies": dict(base=dict(n=6000, layout="velodyne", seed=35, deskew=False), incre=CAR),
    "end_equals_cur": dict(base=dict(n=4000, layout="velodyne", seed=36), incre=CAR, end=PR.TIME_SCAN_CUR),
    "end_equals_cur_zero_increment": dict(base=dict(n=4000, layout="ouster", seed=37), incre=(0.0, 1.0, 0.0), end=PR.TIME_SCAN_CUR),
    "large_rotations_car": dict(base=dict(n=20000, layout="ouster", seed=38, entries=2000, rate=200.0), incre=CAR, end=PR.TIME_SCAN_CUR + 2002 * 2.0 ** -9),
    "size_131072_car": dict(base=dict(n=131072, layout="ouster", seed=39), incre=CAR),
    "size_4097_walk": dict(base=dict(n=4097, layout="custom40", seed=40), incre=WALK),
    "nothing_survives": dict(base=dict(n=3000, seed=41, params=dict(lidar_min_range=5000.0, lidar_max_range=6000.0)), incre=CAR),
    "disabled": dict(base=dict(n=6000, layout="velodyne", seed=42), incre=CAR, enabled=0),
})


def get_motion_case(name):
    spec = MOTION_CASES[name]
    case = PR.make_case(**spec["base"])
    mulran = case["layout"][6] == 2                 # whole-second record times: the table is spaced in seconds
    end = spec.get("end", PR.TIME_SCAN_CUR + (54.0 if mulran else SPAN))
    case["motion"] = dict(enabled=spec.get("enabled", 1), time_scan_end=float(end), odom_incre=tuple(spec["incre"]))
    return case
