"""Checkers of the point filter and IMU deskew, and the cases both test files run.

* `lib()` compiles tests/ref/project_ref.c (the C restatement of the reference's src/imageProjection.cpp) with
  `gcc -O2 -ffp-contract=off` into a temporary directory and loads it with ctypes; `c_project` / `c_imu_deskew_info` call it.
* `np_project` is an independent, vectorised numpy statement of the same arithmetic: float32 ufuncs (one rounding per
  operation), the host libm's sinf / cosf through ctypes, numpy's searchsorted for the table walk.
* `CASES` / `make_case` build the raw records, layouts, parameters and IMU tables of every case of tests/test_project_gpu.py;
  tests/test_project_cpu.py runs the two checkers against each other on all of them.
"""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
QUEUE_LENGTH = 2000
_LIBS = {}


class RefLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("off_x", C.c_uint32), ("off_intensity", C.c_uint32), ("off_ring", C.c_uint32),
                ("off_time", C.c_uint32), ("ring_type", C.c_int32), ("time_type", C.c_int32)]


def lib(opt: str = "-O2"):
    if opt in _LIBS:
        return _LIBS[opt]
    d = tempfile.mkdtemp(prefix="project_ref_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libproject_ref.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "project_ref.c"), "-lm"])
    L = C.CDLL(so)
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.ref_imu_deskew_info.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, dp, dp, dp, dp, i32p, i32p]
    L.ref_project.restype = C.c_size_t
    L.ref_project.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(RefLayout), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                              C.c_int, C.c_double, C.c_int, dp, dp, dp, dp, C.c_void_p]
    _LIBS[opt] = L
    return L


# ---- layouts (the reference's structs, src/imageProjection.cpp:4-57, written down independently of the product) --------
#              stride x  intensity ring time ring_type time_type
LAYOUTS = {
    "velodyne":  (32, 0, 16, 20, 24, 1, 0),
    "livox":     (32, 0, 16, 20, 24, 1, 0),
    "ouster":    (48, 0, 16, 26, 20, 0, 1),
    "mulran":    (32, 0, 16, 24, 20, 2, 2),
    "robosense": (32, 0, 16, 20, 24, 1, 3),
    "custom64":  (64, 16, 36, 42, 48, 1, 0),      # hand-made: x not at 0, other offsets, stride 64
    "custom40":  (40, 4, 20, 24, 32, 2, 3),       # x not 16-byte aligned, stride not a multiple of 16, f64 time
}
SENSOR_ID = {"velodyne": 0, "livox": 1, "ouster": 2, "mulran": 3, "robosense": 4}


def make_records(layout, xyz, intensity, ring, time, rng, stamp0=1.7e9):
    """Raw records: random filler bytes, then the fields. `time` is what laserCloudIn->points[i].time shall become:
    seconds for f32 / u32-ns / f64 layouts, whole numbers for the u32 layout."""
    stride, ox, oi, orr, ot, rt, tt = layout
    n = xyz.shape[0]
    rec = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    rec[:, ox:ox + 12] = np.ascontiguousarray(xyz, np.float32).view(np.uint8).reshape(n, 12)
    rec[:, oi:oi + 4] = np.ascontiguousarray(intensity, np.float32).view(np.uint8).reshape(n, 4)
    rdt = [np.uint8, np.uint16, np.int32][rt]
    rb = np.dtype(rdt).itemsize
    rec[:, orr:orr + rb] = np.ascontiguousarray(np.asarray(ring).astype(np.int64).astype(rdt)).view(np.uint8).reshape(n, rb)
    if tt == 0:
        tb = np.ascontiguousarray(time, np.float32).view(np.uint8).reshape(n, 4)
    elif tt == 1:
        tb = np.ascontiguousarray(np.round(np.asarray(time, np.float64) * 1e9).clip(0, 2**32 - 1).astype(np.uint32)).view(np.uint8).reshape(n, 4)
    elif tt == 2:
        tb = np.ascontiguousarray(np.round(np.asarray(time, np.float64)).clip(0, 2**32 - 1).astype(np.uint32)).view(np.uint8).reshape(n, 4)
    else:
        tb = np.ascontiguousarray(stamp0 + np.asarray(time, np.float64)).view(np.uint8).reshape(n, 8)
    rec[:, ot:ot + tb.shape[1]] = tb
    return np.ascontiguousarray(rec).reshape(-1)


def c_imu_deskew_info(imu, time_scan_cur, time_scan_end, opt="-O2"):
    a = np.ascontiguousarray(imu, np.float64).reshape(-1, 4)
    tabs = [np.zeros(QUEUE_LENGTH, np.float64) for _ in range(4)]
    cur, avail = C.c_int32(0), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    rc = lib(opt).ref_imu_deskew_info(a.ctypes.data_as(dp), a.shape[0], time_scan_cur, time_scan_end,
                                      *[t.ctypes.data_as(dp) for t in tabs], C.byref(cur), C.byref(avail))
    return (rc, *tabs, cur.value, bool(avail.value))


def c_project(case, opt="-O2"):
    """(m, 8) float32: the C restatement's fullCloud for a case."""
    raw, lay, prm, dk = case["raw"], RefLayout(*case["layout"]), case["params"], case["deskew"]
    n = raw.size // lay.stride
    out = np.zeros((max(n, 1), 8), np.float32)
    dp = C.POINTER(C.c_double)
    tabs = [np.ascontiguousarray(t, np.float64) for t in dk["tables"]]
    m = lib(opt).ref_project(raw.ctypes.data, n, C.byref(lay), prm["n_scan"], prm["downsample_rate"], prm["point_filter_num"],
                             prm["lidar_min_range"], prm["lidar_max_range"], 1 if dk["deskew"] else 0, dk["time_scan_cur"],
                             dk["imu_pointer_cur"], *[t.ctypes.data_as(dp) for t in tabs], out.ctypes.data)
    return out[:m]


def c_project_prepared(case, opt="-O2"):
    """(call, out): `call()` runs the C restatement alone - output, tables and arguments are made here, once - and returns
    the survivor count; the cloud is out[:count]. For timing the C loop without Python and page-fault overhead."""
    raw, lay, prm, dk = case["raw"], RefLayout(*case["layout"]), case["params"], case["deskew"]
    n = raw.size // lay.stride
    out = np.ones((max(n, 1), 8), np.float32)         # written once here: the pages exist before anything is timed
    dp = C.POINTER(C.c_double)
    tabs = [np.ascontiguousarray(t, np.float64) for t in dk["tables"]]
    fn = lib(opt).ref_project
    args = (C.c_void_p(raw.ctypes.data), C.c_size_t(n), C.byref(lay), C.c_int(prm["n_scan"]), C.c_int(prm["downsample_rate"]),
            C.c_int(prm["point_filter_num"]), C.c_float(prm["lidar_min_range"]), C.c_float(prm["lidar_max_range"]),
            C.c_int(1 if dk["deskew"] else 0), C.c_double(dk["time_scan_cur"]), C.c_int(dk["imu_pointer_cur"]),
            *[t.ctypes.data_as(dp) for t in tabs], C.c_void_p(out.ctypes.data))
    keep = (raw, lay, tabs, out)

    def call(_keep=keep):
        return fn(*args)
    return call, out


# ---- the numpy statement -------------------------------------------------------------------------------------------
_LIBM = None


def _trig(a):
    global _LIBM
    if _LIBM is None:
        _LIBM = C.CDLL("libm.so.6")
        for f in (_LIBM.sinf, _LIBM.cosf):
            f.restype, f.argtypes = C.c_float, [C.c_float]
    v = a.tolist()
    return (np.array(list(map(_LIBM.sinf, v)), np.float32).reshape(a.shape), np.array(list(map(_LIBM.cosf, v)), np.float32).reshape(a.shape))


def _fields(raw, layout):
    stride, ox, oi, orr, ot, rt, tt = layout
    n = raw.size // stride
    rec = raw.reshape(n, stride)

    def col(off, dt):
        return np.ascontiguousarray(rec[:, off:off + np.dtype(dt).itemsize]).view(dt).reshape(n)
    x, y, z, inten = col(ox, np.float32), col(ox + 4, np.float32), col(ox + 8, np.float32), col(oi, np.float32)
    ring = col(orr, [np.uint8, np.uint16, np.int32][rt]).astype(np.int64)
    if tt == 0:
        t = col(ot, np.float32)
    elif tt == 1:
        t = col(ot, np.uint32).astype(np.float32) * np.float32(1e-9)
    elif tt == 2:
        t = col(ot, np.uint32).astype(np.float32)
    else:
        ts = col(ot, np.float64)
        t = (ts - ts[0]).astype(np.float32) if n else ts.astype(np.float32)
    return x, y, z, inten, ring, t


def _rotation(rx, ry, rz):
    """pcl::getTransformation's linear part for arrays of roll, pitch, yaw (float32): dict of the nine entries."""
    B, A = _trig(rz)
    D, Cc = _trig(ry)
    F, E = _trig(rx)
    DE, DF = D * E, D * F
    return {(0, 0): A * Cc, (0, 1): A * DF - B * E, (0, 2): B * F + A * DE,
            (1, 0): B * Cc, (1, 1): A * E + B * DF, (1, 2): B * DE - A * F,
            (2, 0): -D, (2, 1): Cc * F, (2, 2): Cc * E}


def np_project(case):
    raw, layout, prm, dk = case["raw"], case["layout"], case["params"], case["deskew"]
    x, y, z, inten, ring, t = _fields(raw, layout)
    n = x.size
    f32 = np.float32
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
        if not dk["deskew"] or m == 0:
            out[:, 0], out[:, 1], out[:, 2] = x, y, z
            return out
        cur = dk["imu_pointer_cur"]
        T, RX, RY, RZ = [np.asarray(a, np.float64) for a in dk["tables"]]
        pt = dk["time_scan_cur"] + t.astype(np.float64)
        front = np.searchsorted(T[:cur], pt, side="right")          # first index in [0, cur) with pt < T[index], else cur
        back = np.maximum(front - 1, 0)
        copy = (pt > T[front]) | (front == 0)
        rf = (pt - T[back]) / (T[front] - T[back])
        rb = (T[front] - pt) / (T[front] - T[back])
        rot = [np.where(copy, A[front], A[front] * rf + A[back] * rb).astype(f32) for A in (RX, RY, RZ)]
        R = _rotation(*rot)
        m0 = {k: v[0] for k, v in R.items()}                          # the first survivor's transform

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
            S[r, 3] = -((S[r, 0] * f32(0) + S[r, 1] * f32(0)) + S[r, 2] * f32(0))
        zero, one = f32(0), f32(1)
        p = (x, y, z)
        for a in range(3):
            Bm = [((S[a, 0] * R[(0, b)] + S[a, 1] * R[(1, b)]) + S[a, 2] * R[(2, b)]) + S[a, 3] * zero for b in range(3)]
            B3 = ((S[a, 0] * zero + S[a, 1] * zero) + S[a, 2] * zero) + S[a, 3] * one
            out[:, a] = ((Bm[0] * p[0] + Bm[1] * p[1]) + Bm[2] * p[2]) + B3
    return out


def same_cloud(a, b):
    """Bit for bit, except that a NaN matches any NaN: an x86 host and the device propagate different NaN payloads."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))


# ---- cases ---------------------------------------------------------------------------------------------------------
TIME_SCAN_CUR = 1000.0          # exact in double; table times are TIME_SCAN_CUR + k * 2^-9, record times multiples of 2^-12


def make_table(entries, rng, rate=1.0, t0=TIME_SCAN_CUR - 2.0 ** -8, dt=2.0 ** -9):
    T = t0 + dt * np.arange(entries)
    w = rng.normal(0, rate, (entries, 3))
    rot = np.concatenate([np.zeros((1, 3)), np.cumsum(w[1:] * dt, 0)], 0)
    tabs = [np.zeros(QUEUE_LENGTH) for _ in range(4)]
    tabs[0][:entries] = T
    for k in range(3):
        tabs[1 + k][:entries] = rot[:, k]
    return tabs


def default_params(**kw):
    p = dict(n_scan=16, downsample_rate=1, point_filter_num=3, lidar_min_range=1.0, lidar_max_range=1000.0)
    p.update(kw)
    return p


def make_case(n, layout="velodyne", seed=1, entries=50, deskew=True, params=None, n_scan=16, edit=None, time_span=None, rate=1.0):
    """Random records: points N(0, 20 m), rings uniform in [0, n_scan), times increasing over the table's span (and a little
    before and after it), multiples of 2^-12 s so that some equal a table time. `edit(fields)` changes the field arrays
    (dict xyz, intensity, ring, time) before they are packed."""
    rng = np.random.default_rng(seed)
    lay = LAYOUTS[layout]
    prm = default_params(n_scan=n_scan)
    prm.update(params or {})
    xyz = rng.normal(0, 20.0, (n, 3)).astype(np.float32)
    inten = rng.uniform(0, 255, n).astype(np.float32)
    ring = rng.integers(0, n_scan, n)
    if lay[6] == 2:                                  # (float)t of a u32: whole numbers; the table is spaced in seconds
        tabs = make_table(entries, rng, rate=0.02, t0=TIME_SCAN_CUR + 2.0, dt=1.0)
        time = np.sort(rng.integers(0, entries + 4, n)).astype(np.float64)
    else:
        tabs = make_table(entries, rng, rate=rate)
        span = time_span if time_span is not None else (entries + 2) * 2.0 ** -9
        time = np.round(np.sort(rng.uniform(0.0, span, n)) * 4096.0) / 4096.0
    f = dict(xyz=xyz, intensity=inten, ring=ring, time=time)
    if edit:
        edit(f)
    raw = make_records(lay, f["xyz"], f["intensity"], f["ring"], f["time"], rng)
    return dict(raw=raw, layout=lay, params=prm,
                deskew=dict(deskew=deskew, time_scan_cur=TIME_SCAN_CUR, imu_pointer_cur=entries - 1 if deskew else 0, tables=tabs))


def _e_range(f):
    f["xyz"][2::5] *= np.float32(0.01)               # inside lidarMinRange
    f["xyz"][1::7] *= np.float32(100.0)              # beyond lidarMaxRange (most of them)


def _e_ring(f):
    f["ring"][::5] = 16
    f["ring"][1::9] = 40


def _e_first_out(f):
    f["ring"][:5] = 99


def _e_neg_ring(f):
    f["ring"][::3] = -1
    f["ring"][1::11] = -2147483648
    f["ring"][2::13] = 16


def _e_limits(f):
    k = f["xyz"].shape[0] // 4
    f["xyz"][:k] = np.float32([1.0, 0.0, 0.0])                     # range == lidarMinRange: kept
    f["xyz"][k:2 * k] = np.float32([600.0, 800.0, 0.0])            # range == lidarMaxRange: kept
    f["xyz"][2 * k:3 * k] = np.float32([0.99999994, 0.0, 0.0])     # one ulp inside
    f["xyz"][3 * k:] = np.float32([600.0, 800.00006, 0.0])         # one ulp beyond


def _e_nan(f):
    f["xyz"][3::6, 0] = np.nan
    f["xyz"][4::10, 2] = np.nan


def _e_times(f):
    n = f["time"].size
    t = f["time"]
    t[: n // 8] = -2.0 ** -7                          # before the first table time
    t[n // 8: n // 4] = -2.0 ** -8                    # equal to the first table time
    t[n // 4: n // 2] = 6 * 2.0 ** -9                 # equal to an inner table time
    t[n // 2: 5 * n // 8] = 47 * 2.0 ** -9            # equal to the last of 50 (t0 = cur - 2^-8)
    t[5 * n // 8: 3 * n // 4] = 1.0                   # after the last


CASES = {}
for _name in ("velodyne", "ouster", "mulran", "robosense", "custom64", "custom40"):
    CASES["layout_" + _name] = dict(n=5000, layout=_name)
for _n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 131072, 262144, 1000000):
    CASES["size_%d" % _n] = dict(n=_n, layout="ouster" if _n == 131072 else "velodyne", seed=10 + _n % 97)
CASES.update({
    "filter_range": dict(n=6000, params=dict(point_filter_num=1), edit=_e_range),
    "filter_ring": dict(n=6000, params=dict(point_filter_num=1), edit=_e_ring),
    "filter_downsample": dict(n=6000, params=dict(point_filter_num=1, downsample_rate=2)),
    "filter_point_num": dict(n=6000, params=dict(point_filter_num=3)),
    "filter_all_four": dict(n=6000, params=dict(point_filter_num=4, downsample_rate=2), edit=lambda f: (_e_range(f), _e_ring(f))),
    "filter_nothing_survives": dict(n=6000, params=dict(lidar_min_range=5000.0, lidar_max_range=6000.0)),
    "first_record_filtered": dict(n=6000, edit=_e_first_out),
    "pfn_1": dict(n=7001, params=dict(point_filter_num=1)),
    "pfn_4": dict(n=7001, params=dict(point_filter_num=4)),
    "rings_beyond_and_negative": dict(n=6000, layout="mulran", params=dict(point_filter_num=2), edit=_e_neg_ring),
    "rings_64_of_128": dict(n=6000, layout="ouster", n_scan=128, params=dict(downsample_rate=2)),
    "range_limits": dict(n=4000, params=dict(point_filter_num=1), edit=_e_limits),
    "nan_coordinates": dict(n=4000, edit=_e_nan),
    "nan_coordinates_no_deskew": dict(n=4000, edit=_e_nan, deskew=False),
    "point_times": dict(n=8000, params=dict(point_filter_num=1), edit=_e_times),
    "no_deskew": dict(n=5000, deskew=False),
    "table_2": dict(n=5000, entries=2, time_span=2.0 ** -7),
    "table_2000": dict(n=20000, entries=2000),
    # rotations of several radians (a random walk of rate * 2^-9 rad steps): sinf / cosf beyond pi/4, every quadrant
    "table_50_large_rotations": dict(n=20000, entries=50, rate=200.0),
    "table_2000_large_rotations": dict(n=20000, entries=2000, rate=200.0, layout="ouster"),
})


def get_case(name):
    return make_case(**CASES[name])
