"""The stage between the plane fit and the LM close, stated in floats (tests/test_lm_rows_cpu.py and
tests/test_lm_rows_gpu.py share it): the Jacobian row of one correspondence (reference src/mapOptmization.cpp:1170-1175,
1216-1234), the 28 products of a row, and which scan points a workgroup's partial row sums.

The Jacobian is kept as a table (JAC) and evaluated by one loop, one numpy fp32 operation per source operation in source
order: a matrix entry is a sum of groups `(sum of factor * coordinate) * coeff`, a factor a sum of signed products of the six
trig values.  Where the source negates (`-srx * cry * x`, `a - b * y`) the table carries a sign: negation is exact and
a - b == a + (-b), so signs change no rounding.  The table is what the discrimination test mutates term by term.
"""
import ctypes
import math

import numpy as np

F32 = np.float32
UT = [(a, b) for a in range(6) for b in range(a, 6)]      # sum number k <-> entry (a, b), a <= b
TRIG = ("srx", "crx", "sry", "cry", "srz", "crz")        # sin / cos of yaw, pitch, roll (:1170-1175: lidar -> camera)

# The attitudes (roll, pitch, yaw) the rows are held at: the suite's own, one angle at a time, three general ones, pitch
# within 1e-3 of pi / 2, yaw at the last fp32 below pi.  synth.POSE_DELTA is added for the start of a registration.
YAW_EDGE = float(np.nextafter(F32(np.pi), F32(0.0)))
ATTITUDES = {
    "gt": (0.01, -0.02, 0.3),
    "roll": (0.5, 0.0, 0.0), "pitch": (0.0, -0.45, 0.0), "yaw": (0.0, 0.0, 2.6),
    "a": (0.5, -0.4, 2.5), "b": (-0.6, 0.55, -1.9), "c": (1.2, -1.0, -3.0),
    "pitch_edge": (0.3, float(F32(math.pi / 2 - 5e-4)), 0.8),
    "yaw_edge": (-0.2, 0.15, YAW_EDGE),
}


def _f(*terms):
    return [(s, tuple(names.split())) for s, names in terms]


# matrix entry -> groups (coefficient index, [(sign of the coordinate term, factor, coordinate index)])
JAC = {
    "arx": [  # :1216-1217
        (0, [(+1, _f((-1, "srx cry")), 0), (-1, _f((+1, "srx sry srz"), (+1, "crx crz")), 1), (+1, _f((+1, "crx srz"), (-1, "srx sry crz")), 2)]),
        (1, [(+1, _f((+1, "crx cry")), 0), (-1, _f((+1, "srx crz"), (-1, "crx sry srz")), 1), (+1, _f((+1, "crx sry crz"), (+1, "srx srz")), 2)]),
    ],
    "ary": [  # :1219-1221 (the middle term of the second group reads sry where the derivative has cry: kept, it is the reference)
        (0, [(+1, _f((-1, "crx sry")), 0), (+1, _f((+1, "crx cry srz")), 1), (+1, _f((+1, "crx cry crz")), 2)]),
        (1, [(+1, _f((-1, "srx sry")), 0), (+1, _f((+1, "srx sry srz")), 1), (+1, _f((+1, "srx cry crz")), 2)]),
        (2, [(+1, _f((-1, "cry")), 0), (-1, _f((+1, "sry srz")), 1), (-1, _f((+1, "sry crz")), 2)]),
    ],
    "arz": [  # :1223-1225
        (0, [(+1, _f((+1, "crx sry crz"), (+1, "srx srz")), 1), (+1, _f((+1, "srx crz"), (-1, "crx sry srz")), 2)]),
        (1, [(+1, _f((-1, "crx srz"), (+1, "srx sry crz")), 1), (+1, _f((-1, "srx sry srz"), (-1, "crx crz")), 2)]),
        (2, [(+1, _f((+1, "cry crz")), 1), (-1, _f((+1, "cry srz")), 2)]),
    ],
}


def products(jac=JAC):
    """Every product term of the table as (entry, group, coordinate term, product) indices."""
    return [(e, g, t, p) for e in ("arx", "ary", "arz") for g, (_, terms) in enumerate(jac[e])
            for t, (_, factor, _) in enumerate(terms) for p in range(len(factor))]


def mutate(where, kind):
    """JAC with ONE product term changed: kind "sign" flips its sign, "swap" exchanges sry and cry in it (None when the
    term holds neither)."""
    e, g, t, p = where
    s, names = JAC[e][g][1][t][1][p]
    if kind == "sign":
        new = (-s, names)
    else:
        swapped = tuple({"sry": "cry", "cry": "sry"}.get(n, n) for n in names)
        if swapped == names:
            return None
        new = (s, swapped)
    out = {k: [(c, [(ts, list(f), x) for ts, f, x in terms]) for c, terms in v] for k, v in JAC.items()}
    out[e][g][1][t][1][p] = new
    return out


_LIBM = None


def libm_trig(pose):
    """srx, crx, sry, cry, srz, crz of a pose (roll, pitch, yaw, ...) by the host libm's sinf / cosf, as the reference takes
    them (np.sin on float32 is not glibc's)."""
    global _LIBM
    if _LIBM is None:
        _LIBM = ctypes.CDLL("libm.so.6")
        for fn in (_LIBM.sinf, _LIBM.cosf):
            fn.restype = ctypes.c_float
            fn.argtypes = [ctypes.c_float]
    p = np.asarray(pose, F32)
    out = []
    for k in (2, 1, 0):
        out += [_LIBM.sinf(float(p[k])), _LIBM.cosf(float(p[k]))]
    return np.array(out, F32)


def device_trig(gpu, pose):
    """The same six values as the device rebuilds them between launches (s2m_debug_device_trig)."""
    p = np.asarray(pose, F32)
    sn, cs, _ = gpu.deviceTrig(p[[2, 1, 0]])
    return np.array([sn[0], cs[0], sn[1], cs[1], sn[2], cs[2]], F32)


def jac_rows(pose, P, C4, trig=None, jac=JAC):
    """(rows (n, 6) fp32, rhs (n,) fp32) of n correspondences: P (n, 3) pointOri, C4 (n, 4) coeffSel.  `trig`: the six values
    to use instead of libm's at `pose`."""
    P, C4 = np.ascontiguousarray(P, F32), np.ascontiguousarray(C4, F32)
    tv = dict(zip(TRIG, (libm_trig(pose) if trig is None else np.asarray(trig, F32))))
    assert all(type(v) is F32 for v in tv.values())

    def factor(f):
        acc = None
        for s, names in f:
            v = tv[names[0]]
            for n in names[1:]:
                v = v * tv[n]
            v = v if s > 0 else -v
            acc = v if acc is None else acc + v
        assert type(acc) is F32
        return acc

    def entry(groups):
        total = None
        for c, terms in groups:
            acc = None
            for s, f, x in terms:
                v = factor(f) * P[:, x]
                v = v if s > 0 else -v
                acc = v if acc is None else acc + v
            acc = acc * C4[:, c]
            total = acc if total is None else total + acc
        assert total.dtype == F32
        return total

    rows = np.empty((P.shape[0], 6), F32)
    rows[:, 0], rows[:, 1], rows[:, 2] = entry(jac["arz"]), entry(jac["ary"]), entry(jac["arx"])      # :1228-1230
    rows[:, 3:] = C4[:, :3]
    return rows, -C4[:, 3]


def row_products(rows, rhs):
    """(n, 28) fp64: the 21 upper-triangular products of a row, its 6 products with the right-hand side, and 1.  A product of
    two fp32 values is exact in fp64."""
    r, b = rows.astype(np.float64), rhs.astype(np.float64)
    out = np.empty((rows.shape[0], 28))
    for k, (a, c) in enumerate(UT):
        out[:, k] = r[:, a] * r[:, c]
    out[:, 21:27] = r * b[:, None]
    out[:, 27] = 1.0
    return out


def active_rows(n_waves, wpb, nblocks):
    """Workgroups the wave table needs (k_register's nb_act)."""
    return min((n_waves + wpb - 1) // wpb, nblocks)


def row_members(wave_table, n_waves, nb_act, n_q=None):
    """Per workgroup row b the scan points, in sorted order, that it sums: the lanes of every wave-table entry e < n_waves with
    e % nb_act == b (wave w of workgroup b starts at entry w * nb_act + b and advances by nb_act * waves per workgroup,
    liorf_amd/csrc/s2m_register.hpp).  Lane l of an entry {first, count} is live when l < count and first + l < n_q."""
    t = np.asarray(wave_table, np.int64).reshape(-1, 2)[:n_waves]
    out = [[] for _ in range(nb_act)]
    for e, (first, count) in enumerate(t):
        end = first + min(int(count), 64)
        if n_q is not None:
            end = min(end, n_q)
        if end > first:
            out[e % nb_act].append(np.arange(first, end))
    return [np.concatenate(m) if m else np.zeros(0, np.int64) for m in out]


def expected_rows(P, C4, flag, members, qperm, pose=None, trig=None, jac=JAC):
    """(exact, bound, counts), each per row: exact[b, k] the exactly rounded sum (math.fsum) of product k over the kept points
    of row b, bound[b, k] = m * 2^-52 * sum |p| with m the kept points of the row - the worst case of m - 1 fp64 additions in
    any order ((m - 1) * 2^-53 * sum |p| to first order), doubled; derived, not measured.  Column 27 is the count, exact.
    P, C4, flag in original scan order; `members` in sorted order, `qperm` sorted -> original."""
    keep = np.asarray(flag) != 0
    rows, rhs = jac_rows(pose, P, C4, trig, jac)
    prod = row_products(rows, rhs)
    qperm = np.asarray(qperm, np.int64)
    nb = len(members)
    exact, bound, counts = np.zeros((nb, 28)), np.zeros((nb, 28)), np.zeros(nb, np.int64)
    for b, mem in enumerate(members):
        o = qperm[mem]
        o = o[keep[o]]
        counts[b] = len(o)
        if len(o) == 0:
            continue
        p = prod[o]
        for k in range(28):
            exact[b, k] = math.fsum(p[:, k])
        bound[b] = len(o) * 2.0 ** -52 * np.abs(p).sum(0)
        bound[b, 27] = 0.0
    return exact, bound, counts


def worst_ratio(got, exact, bound):
    """Largest |got - exact| / bound over all sums (0 / 0 counts as 0, anything else over 0 as inf)."""
    d = np.abs(np.asarray(got) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- any configuration at any attitude -------------------------------------------------------------------------------
def rotation_rpy(rpy):
    from liorf_amd import synth
    return synth.rotation_rpy(*(float(v) for v in rpy))


def rpy_of(R):
    return np.array([math.atan2(R[2, 1], R[2, 2]), math.atan2(-R[2, 0], math.hypot(R[0, 0], R[1, 0])), math.atan2(R[1, 0], R[0, 0])])


def rotated(cfg, G):
    """The configuration under the rigid motion G = (R 3x3, t 3): the map moved by it, pose_gt composed with it in fp64 and
    its xyzrpy re-extracted, pose_init = pose_gt + synth.POSE_DELTA, the scan untouched."""
    from liorf_amd import synth
    R, t = np.asarray(G[0], np.float64), np.asarray(G[1], np.float64)
    out = dict(cfg)
    out["map"] = (cfg["map"].astype(np.float64) @ R.T + t).astype(F32)
    p = cfg["pose_gt"].astype(np.float64)
    q = np.concatenate([rpy_of(R @ rotation_rpy(p[:3])), R @ p[3:] + t]).astype(F32)
    out["pose_gt"], out["pose_init"] = q, synth.pose_init_from(q)
    return out


def at_attitude(cfg, rpy):
    """`rotated` by the rotation about the sensor that brings pose_gt to the attitude rpy (fp32 values); the re-extracted angles
    are replaced by rpy itself once they are seen to describe the same rotation."""
    from liorf_amd import synth
    rpy = np.asarray(rpy, F32)
    p = cfg["pose_gt"].astype(np.float64)
    R = rotation_rpy(rpy.astype(np.float64)) @ rotation_rpy(p[:3]).T
    out = rotated(cfg, (R, p[3:] - R @ p[3:]))
    assert np.abs(rotation_rpy(out["pose_gt"][:3].astype(np.float64)) - rotation_rpy(rpy.astype(np.float64))).max() < 1e-5
    q = out["pose_gt"].copy()
    q[:3] = rpy
    out["pose_gt"], out["pose_init"] = q, synth.pose_init_from(q)
    return out
