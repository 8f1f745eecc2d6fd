"""Model of the session blob (include/liorf_s2m.h "Saving and loading a session"): a writer and a parser
in numpy, restated from the format's description and from nothing in the library, plus what the add calls make of their inputs
(Rot3::RzRyRx in fp64, sw = 1 / sqrt(variance), the odometry between) so that a session scripted here is, byte for byte, the
session the library saves after the same calls. Shared by test_session_cpu.py and test_session_gpu.py.

Layout, little-endian, every section a multiple of 4 bytes:
  header (112)   0 magic "S2MSESS\\0" | 8 u32 version 1 | 12 u32 112 | 16 i32 n_keys, n_descriptors, n_search, counter, n_loop_pairs,
                 n_variables, n_factors | 44 u32 0 | 48 u64 n_points | 56 u64 x 6 section bytes | 104 u64 total bytes
  KEYS           per key 40: f32 x 6 pose {x, y, z, roll, pitch, yaw} | f64 time | i32 point count | u32 0
  CLOUD          every key's 32-byte records, all eight words, in key order
  DESC           n_descriptors x 1200 f64
  LOOPS          per pair 8: i32 key_cur, i32 key_pre, ascending in key_cur
  FACTORS        per factor 168: i32 type, i, j, rows | f64 R[9], t[3], sw[6], k
  VARS           n_variables x 12 f64, then n_variables x u32 has_init
  footer (112)   (u64 s1, u64 s2) x 6 sections | (u64 s1, u64 s2) over the header's and these 96 bytes' words as one run
Checksum over 32-bit words w[0..m): s1 = sum w[i], s2 = sum (i + 1) w[i], both mod 2^64.
"""
import math
import struct

import numpy as np

MAGIC = b"S2MSESS\0"
VERSION = 1
HEADER, FOOTER = 112, 112
SECTIONS = ("keys", "cloud", "desc", "loops", "factors", "vars")
KEY_BYTES, REC_BYTES, DESC_BYTES, PAIR_BYTES, FACTOR_BYTES, VAR_BYTES = 40, 32, 9600, 8, 168, 100
PRIOR, BETWEEN, GPS = 0, 1, 2
M64 = (1 << 64) - 1
PRIOR_VAR = (1e-2, 1e-2, math.pi * math.pi, 1e8, 1e8, 1e8)      # s2m_pg_default_params
ODOM_VAR = (1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4)


def checksum(data, first=0):
    """(s1, s2) of the words of `data` (bytes, a multiple of 4), the first of them word `first` of its section."""
    w = np.frombuffer(bytes(data), "<u4")
    s1 = s2 = 0
    for k in range(0, w.size, 1 << 16):                # exact: python integers, in blocks to stay quick
        blk = [int(x) for x in w[k:k + (1 << 16)]]
        s1 += sum(blk)
        s2 += sum((first + k + i + 1) * x for i, x in enumerate(blk))
    return s1 & M64, s2 & M64


def checksum_fast(data):
    """The same in numpy: uint64 arithmetic wraps mod 2^64 (for the large sections)."""
    w = np.frombuffer(bytes(data), "<u4").astype(np.uint64)
    i = np.arange(1, w.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)), int((w * i).sum(dtype=np.uint64))


def combine(a, b, base):
    """The checksum of a section from those of two chunks, b's computed as if it began at word 0, `base` its first word."""
    return (a[0] + b[0]) & M64, (a[1] + base * b[0] + b[1]) & M64


# ---- what the add calls make of their inputs -------------------------------------------------------------------------

def state_of(pose_xyzrpy):
    """pose_to_state: Rot3::RzRyRx(roll, pitch, yaw) and t of a float32 pose, in fp64 with libm's sin / cos: 12 doubles."""
    p = [float(np.float32(v)) for v in pose_xyzrpy]
    cr, sr, cp, sp, cy, sy = math.cos(p[3]), math.sin(p[3]), math.cos(p[4]), math.sin(p[4]), math.cos(p[5]), math.sin(p[5])
    return [cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr,
            sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr,
            -sp, cp * sr, cp * cr, p[0], p[1], p[2]]


def factor(kind, i, j, X, var, rows, k=0.0):
    return dict(type=kind, i=i, j=j, rows=rows, R=list(X[:9]), t=list(X[9:12]),
                sw=[1.0 / math.sqrt(float(var[a])) if a < rows else 0.0 for a in range(6)], k=float(k))


class Graph:
    """The host side of the pose graph as the s2m_pg_add_* calls leave it (no optimise: the estimates are the initial values)."""

    def __init__(self):
        self.factors, self.X, self.has_init = [], [], []

    def _touch(self, key):
        assert 0 <= key <= len(self.X)
        if key == len(self.X):
            self.X.append([0.0] * 12)
            self.has_init.append(0)

    def _add(self, f):
        lo, hi = (min(f["i"], f["j"]), max(f["i"], f["j"])) if f["type"] == BETWEEN else (f["i"], f["i"])
        self._touch(lo)
        self._touch(hi)
        self.factors.append(f)

    def add_prior(self, key, pose, var):
        self._add(factor(PRIOR, key, -1, state_of(pose), var, 6))

    def add_between(self, a, b, rel, var, k=0.0):
        self._add(factor(BETWEEN, a, b, state_of(rel), var, 6, k))

    def add_gps(self, key, xyz, var):
        x = [float(np.float32(v)) for v in xyz]
        self._add(factor(GPS, key, -1, [1, 0, 0, 0, 1, 0, 0, 0, 1] + x, var, 3))

    def set_initial(self, key, pose):
        self._touch(key)
        self.X[key] = state_of(pose)
        self.has_init[key] = 1

    def add_odometry(self, pose):
        n = len(self.X)
        if n == 0:
            self.add_prior(0, pose, PRIOR_VAR)
            self.set_initial(0, pose)
            return
        L, Xn = self.X[n - 1], state_of(pose)
        Z = [0.0] * 12
        for a in range(3):                               # L^-1 Xn, every sum left to right
            for b in range(3):
                Z[a * 3 + b] = L[a] * Xn[b] + L[3 + a] * Xn[3 + b] + L[6 + a] * Xn[6 + b]
            Z[9 + a] = L[a] * (Xn[9] - L[9]) + L[3 + a] * (Xn[10] - L[10]) + L[6 + a] * (Xn[11] - L[11])
        self._add(factor(BETWEEN, n - 1, n, Z, ODOM_VAR, 6))
        self.X[n] = Xn
        self.has_init[n] = 1


# ---- the session ---------------------------------------------------------------------------------------------------

class Session:
    def __init__(self):
        self.poses = np.zeros((0, 6), np.float32)        # key frames
        self.times = np.zeros(0, np.float64)
        self.clouds = []                                 # per key (m, 8) uint32: the records' words as they are stored
        self.desc = np.zeros((0, 1200), np.float64)
        self.n_search, self.counter = 0, 0
        self.pairs = []                                  # (key_cur, key_pre), ascending in key_cur
        self.factors, self.X, self.has_init = [], np.zeros((0, 12), np.float64), np.zeros(0, np.uint32)

    def add_key(self, pose, time, cloud):
        """cloud: (m, >= 3) float32 records as s2m_kf_add takes them: the words a record lacks are stored as 0."""
        c = np.ascontiguousarray(cloud, np.float32)
        rec = np.zeros((c.shape[0], 8), np.uint32)
        rec[:, :min(c.shape[1], 8)] = c[:, :8].view(np.uint32)
        self.poses = np.vstack([self.poses, np.asarray(pose, np.float32).reshape(1, 6)])
        self.times = np.append(self.times, float(time))
        self.clouds.append(rec)

    def set_graph(self, g):
        self.factors = list(g.factors)
        self.X = np.array(g.X, np.float64).reshape(-1, 12)
        self.has_init = np.array(g.has_init, np.uint32)

    def counts(self):
        return dict(n_keys=len(self.clouds), n_descriptors=self.desc.shape[0], n_loop_pairs=len(self.pairs),
                    n_variables=self.X.shape[0], n_factors=len(self.factors), n_points=sum(c.shape[0] for c in self.clouds))

    def sections(self):
        keys = b"".join(struct.pack("<6fdiI", *[float(v) for v in self.poses[k]], float(self.times[k]), self.clouds[k].shape[0], 0)
                        for k in range(len(self.clouds)))
        cloud = b"".join(c.astype("<u4").tobytes() for c in self.clouds)
        desc = np.ascontiguousarray(self.desc, "<f8").tobytes()
        loops = b"".join(struct.pack("<ii", a, b) for a, b in self.pairs)
        factors = b"".join(struct.pack("<4i19d", f["type"], f["i"], f["j"], f["rows"], *f["R"], *f["t"], *f["sw"], f["k"]) for f in self.factors)
        var = np.ascontiguousarray(self.X, "<f8").tobytes() + np.ascontiguousarray(self.has_init, "<u4").tobytes()
        return [keys, cloud, desc, loops, factors, var]


def header_bytes(counts7, n_points, sizes, total, magic=MAGIC, version=VERSION):
    return magic + struct.pack("<II7iIQ6QQ", version, HEADER, *counts7, 0, n_points, *sizes, total)


def assemble(header, secs, sums=None):
    """header + sections + footer; sums: the six section checksums to state (None: the true ones)."""
    if sums is None:
        sums = [checksum_fast(s) for s in secs]
    foot = b"".join(struct.pack("<QQ", *s) for s in sums)
    foot += struct.pack("<QQ", *checksum(header + foot))
    return header + b"".join(secs) + foot


def write(s):
    secs = s.sections()
    c = s.counts()
    sizes = [len(x) for x in secs]
    total = HEADER + sum(sizes) + FOOTER
    hdr = header_bytes([c["n_keys"], c["n_descriptors"], s.n_search, s.counter, c["n_loop_pairs"], c["n_variables"], c["n_factors"]],
                       c["n_points"], sizes, total)
    assert len(hdr) == HEADER
    return assemble(hdr, secs)


def split(blob):
    """(header fields, the six sections' bytes, footer bytes) of a well-formed blob; ValueError on a broken structure."""
    if len(blob) < HEADER + FOOTER or blob[:8] != MAGIC:
        raise ValueError("magic")
    f = struct.unpack("<II7iIQ6QQ", blob[8:HEADER])
    if f[0] != VERSION or f[1] != HEADER or f[-1] != len(blob):
        raise ValueError("version or size")
    sizes = f[11:17]
    if HEADER + sum(sizes) + FOOTER != len(blob):
        raise ValueError("section sizes")
    secs, at = [], HEADER
    for n in sizes:
        secs.append(blob[at:at + n])
        at += n
    return dict(zip(("n_keys", "n_descriptors", "n_search", "counter", "n_loop_pairs", "n_variables", "n_factors"), f[2:9]),
                n_points=f[10], sizes=sizes, total=f[-1]), secs, blob[at:]


def parse(blob):
    """The Session a blob holds; ValueError on a broken structure or a wrong checksum."""
    hd, secs, foot = split(blob)
    for k, sec in enumerate(secs):
        if checksum_fast(sec) != struct.unpack("<QQ", foot[16 * k:16 * k + 16]):
            raise ValueError("checksum of section " + SECTIONS[k])
    if checksum(blob[:HEADER] + foot[:96]) != struct.unpack("<QQ", foot[96:112]):
        raise ValueError("checksum of the header")
    s = Session()
    n = hd["n_keys"]
    s.poses, s.times, counts = np.zeros((n, 6), np.float32), np.zeros(n, np.float64), []
    for k in range(n):
        r = struct.unpack("<6fdiI", secs[0][KEY_BYTES * k:KEY_BYTES * (k + 1)])
        s.poses[k], s.times[k] = r[:6], r[6]
        counts.append(r[7])
    words = np.frombuffer(secs[1], "<u4").reshape(-1, 8)
    at = 0
    for m in counts:
        s.clouds.append(words[at:at + m].copy())
        at += m
    assert at == words.shape[0] == hd["n_points"]
    s.desc = np.frombuffer(secs[2], "<f8").reshape(hd["n_descriptors"], 1200).copy()
    s.n_search, s.counter = hd["n_search"], hd["counter"]
    s.pairs = [struct.unpack("<ii", secs[3][8 * k:8 * k + 8]) for k in range(hd["n_loop_pairs"])]
    for k in range(hd["n_factors"]):
        r = struct.unpack("<4i19d", secs[4][FACTOR_BYTES * k:FACTOR_BYTES * (k + 1)])
        s.factors.append(dict(type=r[0], i=r[1], j=r[2], rows=r[3], R=list(r[4:13]), t=list(r[13:16]), sw=list(r[16:22]), k=r[22]))
    nv = hd["n_variables"]
    s.X = np.frombuffer(secs[5][:96 * nv], "<f8").reshape(nv, 12).copy()
    s.has_init = np.frombuffer(secs[5][96 * nv:], "<u4").copy()
    return s


def same(a, b):
    """Two sessions hold the same bits."""
    return write(a) == write(b)


# ---- the scripted session of the tests ---------------------------------------------------------------------------------

def scripted(n_keys=40, n_desc=35, seed=11):
    """About 40 keys (clouds of 0 .. 300 points, some with bits in every word and a NaN), descriptors for 35 of them, three loop
    pairs, and a graph with a prior, odometry, two plain betweens, one Cauchy between and one GPS factor."""
    rng = np.random.default_rng(seed)
    s, g = Session(), Graph()
    for k in range(n_keys):
        pose = np.array([0.5 * k, 0.1 * k * k, 0.01 * k, 0.002 * k, -0.001 * k, 0.05 * k], np.float32)
        c = rng.normal(0, 5, (int(rng.integers(0, 300)), 8)).astype(np.float32)
        if k % 3 == 0:
            c[:, 3:] = 0
        s.add_key(pose, 100.0 + 0.5 * k, c)
        g.add_odometry(pose)
    next(c for c in s.clouds if c.shape[0])[0, 1] = 0x7fc00001      # a NaN coordinate with a payload
    d = rng.uniform(0, 3, (n_desc, 1200))
    d[rng.uniform(size=d.shape) < 0.4] = 0.0
    s.desc, s.n_search, s.counter = d, n_desc - 30, 7
    s.pairs = [(20, 3), (31, 9), (39, 0)]
    g.add_between(20, 3, [0.1, 0.2, 0.0, 0.0, 0.0, 0.3], [0.04] * 6)
    g.add_between(31, 9, [-0.3, 0.1, 0.02, 0.01, 0.0, -0.2], [0.09] * 6)
    g.add_between(39, 0, [0.5, -0.4, 0.0, 0.0, 0.02, 1.1], [0.5] * 6, 1.0)
    g.add_gps(17, [8.4, 29.0, 0.2], [1.0, 1.0, 4.0])
    s.set_graph(g)
    return s
