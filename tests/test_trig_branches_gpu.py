"""The device's sinf / cosf (glibc_sincosf of s2m_device.hpp, through s2m_abi_debug.hip's k_debug_sincos hook) on every branch of the restated
arithmetic, against the test host's libm the way tests/test_parity_gpu.py::test_device_trig_is_the_hosts compares them, bit for
bit: the neighbours (three ulps each side, both signs) of the branch boundaries 2^-12, 0x1.921FB6p-1 (pi/4) and 120, k*pi/2
with its neighbours (two ulps each side) for k = -76..76 - every quadrant and both coefficient sets - and 1e5 pose-like
angles in [-0.05, 0.05].

The arguments at which the restated reduction and glibc's differ (tests/test_trig_host_cpu.py holds the set: six arguments
one ulp from 37, 41 and 74 times pi/2) are compared with the host build of the same statement's results instead: there the
device has to give what the host twin gives."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m
from test_trig_host_cpu import ADMITTED

pytestmark = pytest.mark.gpu


def _step(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


def _arguments():
    xs = []
    for e in (np.float32(2.0 ** -12), np.float32(float.fromhex("0x1.921FB6p-1")), np.float32(120.0)):
        for d in range(-3, 4):
            v = _step(e, d)
            xs += [v, -v]
    for k in range(-76, 77):
        base = np.float32(k * float.fromhex("0x1.921FB54442D18p0"))
        xs += [_step(base, d) for d in range(-2, 3)]
    pose_like = np.random.default_rng(11).uniform(-0.05, 0.05, 100000).astype(np.float32)
    return np.concatenate([np.array(xs, np.float32), pose_like])


def test_every_branch_is_the_hosts_libm():
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = C.c_float; libm.sinf.argtypes = [C.c_float]
    libm.cosf.restype = C.c_float; libm.cosf.argtypes = [C.c_float]
    x = _arguments()
    g = s2m.MapOptimizationS2M()
    try:
        sn, cs, _ = g.deviceTrig(x)
    finally:
        g.close()
    ref_s = np.array([libm.sinf(v) for v in x.tolist()], np.float32)
    ref_c = np.array([libm.cosf(v) for v in x.tolist()], np.float32)
    bits = x.view(np.uint32)
    known_s = np.isin(bits, [int(a, 16) for a, w in ADMITTED if "s" in w])
    known_c = np.isin(bits, [int(a, 16) for a, w in ADMITTED if "c" in w])
    bad_s = sn.view(np.uint32) != ref_s.view(np.uint32)
    bad_c = cs.view(np.uint32) != ref_c.view(np.uint32)
    print("arguments", x.size, "sin mismatches", int(bad_s.sum()), "cos mismatches", int(bad_c.sum()),
          [hex(b) for b in bits[bad_s | bad_c]])
    # off the admitted arguments: libm's bits; on them: a mismatch, as on the host (the same statement gives the same bits)
    assert not (bad_s & ~known_s).any() and not (bad_c & ~known_c).any()
    assert bad_s[known_s].all() and bad_c[known_c].all()
    assert known_s.sum() == 2 and known_c.sum() == 4
