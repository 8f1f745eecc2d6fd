"""CPU checks of the launched pose-graph optimise (include/liorf_s2m.h, s2m_pg_optimize_launch / _poll / _collect): the entry
points' null-handle answers, the two status constants, and the tail rule s2m_debug_pg_rebase - the code the library runs
when a launched optimise delivers its result - against the same formula in numpy fp64.

Bound for every element of the re-based state: 1e-12 x max(1, largest |t| involved).  Derived, not measured: fp64 unit
roundoff is 1.1e-16, about ten roundings per element act on values of that size, and the margin is three decades; it is
still five decades below a float ulp at 1 km."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _state(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def _rebase_numpy(a, b, x):
    A, At, B, Bt, X, Xt = a[:9].reshape(3, 3), a[9:], b[:9].reshape(3, 3), b[9:], x[:9].reshape(3, 3), x[9:]
    D = B @ A.T
    Dt = Bt - D @ At
    return _state(D @ X, D @ Xt + Dt)


def _check(a, b, x):
    got, want = s2m.pg_rebase(a, b, x), _rebase_numpy(a, b, x)
    bound = 1e-12 * max(1.0, float(np.abs(np.concatenate([a[9:], b[9:], x[9:], want[9:]])).max()))
    gap = float(np.abs(got - want).max())
    print("rebase gap", gap, "bound", bound)
    assert gap <= bound
    return got, bound


def test_null_handle_is_invalid_arg():
    lib = s2m.load_library()
    r = s2m.PgResult()
    assert lib.s2m_pg_optimize_launch(None, None, C.byref(r)) == -1
    assert lib.s2m_pg_optimize_launch(None, None, None) == -1
    assert lib.s2m_pg_optimize_poll(None, C.byref(r)) == -1
    assert lib.s2m_pg_optimize_collect(None, C.byref(r)) == -1
    assert lib.s2m_debug_pg_rebase(None, None, None) == -1


def test_status_constants():
    assert s2m.S2M_PG_PENDING > 0 and s2m.S2M_PG_IDLE > 0 and s2m.S2M_PG_PENDING != s2m.S2M_PG_IDLE
    assert s2m.S2M_WARN_LEAF_TOO_SMALL not in (s2m.S2M_PG_PENDING, s2m.S2M_PG_IDLE)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "liorf_s2m.h")).read()
    assert int(re.search(r"#define\s+S2M_PG_PENDING\s+(\d+)", hdr).group(1)) == s2m.S2M_PG_PENDING
    assert int(re.search(r"#define\s+S2M_PG_IDLE\s+(\d+)", hdr).group(1)) == s2m.S2M_PG_IDLE


@pytest.mark.parametrize("scale", [1.0, 100.0, 1e4])
def test_rebase_random_rotations_and_translations(scale):
    rng = np.random.default_rng(20260 + int(scale))
    for _ in range(50):
        a = _state(_rot(rng), rng.uniform(-scale, scale, 3))
        b = _state(_rot(rng), rng.uniform(-scale, scale, 3))
        x = _state(_rot(rng), rng.uniform(-scale, scale, 3))
        _check(a, b, x)


def test_rebase_without_a_correction_gives_the_state_back():
    rng = np.random.default_rng(7)
    for scale in (1.0, 1e4):
        a = _state(_rot(rng), rng.uniform(-scale, scale, 3))
        x = _state(_rot(rng), rng.uniform(-scale, scale, 3))
        got, bound = _check(a, a.copy(), x)
        assert float(np.abs(got - x).max()) <= bound


def test_rebase_pure_yaw_correction_with_a_shift():
    """The last variable of the solve turns by 0.1 rad about z and moves 50 m; a variable 3 m ahead of it follows rigidly."""
    c, s = np.cos(0.1), np.sin(0.1)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    a = _state(np.eye(3), [10.0, 20.0, 1.0])
    b = _state(Rz, [10.0 + 50.0, 20.0, 1.0])
    x = _state(np.eye(3), [13.0, 20.0, 1.0])
    got, bound = _check(a, b, x)
    want = _state(Rz, np.array([60.0, 20.0, 1.0]) + Rz @ np.array([3.0, 0.0, 0.0]))
    assert float(np.abs(got - want).max()) <= bound
