"""The stages between the ICP search and T on the device, each against a reference of its own (CPU side: tests/test_icp_close_cpu.py).

* The close (k_icp_close through s2m_debug_icp_close, 64 slots to a launch): every word of every outgoing state equal to the
  stand-alone host program's (tests/ref/icp_close_main.cpp, the host compiler alone), for every Umeyama class - the exact ranks
  0 and 1 among them - and every state-machine case of tests/ref/icp_close_ref.py, which the CPU tests hold to numpy's SVD.
* The 17 fp64 sums (one search, k_icp_sums_dev, k_icp_fold_dev through s2m_debug_icp_sums) at the edges of their stride, in the
  slot form and in the table form: the count exact, every other sum within m 2^-53 sum|term| of math.fsum over the
  correspondences the returned keys name (m = the count; products of two floats and a float d2 are exact in fp64, so this is
  the worst-case bound of any summation order), the fold a left-to-right sum of the partial rows, the rows striding the source by
  rows x 256.
* The covariance in the map frame, as the close forms it from the device's sums, against the two-pass float64 covariance.
"""
import math
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_edges_cpu import MAP_OFFSETS, moved_scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import icp_close_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
NO_MATCH = np.uint64(0xFFFFFFFFFFFFFFFF)
SLOTS = 64                                                      # S2M_LOOP_MANY_MAX_PAIRS: the slots of one launch
N_TGT = 1025
SIZES = [3, 255, 256, 257, 65536, 65537, 65793]                 # one lane, a row short / full / over, 256 rows full, a second trip
BIG = 65793


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@pytest.fixture(scope="module")
def close_exe(tmp_path_factory):
    return R.build_close_exe(tmp_path_factory.mktemp("icp_close"))


# ---- the close ----------------------------------------------------------------------------------------------------------------

def _close_on_device(gpu, cases):
    """cases: [(name, sums, state, max_iter, trans_eps, fit_eps)] -> outgoing states in the cases' order; a launch takes up to 64
    cases of one parameter set"""
    out = np.zeros((len(cases), R.STATE_WORDS), np.uint32)
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault(tuple(c[3:6]), []).append(k)
    launches = 0
    for (max_iter, te, fe), idx in groups.items():
        for a in range(0, len(idx), SLOTS):
            ks = idx[a:a + SLOTS]
            out[ks] = gpu.debugIcpClose(np.array([cases[k][1] for k in ks]), np.array([cases[k][2] for k in ks]),
                                        max_iterations=int(max_iter), transformation_epsilon=te, euclidean_fitness_epsilon=fe)
            launches += 1
    return out, launches


def _assert_words(cases, got, want):
    for c, a, b in zip(cases, got, want):
        assert np.array_equal(a, b), (c[0], R.state_fields(a), R.state_fields(b))


def test_close_of_every_umeyama_class_has_the_host_programs_words(gpu, close_exe):
    cases = R.umeyama_close_cases()
    want = R.run_close(close_exe, [c[1:] for c in cases])
    got, launches = _close_on_device(gpu, cases)
    assert launches == -(-len(cases) // SLOTS) and sum(R.is_degenerate(c[0]) for c in cases) >= 5
    _assert_words(cases, got, want)


def test_close_of_every_state_machine_case_has_the_host_programs_words(gpu, close_exe):
    cases = R.state_cases() + R.done_cases()
    want = R.run_close(close_exe, [c[1:] for c in cases])
    got, _ = _close_on_device(gpu, cases)
    _assert_words(cases, got, want)


def test_one_launch_of_done_and_live_slots(gpu, close_exe):
    """Slots that have ended between slots that have not, in one launch: the ended ones come back untouched, the others closed."""
    live = [c for c in R.state_cases() if c[3:6] == (100, R.TRANS_EPS, R.FIT_EPS)]
    done = R.done_cases()
    cases = []
    for k in range(SLOTS):
        cases.append(done[(k // 2) % len(done)] if k % 2 == 0 else live[(k // 2) % len(live)])
    want = R.run_close(close_exe, [c[1:] for c in cases])
    got, launches = _close_on_device(gpu, cases)
    assert launches == 1
    _assert_words(cases, got, want)
    for k in range(0, SLOTS, 2):
        assert np.array_equal(got[k], cases[k][2])
    assert any(not np.array_equal(got[k], cases[k][2]) for k in range(1, SLOTS, 2))


# ---- the sums -------------------------------------------------------------------------------------------------------------------

def _cloud(rng, n, half):
    p = np.zeros((n, 4), F)
    p[:, :3] = rng.uniform(-half, half, (n, 3)).astype(F)
    for k, i in enumerate(range(0, n, 7)):                        # every 7th point: a coordinate that is not finite
        p[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    return p


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(12)
    tgt = _cloud(rng, N_TGT, 20.0)
    return {n: _cloud(rng, n, 22.0) for n in SIZES}, tgt, _cloud(rng, BIG, 22.0)


def _terms(src, tgt, keys, reach):
    """The correspondences the keys name within the reach: (indices of the sources, 16 columns of fp64 terms in the sums' order)"""
    ok = keys != NO_MATCH
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok &= d2 <= reach * reach
    i = np.nonzero(ok)[0]
    j = (keys[i] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert j.size == 0 or j.max() < tgt.shape[0]
    s, t = src[i, :3].astype(np.float64), tgt[j, :3].astype(np.float64)
    assert np.isfinite(s).all() and np.isfinite(t).all()
    cols = np.concatenate([d2[i, None], s, t, (t[:, :, None] * s[:, None, :]).reshape(-1, 9)], 1)
    return i, cols


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("reach", [30.0, 1.0])
@pytest.mark.parametrize("n_src", SIZES)
def test_sums_at_the_edges_of_their_stride(gpu, clouds, n_src, reach):
    srcs, tgt, big = clouds
    src = srcs[n_src]
    slot = gpu.debugIcpSums([(src, tgt)], False, reach, want_parts=True, want_keys=True)[0]
    rows = min(-(-n_src // 256), 256)
    assert slot["rows"] == rows
    i, cols = _terms(src, tgt, slot["keys"], reach)
    m = i.size
    assert (n_src == 3 or 0 < m < n_src) and slot["sums"][0] == m             # the count, exactly
    for k in range(16):
        exact = math.fsum(cols[:, k])
        bound = m * 2.0 ** -53 * math.fsum(np.abs(cols[:, k]))
        assert abs(slot["sums"][1 + k] - exact) <= bound, (k, slot["sums"][1 + k], exact, bound)
    # the fold: the rows added left to right from zero; the rows: workgroup b sums the sources i with (i mod rows * 256) / 256 = b
    a = np.zeros(17)
    for b in range(rows):
        a = a + slot["parts"][b]
    assert _same_bits(a, slot["sums"])
    per_row = np.bincount((i % (rows * 256)) // 256, minlength=rows)
    assert np.array_equal(slot["parts"][:, 0], per_row.astype(np.float64))
    # the table form: the pair alone, and second behind a pair whose launch is larger - the bits of the slot form
    alone = gpu.debugIcpSums([(src, tgt)], True, reach, want_parts=True, want_keys=True)[0]
    behind = gpu.debugIcpSums([(big, tgt), (src, tgt)], True, reach, want_parts=True, want_keys=True)
    assert behind[0]["rows"] == 256
    for other in (alone, behind[1]):
        assert other["rows"] == rows and np.array_equal(other["keys"], slot["keys"])
        assert _same_bits(other["sums"], slot["sums"]) and _same_bits(other["parts"], slot["parts"])


def test_sums_of_several_slots_are_those_of_each_alone(gpu, clouds):
    """One source against three targets in the slot form: every slot has the sums it has alone."""
    srcs, tgt, _ = clouds
    src = srcs[257]
    tgts = [tgt, tgt[:700], np.ascontiguousarray(tgt[::-1])]
    many = gpu.debugIcpSums([(src, t) for t in tgts], False, 30.0)
    for t, got in zip(tgts, many):
        assert _same_bits(got["sums"], gpu.debugIcpSums([(src, t)], False, 30.0)[0]["sums"])


# ---- the covariance in the map frame --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", MAP_OFFSETS)
def test_covariance_in_the_map_frame(gpu, offset):
    """sigma = S8 / n - (S5 / n)(S2 / n)^T rounded to fp32, as icp_close_step forms it from the device's sums, against the
    two-pass float64 covariance of the same correspondences, 5 km, 20 km and 100 km from the origin. The raw moments are
    ~|offset|^2 there and the covariance a few m^2, so the formula cancels; the yardstick is the error of the same formula on
    numpy's own in-order fp64 sums, and the bar four times that (the device sums in another order) plus one fp32 ulp of
    max|sigma| (the rounding to fp32).
    Measured on an MI355X at the three offsets: |sigma - two-pass| 4.44e-6 / 3.60e-6 / 3.06e-6 m^2, the yardstick 2.45e-8 /
    2.18e-7 / 6.87e-6, one fp32 ulp of max|sigma| 1.53e-5, so bars of 1.54e-5 / 1.61e-5 / 4.27e-5: the error is the rounding of
    sigma to fp32 at every offset."""
    src, tgt, _ = moved_scene(1500, 700, 5, offset)
    got = gpu.debugIcpSums([(src, tgt)], False, 30.0, want_keys=True)[0]
    i, cols = _terms(src, tgt, got["keys"], 30.0)
    n = i.size
    assert n >= 600 and got["sums"][0] == n
    s, t = cols[:, 1:4], cols[:, 4:7]
    two_pass = (t - t.mean(0)).T @ (s - s.mean(0)) / n

    def raw(S):
        return S[8:17].reshape(3, 3) / S[0] - np.outer(S[5:8] / S[0], S[2:5] / S[0])

    in_order = np.concatenate([[float(n)], np.cumsum(cols, 0)[-1]])
    yard = np.abs(raw(in_order) - two_pass).max()
    sigma = raw(got["sums"]).astype(F)
    err = np.abs(sigma.astype(np.float64) - two_pass).max()
    ulp = float(np.spacing(F(np.abs(two_pass).max())))
    print(f"offset {offset}: |sigma - two-pass| {err:.3g}, numpy in-order raw moments {yard:.3g}, fp32 ulp of max|sigma| {ulp:.3g}, "
          f"bar {4 * yard + ulp:.3g}")
    assert err <= 4 * yard + ulp
