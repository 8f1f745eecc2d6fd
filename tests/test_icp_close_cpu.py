"""The close of an ICP iteration (liorf_amd/csrc/s2m_icp_close.hpp: Umeyama, the float composition of T, PCL's convergence state
machine), built stand-alone by the host compiler, against a float64 reference that shares none of its arithmetic
(tests/ref/icp_close_ref.py: numpy.linalg.svd, and the state machine restated from the contract). The device runs the same
cases in tests/test_icp_close_gpu.py, held word for word to the stand-alone program.

Bars (none of them taken from the code under test):
* |R R^T - I| and |det R - 1| <= 4e-7: nine fp32 roundings of at most 2^-25 each on entries <= 1, through a 3-term product,
  times two.
* tr(R^T sigma) >= s1 + s2 + d s3 - 4e-7 s1: R is optimal (d = sign(det U det V^T)).
* |R - R_ref| <= 2^-24 where the rotation is determined: min over i < j of (s_i + d_j s_j) >= 1e-3 s1.
* |t - t_ref| <= 2^-23 (|mean_tgt| + |R| |mean_src|) wherever R was compared, in Euclidean norms (|R| = 1): an entry of R is
  off by up to 2^-25 whatever its size, so the error of a component of t scales with |mean_src|, not with that row's |R_ij|.
* sigma = 0 exactly: R = I bit for bit.
* T words equal to tests/golden/icp_umeyama_bits.npz (recorded before U was completed for rank 0 and 1) wherever the
  cross-covariance is not of exact rank 0 or 1.
* done, conv, it, similar equal to the restatement's wherever the deciding quantity is more than 1e-6 (relative) from its
  threshold; T_step and T within 2^-23 max|entry| of the float64 composition where an iteration ran.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_grid_cpu import _umeyama_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import icp_close_ref as R  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "icp_umeyama_bits.npz")
ROT_BAR = 4e-7


@pytest.fixture(scope="module")
def close_exe(tmp_path_factory):
    return R.build_close_exe(tmp_path_factory.mktemp("icp_close"))


@pytest.fixture(scope="module")
def umeyama_T(close_exe):
    """T of every class case by the stand-alone program: (cases, T float32 (n, 4, 4))"""
    cases = R.umeyama_classes()
    T = R.run_umeyama(close_exe, [c[1:] for c in cases])
    return cases, T.view(F).reshape(-1, 4, 4)


def rotation_defect(Rm):
    Rm = np.asarray(Rm, np.float64)
    return max(np.abs(Rm @ Rm.T - np.eye(3)).max(), abs(np.linalg.det(Rm) - 1.0))


# ---- Umeyama --------------------------------------------------------------------------------------------------------------

def test_classes_are_what_they_say():
    """The classes hold what their names say, by numpy alone: the exact degenerate ones have zero singular values (rank 0: all,
    rank 1: two, exactly), the others rank >= 2 above fp32 rounding noise of the largest."""
    cases = R.umeyama_classes()
    names = [c[0] for c in cases]
    for want in ("random", "rank2", "noisy_rank1", "equal_s", "two_equal_s", "near_reflection", "ratio_1e7", "tiny", "huge",
                 "exact_rank0_zero", "exact_rank1_diag200", "exact_rank1_e1e2T", "exact_rank1_e1vT", "exact_diag110",
                 "exact_minus_identity", "exact_diag_3_2_-1e-20", "exact_subnormal"):
        assert want in names
    for name, _, _, sg in cases:
        A = sg.astype(np.float64)
        nz_rows, nz_cols = int(np.any(A != 0, 1).sum()), int(np.any(A != 0, 0).sum())
        if name.startswith("exact_rank0"):
            assert not A.any()
        elif R.is_degenerate(name):
            assert min(nz_rows, nz_cols) == 1                  # one non-zero row or column: rank 1 with no rounding in it
        else:
            s = np.linalg.svd(A, compute_uv=False)
            assert s[0] > 0 and (name == "noisy_rank1" or s[1] > 1e-9 * s[0]), (name, s)
    sub = dict((c[0], c[3]) for c in cases)["exact_subnormal"]
    assert np.all(np.abs(sub) < np.finfo(F).tiny) and np.count_nonzero(sub) >= 6


def test_umeyama_returns_an_optimal_rotation(umeyama_T):
    cases, T = umeyama_T
    worst_rot, worst_opt = 0.0, 0.0
    for (name, ms, mt, sg), Tk in zip(cases, T):
        Rk = Tk[:3, :3].astype(np.float64)
        _, _, s, d = R.umeyama_ref(ms, mt, sg)
        defect = rotation_defect(Rk)
        worst_rot = max(worst_rot, defect)
        assert defect <= ROT_BAR, (name, sg, Tk)
        assert np.array_equal(Tk[3], np.array([0, 0, 0, 1], F))
        if s[0] > 0:
            short = ((s[0] + s[1] + d * s[2]) - np.trace(Rk.T @ sg.astype(np.float64))) / s[0]
            worst_opt = max(worst_opt, short)
            assert short <= ROT_BAR, (name, sg, short)
    print(f"worst |R R^T - I| or |det R - 1| {worst_rot:.3g}, worst optimality shortfall {worst_opt:.3g} s1 (bars {ROT_BAR:g})")


def test_umeyama_against_the_float64_reference(umeyama_T):
    cases, T = umeyama_T
    compared, plain, worst_R, worst_t = 0, 0, 0.0, 0.0
    for (name, ms, mt, sg), Tk in zip(cases, T):
        Rr, tr, s, d = R.umeyama_ref(ms, mt, sg)
        exact = name.startswith("exact_")
        plain += not exact
        if s[0] == 0 or not R.determined(s, d):
            continue
        compared += not exact
        dR = np.abs(Tk[:3, :3].astype(np.float64) - Rr).max()
        bar_t = 2.0 ** -23 * (np.linalg.norm(mt.astype(np.float64)) + np.linalg.norm(Rr, 2) * np.linalg.norm(ms.astype(np.float64)))
        dt = np.abs(Tk[:3, 3].astype(np.float64) - tr).max()
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt / bar_t)
        assert dR <= 2.0 ** -24, (name, sg, dR)
        assert dt <= bar_t, (name, sg, dt, bar_t)
    print(f"R compared in {compared} of {plain} non-degenerate cases: worst |R - R_ref| {worst_R:.3g} (bar {2.0 ** -24:.3g}), "
          f"worst |t - t_ref| {worst_t:.3g} of its bar")
    assert compared >= 0.8 * plain


def test_a_zero_covariance_gives_the_identity_bit_for_bit(umeyama_T):
    cases, T = umeyama_T
    hit = 0
    for (name, ms, mt, sg), Tk in zip(cases, T):
        if sg.any():
            continue
        hit += 1
        assert np.array_equal(Tk[:3, :3].view(np.uint32), np.eye(3, dtype=F).view(np.uint32))
        assert np.array_equal(Tk[:3, 3], mt - ms)              # t = mean_tgt - I mean_src: (1 * x + 0 * y) + 0 * z is x
    assert hit >= 1


def test_one_target_at_the_origin_and_targets_on_an_axis(close_exe):
    """The scenes the defect showed in: 50 sources on one target at the origin (sigma exactly zero), on targets (+-1, 0, 0) and on
    40 targets along the x axis (rows 1 and 2 of sigma exactly zero). One iteration ends converged with a rigid T."""
    rng = np.random.default_rng(5)
    src = rng.normal(0, 2, (50, 3)).astype(F).astype(np.float64)
    scenes = {"origin": np.zeros((1, 3)), "pm1": np.array([[1.0, 0, 0], [-1.0, 0, 0]]),
              "x_axis": np.stack([np.linspace(-4, 4, 40).astype(F).astype(np.float64), np.zeros(40), np.zeros(40)], 1)}
    todo = []
    for name, tgt in scenes.items():
        j = ((src[:, None, :] - tgt[None, :, :]) ** 2).sum(2).argmin(1)
        d2 = ((src - tgt[j]) ** 2).sum(1)
        todo.append((R.sums_of(src, tgt[j], d2.sum()), R.state_words(), 1, 1e-6, 1e-6))
    out = R.run_close(close_exe, todo)
    for name, w in zip(scenes, out):
        f = R.state_fields(w)
        assert (f["done"], f["conv"], f["it"]) == (1, 1, 1), name
        assert rotation_defect(f["T"][:3, :3]) <= ROT_BAR, (name, f["T"])
        assert np.array_equal(f["T"].view(np.uint32), f["T_step"].view(np.uint32))
        if name == "origin":
            assert np.array_equal(f["T"][:3, :3], np.eye(3, dtype=F))


def test_rank_two_and_three_keep_the_recorded_bits(close_exe):
    """Every non-degenerate class case and every case of test_icp_grid_cpu._umeyama_cases() gives the T words recorded before
    host_svd3 completed U for rank 0 and rank 1 (tests/golden/make_golden_icp_umeyama.py); the degenerate rows are excepted."""
    g = np.load(GOLDEN)
    names, inputs, want = g["names"], g["inputs"], g["T"]
    ours = [(n, np.concatenate([ms, mt, sg.reshape(-1)])) for n, ms, mt, sg in R.umeyama_classes() if not R.is_degenerate(n)]
    ours += [(f"grid_cpu_{k}", np.concatenate([ms, mt, sg.reshape(-1)])) for k, (ms, mt, sg) in enumerate(_umeyama_cases())]
    assert [n for n, _ in ours] == list(names)
    assert np.array_equal(np.array([r for _, r in ours], F).view(np.uint32), inputs.view(np.uint32))     # the fixture's inputs are today's
    got = R.run_umeyama(close_exe, [(r[0:3], r[3:6], r[6:15]) for r in inputs])
    checked = 0
    for n, r, a, b in zip(names, inputs, got, want):
        sg = r[6:15].reshape(3, 3)
        if min(int(np.any(sg != 0, 1).sum()), int(np.any(sg != 0, 0).sum())) <= 1:     # exact rank 0 or 1 (in _umeyama_cases)
            continue
        checked += 1
        assert np.array_equal(a, b), (n, sg, a.view(F), b.view(F))
    assert checked >= len(names) - 4


# ---- the state machine ----------------------------------------------------------------------------------------------------

def test_state_machine_against_the_restatement(close_exe):
    cases = R.state_cases() + R.done_cases()
    out = R.run_close(close_exe, [c[1:] for c in cases])
    in_band, worst_T = [], 0.0
    for (name, S, st, max_iter, te, fe), w in zip(cases, out):
        f_in, f = R.state_fields(st), R.state_fields(w)
        if f_in["done"]:
            assert np.array_equal(w, st), name                 # a slot that has ended is not touched
            continue
        ref = R.close_ref(S, f_in, max_iter, te, fe)
        if ref["ran"]:
            for key in ("T_step", "T"):
                err = np.abs(f[key].astype(np.float64) - ref[key]).max() / np.abs(ref[key]).max()
                worst_T = max(worst_T, err)
                assert err <= 2.0 ** -23, (name, key, err)
        else:
            assert np.array_equal(w[0:34], st[0:34]), name      # T, T_step and prev_mse stay as they were
        if ref["margin"] <= 1e-6:
            in_band.append(name)
            continue
        assert (f["done"], f["conv"], f["it"], f["similar"]) == (ref["done"], ref["conv"], ref["it"], ref["similar"]), (name, f, ref)
        assert f["prev_mse"] == ref["prev_mse"], name
    print(f"{len(in_band)} of {len(cases)} cases inside the 1e-6 band: {in_band}; worst |T - T_ref| / max|T_ref| {worst_T:.3g} (bar {2.0 ** -23:.3g})")
    assert len(in_band) <= len(cases) // 4


def test_state_cases_sit_on_both_sides_of_every_threshold():
    """By the restatement alone: each threshold is decided both ways outside the band, and the special exits are all taken."""
    seen = {}
    for name, S, st, max_iter, te, fe in R.state_cases():
        ref = R.close_ref(S, R.state_fields(st), max_iter, te, fe)
        if ref["margin"] > 1e-6:
            seen.setdefault(name.split("_")[0], set()).add((ref["done"], ref["conv"]))
    for key in ("rot", "trl", "abs", "rel"):
        assert seen[key] == {(0, 0), (1, 1)}, (key, seen[key])
    assert seen["cnt"] == {(1, 0), (0, 0)} and (1, 1) in seen["cap"] and (0, 0) in seen["cap"] and seen["first"] == {(0, 0), (1, 1)}


def test_umeyama_classes_through_the_close_give_umeyamas_bits(close_exe, umeyama_T):
    """The sums tests/test_icp_close_gpu.py hands the device for the Umeyama classes reproduce sigma exactly, so the close's
    T_step is host_umeyama's T for (mean_src, mean_tgt, sigma) of the case."""
    cases, _ = umeyama_T
    todo = R.umeyama_close_cases()
    out = R.run_close(close_exe, [c[1:] for c in todo])
    direct = R.run_umeyama(close_exe, [c[1:] for c in R.umeyama_close_inputs()])
    assert len(todo) == len(cases)
    for (name, *_), w, d in zip(todo, out, direct):
        assert np.array_equal(w[16:32], d), name


# ---- the hooks' boundary ------------------------------------------------------------------------------------------------------

NEW = ["s2m_debug_icp_close", "s2m_debug_icp_close_check_args", "s2m_debug_icp_sums", "s2m_debug_icp_sums_check_args"]


def test_hooks_declared_bound_and_exported():
    lib = C.CDLL(s2m.LIB_PATH)
    dbg = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    for n in NEW:
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, dbg)
    assert C.sizeof(s2m.IcpLoopStateWords) == 4 * R.STATE_WORDS


def test_hook_argument_checks_need_no_gpu():
    lib = s2m.load_library()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    sums, st = np.zeros((2, 17)), np.zeros((2, R.STATE_WORDS), np.uint32)
    prm = s2m.IcpParams(30.0, 100, 1e-6, 1e-6)
    chk = lib.s2m_debug_icp_close_check_args
    ok = (sums.ctypes.data_as(dp), st.ctypes.data, C.byref(prm), st.ctypes.data)
    assert chk(2, *ok) == 0 and chk(64, *ok) == 0
    assert chk(0, *ok) == -1 and chk(65, *ok) == -1
    for k in range(4):
        bad = list(ok)
        if k == 2:
            continue                                           # (null parameters: the defaults)
        bad[k] = None
        assert chk(2, *bad) == -1, k
    assert chk(2, ok[0], ok[1], None, ok[3]) == 0
    assert chk(2, ok[0], ok[1], C.byref(s2m.IcpParams(30.0, 0, 1e-6, 1e-6)), ok[3]) == -1
    pts = np.zeros((5, 4), F)
    ptr = (vp * 2)(pts.ctypes.data, pts.ctypes.data)
    ns = (C.c_size_t * 2)(5, 5)
    out = np.zeros((2, 17))
    nrows = np.zeros(2, np.int32)
    chk2 = lib.s2m_debug_icp_sums_check_args
    args = dict(srcs=ptr, n_srcs=ns, tgts=ptr, n_tgts=ns, n_pairs=2, stride=16, form=1, sums=out.ctypes.data_as(dp),
                n_rows=nrows.ctypes.data_as(C.POINTER(C.c_int32)))
    call = lambda **kw: chk2(*[{**args, **kw}[k] for k in ("srcs", "n_srcs", "tgts", "n_tgts", "n_pairs", "stride", "form", "sums", "n_rows")])  # noqa: E731
    assert call() == 0 and call(form=0) == 0
    assert call(form=2) == -1 and call(n_pairs=0) == -1 and call(n_pairs=65) == -1 and call(form=0, n_pairs=9) == -1
    assert call(stride=8) == -1 and call(stride=18) == -1 and call(sums=None) == -1 and call(n_rows=None) == -1
    assert call(srcs=None) == -1 and call(n_tgts=None) == -1
    assert call(n_srcs=(C.c_size_t * 2)(5, 0)) == -1           # an empty cloud has no sums
    two = (vp * 2)(pts.ctypes.data, pts[1:].ctypes.data)
    assert call(form=0, srcs=two) == -1                        # the slot form has one source


def test_hooks_reject_a_null_handle():
    lib = s2m.load_library()
    assert lib.s2m_debug_icp_close(None, 1, None, None, None, None) == -1
    assert lib.s2m_debug_icp_sums(None, None, None, None, None, 1, 16, 0, 0.0, None, None, None, None) == -1
