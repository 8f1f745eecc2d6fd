"""The LM closing step on the device against the oracle's orc_lm_close, bit for bit.

s2m_debug_lm_close hands the device the partial sums of one iteration and runs what the loop runs: k_finalize (form 0)
or the prologue of the next fused registration launch (form 1).  Everything the close writes - matAtA / matAtB, the count,
the step, the pose, deltaR / deltaT, the flags, at iteration 0 isDegenerate and matP - is compared with the oracle on the
same fp32 normal equations as 32-bit patterns (a NaN matches any NaN).  The cases are tests/ref/lm_close_cases.py;
tests/test_lm_close_cpu.py shows on the CPU that they sit where they claim to sit.

Cases run (the tests assert these numbers, nothing is skipped): on the scan that takes the 8-wave workgroup shape
(131 072 points, 256 active rows) every case in form 0 - a 22 (a_rows257, a_rows511 and a_rows512 ask for more rows than
any scan has active workgroups, 256 at most in either shape: they are answered S2M_ERR_INVALID_ARG, which is asserted, so
19 run), b 336, c 145, d 13, e 34 - and in form 1 every case of a, b, d, e with iter >= 1 whose pose the oracle calls
finite and within 100 m / pi rad: a 16, b 327, d 13, e 34.  On the scan above 2 048 wave-table entries (140 000 points,
16-wave shape) the a and b cases again: form 0 a 17 + b 336 (a_rows255 / a_rows256 need more rows than that scan has),
form 1 a 14 + b 327.  Through the public ABI: the persistence sequence (five registrations and a wall on one handle) and
13 threshold scenes, all 13 compared (none lies within 1e-3 of the threshold).

Measured on the MI355X: the file runs in 1.0 s of the GPU suite's 139 s.  With the device library's own hypotf in
eigen6_sym (the state before glibc_hypotf) test_degeneracy_analysis fails on 35 of its 145 cases: matP off by 1 .. 1 208
ulps, the projected step by up to 2 531 ulps, isDegenerate itself on two (c_qr_100+2ulp, c_qr_pair_at_100).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import lm_close_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_ITER = 30


def _same(a, b):
    a, b = np.ascontiguousarray(a, F32).ravel(), np.ascontiguousarray(b, F32).ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _ulps(a, b):
    """Largest distance in fp32 steps between two arrays (inf when only one side is NaN)."""
    a, b = np.ascontiguousarray(a, F32).ravel(), np.ascontiguousarray(b, F32).ravel()
    both, one = np.isnan(a) & np.isnan(b), np.isnan(a) ^ np.isnan(b)
    if one.any():
        return math.inf
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    d[both] = 0
    return int(d.max()) if d.size else 0


def _resident(n_q, seed=5):
    """A map and a scan for the hook to sit on: ground, two walls, n_q scan points."""
    m, _ = LC.scene_threshold(150)
    rng = np.random.default_rng(seed)
    q = np.concatenate([LC._ground(rng, n_q - n_q // 4, 25.0), LC._wall_x(rng, n_q // 4, half=8.0)]).astype(F32)
    return m, q


@pytest.fixture(scope="module")
def gpu8():
    g = s2m.MapOptimizationS2M()
    m, q = _resident(131072)
    g.setInputCloud(m)
    g.setScan(q)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gpu16():
    g = s2m.MapOptimizationS2M()
    m, q = _resident(140000)
    g.setInputCloud(m)
    g.setScan(q)
    yield g
    g.close()


def check_case(gpu, case, form, AtA=None, AtB=None, n_sel=None):
    """Runs the case on the device; returns the list of fields that differ from the oracle (empty: all bits agree)."""
    prm = LC.params_of(case)
    gpu.setParams(**prm)
    try:
        out = gpu.lmClose(form, case.it, case.rows, case.pose0, case.degen_in, case.matP_in)
    finally:
        gpu.setParams(**LC.DEFAULTS)
    bad = []
    if case.inexact:                                        # the derived bar: any order of n - 1 fp64 additions
        lo, hi = LC.inexact_bounds(case.rows)
        got = np.array([out.AtA[a * 6 + b] for a, b in LC.UT] + list(out.AtB), F32)
        low = np.array([out.AtA[b * 6 + a] for a, b in LC.UT], F32)
        if not (np.all(got >= lo) and np.all(got <= hi)):
            bad.append(("sums outside the bound", got, lo, hi))
        if not _same(got[:21], low):
            bad.append(("AtA not symmetric", got[:21], low))
        return bad
    if AtA is None:
        AtA, AtB, n_sel = LC.intended(case.rows) if case.rows.shape[0] else (np.zeros((6, 6), F32), np.zeros(6, F32), 0)
    conv, pose, dg, matP, tr = LC.oracle_close(O, case, AtA, AtB, n_sel)

    def cmp(name, got, want):
        if not _same(got, want):
            bad.append((name, _ulps(got, want), np.array(got, F32), np.array(want, F32)))

    def eq(name, got, want):
        if int(got) != int(want):
            bad.append((name, int(got), int(want)))

    cmp("AtA", out.AtA, AtA)
    cmp("AtB", out.AtB, AtB)
    eq("n_sel_last", out.n_sel_last, n_sel)
    eq("trace.n_sel", out.trace.n_sel, tr.n_sel)
    eq("trace.stepped", out.trace.stepped, tr.stepped)
    cmp("delta", out.trace.delta, tr.delta)
    cmp("trace.pose", out.trace.pose, tr.pose)
    cmp("deltaR", [out.trace.deltaR], [tr.deltaR])
    cmp("deltaT", [out.trace.deltaT], [tr.deltaT])
    cmp("pose", out.pose, pose)
    stepped = tr.stepped != 0
    if stepped:
        cmp("pose_next", out.pose_next, pose)
    elif not np.all(np.isnan(np.array(out.pose_next))):
        bad.append(("pose_next written by a close that did not step", np.array(out.pose_next)))
    eq("stalled", out.stalled, 0 if stepped else 1)
    eq("converged", out.converged, conv)
    eq("done", out.done, 1 if (not stepped or (conv and prm["early_exit"])) else 0)
    eq("iters_run", out.iters_run, case.it + 1 if stepped else MAX_ITER)
    eq("isDegenerate", out.is_degenerate, dg)
    if case.it == 0 and stepped:
        # Degenerate: the oracle's matP.  Not degenerate: the Cholesky shortcut (all eigenvalues above eig_thresh + 1e-5 x trace)
        # leaves matP alone - it is not read before the next iteration 0 - and otherwise the full analysis writes the oracle's;
        # well inside either side of the shortcut's margin the test says which of the two it has to be.
        kept, full = _same(out.matP, case.matP_in), _same(out.matP, matP)
        side = 0
        if np.all(np.isfinite(AtA)):
            w = np.linalg.eigvalsh(np.asarray(AtA, np.float64))
            trace, th = float(np.trace(np.asarray(AtA, np.float64))), float(F32(prm["eig_thresh"]))
            if 0.0 < trace < 1e29 and w[0] > th + 2e-5 * trace:
                side = 1
            elif not (0.0 < trace < 1e31) or w[0] < th + 0.5e-5 * trace:
                side = -1
        if dg or side < 0:
            cmp("matP", out.matP, matP)
        elif side > 0:
            cmp("matP kept (shortcut)", out.matP, case.matP_in)
        elif not (kept or full):
            bad.append(("matP neither kept nor the oracle's", _ulps(out.matP, matP)))
    else:                                                   # not written: later iterations, a stall
        cmp("matP kept", out.matP, case.matP_in)
    return bad


def run_family(gpu, fams, forms, expect):
    ran, failed = {}, []
    active = gpu.lmClose(0, 1, np.zeros((1, 28)), LC.POSE0, 0, LC.IDENT).n_rows_active
    for case in LC.all_cases():
        if case.fam not in fams:
            continue
        if case.rows.shape[0] > active:                     # more rows than this scan has active workgroups: refused, not run
            with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
                gpu.lmClose(0, case.it, case.rows, case.pose0, case.degen_in, case.matP_in)
            continue
        for form in forms:
            if form == 1 and (case.inexact or not LC.form1_ok(case, LC.oracle_close(O, case)[1])):
                continue
            bad = check_case(gpu, case, form)
            ran[(case.fam, form)] = ran.get((case.fam, form), 0) + 1
            if bad:
                failed.append((case.name, form, bad))
    print("cases run (family, form):", sorted(ran.items()), "active rows:", active)
    for name, form, bad in failed[:40]:
        print("MISMATCH", name, "form", form, [(b[0], b[1]) for b in bad])
    assert not failed, f"{len(failed)} case/form pairs differ from the oracle; first: {failed[0]}"
    assert ran == expect, (ran, expect)


def test_reduction_and_fill(gpu8):
    run_family(gpu8, "a", (0, 1), {("a", 0): 19, ("a", 1): 16})


def test_qr_solve(gpu8):
    run_family(gpu8, "b", (0, 1), {("b", 0): 336, ("b", 1): 327})


def test_degeneracy_analysis(gpu8):
    run_family(gpu8, "c", (0,), {("c", 0): 145})


def test_later_iterations(gpu8):
    run_family(gpu8, "d", (0, 1), {("d", 0): 13, ("d", 1): 13})


def test_convergence(gpu8):
    run_family(gpu8, "e", (0, 1), {("e", 0): 34, ("e", 1): 34})


def test_sixteen_wave_shape(gpu16):
    run_family(gpu16, "ab", (0, 1), {("a", 0): 17, ("a", 1): 14, ("b", 0): 336, ("b", 1): 327})


def test_both_forms_give_the_same_record(gpu8):
    """Form 0 and form 1 against each other directly (not only each against the oracle), on the 256-row case."""
    case = next(c for c in LC.all_cases() if c.name == "a_rows256")
    a = gpu8.lmClose(0, case.it, case.rows, case.pose0, 0, LC.IDENT)
    b = gpu8.lmClose(1, case.it, case.rows, case.pose0, 0, LC.IDENT)
    assert a.n_rows_active == 256
    assert bytes(a) == bytes(b)


def test_the_handle_stays_usable():
    """A registration after the hook (both forms, a stall, a degenerate iteration 0) is the registration of a handle that
    never saw it, bit for bit; isDegenerate / matP that persist from scan to scan are not touched."""
    cfg = synth.make_config("small")
    m, s = synth.to_xyzi(cfg["map"]), synth.to_xyzi(cfg["scan"])

    def register(g):
        g.transformTobeMapped = cfg["pose_init"].copy()
        r = g.scan2MapOptimization()
        return bytes(r), [bytes(t) for t in g.trace()]

    used, fresh = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for g in (used, fresh):
            g.setInputCloud(m)
            g.setScan(s)
        byname = {c.name: c for c in LC.all_cases()}
        for name, form in (("b_rand0", 0), ("b_rand1", 1), ("a_stall_it3", 0), ("c_qr_3_below", 0), ("d_it29_degen1_full", 1),
                           ("e_Rin_Tin_early1", 1), ("b_nan_entry", 0)):
            c = byname[name]
            used.setParams(**LC.params_of(c))
            used.lmClose(form, c.it, c.rows, c.pose0, c.degen_in, c.matP_in)
        used.setParams(**LC.DEFAULTS)
        assert register(used) == register(fresh)
        assert register(used) == register(fresh)
    finally:
        used.close()
        fresh.close()


def _registration_matches(g, orc, m, q, pose, what):
    g.setInputCloud(m)
    g.setScan(q)
    orc.set_map(m)
    orc.set_scan(q)
    g.transformTobeMapped = np.array(pose, F32)
    r, ro = g.scan2MapOptimization(), orc.scan2MapOptimization(pose)
    assert (r.skipped, r.is_degenerate) == (ro.skipped, ro.is_degenerate), what
    return r, ro


def test_degeneracy_persists_across_scans_like_the_members():
    """isDegenerate and matP are members of the reference's node: a scan that never reaches the analysis (too few
    correspondences, too few points, no map) reports the flag of the scan before it; an ordinary scan clears it; and a scan
    that is degenerate in another subspace rebuilds matP instead of carrying the old one.  Public ABI only, one handle and
    one Oracle object all the way through."""
    g, orc = s2m.MapOptimizationS2M(), O.Oracle(knn_backend=1, num_threads=8)
    try:
        flags = []
        for name, m, q, pose in LC.persistence_sequence():
            r, ro = _registration_matches(g, orc, m, q, pose, name)
            flags.append(r.is_degenerate)
            assert (r.iters_run, r.converged) == (ro.iters_run, ro.converged), name
        assert flags == [1, 1, 1, 1, 0]
        m, q = LC.scene_wall()
        r, ro = _registration_matches(g, orc, m, q, LC.SCENE_POSE, "single wall")
        assert r.is_degenerate == 1 and r.iters_run == ro.iters_run
        tg, to = g.trace(), orc.trace()
        assert len(tg) == len(to) == r.iters_run
        for a, b in zip(tg, to):
            assert np.abs(np.array(a.delta) - np.array(b.delta)).max() <= 1e-4
        # iteration 0 of the wall on the device's own normal equations: the close against the oracle's, matP included
        AtA, AtB, n = g.normal_eq(LC.SCENE_POSE)
        case = LC.Case("wall_iteration0", "c", LC.spread_rows(LC.sums_of(AtA, AtB, n)), it=0, pose0=LC.SCENE_POSE.copy(),
                       degen_in=0, matP_in=np.full((6, 6), 1.0e6, F32), form0_only=True)
        assert check_case(g, case, 0) == []
        assert LC.oracle_close(O, case)[2] == 1
    finally:
        g.close()


def test_threshold_scenes():
    """The wall patches step the smallest eigenvalue of iteration 0 across eig_thresh: the flag, the iteration count and
    convergence are the oracle's.  Only a scene whose fp64 l_min (of the ORACLE's matAtA) lies within 1e-3 relative of the
    threshold is left out - there the order of the fp64 sums, which legitimately differs, can move an fp32 entry by an ulp;
    tests/test_lm_close_cpu.py asserts that at most 2 of the scenes are such."""
    g = s2m.MapOptimizationS2M()
    compared = 0
    try:
        for n in LC.PATCH_SIZES:
            m, q = LC.scene_threshold(n)
            _, _, _, lmin = LC.iteration0_lmin(O, m, q, LC.SCENE_POSE)
            orc = O.Oracle(knn_backend=1, num_threads=8)
            g.setInputCloud(m)
            g.setScan(q)
            orc.set_map(m)
            orc.set_scan(q)
            g.transformTobeMapped = LC.SCENE_POSE.copy()
            r, ro = g.scan2MapOptimization(), orc.scan2MapOptimization(LC.SCENE_POSE)
            print("patch", n, "l_min", lmin, "device", (r.is_degenerate, r.iters_run, r.converged), "oracle", (ro.is_degenerate, ro.iters_run, ro.converged))
            if abs(lmin - 100.0) <= 1e-3 * 100.0:
                continue
            compared += 1
            assert (r.is_degenerate, r.iters_run, r.converged) == (ro.is_degenerate, ro.iters_run, ro.converged), n
        assert compared >= len(LC.PATCH_SIZES) - 2
    finally:
        g.close()


def test_hook_needs_a_scan_and_a_map():
    g = s2m.MapOptimizationS2M()
    try:
        with pytest.raises(s2m.S2MError, match="NO_SCAN"):
            g.lmClose(0, 1, np.zeros((1, 28)), LC.POSE0, 0, LC.IDENT)
        g.setParams(max_iter=5)
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):        # iter outside 0 .. max_iter-1 of the CURRENT parameters
            g.lmClose(0, 5, np.zeros((1, 28)), LC.POSE0, 0, LC.IDENT)
    finally:
        g.close()


def test_device_hypot_is_the_hosts(gpu8):
    """cv::eigen's rotations call the host's hypotf; the device computes it with glibc's arithmetic (glibc_hypotf).  The
    results have to be the test host's libm results bit for bit, over the exponents the Jacobi sweep sees."""
    libm = C.CDLL("libm.so.6")
    libm.hypotf.restype = C.c_float
    libm.hypotf.argtypes = [C.c_float, C.c_float]
    rng = np.random.default_rng(11)
    n = 120000
    p = (10.0 ** rng.uniform(-7, 6, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    y = (10.0 ** rng.uniform(-9, 7, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    y[::50] = 0.0
    y[1::50] = -0.0
    k = n // 2                                              # half of them with both arguments of similar size
    y[:k:2] = (p[:k:2] * rng.uniform(0.25, 4.0, len(p[:k:2]))).astype(F32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1e38, 3e38, 1.0], F32)
    p = np.concatenate([p, np.repeat(sp, len(sp))])
    y = np.concatenate([y, np.tile(sp, len(sp))])
    got = gpu8.deviceHypot(p, y)
    want = np.array([libm.hypotf(a, b) for a, b in zip(p.tolist(), y.tolist())], F32)
    diff = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert len(p) >= 100000 and diff.sum() == 0, (int(diff.sum()), p[diff][:5], y[diff][:5], got[diff][:5], want[diff][:5])
