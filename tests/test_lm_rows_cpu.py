"""CPU companions of tests/test_lm_rows_gpu.py: the float statement of the Jacobian row and of the partial-row sums
(tests/ref/lm_rows_ref.py) held against the oracle and against finite differences at the attitudes the GPU tests use, and the
proof that the row sums tell a wrong Jacobian term from a right one.

Why the file exists: test_the_old_bar_lets_a_sign_flip_through flips the sign of srx*sry*srz in arx.  At the suite's one
attitude (synth.POSE_GT + POSE_DELTA: roll 0.02, pitch -0.025, yaw 0.32) matAtA and matAtB of the flipped Jacobian still pass
the allclose(rtol 1e-5, atol 1e-5 max) of test_parity_gpu.py::test_normal_equations - every term with two small sines in it is
invisible there - while the partial-row bound of expected_rows catches it at that very attitude by orders of magnitude.
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
import lm_rows_ref as LR  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def cases(cfg_tiny):
    """Per attitude: the tiny scene there, and per pose (pose_init, pose_gt) the oracle's correspondences."""
    out = {}
    for name, rpy in LR.ATTITUDES.items():
        cfg = LR.at_attitude(cfg_tiny, rpy)
        orc = O.Oracle(knn_backend=1, num_threads=8)
        orc.set_map(synth.to_xyzi(cfg["map"]))
        orc.set_scan(synth.to_xyzi(cfg["scan"]))
        per = []
        for which in ("pose_init", "pose_gt"):
            _, _, flag, coeff = orc.surfOptimization(cfg[which])
            per.append((cfg[which].copy(), flag.copy(), coeff.copy()))
        orc.close()
        out[name] = (cfg, per)
    return out


def _table(n, lanes):
    """A wave table of `lanes`-point entries over n sorted points."""
    first = np.arange(0, n, lanes)
    return np.stack([first, np.full_like(first, lanes)], 1).astype(np.int32)


# ---- the hook's boundary ---------------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    lib = s2m.load_library()
    rows = np.zeros((4, 28))
    rp = rows.ctypes.data_as(C.POINTER(C.c_double))
    pose, out = np.zeros(6, F32), s2m.LmRowsOut()
    pp = pose.ctypes.data_as(C.POINTER(C.c_float))
    chk = lib.s2m_debug_lm_rows_check_args
    assert chk(pp, 0, 30, 1, rp, 4, C.byref(out)) == 0              # launch 0 whatever early_exit says
    assert chk(pp, 0, 30, 0, None, 0, C.byref(out)) == 0            # no room for rows: the sizes alone
    assert chk(pp, 1, 30, 0, rp, 4, C.byref(out)) == 0
    assert chk(pp, 29, 30, 0, rp, 4, C.byref(out)) == 0
    assert chk(pp, 1, 30, 1, rp, 4, C.byref(out)) == -1             # a loop that may end early
    assert chk(pp, 30, 30, 0, rp, 4, C.byref(out)) == -1            # launch == max_iter
    assert chk(pp, 0, 0, 0, rp, 4, C.byref(out)) == -1
    assert chk(pp, -1, 30, 0, rp, 4, C.byref(out)) == -1
    assert chk(None, 0, 30, 0, rp, 4, C.byref(out)) == -1
    assert chk(pp, 0, 30, 0, None, 4, C.byref(out)) == -1
    assert chk(pp, 0, 30, 0, rp, -1, C.byref(out)) == -1
    assert chk(pp, 0, 30, 0, rp, 4, None) == -1
    assert lib.s2m_debug_lm_rows(None, pp, 0, rp, 4, C.byref(out), None) == -1


def test_out_struct_matches_the_header():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "liorf_s2m_debug.h")).read()
    body = txt[txt.index("typedef struct s2m_debug_lm_rows_out"):txt.index("} s2m_debug_lm_rows_out;")]
    order = [n for n, _ in s2m.LmRowsOut._fields_]
    assert order == ["n_rows_active", "wpb", "nblocks", "n_waves", "pose_used", "done"]
    pos = [body.index(n) for n in order]
    assert pos == sorted(pos)
    assert C.sizeof(s2m.LmRowsOut) == 4 * (4 + 6 + 1)


# ---- the statement ---------------------------------------------------------------------------------------------------
def test_every_case_keeps_a_fifth_of_its_scan(cases):
    """A case that loses its correspondences checks nothing: it fails here, it is not skipped."""
    for name, (cfg, per) in cases.items():
        for pose, flag, _ in per:
            kept = int(np.count_nonzero(flag))
            print(name, pose[:3], "kept", kept, "of", len(flag))
            assert kept >= 0.2 * len(flag), (name, kept)


def test_statement_is_the_oracles_row_bit_for_bit(cases):
    total = 0
    for name, (cfg, per) in cases.items():
        for pose, flag, coeff in per:
            k = np.flatnonzero(flag)
            rows, rhs = LR.jac_rows(pose, cfg["scan"][k], coeff[k])
            for j, i in enumerate(k):
                r, b = O.jacobian_row(pose, cfg["scan"][i], coeff[i])
                assert np.array_equal(r.view(np.uint32), rows[j].view(np.uint32)) and F32(b).view(np.uint32) == rhs[j].view(np.uint32), (name, i)
            total += len(k)
    assert total > 9 * 2 * 400


def test_statement_against_finite_differences(cases):
    """d(coeff . R(rpy) p) / d(roll, pitch, yaw) by central differences in fp64, plus the reference's one known deviation:
    the middle term of the coeff.y factor of ary reads srx*sry*srz*y where the derivative has srx*cry*srz*y (:1220).
    Bar: an entry is at most 18 products |factor| <= 2 times |p| |c|, each behind at most 6 fp32 roundings:
    18 * 6 * 2^-24 = 6.4e-6 of max|p| * max|c|; the differences themselves (h = 1e-6) add 1e-10 of it.  1e-5 holds both."""
    h = 1e-6
    for name, (cfg, per) in cases.items():
        for pose, flag, coeff in per:
            k = np.flatnonzero(flag)
            P, Cf = cfg["scan"][k], coeff[k]
            rows, rhs = LR.jac_rows(pose, P, Cf)
            P64, C64 = P.astype(np.float64), Cf[:, :3].astype(np.float64)
            rpy = pose[:3].astype(np.float64)

            def f(a):
                return np.einsum("ij,ij->i", C64, P64 @ LR.rotation_rpy(a).T)
            fd = np.zeros((len(k), 3))
            for a in range(3):
                up, dn = rpy.copy(), rpy.copy()
                up[a] += h
                dn[a] -= h
                fd[:, a] = (f(up) - f(dn)) / (2 * h)
            srx, sry, cry, srz = math.sin(rpy[2]), math.sin(rpy[1]), math.cos(rpy[1]), math.sin(rpy[0])
            fd[:, 1] += srx * srz * (sry - cry) * P64[:, 1] * C64[:, 1]
            scale = np.abs(P64).max(1) * np.abs(C64).max(1)
            err = np.abs(rows[:, :3].astype(np.float64) - fd).max(1)
            assert np.all(err <= 1e-5 * scale), (name, float((err / scale).max()))
            assert np.array_equal(rows[:, 3:], Cf[:, :3]) and np.array_equal(rhs, -Cf[:, 3])


# ---- discrimination --------------------------------------------------------------------------------------------------
def _sums(cfg, pose, flag, coeff, jac):
    n = len(flag)
    tab = _table(n, 8)
    mem = LR.row_members(tab, len(tab), LR.active_rows(len(tab), 8, 128), n)
    return LR.expected_rows(cfg["scan"], coeff, flag, mem, np.arange(n), pose=pose, jac=jac)


def test_every_single_term_mutation_moves_a_row_sum(cases):
    """Each product term's sign, and sry <-> cry in each term that holds one: at some listed attitude some row sum of the
    mutated Jacobian lies more than 100 bounds from the statement's."""
    base = {name: _sums(cfg, *per[0], LR.JAC) for name, (cfg, per) in cases.items()}
    n_sign = n_swap = 0
    for where in LR.products():
        for kind in ("sign", "swap"):
            jac = LR.mutate(where, kind)
            if jac is None:
                continue
            n_sign, n_swap = n_sign + (kind == "sign"), n_swap + (kind == "swap")
            worst = 0.0
            for name, (cfg, per) in cases.items():
                exact, bound, _ = base[name]
                got, _, _ = _sums(cfg, *per[0], jac)
                worst = max(worst, LR.worst_ratio(got, exact, bound))
                if worst > 100.0:
                    break
            assert worst > 100.0, (where, kind, worst)
    assert (n_sign, n_swap) == (29, 21)


def test_the_old_bar_lets_a_sign_flip_through(cases):
    """The reason this file exists (see the module docstring)."""
    where = next(w for w in LR.products() if w[0] == "arx" and LR.JAC[w[0]][w[1]][1][w[2]][1][w[3]][1] == ("srx", "sry", "srz")
                 and w[1] == 0)
    flipped = LR.mutate(where, "sign")

    def normal_eq(cfg, pose, flag, coeff, jac):
        k = np.flatnonzero(flag)
        rows, rhs = LR.jac_rows(pose, cfg["scan"][k], coeff[k], jac=jac)
        tot = np.array([math.fsum(c) for c in LR.row_products(rows, rhs).T])
        AtA = np.zeros((6, 6), F32)
        for n, (a, b) in enumerate(LR.UT):
            AtA[a, b] = AtA[b, a] = F32(tot[n])
        return AtA, tot[21:27].astype(F32)

    def old_bar(a, b):
        return all(np.allclose(x, y, rtol=1e-5, atol=1e-5 * np.abs(y).max()) for x, y in zip(a, b))

    cfg, per = cases["gt"]
    assert old_bar(normal_eq(cfg, *per[0], flipped), normal_eq(cfg, *per[0], LR.JAC))          # passes: invisible at the suite's attitude
    exact, bound, _ = _sums(cfg, *per[0], LR.JAC)
    got, _, _ = _sums(cfg, *per[0], flipped)
    assert LR.worst_ratio(got, exact, bound) > 1e6                                             # the row bound sees it there
    for name in ("a", "c"):
        cfg, per = cases[name]
        assert not old_bar(normal_eq(cfg, *per[0], flipped), normal_eq(cfg, *per[0], LR.JAC)), name


def test_bound_is_far_below_one_ulp_of_one_entry(cases):
    """One fp32 ulp in a single Jacobian entry of a single point moves its row's sums by far more than the bound (rows of up
    to 1 024 points: 16 waves of 64)."""
    cfg, per = cases["a"]
    pose, flag, coeff = per[0]
    n = len(flag)
    mem = [np.arange(n)[:1024]]
    exact, bound, counts = LR.expected_rows(cfg["scan"], coeff, flag, mem, np.arange(n), pose=pose)
    k = np.flatnonzero(flag[:1024])
    rows, rhs = LR.jac_rows(pose, cfg["scan"][k], coeff[k])
    j = int(np.argmax(np.abs(rows[:, 0])))
    bumped = rows.copy()
    bumped[j, 0] = np.nextafter(bumped[j, 0], F32(np.inf))
    moved = np.abs(LR.row_products(bumped, rhs).sum(0) - LR.row_products(rows, rhs).sum(0))
    assert counts[0] == len(k) >= 300
    assert moved[0] > 100.0 * bound[0, 0]


# ---- which points a row sums -----------------------------------------------------------------------------------------
def _flat(mem):
    return [m.tolist() for m in mem]


def test_row_members_one_entry_per_wave():
    # 20 entries, 8 waves per workgroup: 3 workgroups, nb_act * wpb = 24 >= n_waves
    tab = _table(20 * 64, 64)
    nb = LR.active_rows(20, 8, 64)
    assert nb == 3
    mem = LR.row_members(tab, 20, nb, 20 * 64)
    for b in range(3):
        want = [p for e in range(b, 20, 3) for p in range(64 * e, 64 * e + 64)]
        assert mem[b].tolist() == want
    assert sorted(np.concatenate(mem).tolist()) == list(range(20 * 64))


def test_row_members_several_entries_per_wave():
    # 11 entries on a grid of 2 workgroups of 2 waves: nb_act * wpb = 4 < n_waves, wave w of workgroup b walks
    # entries w * 2 + b, + 4, + 8
    tab = _table(11 * 64, 64)
    nb = LR.active_rows(11, 2, 2)
    assert nb == 2 and nb * 2 < 11
    mem = LR.row_members(tab, 11, nb, 11 * 64)
    by_wave = {b: sorted(e for w in range(2) for e in range(w * nb + b, 11, nb * 2)) for b in range(nb)}
    assert by_wave == {0: [0, 2, 4, 6, 8, 10], 1: [1, 3, 5, 7, 9]}
    for b in range(nb):
        assert mem[b].tolist() == [p for e in by_wave[b] for p in range(64 * e, 64 * e + 64)]


def test_row_members_short_entries_and_the_end_of_the_scan():
    # counts under 64, entries behind n_waves that are not read, and a last entry that reaches past n_q
    tab = np.array([[0, 8], [8, 16], [24, 1], [25, 37], [62, 8], [70, 64], [999, 64]], np.int32)
    mem = LR.row_members(tab, 5, 2, 66)
    assert _flat(mem) == [list(range(0, 8)) + [24] + list(range(62, 66)), list(range(8, 24)) + list(range(25, 62))]
    assert _flat(LR.row_members(tab, 5, 2)) == [list(range(0, 8)) + [24] + list(range(62, 70)), list(range(8, 24)) + list(range(25, 62))]
    assert _flat(LR.row_members(tab[:0], 0, 0)) == []
    # an empty entry contributes nothing
    assert _flat(LR.row_members(np.array([[0, 0], [0, 3]], np.int32), 2, 1, 10)) == [[0, 1, 2]]


def test_expected_rows_counts_and_bound():
    """Hand-made: two rows over five points, one of them not a correspondence."""
    P = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 1], [2, 2, 2]], F32)
    C4 = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0.25], [0, 0, 1, 1], [1, 0, 0, 2], [0, 1, 0, 4]], F32)
    flag = np.array([1, 1, 0, 1, 1], np.uint8)
    qperm = np.array([4, 3, 2, 1, 0])
    mem = [np.array([0, 1, 2]), np.array([3, 4])]          # sorted positions -> original points {4, 3, 2}, {1, 0}
    pose = np.zeros(6, F32)
    exact, bound, counts = LR.expected_rows(P, C4, flag, mem, qperm, pose=pose)
    assert counts.tolist() == [2, 2] and exact[:, 27].tolist() == [2.0, 2.0] and bound[:, 27].tolist() == [0.0, 0.0]
    # rows[3:] = coeff, rhs = -coeff.w: the sum of entry (3, 3) and number 24, row[3] * rhs
    k = LR.UT.index((3, 3))
    assert exact[0, k] == 1.0 and exact[1, k] == 1.0 and exact[0, 24] == -2.0 and exact[1, 24] == -0.5
    assert bound[0, k] == 2 * 2.0 ** -52 * 1.0
