"""CPU checks of the mutually consistent loops (s2m_pg_consistent_loops): the symbols and the host-only
argument table, the properties of the model tests/ref/pg_consistency_ref.py, the scene that motivates the call and one scene on
which the heuristic is not optimal."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pg_consistency_ref as R  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m  # noqa: E402

OK, BAD = s2m.S2M_OK, -1
NAMES = ("s2m_pg_consistency_default_params", "s2m_pg_consistency_check_args", "s2m_pg_consistent_loops")


def _header():
    return open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    lib, raw, main = s2m.load_library(), C.CDLL(s2m.LIB_PATH), _header()
    dbg = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    for n, nargs in zip(NAMES, (1, 6, 10)):
        assert n in s2m.ABI_SYMBOLS and hasattr(raw, n) and len(getattr(lib, n).argtypes) == nargs, n
        assert n + "(" in main and n + "(" not in dbg
    for f in ("pgConsistentLoops", "selectConsistentLoops"):
        assert callable(getattr(s2m.MapOptimizationS2M, f))
    hpp = open(os.path.join(ROOT, "liorf_amd", "host", "map_optimization_s2m.hpp")).read()
    assert "pgConsistentLoops(" in hpp and "selectConsistentLoops(" in hpp


def test_the_cap_and_the_structures_are_the_headers():
    h = _header()
    assert int(re.search(r"#define\s+S2M_PG_CONSISTENCY_MAX\s+(\d+)", h).group(1)) == s2m.S2M_PG_CONSISTENCY_MAX == R.MAX == 4096
    assert C.sizeof(s2m.PgConsistencyParams) == 48 and C.sizeof(s2m.PgConsistencyResult) == 24
    p = s2m.default_pg_consistency_params()
    assert (p.tol_m, p.tol_chord, p.rate_m, p.rate_chord) == (0.3, 0.03, 0.02, 0.0005) and list(p.reserved) == [0, 0, 0, 0]
    assert R.DEFAULTS == dict(tol_m=p.tol_m, tol_chord=p.tol_chord, rate_m=p.rate_m, rate_chord=p.rate_chord)
    assert s2m.load_library().s2m_pg_consistency_default_params(None) == BAD
    # the unmeasured defaults are named as such where a caller reads them
    assert "not been measured" in h[h.index("The mutually consistent loops"):h.index("#define S2M_PG_CONSISTENCY_MAX")]


def _good(m=5, n=9):
    kf = np.arange(m, dtype=np.int32) % n
    kt = (kf + 1 + np.arange(m, dtype=np.int32) % (n - 1)) % n
    rel = np.linspace(-1.0, 1.0, 6 * m).astype(np.float32).reshape(m, 6)
    return n, kf, kt, rel


def test_check_args_accepts_what_the_call_takes():
    n, kf, kt, rel = _good()
    assert s2m.pg_consistency_check_args(n, kf, kt, rel) == OK
    assert s2m.pg_consistency_check_args(n, kf, kt, rel, s2m.default_pg_consistency_params()) == OK
    assert s2m.pg_consistency_check_args(n, kf, kt, rel, s2m.default_pg_consistency_params(tol_m=0.0, tol_chord=0.0, rate_m=0.0, rate_chord=0.0)) == OK
    assert s2m.pg_consistency_check_args(n, None, None, None, m=0) == OK            # the empty call, null arrays
    assert s2m.pg_consistency_check_args(0, None, None, None, m=0) == OK
    m = s2m.S2M_PG_CONSISTENCY_MAX
    big = _good(m, 50)
    assert s2m.pg_consistency_check_args(*big) == OK


def test_check_args_rejects_every_listed_error_wherever_it_stands():
    n, kf, kt, rel = _good()
    m = len(kf)
    chk = s2m.pg_consistency_check_args
    assert chk(n, kf, kt, rel, m=-1) == BAD
    big = _good(s2m.S2M_PG_CONSISTENCY_MAX + 1, 50)
    assert chk(*big) == BAD
    assert chk(n, None, kt, rel, m=m) == BAD and chk(n, kf, None, rel, m=m) == BAD and chk(n, kf, kt, None, m=m) == BAD
    assert chk(-1, kf, kt, rel) == BAD
    for i in range(m):
        for bad in (-1, n, n + 7, -2 ** 31, 2 ** 31 - 1):
            for which in (0, 1):
                a, b = kf.copy(), kt.copy()
                (a if which == 0 else b)[i] = bad
                assert chk(n, a, b, rel) == BAD, (i, bad, which)
        b = kt.copy()
        b[i] = kf[i]                                                                  # key_from == key_to
        assert chk(n, kf, b, rel) == BAD, i
        for k in range(6):
            for bad in (np.nan, np.inf, -np.inf):
                r = rel.copy()
                r[i, k] = bad
                assert chk(n, kf, kt, r) == BAD, (i, k, bad)
    for field in ("tol_m", "tol_chord", "rate_m", "rate_chord"):
        for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
            assert chk(n, kf, kt, rel, s2m.default_pg_consistency_params(**{field: bad})) == BAD, (field, bad)
            assert chk(n, None, None, None, s2m.default_pg_consistency_params(**{field: bad}), m=0) == BAD, (field, bad)
    for k in range(4):
        p = s2m.default_pg_consistency_params()
        p.reserved[k] = 1
        assert chk(n, kf, kt, rel, p) == BAD, k


# ---- the model's properties ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene129():
    X, kf, kt, rel = R.random_scene(129)
    return X, kf, kt, rel, R.run(X, kf, kt, rel)


def test_matrix_is_symmetric_with_a_zero_diagonal(scene129):
    out = scene129[4]
    M = out["matrix"]
    assert M.any() and not M.all()
    assert np.array_equal(M, M.T) and not M.diagonal().any()
    assert np.array_equal(out["degree"], M.sum(1)) and out["n_consistent_pairs"] * 2 == M.sum()
    w = out["words"]
    assert w.shape == (129, 3) and not (w[:, 2] >> np.uint64(1)).any()              # no stray bits behind m
    for p, q in ((0, 1), (5, 64), (128, 127), (70, 128)):
        assert bool((w[p, q // 64] >> np.uint64(q % 64)) & np.uint64(1)) == bool(M[p, q])


def test_selected_set_is_a_clique(scene129):
    out = scene129[4]
    sel = out["selected"]
    assert sel.sum() == out["n_selected"] >= 2 and sel[out["start"]]
    assert R.is_clique(out["matrix"], sel)
    assert out["n_selected"] == out["sizes"].max() == out["sizes"][out["start"]]
    one = R.run(scene129[0], scene129[1][:1], scene129[2][:1], scene129[3][:1])     # m == 1: the candidate is selected
    assert one["selected"].tolist() == [True] and one["n_selected"] == 1 and one["start"] == 0 and one["n_consistent_pairs"] == 0
    none = R.select(np.zeros((0, 0), bool))
    assert none["n_selected"] == 0 and none["start"] == -1


def test_matrix_follows_a_permutation_of_the_candidates(scene129):
    """A pair is evaluated with its operands in candidate order, so a permutation exchanges the operands of some pairs.  The
    exchanged measure is D^-1 conjugated by O_t: the same chord, but a d2 that differs by the lever arm of O_t, so a pair near
    its threshold can change sides (which is why the operand order is part of the contract).  Precondition, asserted: in this
    scene - families of loops that agree to centimetres within and are tens of metres apart across - no verdict hangs on the
    order, and none lies within rounding of a threshold.  The random scene does not meet it, and that is asserted too."""
    X, kf, kt, rel, out = scene129
    assert not np.array_equal(R.matrix(X, kf, kt, R.rel_to_state(rel), swap=True), out["matrix"])
    X, kf, kt, rel = R.structured_scene(129, 300, 4)
    Z = R.rel_to_state(rel)
    M, margin = R.matrix(X, kf, kt, Z, with_margin=True)
    assert M.any() and np.array_equal(R.matrix(X, kf, kt, Z, swap=True), M) and margin > 1e-9, margin
    rng = np.random.default_rng(3)
    for _ in range(3):
        perm = rng.permutation(len(kf))
        Mp = R.matrix(X, kf[perm], kt[perm], Z[perm])
        assert np.array_equal(Mp, M[np.ix_(perm, perm)])


def test_selection_follows_a_permutation_when_no_degrees_tie():
    """Holds only without equal degrees among the members that matter - every pick of every growth has one best-ranked member
    by degree alone, and so has the winning start (select()'s tie_free) - which the input is built for and the test asserts."""
    M = R.tie_free_graph()
    base = R.select(M)
    assert base["tie_free"] and base["n_selected"] == 5 and np.flatnonzero(base["selected"]).tolist() == [0, 1, 2, 3, 4] and base["start"] == 4
    rng = np.random.default_rng(11)
    for _ in range(20):
        perm = rng.permutation(M.shape[0])                  # candidate i of the permuted input is candidate perm[i]
        got = R.select(M[np.ix_(perm, perm)])
        assert got["tie_free"]
        back = np.zeros(M.shape[0], bool)
        back[perm] = got["selected"]
        assert np.array_equal(back, base["selected"]) and perm[got["start"]] == base["start"] and got["n_selected"] == 5
        deg = np.zeros(M.shape[0], np.int32)
        deg[perm] = got["degree"]
        assert np.array_equal(deg, base["degree"])


def test_chain_length_is_integer_and_order_free():
    X = R.random_scene(1)[0]
    s = R.chain_length(X)
    assert s.dtype == np.int64 and s[0] == 0 and (np.diff(s) >= 0).all()
    d = np.linalg.norm(np.diff(X[:, 9:], axis=0), axis=1)
    assert np.abs(np.diff(s) - 1e6 * d).max() <= 0.5 + 1e-6
    step = np.diff(s, prepend=0)
    assert sum(int(v) for v in step[::-1]) == int(s[-1])                # any order of the integer steps gives the same sum
    far = X.copy()
    far[5, 9] = np.nan
    far[9, 10] = 1e300
    sf = R.chain_length(far)
    assert (np.diff(sf)[[4, 5, 8, 9]] == int(R.STEP_CAP)).all()         # a step that is not finite, or too long, counts as the cap


# ---- the scene that motivates the call -------------------------------------------------------------------------------

def _mean_gap(g, truth):
    return float(np.mean([np.linalg.norm(t - tt) for (_, t), (_, tt) in zip(g.X, truth)]))


def test_one_mirror_place_loop_bends_the_map_and_the_selection_leaves_it_out():
    """The figure-of-eight with drifted estimates: its true loops, one loop that takes the mirror place 40 m away for the same
    place, and three false loops that agree with each other.  The selected candidates are exactly the true loops, and the graph
    optimised with them ends nearer the ground truth than the graph optimised with all candidates (the ordering is asserted,
    not a size)."""
    sc = R.motivating_scene()
    g, truth, cand = sc["graph"], sc["truth"], sc["cand"]
    assert 35.0 < sc["mirror_gap"] < 45.0
    out = R.run(R.states_of(g.X), [c[0] for c in cand], [c[1] for c in cand], np.array([c[2] for c in cand]))
    print("degrees", out["degree"].tolist(), "selected", out["selected"].astype(int).tolist())
    assert np.array_equal(out["selected"], sc["true"])
    assert out["n_selected"] == int(sc["true"].sum()) and R.is_clique(out["matrix"], out["selected"])
    false3 = np.flatnonzero(~sc["true"])[1:]
    assert out["matrix"][np.ix_(false3, false3)].sum() == 6                # the three agree with each other
    assert not out["matrix"][np.ix_(~sc["true"], sc["true"])].any()        # and no false one with a true one
    gaps = {}
    for name, keep in (("all", np.ones(len(cand), bool)), ("selected", out["selected"])):
        h = P.figure_eight(g.n, 0)
        for (i, j, rel), k in zip(cand, keep):
            if k:
                h.add_between(i, j, rel, np.full(6, 0.3), 0.0)
        res = P.optimize(h, "chain_sqrt")
        gaps[name] = _mean_gap(h, truth)
        print(name, "iterations", res.iterations, "mean distance to the ground truth", gaps[name])
    print("dead reckoning", _mean_gap(g, truth))
    assert gaps["selected"] < gaps["all"]


def test_the_heuristic_is_not_the_maximum_clique():
    """The contract is the heuristic, not the optimum: on this graph the maximum clique {0, 1, 2, 3} is missed, because every
    growth from one of its members first takes that member's hub, whose degree is higher.  The model's answer is pinned."""
    M, clique = R.heuristic_miss()
    assert R.is_clique(M, np.isin(np.arange(M.shape[0]), clique))
    out = R.select(M)
    assert out["n_selected"] == 2 < len(clique)
    assert np.flatnonzero(out["selected"]).tolist() == [0, 4] and out["start"] == 4
    assert out["degree"][:8].tolist() == [4, 4, 4, 4, 6, 6, 6, 6] and out["sizes"].tolist() == [2] * M.shape[0]
