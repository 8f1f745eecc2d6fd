"""CPU tests of the covariance references and fixtures behind tests/test_pose_graph_cov_gpu.py
(tests/ref/pose_graph_cov_ref.py, tests/golden/pose_graph_cov_golden.npz, tests/golden/pose_graph_cov_bounds.json): the committed
mpmath blocks solve the normal equations, the fp64 routes that do not square J lie where the bounds file says, the fp64 inverse
of J^T J does not, and each bound rejects a wrong block.  Nothing here factorises in mpmath; every graph is linearised at the
committed estimates, so no optimise runs either."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cov_ref as V  # noqa: E402

GOLD, BOUNDS = V.load_golden()
MARGIN, CAP = 10.0, 1e-2
_graphs, _chain = {}, {}


def _graph(name):
    """The graph at the committed estimates, built once and only read afterwards."""
    if name not in _graphs:
        g = V.build(name)
        g.X = V.state_list(GOLD[name]["X"])
        _graphs[name] = g
    return _graphs[name]


def _neighbours(name):
    """cov_chain (2e-15 from mpmath in rr and tt) over every listed key and its neighbours, once per graph."""
    if name not in _chain:
        n = BOUNDS[name]["n"]
        ks = sorted({q for k in BOUNDS[name]["keys"] for q in (k - 1, k, k + 1) if 0 <= q < n})
        _chain[name] = (ks, V.cov_chain(_graph(name), ks))
    return _chain[name]


def test_bounds_are_ten_floors_informative_and_hold_every_listed_block():
    assert set(BOUNDS) == set(V.GRAPHS) == set(GOLD)
    for name, c in BOUNDS.items():
        n = c["n"]
        assert c["keys"] == V.keys_of(name, n) and [tuple(p) for p in c["pairs"]] == V.pairs_of(name, n)
        assert GOLD[name]["keys"] == V.all_keys_of(name, n) and GOLD[name]["cov"].shape == (6 * len(GOLD[name]["keys"]),) * 2
        assert set(c["floor"]) == set(c["bound"]) and set(V.TYPES) <= set(c["bound"])
        for k, v in c["bound"].items():
            assert v == pytest.approx(MARGIN * c["floor"][k], rel=1e-12, abs=0.0)        # a hand-edited bound is caught
            assert k.endswith("_held") or v < CAP, (name, k, v)
        for a, b, ty in c["held"]:                       # scale-held: only a rotation against key 0's translation
            assert (ty == "rt" and b == 0) or (ty == "tr" and a == 0), (name, a, b, ty)


@pytest.mark.parametrize("name", V.SMALL)
def test_committed_columns_solve_the_normal_equations_in_mpmath(name):
    """(J^T J) x = e for the two committed whole columns, hi + lo.  Both parts together carry 106 bits: entries of up to 1e8
    under rows of J^T J of up to 24 entries of 1e6 leave 24 * 1e6 * 1e8 * 2^-106 = 3e-17; held to 1e-15."""
    import mpmath as mp
    mp.mp.dps = 60
    gold = GOLD[name]
    H = V.normal_matrix_mp(_graph(name), dps=60)
    m = H.rows
    nz = [[(j, H[i, j]) for j in range(m) if H[i, j] != 0] for i in range(m)]
    idx = V.rows_of(gold["keys"])
    for at, hi, lo in zip(gold["col_at"], gold["col_hi"], gold["col_lo"]):
        x = [mp.mpf(float(h)) + mp.mpf(float(l)) for h, l in zip(hi, lo)]
        res = max(abs(sum(v * x[j] for j, v in row) - (1 if i == int(at) else 0)) for i, row in enumerate(nz))
        print(name, "column", int(at), "residual", float(res))
        assert res < mp.mpf("1e-15")
        c = int(np.nonzero(idx == int(at))[0][0])
        assert np.array_equal(gold["cov"][:, c], hi[idx])                # the committed block is this column, rounded once
    assert not V.within(V.symmetry_gaps(gold["cov"], gold["cov"]), {k: 2.0 ** -50 for k in BOUNDS[name]["bound"]})


@pytest.mark.parametrize("name", V.GRAPHS)
def test_routes_that_do_not_square_J_agree_inside_the_bounds(name):
    """cov_qr and cov_chain (and cov_svd on the small graphs) against the committed reference.  The recorded floor is the
    largest of their gaps as the golden script measured them; with the same BLAS and thread count a recomputation repeats them
    exactly.  A route's gap is the norm of its accumulated rounding, and LAPACK with another thread count sums in another order
    and draws that rounding again: eight_65's SVD gave rr 9.2e-12 where the floors were written and 2.07e-11 with 16 threads
    on another host, 2.25 x the floor.  The project's margin for differing summation orders is 10, so each route is held to the
    bound, 10 x the floor, and the figures are printed beside the floor.  cov_chain on the small graphs, 2e-15 from mpmath
    where the floor is the SVD's 1e-8, must lie inside the floor itself."""
    g, gold, c = _graph(name), GOLD[name], BOUNDS[name]
    allk = gold["keys"]
    routes = {"qr": V.cov_qr, "chain": V.cov_chain}
    if name in V.SMALL:
        routes["svd"] = V.cov_svd
    for r, f in routes.items():
        gaps, _held = V.tested_gaps(f(g, allk), gold["cov"], allk, c["keys"], c["pairs"])
        print(name, r, {k: "%.3g (floor %.3g)" % (v, c["floor"][k]) for k, v in sorted(gaps.items())})
        for k, v in gaps.items():
            assert v <= c["bound"][k], (r, k)
            if r == "chain" and name in V.SMALL:
                assert v <= c["floor"][k], k


def test_the_chain_route_is_left_out_of_a_floor_only_where_it_is_the_outlier():
    """pose_graph_cov_ref.floors on made-up gaps, and on gps_120, the one case where it applies: at the key the GPS factor
    pins, the SVD, the QR and the inverse of J^T J agree in tt to 1e-7 and far better while the chain route's Woodbury step is
    1e-7 off all of them, and the bounds file records that gap as left out, not as the floor."""
    import json
    import pose_graph_cases as CS
    import pose_graph_ref as P
    fl, out = V.floors({"qr": {"tt": 1e-11, "rt": 2e-4}, "chain": {"tt": 2e-7, "rt": 3e-4}, "svd": {"tt": 5e-12, "rt": 1e-4}})
    assert fl == {"tt": 1e-11, "rt": 3e-4} and out == {"tt": 2e-7}
    fl, out = V.floors({"qr": {"tt": 1e-11}, "chain": {"tt": 9.9e-11}})
    assert fl == {"tt": 9.9e-11} and out == {}
    g = CS.build("gps_120")
    P.optimize(g, "dense_sqrt")
    keys = CS.marginal_keys(g.n)
    want = V.cov_svd(g, keys)
    tt = {r: V.tested_gaps(f(g, keys), want, keys, keys, ())[0]["tt"] for r, f in (("qr", V.cov_qr), ("dense", V.cov_dense), ("chain", V.cov_chain))}
    print("gps_120 tt gaps to the SVD", tt)
    assert tt["qr"] < 1e-9 and tt["dense"] < 1e-6 and tt["chain"] > V.MARGIN * tt["qr"]
    b = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_bounds.json")))["gps_120"]
    assert set(b["chain_route_left_out"]) == {"marginal_tt"} and b["floor"]["marginal_tt"] < 1e-9
    for name in V.GRAPHS:
        assert BOUNDS[name]["chain_route_left_out"] == {}


@pytest.mark.parametrize("name", ("eight_40", "eight_65", "loops_200", "cauchy_outlier_300"))
def test_the_inverse_of_JtJ_lies_outside_the_new_bounds(name):
    """Why the reference changed: the fp64 inverse of J^T J misses the tt, rt and tr bounds it used to define."""
    g, gold, c = _graph(name), GOLD[name], BOUNDS[name]
    gaps, _held = V.tested_gaps(V.cov_dense(g, gold["keys"]), gold["cov"], gold["keys"], c["keys"], c["pairs"])
    print(name, {k: "%.3g (bound %.3g)" % (v, c["bound"][k]) for k, v in sorted(gaps.items())})
    for ty in ("tt", "rt", "tr"):
        assert gaps[ty] > c["bound"][ty], ty


@pytest.mark.parametrize("name", V.GRAPHS)
def test_each_bound_rejects_a_wrong_block(name):
    """The reference's own 6x6 of every listed key, spoiled in one way at a time, must leave the bounds: the rt block with its
    sign flipped; the rt block replaced by the transposed tr block of another listed key; the tt block times 1 + 1e-4; the
    whole 6x6 of key k - 1 and of key k + 1.  Key 0's rt block is zero to rounding (scale-held), so its flipped sign is the same
    block and is not asked for; another key's block in its place is."""
    gold, c = GOLD[name], BOUNDS[name]
    nk, near = _neighbours(name)
    keys = c["keys"]
    r, t = slice(0, 3), slice(3, 6)
    for q, k in enumerate(keys):
        want = V.sub(gold["cov"], gold["keys"], [k])
        held = V.block_gaps(want, want)[(0, 0, "rt")][1]
        assert not V.within(V.block_gaps(want, want), c["bound"])
        spoiled = {}
        if not held:
            spoiled["rt flipped"] = want.copy()
            spoiled["rt flipped"][r, t] *= -1.0
        other = V.sub(gold["cov"], gold["keys"], [keys[(q + 1) % len(keys)]])
        spoiled["rt from another key"] = want.copy()
        spoiled["rt from another key"][r, t] = other[t, r].T
        spoiled["tt scaled"] = want.copy()
        spoiled["tt scaled"][t, t] *= 1.0 + 1e-4
        for d in (-1, 1):
            if 0 <= k + d < c["n"]:
                spoiled["key %+d" % d] = V.sub(near, nk, [k + d])
        for what, cov in spoiled.items():
            bad = V.within(V.block_gaps(cov, want), c["bound"])
            assert bad, (name, k, what)
            if what.startswith("rt"):
                assert [b[0][2] for b in bad] == ["rt"], (name, k, what)
            if what == "tt scaled":
                assert [b[0][2] for b in bad] == ["tt"], (name, k, what)
        # the neighbour's block is told apart by the same route that is 2e-15 from mpmath: the route itself passes
        assert not V.within(V.block_gaps(V.sub(near, nk, [k]), want), c["bound"]), (name, k)


def test_a_joint_marginal_with_swapped_or_flipped_cross_blocks_is_rejected():
    for name in V.GRAPHS:
        gold, c = GOLD[name], BOUNDS[name]
        for a, b in c["pairs"]:
            want = V.sub(gold["cov"], gold["keys"], [a, b])
            assert not V.within(V.block_gaps(want, want), c["bound"]) and not V.within(V.symmetry_gaps(want, want), c["bound"])
            flipped = want.copy()
            flipped[:6, 6:] *= -1.0
            assert V.within(V.block_gaps(flipped, want), c["bound"]) and V.within(V.symmetry_gaps(flipped, want), c["bound"])
            swapped = want.copy()
            swapped[:6, 6:], swapped[6:, :6] = want[6:, :6].copy(), want[:6, 6:].copy()      # the two blocks without the transpose
            assert V.within(V.block_gaps(swapped, want), c["bound"]), (name, a, b)
