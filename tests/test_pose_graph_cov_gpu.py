"""GPU tests of the pose graph's covariances (s2m_pg_marginal, s2m_pg_marginals, s2m_pg_joint_marginal)
against references that never square J: tests/golden/pose_graph_cov_golden.npz holds mpmath blocks (60 digits) of two small
graphs and SVD blocks of the suite's graphs, tests/golden/pose_graph_cov_bounds.json the bounds, 10 x the floor that the CPU
routes of tests/ref/pose_graph_cov_ref.py leave to those references (tests/golden/make_golden_pose_graph_cov.py).  Every 3x3
block type (rr, rt, tr, tt) of every listed key and pair is held, values and symmetry, each block relative to its own norm in
the reference; the covariances of a rotation with key 0's translation, which are zero to rounding, relative to their scale."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_cov_ref as V  # noqa: E402
from liorf_amd import s2m  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD, BOUNDS = V.load_golden()
OK, PENDING = s2m.S2M_OK, s2m.S2M_PG_PENDING


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _optimised(gpu, name):
    g = V.build(name)
    CS.load_into(gpu, g)
    res = gpu.pgOptimize()
    assert res.converged == 1
    return g, res


def _held(label, cov, want, bound):
    """Values and symmetry of `cov` inside `bound`, block type by block type; the figures are printed first."""
    gaps, sym = V.block_gaps(cov, want), V.symmetry_gaps(cov, want)
    wg, ws = V.worst(gaps), V.worst(sym)
    print(label, " ".join("%s gap %.3g sym %.3g bound %.3g;" % (k, wg[k], ws[k], bound[k]) for k in sorted(wg)))
    assert np.all(np.isfinite(cov))
    assert not V.within(gaps, bound), label
    assert not V.within(sym, bound), label


# ---- 1. s2m_pg_marginal at every listed key, s2m_pg_marginals beside it --------------------------------------------

@pytest.mark.parametrize("name", V.GRAPHS)
def test_marginal_of_every_listed_key(gpu, name):
    g, res = _optimised(gpu, name)
    if name == "cauchy_outlier_300":                     # the covariance of the reweighted Jacobian: the weights matter here
        print(name, "robust weight", res.robust_weight_min)
        assert res.robust_weight_min < 0.05
    gold, c = GOLD[name], BOUNDS[name]
    assert c["n"] == g.n
    got = []
    for k in c["keys"]:
        got.append(gpu.pgMarginal(k))
        assert got[-1].shape == (6, 6)
        _held("%s key %d:" % (name, k), got[-1], V.sub(gold["cov"], gold["keys"], [k]), c["bound"])
    assert np.array_equal(gpu.pgMarginals(c["keys"]), np.stack(got))      # the block solve returns the same bits


# ---- 2. s2m_pg_joint_marginal on the listed pairs ------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in V.GRAPHS if BOUNDS[n]["pairs"]])
def test_joint_marginal_of_every_listed_pair(gpu, name):
    _optimised(gpu, name)
    gold, c = GOLD[name], BOUNDS[name]
    for a, b in c["pairs"]:
        cov = gpu.pgJointMarginal(a, b)
        assert cov.shape == (12, 12)
        _held("%s pair %d %d:" % (name, a, b), cov, V.sub(gold["cov"], gold["keys"], [a, b]), c["bound"])
        w = np.linalg.eigvalsh(0.5 * (cov + cov.T))
        print(name, a, b, "eigenvalues", w[0], w[-1])
        assert w[0] >= -c["bound"]["tt"] * w[-1]


# ---- 3. after the launched optimise ---------------------------------------------------------------------------------

def test_marginals_after_the_launched_optimise(gpu):
    name = "eight_40"
    _optimised(gpu, name)
    gold, c = GOLD[name], BOUNDS[name]
    want = gpu.pgMarginals(c["keys"])
    joint = gpu.pgJointMarginal(*c["pairs"][0])
    twin = s2m.MapOptimizationS2M()
    try:
        CS.load_into(twin, V.build(name))
        code, _early = twin.pgOptimizeLaunch()
        assert code == PENDING
        code, res = twin.pgOptimizeCollect()
        assert code == OK and res.converged == 1
        got = np.stack([twin.pgMarginal(k) for k in c["keys"]])
        assert np.array_equal(got, want)
        assert np.array_equal(twin.pgJointMarginal(*c["pairs"][0]), joint)
        for k, cov in zip(c["keys"], got):
            _held("%s launched, key %d:" % (name, k), cov, V.sub(gold["cov"], gold["keys"], [k]), c["bound"])
    finally:
        twin.close()
