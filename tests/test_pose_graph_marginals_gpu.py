"""GPU tests of s2m_pg_marginals and s2m_pg_joint_marginal (include/liorf_s2m.h; DESIGN.md section 16, "block solve"):
every block bit for bit s2m_pg_marginal's, the joint marginal's off-diagonal blocks against the SVD of J
(tests/ref/pose_graph_marginals_ref.joint_svd) inside tests/golden/pose_graph_marginals_bounds.json (10 x the floor that the QR
and the chain route leave to it; none of the three squares J)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
BOUNDS = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_marginals_bounds.json")))
PASS = s2m.PG_MARGINALS_KEYS_PER_PASS


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@pytest.fixture(scope="module")
def solved_ref():
    """The CPU reference's optimised graphs of the joint-marginal cases, computed once and left unchanged."""
    out = {}
    for name in sorted({c[0] for c in M.CASES}):
        out[name] = CS.build(name)
        P.optimize(out[name], "dense_sqrt")
    return out


def _single(gpu, keys):
    return np.stack([gpu.pgMarginal(int(k)) for k in keys])


# ---- 1. bitwise against the single path --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("loops_200", "gps_120", "cauchy_outlier_300"))
def test_marginals_equal_the_single_path_bit_for_bit(gpu, name):
    g = CS.build(name)
    CS.load_into(gpu, g)
    gpu.pgOptimize()
    n = g.n
    keys = [0, 31, 32, 33, n // 2, n - 1, n - 1, 0]
    got = gpu.pgMarginals(keys)
    want = _single(gpu, keys)
    assert got.shape == (len(keys), 6, 6) and np.all(np.isfinite(got))
    assert np.array_equal(got, want)
    assert not np.array_equal(got[0], got[1])            # different keys, different blocks: the columns were not mixed up


# ---- 2. scan levels and pass edges ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,loops", ((33, 1), (1025, 3)))
def test_scan_levels_and_pass_edges(gpu, n, loops):
    g = P.figure_eight(n, loops)
    CS.load_into(gpu, g)
    gpu.pgOptimize()
    pool = [n - 1, 0, 32, n // 2, 31, 33 % n, n - 2, 1, n // 3]
    for count in (1, PASS, PASS + 1):
        keys = [pool[k % len(pool)] for k in range(count)]
        got = gpu.pgMarginals(keys)
        assert np.array_equal(got, _single(gpu, keys)), count


# ---- 3. no off-chain factor ---------------------------------------------------------------------------------------

def test_without_an_off_chain_factor(gpu):
    g = CS.build("prior_only_50")
    CS.load_into(gpu, g)
    gpu.pgOptimize()
    keys = [0, 49]
    assert np.array_equal(gpu.pgMarginals(keys), _single(gpu, keys))
    assert gpu.pgMarginals([]).shape == (0, 6, 6)


# ---- 4. the joint marginal ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,a,b", M.CASES)
def test_joint_marginal(gpu, solved_ref, name, a, b):
    g = CS.build(name)
    CS.load_into(gpu, g)
    gpu.pgOptimize()
    poses = gpu.pgPoses().copy()
    cov = gpu.pgJointMarginal(a, b)
    assert cov.shape == (12, 12) and np.all(np.isfinite(cov))
    assert np.array_equal(cov[:6, :6], gpu.pgMarginal(a)) and np.array_equal(cov[6:, 6:], gpu.pgMarginal(b))
    case = BOUNDS[M.case_id(name, a, b)]
    bound = dict(case["bound"], **case["held_bound"])
    want = M.joint_svd(solved_ref[name], a, b)
    gaps, sym = M.cross_gaps(cov, want), M.symmetry_gaps(cov, want)
    assert set(gaps) == set(sym) == set(bound)
    for k in sorted(bound):
        print(name, a, b, k, "gap", gaps[k], "symmetry", sym[k], "bound", bound[k])
    for k in bound:
        assert gaps[k] <= bound[k], k
        assert sym[k] <= bound[k], k
    for ka, kb in ((a, a), (-1, b), (a, g.n), (g.n, -1)):
        with pytest.raises(s2m.S2MError) as e:
            gpu.pgJointMarginal(ka, kb)
        assert "S2M_ERR_INVALID_ARG" in str(e.value)
    with pytest.raises(s2m.S2MError):
        gpu.pgMarginals([0, g.n])
    assert np.array_equal(poses, gpu.pgPoses())          # the graph is as it was


# ---- 5. reproducible -----------------------------------------------------------------------------------------------

def test_reproducible_on_the_same_and_on_a_fresh_handle(gpu):
    g = CS.build("gps_120")
    keys = [0, 60, 119, 33, 7]
    CS.load_into(gpu, g)
    gpu.pgOptimize()
    first, joint = gpu.pgMarginals(keys), gpu.pgJointMarginal(60, 119)
    assert np.array_equal(first, gpu.pgMarginals(keys)) and np.array_equal(joint, gpu.pgJointMarginal(60, 119))
    m = s2m.MapOptimizationS2M()
    try:
        CS.load_into(m, CS.build("gps_120"))
        m.pgOptimize()
        assert np.array_equal(first, m.pgMarginals(keys)) and np.array_equal(joint, m.pgJointMarginal(60, 119))
    finally:
        m.close()


# ---- 6. the C++ host mirror through s2m_harness ----------------------------------------------------------------------

def test_harness_prints_equal_old_and_new_last_key_blocks(tmp_path):
    rng = np.random.default_rng(P.SEED + 3)
    n = 40
    truth = P.figure_eight(n, 0, truth_only=True)
    poses = np.array([P.xyzrpy_from_pose(R, t) for R, t in truth])
    poses[:, :3] += np.cumsum(rng.normal(0, 0.01, (n, 3)), 0)
    poses = poses.astype(F)
    clouds = [synth.to_xyzi(rng.uniform(-20, 20, (200, 3)).astype(F)) for _ in range(n)]
    loop = (35, 34, 14, s2m.between_xyzrpy(poses[34], poses[14]) + np.array([0.04, -0.02, 0.0, 0, 0, 0.002], F), 0.3, 0.0)
    np.concatenate(clouds).astype(F).tofile(tmp_path / "keys.bin")
    with open(tmp_path / "keys.txt", "w") as f:
        for k in range(n):
            f.write("%d %.17g %s\n" % (len(clouds[k]), float(k), " ".join("%.9g" % v for v in poses[k])))
    with open(tmp_path / "loops.txt", "w") as f:
        at, kc, kp, rel, var, rk = loop
        f.write("%d %d %d %s %.17g %.17g\n" % (at, kc, kp, " ".join("%.9g" % v for v in rel.astype(F)), var, rk))
    harness = os.path.join(ROOT, "liorf_amd", "host", "s2m_harness")
    run = subprocess.run([harness, "--pose-graph", str(tmp_path / "keys.bin"), str(tmp_path / "keys.txt"), "0.3", str(tmp_path / "loops.txt"),
                          str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, check=True)
    lines = {s.split(" ", 1)[0]: s.split(" ", 1)[1].split() for s in run.stderr.split("\n") if s.startswith("marginal_")}
    assert set(lines) == {"marginal_old", "marginal_new"}
    assert len(lines["marginal_old"]) == 36 and lines["marginal_old"] == lines["marginal_new"]
    cov = np.array([float(v) for v in lines["marginal_new"]]).reshape(6, 6)
    assert np.all(np.isfinite(cov)) and np.all(np.diag(cov) > 0.0)
    assert sum(s.startswith("key ") and s.endswith(" 1") for s in run.stdout.split("\n")) == 1      # the loop was closed
