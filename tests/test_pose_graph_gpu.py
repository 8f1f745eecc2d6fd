"""GPU tests of the pose graph (include/liorf_s2m.h, "Pose graph"; reference src/mapOptmization.cpp:1386-1642) against
the CPU reference tests/ref/pose_graph_ref.py.  Bounds: tests/golden/pose_graph_bounds.json, written by
tests/golden/make_golden_pose_graph.py (10 x the disagreement of two CPU solves; for the marginals, of the QR and the chain
route of tests/ref/pose_graph_cov_ref.py with the SVD of J - none of them squares J)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_cov_ref as V  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
BOUNDS = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_bounds.json")))


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _res_tuple(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _solve_on_device(gpu, g, params=None):
    CS.load_into(gpu, g)
    res = gpu.pgOptimize(params)
    return res, gpu.pgPoses().astype(np.float64)


def _check_error(name, got, want):
    b = BOUNDS[name]["bound"]
    gap = abs(got - want)
    print(name, "error", got, "reference", want, "gap", gap, "bounds", b["error_rel"] * want, b["error_abs"])
    assert gap <= max(b["error_rel"] * want, b["error_abs"])


# ---- (a) small graphs against the dense square-root reference, (d) marginals, (f) two runs bitwise equal ---------

@pytest.mark.parametrize("name", CS.SMALL)
def test_small_graph_matches_the_dense_square_root_reference(gpu, name):
    g = CS.build(name)
    res, poses = _solve_on_device(gpu, g)
    mkeys = CS.marginal_keys(g.n)
    covs = [gpu.pgMarginal(k) for k in mkeys]
    ref = P.optimize(g, "dense_sqrt")
    want = CS.to_f32(g.poses())
    b = BOUNDS[name]["bound"]
    rot, trans = P.pose_gap(poses, want)
    print(name, "iterations", res.iterations, ref.iterations, "inner", res.inner_iterations, "abs gap", rot, trans, "bounds", b["abs_rot"], b["abs_trans"])
    assert res.converged == 1 and ref.converged == 1
    assert res.n_variables == g.n and res.n_factors == len(g.priors) + len(g.betweens) + len(g.gps)
    _check_error(name, res.error_after, ref.error_after)
    # the same inputs in the same formulas: residuals no smaller than the float rounding of the inputs (1e-7) from fp64
    # coordinates of up to 1e2 carry 2e-7 of relative rounding, their squares twice that
    assert abs(res.error_before - ref.error_before) <= 1e-5 * ref.error_before
    assert rot <= b["abs_rot"] and trans <= b["abs_trans"]
    if name == "cauchy_outlier_300":
        print(name, "robust weight", res.robust_weight_min, ref.robust_weight_min)
        assert res.robust_weight_min < 0.05 and abs(res.robust_weight_min - ref.robust_weight_min) <= 1e-6 * ref.robust_weight_min
    else:
        assert res.robust_weight_min == 1.0
    # (d) the marginals of the last key, the middle key and key 32 against the SVD of J, values and symmetry per 3x3 block type
    mb = {k[len("marginal_"):]: v for k, v in b.items() if k.startswith("marginal_")}
    want_cov = V.cov_svd(g, mkeys)
    for k, cov in zip(mkeys, covs):
        want = V.sub(want_cov, mkeys, [k])
        gaps, sym = V.block_gaps(cov, want), V.symmetry_gaps(cov, want)
        print(name, "marginal of key", k, "gaps", V.worst(gaps), "symmetry", V.worst(sym), "bounds", mb)
        assert not V.within(gaps, mb), k
        assert not V.within(sym, mb), k
    # a second run of the same case is bitwise the first
    res2, poses2 = _solve_on_device(gpu, CS.build(name))
    assert _res_tuple(res) == _res_tuple(res2) and np.array_equal(poses, poses2)
    assert np.array_equal(covs[0], gpu.pgMarginal(g.n - 1))


# ---- (b) 2 000 and 10 000 keys ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CS.LARGE)
def test_large_graph_error_relative_poses_and_key0(gpu, name):
    g = CS.build(name)
    prior = g.poses()[:1].copy()
    res, poses = _solve_on_device(gpu, g)
    ref = P.optimize(g, "chain_sqrt")
    want = CS.to_f32(g.poses())
    b = BOUNDS[name]["bound"]
    rot, trans = P.pose_gap(poses, want, relative=True)
    k0r, k0t = P.pose_gap(poses[:1], prior)
    print(name, "iterations", res.iterations, ref.iterations, "inner", res.inner_iterations, "rel gap", rot, trans, "bounds", b["rel_rot"], b["rel_trans"],
          "key0", k0r, k0t, "bounds", b["key0_rot"], b["key0_trans"])
    assert res.converged == 1 and ref.converged == 1
    _check_error(name, res.error_after, ref.error_after)
    assert rot <= b["rel_rot"] and trans <= b["rel_trans"]
    assert k0r <= b["key0_rot"] and k0t <= b["key0_trans"]
    res2, poses2 = _solve_on_device(gpu, CS.build(name))
    assert _res_tuple(res) == _res_tuple(res2) and np.array_equal(poses, poses2)


# ---- (c) the store ---------------------------------------------------------------------------------------------

def _cloud(rng, n):
    c = synth.to_xyzi(rng.uniform(-20, 20, (n, 3)).astype(F))
    c[:, 4] = rng.uniform(0, 100, n).astype(F)
    return c


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_apply_to_store_equals_set_poses_bit_for_bit():
    rng = np.random.default_rng(P.SEED)
    g = CS.build("loops_200")
    init = g.poses().astype(F)
    clouds = [_cloud(rng, int(rng.integers(200, 500))) for _ in range(16)]
    outs = []
    for direct in (True, False):
        m = s2m.MapOptimizationS2M()
        try:
            for k in range(g.n):
                m.saveKeyFrame(init[k], float(k), clouds[k % len(clouds)])
            CS.load_into(m, g)
            m.pgOptimize()
            poses = m.pgPoses()
            if direct:
                m.pgApplyToStore(0, g.n)
            else:
                m.correctPoses(poses, 0)
            keys, local = m.extractSurroundingKeyFrames(float(g.n), s2m.default_kf_params(map_leaf=0.4), return_map=True)
            cloud, gkeys = m.publishGlobalMap(s2m.default_gmap_params(pose_density=2.0, leaf=0.5), return_keys=True)
            raw = m.globalMapCloud(0, g.n, 0.0)
            outs.append((poses, keys, local, cloud, gkeys, raw))
        finally:
            m.close()
    assert not np.array_equal(outs[0][0], init)          # the optimise moved the poses
    for a, b in zip(outs[0], outs[1]):
        _same(np.asarray(a), np.asarray(b))


def test_optimise_and_apply_between_two_registrations(cfg_small):
    rng = np.random.default_rng(7)
    scan = synth.to_xyzi(cfg_small["scan"])
    parts = np.array_split(synth.to_xyzi(cfg_small["map"]), 6)
    results = []
    for direct in (True, False):
        m = s2m.MapOptimizationS2M()
        try:
            poses = np.zeros((6, 6), F)
            for i in range(6):
                m.saveKeyFrame(poses[i], float(i), parts[i])
                m.addOdomFactor(poses[i])
            m.extractSurroundingKeyFrames(6.0, s2m.default_kf_params(map_leaf=0.4))
            m.setScan(scan)
            m.transformTobeMapped = cfg_small["pose_init"].copy()
            r1 = m.scan2MapOptimization()
            # a loop that pulls key 5 by a few centimetres
            m.addLoopFactor(5, 0, np.array([0.04, -0.03, 0.01, 0.0, 0.0, 0.002], F), np.zeros(6, F), np.full(6, 1e-4))
            m.pgOptimize()
            if direct:
                assert m.correctPosesFromGraph()
            else:
                m.correctPoses(m.pgPoses(), 0)
            m.extractSurroundingKeyFrames(6.0, s2m.default_kf_params(map_leaf=0.4))
            m.transformTobeMapped = cfg_small["pose_init"].copy()
            r2 = m.scan2MapOptimization()
            results.append((_res_tuple(r1), _res_tuple(r2), m.pgPoses().tobytes()))
        finally:
            m.close()
    assert results[0] == results[1]
    assert np.abs(np.frombuffer(results[0][2], F)).max() > 1e-3        # the loop moved something


# ---- (e) incremental use ----------------------------------------------------------------------------------------

def test_incremental_odometry_then_a_loop_follows_the_reference(gpu):
    rng = np.random.default_rng(P.SEED + 1)
    odo, loop = CS.incremental_inputs()
    ref, ref_latest, rr = CS.incremental_replay(odo, loop, "dense_sqrt")
    ref_latest = CS.to_f32(ref_latest)
    b = BOUNDS[CS.INCREMENTAL]["bound"]
    n = len(odo)
    gpu.pgReset()
    gpu.kfReset()
    cloud = _cloud(rng, 300)
    for k in range(n):
        res, latest = gpu.saveKeyFramesAndFactor(odo[k], float(k), cloud)
        assert res.n_variables == k + 1 and res.converged == 1
        # prior and odometry fit exactly: the latest pose is the front end's, up to the rounding of the float it is returned in
        assert np.all(np.abs(latest.astype(np.float64) - ref_latest[k]) <= np.spacing(np.abs(ref_latest[k]).astype(F)).astype(np.float64)), k
    assert gpu.kfSize() == n and not gpu.correctPosesFromGraph()           # no loop closed: the store stays
    gpu.addLoopFactor(loop[0], loop[1], None, None, loop[3], rel=loop[2])
    gpu.pgOptimize()
    res = gpu.pgOptimize()
    assert gpu.correctPosesFromGraph()
    got, want = gpu.pgPoses().astype(np.float64), CS.to_f32(ref.poses())
    rot, trans = P.pose_gap(got, want, relative=True)
    print("incremental: rel gap", rot, trans, "bounds", b["rel_rot"], b["rel_trans"], "error", res.error_after, rr.error_after)
    assert rot <= b["rel_rot"] and trans <= b["rel_trans"]
    assert abs(res.error_after - rr.error_after) <= max(b["error_rel"] * rr.error_after, b["error_abs"])
    # the store holds the estimates
    raw_a = gpu.globalMapCloud(0, n, 0.0)
    gpu.correctPoses(gpu.pgPoses(), 0)
    _same(raw_a, gpu.globalMapCloud(0, n, 0.0))


# ---- (f) edge cases ---------------------------------------------------------------------------------------------

def test_edge_cases(gpu):
    z6, v6 = np.zeros(6, F), np.ones(6)
    gpu.pgReset()
    res = gpu.pgOptimize()                               # empty graph
    assert (res.iterations, res.inner_iterations, res.n_variables, res.n_factors, res.error_before, res.error_after) == (0, 0, 0, 0, 0.0, 0.0)
    assert gpu.pgSize() == (0, 0) and gpu.pgPoses().shape == (0, 6)
    # one key
    p0 = np.array([1, 2, 3, 0.1, -0.2, 0.3], F)
    gpu.addOdomFactor(p0)
    res = gpu.pgOptimize()
    assert gpu.pgSize() == (1, 1) and res.n_variables == 1 and res.error_after <= 1e-20
    assert np.abs(gpu.pgPoses()[0] - p0).max() <= 4 * CS.Q32 * 3
    cov = gpu.pgMarginal(0)
    assert np.allclose(np.diag(cov), s2m.default_pg_params().prior_var[:], rtol=1e-9)
    # a missing initial value
    gpu.pgAddBetween(0, 1, z6, v6)
    assert gpu.pgSize() == (2, 2)
    with pytest.raises(s2m.S2MError):
        gpu.pgOptimize()
    with pytest.raises(s2m.S2MError):
        gpu.pgPoses()
    assert gpu.pgPoses(0, 1).shape == (1, 6)             # key 0 has its value: only the range asked for is checked
    gpu.pgSetInitial(1, p0)
    assert gpu.pgOptimize().converged == 1
    # a disconnected variable: key 2 has a value and a GPS factor but no odometry
    gpu.pgSetInitial(2, p0)
    gpu.pgAddGps(2, [1, 2, 3], [1, 1, 1])
    with pytest.raises(s2m.S2MError):
        gpu.pgOptimize()
    with pytest.raises(s2m.S2MError):
        gpu.pgMarginal(2)
    # failed adds leave the graph as it was
    size = gpu.pgSize()
    before = gpu.pgPoses(0, 2).copy()
    bad = p0.copy(); bad[2] = np.nan
    for call in (lambda: gpu.pgAddPrior(5, p0, v6), lambda: gpu.pgAddBetween(1, 1, z6, v6), lambda: gpu.pgAddBetween(1, 9, z6, v6),
                 lambda: gpu.pgAddBetween(0, 1, bad, v6), lambda: gpu.pgAddBetween(0, 1, z6, np.zeros(6)), lambda: gpu.pgAddGps(1, [0, np.inf, 0], [1, 1, 1]),
                 lambda: gpu.pgSetInitial(7, p0), lambda: gpu.pgSetInitial(1, bad), lambda: gpu.addOdomFactor(bad),
                 lambda: gpu.pgAddBetween(0, 1, z6, v6, -1.0)):
        with pytest.raises(s2m.S2MError):
            call()
        assert gpu.pgSize() == size
    assert np.array_equal(before, gpu.pgPoses(0, 2))
    # a prior missing on key 0
    gpu.pgReset()
    gpu.pgSetInitial(0, p0)
    with pytest.raises(s2m.S2MError):
        gpu.pgOptimize()
    # ranges
    gpu.pgReset()
    gpu.kfReset()
    gpu.addOdomFactor(p0)
    with pytest.raises(s2m.S2MError):
        gpu.pgApplyToStore(0, 1)                         # the store is empty
    with pytest.raises(s2m.S2MError):
        gpu.pgPoses(0, 2)
    gpu.pgReset()


# ---- (g) the C++ host mirror through s2m_harness -----------------------------------------------------------------

def test_harness_pose_graph_mode_matches_the_python_mirror(tmp_path):
    import subprocess
    rng = np.random.default_rng(P.SEED + 2)
    n = 60
    truth = P.figure_eight(n, 0, truth_only=True)
    poses = np.array([P.xyzrpy_from_pose(R, t) for R, t in truth])
    poses[:, :3] += np.cumsum(rng.normal(0, 0.01, (n, 3)), 0)          # a drifting front end
    poses = poses.astype(F)
    clouds = [_cloud(rng, int(rng.integers(300, 700))) for _ in range(n)]
    times = np.arange(n, dtype=np.float64)
    # two closures: a plain one queued before key 40, a Cauchy one before key 55
    loops = [(40, 39, 9, s2m.between_xyzrpy(poses[39], poses[9]) + np.array([0.05, -0.02, 0.0, 0, 0, 0.003], F), 0.3, 0.0),
             (55, 54, 24, s2m.between_xyzrpy(poses[54], poses[24]) + np.array([-0.03, 0.04, 0.01, 0, 0, -0.002], F), 0.5, 1.0)]
    np.concatenate(clouds).astype(F).tofile(tmp_path / "keys.bin")
    with open(tmp_path / "keys.txt", "w") as f:
        for k in range(n):
            f.write("%d %.17g %s\n" % (len(clouds[k]), times[k], " ".join("%.9g" % v for v in poses[k])))
    with open(tmp_path / "loops.txt", "w") as f:
        for at, kc, kp, rel, var, rk in loops:
            f.write("%d %d %d %s %.17g %.17g\n" % (at, kc, kp, " ".join("%.9g" % v for v in rel.astype(F)), var, rk))
    harness = os.path.join(ROOT, "liorf_amd", "host", "s2m_harness")
    txt = subprocess.run([harness, "--pose-graph", str(tmp_path / "keys.bin"), str(tmp_path / "keys.txt"), "0.3", str(tmp_path / "loops.txt"),
                          str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
    want = []
    m = s2m.MapOptimizationS2M()
    try:
        m.pgReset()
        for k in range(n):
            m.downsampleCurrentScan(clouds[k], 0.3)
            queued = [(kc, kp, None, None, np.full(6, var), rk, rel.astype(F)) for at, kc, kp, rel, var, rk in loops if at == k]
            res, latest = m.saveKeyFramesAndFactor(poses[k], times[k], None, loops=queued)
            corrected = m.correctPosesFromGraph()
            want.append("key %d %d %d %d %d %.17g %s %d" % (k, res.iterations, res.inner_iterations, res.converged, res.n_factors, res.error_after,
                                                            " ".join("%.9g" % v for v in latest), 1 if corrected else 0))
        kp = m.pgPoses()
        raw = m.globalMapCloud(0, n, 0.0)
    finally:
        m.close()
    # after the last closure every later key was added at its own estimate: the store and the graph agree
    want += ["kp %d %s" % (k, " ".join("%.9g" % v for v in kp[k])) for k in range(n)]
    want.append("map_cloud %d" % raw.shape[0])
    got = [s.strip() for s in txt if s]
    assert sum(line.endswith(" 1") and line.startswith("key ") for line in got) == 2
    assert got == want
    _same(np.fromfile(tmp_path / "out.bin", dtype=F).reshape(-1, 8), raw)
