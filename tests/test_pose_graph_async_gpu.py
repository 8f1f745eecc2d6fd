"""The pose-graph optimise beside the scan handler (s2m_pg_optimize_launch / s2m_pg_optimize_poll / s2m_pg_optimize_collect),
two handles filled alike: the launched solve returns the bytes of s2m_pg_optimize and leaves its estimates, the calls that
need the estimates are BUSY while it is pending, everything else - registration and a launched loop closure included - is
bit for bit what it is without a pending optimise, and variables added after the launch follow the last variable of the solve."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402
from test_loop_closure_cpu import scripted_revisit  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
OK, PENDING, IDLE = s2m.S2M_OK, s2m.S2M_PG_PENDING, s2m.S2M_PG_IDLE
POLL_CAP_S = 20.0
KITTI = dict(search_radius=15.0, search_num=25, icp_leaf=0.5)

GRAPHS = {name: (lambda name=name: CS.build(name)) for name in CS.SMALL}
GRAPHS.update({"eight_64": lambda: P.figure_eight(64, 2), "eight_65": lambda: P.figure_eight(65, 2),
               "eight_1100": lambda: P.figure_eight(1100, 4)})


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.close()
    b.close()


_built = {}


def _graph(name):
    """Every case is built once; the reference graph is only read (CS.load_into) afterwards."""
    if name not in _built:
        _built[name] = GRAPHS[name]()
    return _built[name]


def _load(a, b, name):
    g = _graph(name)
    CS.load_into(a, g)
    CS.load_into(b, g)
    return g


def _early(code, early, a):
    assert code == PENDING
    assert (early.n_variables, early.n_factors) == a.pgSize()
    assert (early.iterations, early.inner_iterations, early.converged, early.error_before, early.error_after) == (0, 0, 0, 0.0, 0.0)
    assert early.robust_weight_min == 1.0


def _launch_collect(a, params=None):
    code, early = a.pgOptimizeLaunch(params)
    _early(code, early, a)
    code, got = a.pgOptimizeCollect()
    assert code == OK
    assert a.pgOptimizePoll()[0] == IDLE
    return got


# ---- 1. launch + collect equals the synchronous call ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(GRAPHS))
def test_launch_and_collect_equal_the_synchronous_call(pair, name):
    a, b = pair
    _load(a, b, name)
    want = b.pgOptimize()
    got = _launch_collect(a)
    print(name, "iterations", want.iterations, "inner", want.inner_iterations, "converged", want.converged)
    assert want.iterations >= 1                       # steps were kept: the close ran more than once
    assert _bytes(got) == _bytes(want)
    assert np.array_equal(a.pgPoses(), b.pgPoses())
    # again on the optimised graph: the first step is rejected, or one more is kept
    want2 = b.pgOptimize()
    got2 = _launch_collect(a)
    print(name, "second: iterations", want2.iterations, "inner", want2.inner_iterations)
    assert _bytes(got2) == _bytes(want2)
    assert np.array_equal(a.pgPoses(), b.pgPoses())


@pytest.mark.parametrize("kw", [dict(max_iterations=0), dict(cg_max_iterations=5)])
def test_iteration_caps_equal_the_synchronous_call(pair, kw):
    a, b = pair
    _load(a, b, "loops_200")
    prm = s2m.default_pg_params(**kw)
    want = b.pgOptimize(prm)
    got = _launch_collect(a, prm)
    print(kw, "iterations", want.iterations, "inner", want.inner_iterations, "converged", want.converged)
    assert _bytes(got) == _bytes(want)
    assert np.array_equal(a.pgPoses(), b.pgPoses())


def test_empty_graph_and_launch_errors_leave_nothing_pending(pair):
    a, b = pair
    a.pgReset(); b.pgReset()
    code, early = a.pgOptimizeLaunch()
    assert code == OK and _bytes(early) == _bytes(b.pgOptimize())
    assert a.pgOptimizePoll()[0] == IDLE and a.pgOptimizeCollect()[0] == IDLE
    p0 = np.array([1, 2, 3, 0.1, -0.2, 0.3], F)
    # a variable without a value
    a.addOdomFactor(p0)
    a.pgAddBetween(0, 1, np.zeros(6, F), np.ones(6))
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        a.pgOptimizeLaunch()
    assert a.pgOptimizePoll()[0] == IDLE and a.pgSize() == (2, 2)
    # no prior on key 0
    a.pgReset()
    a.pgSetInitial(0, p0)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        a.pgOptimizeLaunch()
    assert a.pgOptimizePoll()[0] == IDLE and a.pgOptimizeCollect()[0] == IDLE
    bad = s2m.default_pg_params(max_iterations=-1)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        a.pgOptimizeLaunch(bad)
    assert a.pgOptimizePoll()[0] == IDLE
    a.pgReset()


# ---- 2. polled to the end ------------------------------------------------------------------------------------------

def test_polled_to_the_end(pair):
    a, b = pair
    _load(a, b, "loops_200")
    want = b.pgOptimize()
    code, early = a.pgOptimizeLaunch()
    _early(code, early, a)
    lib, h = a.lib, a.h
    out = s2m.PgResult()
    out.iterations, out.n_factors, out.error_after = 77, 78, 79.0
    before = _bytes(out)
    polls, t0 = 0, time.monotonic()
    while True:                                       # each poll returns at once; the device ends every range it was given
        code = lib.s2m_pg_optimize_poll(h, C.byref(out))
        polls += 1
        if code != PENDING:
            break
        assert _bytes(out) == before
        if time.monotonic() - t0 > POLL_CAP_S:
            a.pgOptimizeCollect()
            pytest.fail("the launched optimise did not end within %g s of polling" % POLL_CAP_S)
    print("polls", polls)
    assert code == OK and _bytes(out) == _bytes(want)
    out2 = s2m.PgResult()
    out2.iterations = 55
    before = _bytes(out2)
    assert lib.s2m_pg_optimize_poll(h, C.byref(out2)) == IDLE and _bytes(out2) == before
    assert lib.s2m_pg_optimize_collect(h, C.byref(out2)) == IDLE and _bytes(out2) == before
    assert np.array_equal(a.pgPoses(), b.pgPoses())


# ---- 3. while pending ----------------------------------------------------------------------------------------------

def test_busy_while_pending(pair):
    a, b = pair
    g = _load(a, b, "loops_200")
    n = g.n
    want = b.pgOptimize()
    want_poses = b.pgPoses()
    code, _ = a.pgOptimizeLaunch()
    assert code == PENDING
    lib, h = a.lib, a.h
    r = s2m.PgResult()
    r.iterations, r.n_factors = 77, 78
    before = _bytes(r)
    assert lib.s2m_pg_optimize(h, None, C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    assert lib.s2m_pg_optimize_launch(h, None, C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    buf = np.full((n, 6), 5.0, F)
    assert lib.s2m_pg_get_poses(h, 0, n, buf.ctypes.data_as(C.POINTER(C.c_float))) == s2m.S2M_ERR_BUSY and np.all(buf == 5.0)
    cov = np.full(144, 5.0)
    dp = cov.ctypes.data_as(C.POINTER(C.c_double))
    keys = np.array([1, 2], np.int32)
    assert lib.s2m_pg_marginal(h, 3, dp) == s2m.S2M_ERR_BUSY
    assert lib.s2m_pg_marginals(h, keys.ctypes.data_as(C.POINTER(C.c_int32)), 2, dp) == s2m.S2M_ERR_BUSY
    assert lib.s2m_pg_joint_marginal(h, 1, 2, dp) == s2m.S2M_ERR_BUSY and np.all(cov == 5.0)
    assert lib.s2m_pg_apply_to_store(h, 0, 0) == s2m.S2M_ERR_BUSY
    p = np.array([1, 2, 3, 0.1, -0.2, 0.3], F)
    assert lib.s2m_pg_set_initial(h, n - 1, p.ctypes.data_as(C.POINTER(C.c_float))) == s2m.S2M_ERR_BUSY
    for call in (lambda: a.pgOptimize(), lambda: a.pgOptimizeLaunch(), lambda: a.pgPoses(), lambda: a.pgMarginal(0),
                 lambda: a.pgMarginals([0, 1]), lambda: a.pgJointMarginal(0, 1), lambda: a.pgApplyToStore(0, 0),
                 lambda: a.pgSetInitial(0, p)):
        with pytest.raises(s2m.S2MError, match="BUSY"):
            call()
    assert a.pgSize() == b.pgSize()
    code, got = a.pgOptimizeCollect()
    assert code == OK and _bytes(got) == _bytes(want)            # none of them touched the pending solve
    assert np.array_equal(a.pgPoses(), want_poses)
    # and the same calls serve again
    assert np.array_equal(a.pgMarginal(3), b.pgMarginal(3))


def test_adds_work_while_pending(pair):
    a, b = pair
    g = _load(a, b, "gps_120")
    n, nf = a.pgSize()
    want = b.pgOptimize()
    assert a.pgOptimizeLaunch()[0] == PENDING
    z6 = np.zeros(6, F)
    a.pgAddPrior(5, g.poses()[5].astype(F), np.ones(6))
    a.pgAddBetween(10, 20, z6, np.ones(6), 1.0)
    a.pgAddGps(7, [1.0, 2.0, 3.0], [1.0, 1.0, 1.0])
    a.pgAddBetween(n - 1, n, z6, np.full(6, 1e-4))            # a new variable, and its value
    a.pgSetInitial(n, g.poses()[n - 1].astype(F))
    assert a.pgSize() == (n + 1, nf + 4)
    code, got = a.pgOptimizeCollect()
    assert code == OK and _bytes(got) == _bytes(want)            # the new factors are not part of the pending solve
    assert np.array_equal(a.pgPoses(0, n), b.pgPoses())
    assert a.pgOptimize().n_factors == nf + 4


def _register(g, cfg):
    """A small registration through the resident path: s2m_downsample_scan + s2m_optimize_resident."""
    g.setInputCloud(synth.to_xyzi(cfg["map"]))
    ds = g.downsampleCurrentScan(synth.to_xyzi(cfg["scan"]), 0.2)
    g.transformTobeMapped = cfg["pose_init"].copy()
    res = g.scan2MapOptimization()
    assert ds.shape[0] >= 100 and res.iters_run >= 2               # a registration that ran
    return _bytes(res), b"".join(_bytes(x) for x in g.trace()), g.transformTobeMapped.tobytes(), ds.tobytes()


def test_registration_is_undisturbed_by_a_pending_optimise(pair, cfg_tiny):
    a, b = pair
    _load(a, b, "eight_1100")
    want = b.pgOptimize()
    reg_b = _register(b, cfg_tiny)
    assert a.pgOptimizeLaunch()[0] == PENDING
    reg_a = _register(a, cfg_tiny)
    code, got = a.pgOptimizeCollect()
    assert code == OK and _bytes(got) == _bytes(want)
    assert reg_a == reg_b
    assert np.array_equal(a.pgPoses(), b.pgPoses())


def test_a_launched_loop_closure_pending_at_the_same_time(pair):
    a, b = pair
    clouds, poses, times, _ = scripted_revisit()
    n = len(clouds)
    for m in (a, b):
        m.kfReset()
        for k in range(n):
            m.saveKeyFrame(poses[k], times[k], clouds[k])
    _load(a, b, "loops_200")
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    want_loop = b.loopAlign(n - 1, 0, -1, prm)
    want = b.pgOptimize()
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == s2m.S2M_LOOP_PENDING
    assert a.pgOptimizeLaunch()[0] == PENDING
    code, got = a.pgOptimizeCollect()
    got_loop = a.loopCollect()
    assert code == OK and _bytes(got) == _bytes(want)
    assert _bytes(got_loop) == _bytes(want_loop) and want_loop.status == s2m.S2M_LOOP_ACCEPTED
    assert np.array_equal(a.pgPoses(), b.pgPoses())
    a.kfReset(); b.kfReset()


def test_reset_and_destroy_while_pending(pair):
    a, b = pair
    _load(a, b, "loops_200")
    assert a.pgOptimizeLaunch()[0] == PENDING
    a.pgReset()
    assert a.pgOptimizePoll()[0] == IDLE and a.pgOptimizeCollect()[0] == IDLE and a.pgSize() == (0, 0)
    _load(a, b, "gps_120")                                       # a fresh graph on the handle solves like its twin
    want = b.pgOptimize()
    got = _launch_collect(a)
    assert _bytes(got) == _bytes(want) and np.array_equal(a.pgPoses(), b.pgPoses())
    m = s2m.MapOptimizationS2M()
    try:
        CS.load_into(m, _graph("loops_200"))
        assert m.pgOptimizeLaunch()[0] == PENDING
    finally:
        m.close()                                                 # returns with the optimise still pending
    assert m.h is None


# ---- 4. the tail ---------------------------------------------------------------------------------------------------

def _rel(p_from, p_to):
    """p_from^-1 p_to of two float pose vectors, in fp64: (R, t)."""
    Ra, ta = P.pose_from_xyzrpy(np.asarray(p_from, np.float64))
    Rb, tb = P.pose_from_xyzrpy(np.asarray(p_to, np.float64))
    return Ra.T @ Rb, Ra.T @ (tb - ta)


def test_variables_added_after_the_launch_follow_the_solve(pair):
    a, b = pair
    _load(a, b, "loops_200")
    n, nf = a.pgSize()
    assert n == 200
    want = b.pgOptimize()
    launch_last = a.pgPoses(n - 1, 1)[0]                           # the launch-time estimate of key 199, as a float pose
    assert a.pgOptimizeLaunch()[0] == PENDING
    # three key frames 1 m apart in the last key's frame, then a loop from the newest key to key 10
    Rl, tl = P.pose_from_xyzrpy(launch_last.astype(np.float64))
    handed = []
    for k in range(3):
        Rn = Rl @ P.rzryrx(0.0, 0.0, 0.02 * (k + 1))
        tn = tl + Rl @ np.array([1.0 * (k + 1), 0.1 * k, 0.0])
        handed.append(P.xyzrpy_from_pose(Rn, tn).astype(F))
        a.addOdomFactor(handed[-1])
    a.pgAddBetween(n + 2, 10, np.array([0.3, -0.2, 0.0, 0.0, 0.0, 0.01], F), np.full(6, 0.3))
    assert a.pgSize() == (n + 3, nf + 4)
    code, got = a.pgOptimizeCollect()
    assert code == OK and _bytes(got) == _bytes(want) and got.iterations > 0
    after = a.pgPoses()
    assert np.array_equal(after[:n], b.pgPoses())                  # keys 0..199: the 200-key graph's optimise
    assert not np.array_equal(after[n - 1], launch_last)           # the solve moved the last key
    # the new keys moved with key 199: their poses relative to it are those handed in. Four float quanta: rounding of the
    # float inputs and outputs, no solver in between.
    qr, qt = CS.quanta(np.concatenate([after, np.array(handed)]))
    for k in range(3):
        Rg, tg = _rel(after[n - 1], after[n + k])
        Rw, tw = _rel(launch_last, handed[k])
        rot = float(np.linalg.norm(P.so3_log(Rw.T @ Rg)))
        trans = float(np.abs(tg - tw).max())
        print("tail key", n + k, "rot gap", rot, "bound", 4 * qr, "trans gap", trans, "bound", 4 * qt)
        assert rot <= 4 * qr and trans <= 4 * qt
    res = a.pgOptimize()                                           # the grown graph, loop included, from the re-based values
    print("following optimise", res.iterations, res.error_before, res.error_after)
    assert res.converged == 1 and res.error_after <= res.error_before and (res.n_variables, res.n_factors) == (n + 3, nf + 4)


def test_no_kept_step_leaves_the_tail_untouched(pair):
    """iterations == 0: a launch on the optimised graph when its first step is rejected (the reference takes 0-1 steps there),
    and max_iterations = 0, which keeps no step whatever the graph."""
    a, b = pair
    _load(a, b, "loops_200")
    b.pgOptimize(); a.pgOptimize()
    checked = 0
    for prm in (None, s2m.default_pg_params(max_iterations=0)):
        n = a.pgSize()[0]
        want = b.pgOptimize(prm)
        code, _ = a.pgOptimizeLaunch(prm)
        assert code == PENDING
        p = np.array([3.25, -1.5, 0.75, 0.01, -0.02, 1.5], F) + F(checked)
        for m in (a, b):                                           # b never has an optimise pending
            m.pgAddBetween(n - 1, n, np.zeros(6, F), np.full(6, 1e-4))
            m.pgSetInitial(n, p)
        code, got = a.pgOptimizeCollect()
        assert code == OK and _bytes(got) == _bytes(want)
        print("iterations", want.iterations)
        if want.iterations == 0:
            assert np.array_equal(a.pgPoses(), b.pgPoses())        # the value set before the collect came back bit for bit
            checked += 1
        else:
            assert np.array_equal(a.pgPoses(0, n), b.pgPoses(0, n))
            b.pgSetInitial(n, a.pgPoses(n, 1)[0])                  # (keep the twins alike for the next round)
            a.pgSetInitial(n, a.pgPoses(n, 1)[0])
    assert checked >= 1


# ---- 5. the store --------------------------------------------------------------------------------------------------

def test_launched_optimise_then_apply_to_store(pair):
    a, b = pair
    rng = np.random.default_rng(P.SEED)
    g = _graph("loops_200")
    init = g.poses().astype(F)
    clouds = []
    for _ in range(16):
        c = synth.to_xyzi(rng.uniform(-20, 20, (int(rng.integers(200, 500)), 3)).astype(F))
        c[:, 4] = rng.uniform(0, 100, c.shape[0]).astype(F)
        clouds.append(c)
    outs = []
    for m, launched in ((a, True), (b, False)):
        m.kfReset()
        for k in range(g.n):
            m.saveKeyFrame(init[k], float(k), clouds[k % len(clouds)])
        CS.load_into(m, g)
        if launched:
            assert m.pgOptimizeLaunch()[0] == PENDING
            assert m.pgOptimizeCollect()[0] == OK
        else:
            m.pgOptimize()
        m.pgApplyToStore(0, g.n)
        keys, local = m.extractSurroundingKeyFrames(float(g.n), s2m.default_kf_params(map_leaf=0.4), return_map=True)
        raw = m.globalMapCloud(0, g.n, 0.0)
        outs.append((m.pgPoses(), np.asarray(keys), np.asarray(local), raw))
        m.kfReset()
    assert not np.array_equal(outs[0][0], init)
    for x, y in zip(outs[0], outs[1]):
        assert x.shape == y.shape
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


# ---- 6. the C++ host mirror through s2m_harness --pose-graph ... --async -------------------------------------------

def test_harness_prints_the_launched_optimise_beside_the_synchronous_one(tmp_path):
    import subprocess
    rng = np.random.default_rng(P.SEED + 3)
    n = 40
    truth = P.figure_eight(n, 0, truth_only=True)
    poses = np.array([P.xyzrpy_from_pose(R, t) for R, t in truth])
    poses[:, :3] += np.cumsum(rng.normal(0, 0.01, (n, 3)), 0)          # a drifting front end
    poses = poses.astype(F)
    clouds = [synth.to_xyzi(rng.uniform(-20, 20, (200, 3)).astype(F)) for _ in range(n)]
    rel = s2m.between_xyzrpy(poses[29], poses[9]) + np.array([0.05, -0.02, 0.0, 0, 0, 0.003], F)
    np.concatenate(clouds).astype(F).tofile(tmp_path / "keys.bin")
    with open(tmp_path / "keys.txt", "w") as f:
        for k in range(n):
            f.write("%d %.17g %s\n" % (len(clouds[k]), float(k), " ".join("%.9g" % v for v in poses[k])))
    with open(tmp_path / "loops.txt", "w") as f:
        f.write("30 29 9 %s 0.3 0\n" % " ".join("%.9g" % v for v in rel.astype(F)))
    harness = os.path.join(ROOT, "liorf_amd", "host", "s2m_harness")
    args = [harness, "--pose-graph", str(tmp_path / "keys.bin"), str(tmp_path / "keys.txt"), "0.3", str(tmp_path / "loops.txt"), str(tmp_path / "out.bin")]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    both = subprocess.run(args + ["--async"], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    extra = [s for s in both if s.startswith("optimize_")]
    assert [s for s in both if not s.startswith("optimize_")] == plain          # the record the Python mirror is compared with is unchanged
    assert len(extra) == 2 and extra[0].startswith("optimize_sync ") and extra[1].startswith("optimize_launched ")
    print(extra)
    assert extra[0].split()[1:] == extra[1].split()[1:]                          # %.17g: equal lines are equal bits
    assert int(extra[0].split()[4]) == n and int(extra[0].split()[5]) == n + 1   # variables, factors
