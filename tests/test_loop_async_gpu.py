"""Loop closure beside the scan handler (s2m_loop_align_launch / s2m_loop_closure_rs_launch / s2m_loop_poll / s2m_loop_collect)
on the scripted revisit of tests/test_loop_closure_cpu.py, two handles filled alike: the launched closure returns the bytes of
the synchronous one, early outcomes come straight from the launch, the calls that use the loop's buffers are BUSY while it is
pending and everything else - registration included - is bit for bit what it is without a pending closure."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m, synth
from test_icp_cpu import icp_scene
from test_loop_closure_cpu import scripted_revisit

pytestmark = pytest.mark.gpu

F = np.float32
KITTI = dict(search_radius=15.0, search_num=25, icp_leaf=0.5)
PENDING = s2m.S2M_LOOP_PENDING


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


@pytest.fixture(scope="module")
def revisit():
    return scripted_revisit()


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.close()
    b.close()


def _fill(g, rv):
    clouds, poses, times, _ = rv
    g.kfReset()
    for k in range(len(clouds)):
        g.saveKeyFrame(poses[k], times[k], clouds[k])


def _pending(r, key_cur, key_pre):
    assert (r.status, r.key_cur, r.key_pre) == (PENDING, key_cur, key_pre) and r.n_cur >= 300 and r.n_prev >= 1000
    assert r.icp.iterations == 0 and list(r.pose_from) == [0.0] * 6


@pytest.mark.parametrize("base_key,fitness,status", [(-1, 0.3, s2m.S2M_LOOP_ACCEPTED), (0, 0.3, s2m.S2M_LOOP_ACCEPTED),
                                                     (-1, 0.0, s2m.S2M_LOOP_REJECTED), (0, -1.0, s2m.S2M_LOOP_REJECTED)])
def test_launch_and_collect_equal_the_synchronous_call(pair, revisit, base_key, fitness, status):
    """RS and SC form, accepted and rejected at the fitness gate (gate at 0; the SC pair are the same cloud under the same pose,
    their fitness is exactly 0, so its gate is below that)."""
    a, b = pair
    n = len(revisit[0])
    _fill(a, revisit); _fill(b, revisit)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2 if base_key == -1 else 0, fitness_score=fitness))
    want = b.loopAlign(n - 1, 0, base_key, prm)
    assert want.status == status
    early = a.loopAlignLaunch(n - 1, 0, base_key, prm)
    _pending(early, n - 1, 0)
    assert (early.n_cur, early.n_prev) == (want.n_cur, want.n_prev)
    got = a.loopCollect()
    assert _bytes(got) == _bytes(want)
    assert a.loopPoll().status == s2m.S2M_LOOP_NONE              # nothing pending any more


def test_rs_launch_polled_to_the_end(pair, revisit):
    a, b = pair
    times = revisit[2]
    _fill(a, revisit); _fill(b, revisit)
    prm = s2m.default_loop_params(**KITTI)
    want = b.performRSLoopClosure(times[-1], prm)
    assert want.status == s2m.S2M_LOOP_ACCEPTED
    early = a.performRSLoopClosureLaunch(times[-1], prm)
    _pending(early, want.key_cur, want.key_pre)
    polls = 0
    while True:                                                   # each poll returns at once; the device ends every range it was given
        r = a.loopPoll()
        polls += 1
        if r.status != PENDING:
            break
        assert _bytes(r) == _bytes(early) and polls < 10_000_000
    print("polls", polls)
    assert _bytes(r) == _bytes(want)
    # the container was written by the poll that brought the result: the pair again is closed, on both handles
    for g in (a, b):
        again = g.performRSLoopClosureLaunch(times[-1], prm)
        assert (again.status, again.key_cur, again.key_pre) == (s2m.S2M_LOOP_ALREADY_CLOSED, len(times) - 1, -1)
        assert g.loopPoll().status == s2m.S2M_LOOP_NONE


def test_early_outcomes_leave_nothing_pending(pair, revisit):
    a, _ = pair
    clouds, poses, times, _ = revisit
    n = len(clouds)
    a.kfReset()
    r = a.performRSLoopClosureLaunch(5.0)
    assert (r.status, r.key_cur, r.key_pre) == (s2m.S2M_LOOP_NONE, -1, -1)          # empty store
    assert a.loopAlignLaunch(0, 0).status == s2m.S2M_LOOP_NONE
    _fill(a, revisit)
    r = a.performRSLoopClosureLaunch(times[-1], s2m.default_loop_params(**dict(KITTI, time_diff_s=1e6)))
    assert (r.status, r.key_cur, r.key_pre) == (s2m.S2M_LOOP_NONE, -1, -1)          # no candidate outside the time window
    assert _bytes(r) == _bytes(a.performRSLoopClosure(times[-1], s2m.default_loop_params(**dict(KITTI, time_diff_s=1e6))))
    small = s2m.default_loop_params(**dict(KITTI, search_num=0, icp_leaf=8.0))       # a handful of voxels per submap
    r = a.loopAlignLaunch(n - 1, 0, -1, small)
    assert r.status == s2m.S2M_LOOP_TOO_FEW_POINTS and _bytes(r) == _bytes(a.loopAlign(n - 1, 0, -1, small))
    assert a.loopPoll().status == s2m.S2M_LOOP_NONE and a.loopCollect().status == s2m.S2M_LOOP_NONE
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    assert a.loopAlign(n - 1, 0, -1, prm).status == s2m.S2M_LOOP_ACCEPTED
    r = a.loopAlignLaunch(n - 1, 0, -1, prm)
    assert (r.status, r.key_cur, r.key_pre) == (s2m.S2M_LOOP_ALREADY_CLOSED, n - 1, 0)
    p = a.loopPoll()
    assert (p.status, p.key_cur, p.key_pre) == (s2m.S2M_LOOP_NONE, -1, -1)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        a.loopAlignLaunch(n, 0)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        a.performRSLoopClosureLaunch(float("inf"))
    assert a.loopPoll().status == s2m.S2M_LOOP_NONE


def test_container_is_written_at_collect(pair, revisit):
    a, _ = pair
    n = len(revisit[0])
    _fill(a, revisit)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
    a.kfReset()                                                   # dropped before it was collected: nothing was recorded
    _fill(a, revisit)
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
    assert a.loopCollect().status == s2m.S2M_LOOP_ACCEPTED
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == s2m.S2M_LOOP_ALREADY_CLOSED


def test_busy_while_pending(pair, revisit):
    a, b = pair
    clouds, poses, times, _ = revisit
    n = len(clouds)
    _fill(a, revisit); _fill(b, revisit)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    want = b.loopAlign(n - 1, 0, -1, prm)
    src, tgt, _ = icp_scene(1500, 700, 2)
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
    r = s2m.LoopResult()
    r.status, r.key_cur, r.n_prev = 77, 78, 79
    before = _bytes(r)
    lib, h = a.lib, a.h
    assert lib.s2m_loop_align(h, n - 1, 0, -1, C.byref(prm), C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    assert lib.s2m_loop_closure_rs(h, float(times[-1]), C.byref(prm), C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    assert lib.s2m_loop_align_launch(h, n - 2, 1, -1, C.byref(prm), C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    assert lib.s2m_loop_closure_rs_launch(h, float(times[-1]), C.byref(prm), C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == before
    m = C.c_size_t(123)
    assert lib.s2m_loop_near_keyframes(h, 3, 2, -1, 0.5, None, 32, 0, C.byref(m)) == s2m.S2M_ERR_BUSY and m.value == 123
    for call in (lambda: a.loopAlign(n - 1, 0, -1, prm), lambda: a.performRSLoopClosure(times[-1], prm),
                 lambda: a.loopFindNearKeyframes(3, 2, -1, 0.5), lambda: a.icpAlign(src, tgt),
                 lambda: a.loopAlignLaunch(n - 1, 0, -1, prm), lambda: a.debugIcpAlignDevice(src, tgt),
                 lambda: a.debugIcpNearest(src, tgt, 1)):
        with pytest.raises(s2m.S2MError, match="BUSY"):
            call()
    assert _bytes(a.loopCollect()) == _bytes(want)               # none of them touched the pending closure
    # and the loop's buffers serve the synchronous calls again
    assert a.loopFindNearKeyframes(3, 2, -1, 0.5).shape[0] == b.loopFindNearKeyframes(3, 2, -1, 0.5).shape[0]
    Ta, Tb = a.icpAlign(src, tgt), b.icpAlign(src, tgt)
    assert np.array_equal(Ta[0].view(np.uint32), Tb[0].view(np.uint32)) and Ta[1:] == Tb[1:]


def test_poses_are_those_of_the_launch(pair, revisit):
    a, b = pair
    clouds, poses, times, _ = revisit
    n = len(clouds)
    _fill(a, revisit); _fill(b, revisit)
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    want = b.loopAlign(n - 1, 0, -1, prm)
    assert a.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
    moved = poses.copy()
    moved[0] += F(3.0)
    moved[n - 1] -= F(2.0)
    a.correctPoses(moved)                                       # s2m_kf_set_poses of key_cur and key_pre (and the rest)
    got = a.loopCollect()
    assert _bytes(got) == _bytes(want)
    assert list(got.pose_to) == [float(v) for v in poses[0]]


def test_registration_is_undisturbed_by_a_pending_closure(cfg_tiny, revisit):
    """set_map, set_scan, optimize and saveKeyFrame between launch and collect. The closure cannot end in between: its result is
    formed by a poll that finds the fitness pass ended, and the fitness pass is queued by an earlier poll - so the poll behind
    the registration still says PENDING, and what ran beside the registration is the grid build and the first range of iterations."""
    clouds, poses, times, _ = revisit
    n = len(clouds)
    m, s = synth.to_xyzi(cfg_tiny["map"]), synth.to_xyzi(cfg_tiny["scan"])
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    out = []
    for pending in (False, True):
        g = s2m.MapOptimizationS2M()
        try:
            _fill(g, revisit)
            if pending:
                assert g.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
            g.setInputCloud(m)
            g.setScan(s)
            g.transformTobeMapped = cfg_tiny["pose_init"].copy()
            res = g.scan2MapOptimization()
            tr = b"".join(_bytes(x) for x in g.trace())
            g.saveKeyFrame(poses[-1], times[-1] + 1.0, clouds[1])
            if pending:
                assert g.loopPoll().status == PENDING
            closure = g.loopCollect() if pending else g.loopAlign(n - 1, 0, -1, prm)
            assert g.kfSize() == n + 1
            out.append((_bytes(res), tr, g.transformTobeMapped.tobytes(), _bytes(closure)))
        finally:
            g.close()
    assert out[0] == out[1]
    assert out[0][3][:4] == np.int32(s2m.S2M_LOOP_ACCEPTED).tobytes()


def test_reset_and_destroy_while_pending(revisit):
    n = len(revisit[0])
    prm = s2m.default_loop_params(**dict(KITTI, search_num=2))
    g = s2m.MapOptimizationS2M()
    try:
        _fill(g, revisit)
        assert g.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
        g.kfReset()
        p = g.loopPoll()
        assert (p.status, p.key_cur, p.key_pre) == (s2m.S2M_LOOP_NONE, -1, -1)
        assert g.loopCollect().status == s2m.S2M_LOOP_NONE
        _fill(g, revisit)
        assert g.loopAlignLaunch(n - 1, 0, -1, prm).status == PENDING
    finally:
        g.close()                                                 # returns with the closure still pending
    assert g.h is None
