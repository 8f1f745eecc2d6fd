"""Loop-closure verification (s2m_loop_verify, _launch, _poll, _collect) on the scripted revisit of tests/test_loop_closure_cpu.py,
two handles filled alike: record i is byte for byte the twin's loopAlign(key_cur, key_pre[i]) on a container that does not hold
key_cur, `best` follows the model (least (fitness, position) among the accepted), only that pair goes into the container, and a
pending verification is a pending closure for every other call."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m, synth
from test_icp_cpu import icp_scene
from test_loop_closure_cpu import scripted_revisit

pytestmark = pytest.mark.gpu

KITTI = dict(search_radius=15.0, search_num=25, icp_leaf=0.5)
PENDING, ACCEPTED, REJECTED, FEW, CLOSED, NONE = (s2m.S2M_LOOP_PENDING, s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_REJECTED,
                                                  s2m.S2M_LOOP_TOO_FEW_POINTS, s2m.S2M_LOOP_ALREADY_CLOSED, s2m.S2M_LOOP_NONE)
RS = dict(KITTI, search_num=2)
SC = dict(KITTI, search_num=0)
RS_CAND = [16, 4, 0, 24, 2]
SC_CAND = [0, 1, 16, 2]


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


def _fill(g, rv, extra=False):
    clouds, poses, times, _ = rv
    g.kfReset()
    for k in range(len(clouds)):
        g.saveKeyFrame(poses[k], times[k], clouds[k])
    if extra:                                                     # a 33rd key: the first 600 records of key 5's cloud
        g.saveKeyFrame(poses[5], times[-1] + 1.0, clouds[5][:600])


_TWIN = {}


def _twin(b, rv, key_cur, cand, base_key, fields, extra=False):
    """The twin's loopAlign per candidate, each on a container that does not hold key_cur (the store is refilled before each
    call). Computed once per case and shared."""
    tag = (key_cur, tuple(cand), base_key, tuple(sorted(fields.items())), extra)
    if tag not in _TWIN:
        prm = s2m.default_loop_params(**fields)
        out = []
        for k in cand:
            _fill(b, rv, extra)
            out.append(b.loopAlign(key_cur, k, base_key, prm))
        _TWIN[tag] = out
    return _TWIN[tag]


def _equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _bytes(g) == _bytes(w), (i, g.status, w.status, g.icp.iterations, w.icp.iterations, g.icp.fitness_score, w.icp.fitness_score)


def test_rs_form_records_best_and_container(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    want = _twin(b, revisit, n - 1, RS_CAND, -1, RS)
    print("twin", [(w.key_pre, w.status, w.icp.iterations, w.icp.fitness_score, w.n_prev) for w in want])
    statuses = [w.status for w in want]
    assert ACCEPTED in statuses and REJECTED in statuses          # (not vacuous)
    assert len({(w.icp.iterations - 1) // s2m.S2M_ICP_RANGE for w in want}) > 1     # slots end in different ranges
    _fill(a, revisit)
    prm = s2m.default_loop_params(**RS)
    early, best = a.loopVerifyLaunch(n - 1, RS_CAND, -1, prm)
    assert best == -1
    for e, w, k in zip(early, want, RS_CAND):
        assert (e.status, e.key_cur, e.key_pre, e.n_cur, e.n_prev) == (PENDING, n - 1, k, w.n_cur, w.n_prev)
        assert e.icp.iterations == 0 and list(e.pose_from) == [0.0] * 6
    got, best = a.loopVerifyCollect()
    _equal(got, want)
    assert best == s2m.loop_verify_best(want) and want[best].status == ACCEPTED
    assert a.loopVerifyPoll() == ([], -1) and a.loopVerifyCollect() == ([], -1)
    # the container holds key_cur -> key_pre[best] only: the same call again is closed in every record ...
    again, best2 = a.loopVerify(n - 1, RS_CAND, -1, prm)
    assert best2 == -1 and [(r.status, r.key_cur, r.key_pre, r.n_cur) for r in again] == [(CLOSED, n - 1, k, 0) for k in RS_CAND]
    assert a.loopVerifyPoll() == ([], -1)
    # ... and another accepted candidate was not recorded as a closure of its own key: key 2 against key_cur still aligns
    others = [i for i, w in enumerate(want) if w.status == ACCEPTED and i != best]
    assert others
    assert a.loopAlign(RS_CAND[others[0]], n - 1, -1, prm).status != CLOSED


def test_sc_form_and_a_gate_that_rejects_everything(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    want = _twin(b, revisit, n - 1, SC_CAND, 0, SC)
    print("twin", [(w.key_pre, w.status, w.icp.iterations, w.icp.fitness_score) for w in want])
    assert want[0].icp.fitness_score == 0.0 and ACCEPTED in [w.status for w in want]
    _fill(a, revisit)
    got, best = a.loopVerify(n - 1, SC_CAND, 0, s2m.default_loop_params(**SC))
    _equal(got, want)
    assert best == s2m.loop_verify_best(want) == 0
    none = dict(SC, fitness_score=-1.0)
    want = _twin(b, revisit, n - 1, SC_CAND, 0, none)
    assert [w.status for w in want] == [REJECTED] * 4
    _fill(a, revisit)
    got, best = a.loopVerify(n - 1, SC_CAND, 0, s2m.default_loop_params(**none))
    _equal(got, want)
    assert best == -1
    early, _ = a.loopVerifyLaunch(n - 1, SC_CAND, 0, s2m.default_loop_params(**none))      # the container was not touched
    assert [e.status for e in early] == [PENDING] * 4
    a.loopVerifyCollect()


def test_a_candidate_with_too_few_points_takes_no_slot(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    cand = [0, 16, n, 2]                                          # key n is the short one
    want = _twin(b, revisit, n - 1, cand, 0, SC, extra=True)
    assert [w.status == FEW for w in want] == [False, False, True, False] and want[2].n_prev < 1000
    _fill(a, revisit, extra=True)
    prm = s2m.default_loop_params(**SC)
    early, best = a.loopVerifyLaunch(n - 1, cand, 0, prm)
    assert [e.status for e in early] == [PENDING, PENDING, FEW, PENDING] and best == -1
    assert _bytes(early[2]) == _bytes(want[2])
    got, best = a.loopVerifyCollect()
    _equal(got, want)                                             # in the caller's order
    assert best == s2m.loop_verify_best(want)
    _fill(a, revisit, extra=True)
    only, best = a.loopVerifyLaunch(n - 1, [n], 0, prm)           # final at launch, nothing pending
    assert _bytes(only[0]) == _bytes(want[2]) and best == -1
    assert a.loopVerifyPoll() == ([], -1)
    assert a.loopAlignLaunch(n - 1, 0, 0, prm).status == PENDING   # (the handle is free)
    a.loopCollect()


def test_one_candidate_is_the_single_launch(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    prm = s2m.default_loop_params(**RS)
    _fill(a, revisit); _fill(b, revisit)
    e1 = b.loopAlignLaunch(n - 1, 0, -1, prm)
    want = b.loopCollect()
    early, _ = a.loopVerifyLaunch(n - 1, [0], -1, prm)
    assert _bytes(early[0]) == _bytes(e1)
    got, best = a.loopVerifyCollect()
    assert len(got) == 1 and _bytes(got[0]) == _bytes(want) and best == (0 if want.status == ACCEPTED else -1)
    assert want.status == ACCEPTED


def test_polling_to_the_end_gives_the_collected_bytes(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    want = _twin(b, revisit, n - 1, RS_CAND, -1, RS)
    _fill(a, revisit)
    early, _ = a.loopVerifyLaunch(n - 1, RS_CAND, -1, s2m.default_loop_params(**RS))
    polls = 0
    while True:                                                   # each poll returns at once
        recs, best = a.loopVerifyPoll()
        polls += 1
        if not recs or recs[0].status != PENDING:
            break
        assert best == -1 and [_bytes(r) for r in recs] == [_bytes(e) for e in early] and polls < 10_000_000
    print("polls", polls)
    _equal(recs, want)
    assert best == s2m.loop_verify_best(want)
    assert a.loopVerifyPoll() == ([], -1)


def test_busy_table(pair, revisit):
    a, b = pair
    clouds, poses, times, _ = revisit
    n = len(clouds)
    want = _twin(b, revisit, n - 1, SC_CAND, 0, SC)
    _fill(a, revisit)
    prm = s2m.default_loop_params(**SC)
    src, tgt, _ = icp_scene(1500, 700, 2)
    lib, h = a.lib, a.h
    recs = (s2m.LoopResult * 8)()
    recs[0].status, recs[1].key_cur = 77, 78
    before = C.string_at(C.addressof(recs), C.sizeof(recs))
    nn, bb = C.c_int32(55), C.c_int32(56)
    keys = (C.c_int32 * 2)(3, 4)

    def untouched():
        return C.string_at(C.addressof(recs), C.sizeof(recs)) == before and (nn.value, bb.value) == (55, 56)

    # a single closure pending: the verify forms are BUSY and touch nothing
    assert a.loopAlignLaunch(n - 1, 0, 0, prm).status == PENDING
    assert lib.s2m_loop_verify_poll(h, recs, 8, C.byref(nn), C.byref(bb)) == s2m.S2M_ERR_BUSY and untouched()
    assert lib.s2m_loop_verify_collect(h, recs, 8, C.byref(nn), C.byref(bb)) == s2m.S2M_ERR_BUSY and untouched()
    assert lib.s2m_loop_verify_launch(h, n - 1, keys, 2, 0, C.byref(prm), recs, C.byref(bb)) == s2m.S2M_ERR_BUSY and untouched()
    assert lib.s2m_loop_verify(h, n - 1, keys, 2, 0, C.byref(prm), recs, C.byref(bb)) == s2m.S2M_ERR_BUSY and untouched()
    assert _bytes(a.loopCollect()) == _bytes(want[0])
    # a verification pending: it is a pending closure for every call with a BUSY rule, s2m_loop_poll / _collect included
    _fill(a, revisit)
    early, _ = a.loopVerifyLaunch(n - 1, SC_CAND, 0, prm)
    assert [e.status for e in early] == [PENDING] * 4
    r = s2m.LoopResult()
    r.status, r.key_cur = 77, 78
    rb = _bytes(r)
    assert lib.s2m_loop_poll(h, C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == rb
    assert lib.s2m_loop_collect(h, C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == rb
    assert lib.s2m_loop_align(h, n - 1, 0, -1, C.byref(prm), C.byref(r)) == s2m.S2M_ERR_BUSY and _bytes(r) == rb
    assert lib.s2m_loop_verify_launch(h, n - 1, keys, 2, 0, C.byref(prm), recs, C.byref(bb)) == s2m.S2M_ERR_BUSY and untouched()
    for call in (lambda: a.loopAlign(n - 1, 0, -1, prm), lambda: a.performRSLoopClosure(times[-1], prm),
                 lambda: a.loopFindNearKeyframes(3, 2, -1, 0.5), lambda: a.icpAlign(src, tgt),
                 lambda: a.loopAlignLaunch(n - 1, 0, -1, prm), lambda: a.debugIcpAlignDevice(src, tgt),
                 lambda: a.debugIcpAlignManyDevice(src, [tgt]), lambda: a.debugIcpNearest(src, tgt, 1),
                 lambda: a.loopVerify(n - 1, [0], 0, prm), lambda: a.debugIcpTuning()):
        with pytest.raises(s2m.S2MError, match="BUSY"):
            call()
    assert lib.s2m_loop_verify_poll(h, recs, 2, C.byref(nn), C.byref(bb)) == s2m.S2M_ERR_CAPACITY and nn.value == 4   # cap records written
    assert (recs[0].key_pre, recs[1].key_pre, recs[2].key_pre) == (SC_CAND[0], SC_CAND[1], 0)
    got, best = a.loopVerifyCollect()                             # none of them touched the pending verification
    _equal(got, want)
    assert best == 0
    Ta, Tb = a.icpAlign(src, tgt), b.icpAlign(src, tgt)           # and the loop's buffers serve the synchronous calls again
    assert np.array_equal(Ta[0].view(np.uint32), Tb[0].view(np.uint32)) and Ta[1:] == Tb[1:]


def test_bad_lists_and_an_empty_store(pair, revisit):
    a, _ = pair
    n = len(revisit[0])
    a.kfReset()
    recs, best = a.loopVerify(5, [0, 1], -1)
    assert [(r.status, r.key_cur, r.key_pre) for r in recs] == [(NONE, -1, -1)] * 2 and best == -1
    _fill(a, revisit)
    for cand in ([], list(range(9)), [n], [-1], [3, 3], [n - 1], [0, n - 1]):
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
            a.loopVerifyLaunch(n - 1, cand, -1)
        assert s2m.loop_verify_check_args(n, n - 1, cand, -1) == -1
    assert a.loopVerifyPoll() == ([], -1)


def test_registration_is_undisturbed_by_a_pending_verification(cfg_tiny, revisit):
    """set_map, set_scan, optimize and saveKeyFrame between launch and collect: bit for bit what they are on the idle twin."""
    clouds, poses, times, _ = revisit
    n = len(clouds)
    m, s = synth.to_xyzi(cfg_tiny["map"]), synth.to_xyzi(cfg_tiny["scan"])
    prm = s2m.default_loop_params(**SC)
    out = []
    for pending in (False, True):
        g = s2m.MapOptimizationS2M()
        try:
            _fill(g, revisit)
            if pending:
                assert [e.status for e in g.loopVerifyLaunch(n - 1, SC_CAND, 0, prm)[0]] == [PENDING] * 4
            g.setInputCloud(m)
            g.setScan(s)
            g.transformTobeMapped = cfg_tiny["pose_init"].copy()
            res = g.scan2MapOptimization()
            tr = b"".join(_bytes(x) for x in g.trace())
            g.saveKeyFrame(poses[-1], times[-1] + 1.0, clouds[1])
            recs, best = g.loopVerifyCollect() if pending else g.loopVerify(n - 1, SC_CAND, 0, prm)
            assert g.kfSize() == n + 1
            out.append((_bytes(res), tr, g.transformTobeMapped.tobytes(), b"".join(_bytes(r) for r in recs), best))
        finally:
            g.close()
    assert out[0] == out[1] and out[0][4] == 0


def test_reset_and_destroy_while_pending(revisit):
    n = len(revisit[0])
    prm = s2m.default_loop_params(**SC)
    g = s2m.MapOptimizationS2M()
    try:
        _fill(g, revisit)
        assert g.loopVerifyLaunch(n - 1, SC_CAND, 0, prm)[0][0].status == PENDING
        g.kfReset()                                               # dropped: nothing pending, nothing recorded
        assert g.loopVerifyPoll() == ([], -1) and g.loopPoll().status == NONE
        _fill(g, revisit)
        recs, best = g.loopVerify(n - 1, SC_CAND, 0, prm)
        assert best == 0 and recs[0].status == ACCEPTED
        _fill(g, revisit)
        assert g.loopVerifyLaunch(n - 1, SC_CAND, 0, prm)[0][0].status == PENDING
    finally:
        g.close()                                                 # returns with the verification still pending
    assert g.h is None
