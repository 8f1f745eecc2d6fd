"""Verification of many keys in one call (s2m_loop_verify_many) on the scripted revisit of tests/test_loop_closure_cpu.py, two
handles filled alike: records, best[] and the container afterwards are byte for byte what a loop of s2m_loop_verify over the rows
leaves - every record the twin's loopAlign(key_cur, key_pre[i]) on a refilled store - whatever the passes are, and the call keeps
the BUSY and argument rules of the single verification."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_cpu import icp_scene
from test_loop_closure_cpu import scripted_revisit
from test_loop_verify_gpu import ACCEPTED, CLOSED, FEW, NONE, PENDING, REJECTED, RS, SC, _bytes, _equal, _fill, _twin

pytestmark = pytest.mark.gpu

ROWS = [(31, [16, 4, 0, 24, 2]), (30, [0, 1, 14]), (29, [2]), (20, []), (28, [3, 12])]
PATTERN = 0xA5


@pytest.fixture(scope="module")
def revisit():
    rv = scripted_revisit()
    assert len(rv[0]) == 32
    return rv


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.debugLoopVerifyManyPass(0)
    a.close()
    b.close()


class Raw:
    """s2m_loop_verify_many through the raw C call on pre-patterned outputs."""

    def __init__(self, rows, stride=None, m=None, n_cand=None):
        self.rows = rows
        self.key_cur, self.key_pre, self.n_cand, implied = s2m._verify_many_rows(rows)
        self.stride = implied if stride is None else stride
        self.m = len(rows) if m is None else m
        if n_cand is not None:
            self.n_cand = (C.c_int32 * len(n_cand))(*n_cand)
        self.recs = (s2m.LoopResult * (max(len(rows), 1) * max(implied, 1)))()
        C.memset(self.recs, PATTERN, C.sizeof(self.recs))
        self.best = (C.c_int32 * max(len(rows), 1))(*([55] * max(len(rows), 1)))
        self.width = max(implied, 1)
        self.before = self.image()

    def image(self):
        return C.string_at(C.addressof(self.recs), C.sizeof(self.recs)) + bytes(self.best)

    def untouched(self):
        return self.image() == self.before

    def call(self, g, base_key, prm):
        return g.lib.s2m_loop_verify_many(g.h, self.key_cur, self.key_pre, self.n_cand, self.m, self.stride, base_key,
                                          None if prm is None else C.byref(prm), self.recs, self.best)

    def row(self, r):
        return [self.recs[r * self.width + i] for i in range(len(self.rows[r][1]))]

    def behind(self, r):
        """the bytes of row r's records behind n_cand[r]"""
        return b"".join(_bytes(self.recs[r * self.width + i]) for i in range(len(self.rows[r][1]), self.width))


def _twins(b, rv, rows, base_key, fields, extra=False):
    return [_twin(b, rv, k, c, base_key, fields, extra) if c else [] for k, c in rows]


def _check_rows(raw, want):
    for r, w in enumerate(want):
        _equal(raw.row(r), w)
        assert raw.best[r] == s2m.loop_verify_best(w), (r, raw.best[r])
        assert raw.behind(r) == bytes([PATTERN]) * len(raw.behind(r)), r       # nothing is written behind n_cand[r]


def _closed(g, key_cur, cand, base_key, prm):
    recs, _ = g.loopVerify(key_cur, cand, base_key, prm)
    return [r.status == CLOSED for r in recs]


def test_records_best_and_container_against_the_twin(pair, revisit):
    a, b = pair
    want = _twins(b, revisit, ROWS, -1, RS)
    flat = [w for row in want for w in row]
    print("twin", [(w.key_cur, w.key_pre, w.status, w.icp.iterations, w.icp.fitness_score) for w in flat])
    statuses = [w.status for w in flat]
    assert ACCEPTED in statuses and REJECTED in statuses                                   # (not vacuous)
    assert len({(w.icp.iterations - 1) // s2m.S2M_ICP_RANGE for w in flat}) > 1            # pairs end in different ranges
    _fill(a, revisit)
    prm = s2m.default_loop_params(**RS)
    raw = Raw(ROWS)
    assert raw.call(a, -1, prm) == 0
    _check_rows(raw, want)
    assert raw.best[3] == -1 and raw.behind(3) == bytes([PATTERN]) * (5 * C.sizeof(s2m.LoopResult))   # the row without candidates
    # the container: a row with a winner is closed, one without is open, a winner's key_pre is no closure of its own
    winners = [r for r, w in enumerate(want) if s2m.loop_verify_best(w) >= 0]
    assert winners
    for r, (key_cur, cand) in enumerate(ROWS):
        if r in winners:
            assert _closed(a, key_cur, cand, -1, prm) == [True] * len(cand)
    r0 = winners[0]
    key_pre = ROWS[r0][1][s2m.loop_verify_best(want[r0])]
    assert a.loopAlign(key_pre, ROWS[r0][0], -1, prm).status != CLOSED
    assert a.loopAlign(20, 0, -1, prm).status != CLOSED                                    # the row without candidates
    for r, (key_cur, cand) in enumerate(ROWS):
        if cand and r not in winners:
            assert _closed(a, key_cur, cand[:1], -1, prm) == [False]


def test_sc_form_and_a_gate_that_rejects_everything(pair, revisit):
    a, b = pair
    want = _twins(b, revisit, ROWS, 0, SC)
    _fill(a, revisit)
    raw = Raw(ROWS)
    assert raw.call(a, 0, s2m.default_loop_params(**SC)) == 0
    _check_rows(raw, want)
    none = dict(SC, fitness_score=-1.0)
    want = _twins(b, revisit, ROWS, 0, none)
    assert {w.status for row in want for w in row} == {REJECTED}
    _fill(a, revisit)
    prm = s2m.default_loop_params(**none)
    raw = Raw(ROWS)
    assert raw.call(a, 0, prm) == 0
    _check_rows(raw, want)
    assert [raw.best[r] for r in range(len(ROWS))] == [-1] * len(ROWS)
    for key_cur, cand in ROWS:                                                             # the container was not touched
        if cand:
            assert _closed(a, key_cur, cand[:1], 0, prm) == [False]


def _probe(g, prm, base_key):
    out = []
    for key_cur, cand in ROWS:
        recs, best = g.loopVerify(key_cur, cand[:1] or [0], base_key, prm)
        out.append((b"".join(_bytes(r) for r in recs), best))
    return out


@pytest.mark.parametrize("form", ["rs", "sc"])
def test_the_call_is_the_loop_of_single_verifications(pair, revisit, form):
    a, b = pair
    fields, base_key = (RS, -1) if form == "rs" else (SC, 0)
    prm = s2m.default_loop_params(**fields)
    _fill(a, revisit); _fill(b, revisit)
    got, best = a.loopVerifyMany(ROWS, base_key, prm)
    want = [b.loopVerify(k, c, base_key, prm) if c else ([], -1) for k, c in ROWS]
    for g, (w, _) in zip(got, want):
        _equal(g, w)
    assert best == [w[1] for w in want]
    assert _probe(a, prm, base_key) == _probe(b, prm, base_key)


def _plan_model(n_cand, per_pass):
    first, used = [], 0
    for r, n in enumerate(n_cand):
        if r == 0 or used + n > per_pass:
            first.append(r)
            used = 0
        used += n
    return first + [len(n_cand)]


def test_passes(pair, revisit):
    a, b = pair
    want = _twins(b, revisit, ROWS, -1, RS)
    aligned = sum(w.status in (ACCEPTED, REJECTED) for row in want for w in row)
    prm = s2m.default_loop_params(**RS)
    images = []
    try:
        for per_pass in (0, 8):
            a.debugLoopVerifyManyPass(per_pass)
            _fill(a, revisit)
            raw = Raw(ROWS)
            assert raw.call(a, -1, prm) == 0
            _check_rows(raw, want)
            images.append(raw.image())
            plan = s2m.loop_verify_many_plan([len(c) for _, c in ROWS], per_pass)
            assert plan == _plan_model([len(c) for _, c in ROWS], per_pass or 64)
            passes, pairs, nbytes = a.debugLoopVerifyManyLast()
            print("pairs per pass", per_pass, "plan", plan, "passes", passes, "pairs", pairs, "bytes", nbytes)
            assert (passes, pairs) == (len(plan) - 1, aligned) and nbytes > 0
        assert images[0] == images[1]
        assert len(s2m.loop_verify_many_plan([len(c) for _, c in ROWS], 8)) - 1 > 1        # more than one pass at the smallest size
    finally:
        a.debugLoopVerifyManyPass(0)


def test_gates(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    prm = s2m.default_loop_params(**RS)
    # a key_cur the container holds: closed in its row only
    want = _twins(b, revisit, ROWS, -1, RS)
    _fill(a, revisit)
    key_pre = ROWS[0][1][s2m.loop_verify_best(want[0])]
    assert a.loopAlign(31, key_pre, -1, prm).status == ACCEPTED
    got, best = a.loopVerifyMany(ROWS, -1, prm)
    assert [(r.status, r.key_cur, r.key_pre, r.n_cur) for r in got[0]] == [(CLOSED, 31, k, 0) for k in ROWS[0][1]] and best[0] == -1
    for r in range(1, len(ROWS)):
        _equal(got[r], want[r])
        assert best[r] == s2m.loop_verify_best(want[r])
    # a candidate with too few points: that record only
    prm = s2m.default_loop_params(**SC)
    rows = [(n - 1, [0, 16, n, 2]), (n - 2, [0, 1]), (n, [0, 5])]
    want = _twins(b, revisit, rows, 0, SC, extra=True)
    assert [w.status == FEW for w in want[0]] == [False, False, True, False] and want[0][2].n_prev < 1000
    _fill(a, revisit, extra=True)
    got, best = a.loopVerifyMany(rows, 0, prm)
    for g, w in zip(got, want):
        _equal(g, w)
    assert best == [s2m.loop_verify_best(w) for w in want]
    print("the short key as key_cur: n_cur", want[2][0].n_cur, [w.status for w in want[2]])
    if want[2][0].n_cur < 300:                                                             # what the twin says, not assumed
        assert [w.status for w in want[2]] == [FEW] * 2 and [g.status for g in got[2]] == [FEW] * 2
    assert a.loopAlignLaunch(n - 3, 0, 0, prm).status == PENDING                           # the handle is free
    a.loopCollect()


def test_busy(pair, revisit):
    a, b = pair
    n = len(revisit[0])
    prm = s2m.default_loop_params(**SC)
    want = _twins(b, revisit, ROWS, 0, SC)
    _fill(a, revisit)
    raw = Raw(ROWS)
    assert a.loopAlignLaunch(n - 5, 0, 0, prm).status == PENDING                           # a single closure pending
    assert raw.call(a, 0, prm) == s2m.S2M_ERR_BUSY and raw.untouched()
    a.loopCollect()
    _fill(a, revisit)
    early, _ = a.loopVerifyLaunch(n - 5, [0, 1], 0, prm)                                   # a verification pending
    assert [e.status for e in early] == [PENDING] * 2
    assert raw.call(a, 0, prm) == s2m.S2M_ERR_BUSY and raw.untouched()
    with pytest.raises(s2m.S2MError, match="BUSY"):
        a.loopVerifyMany(ROWS, 0, prm)
    with pytest.raises(s2m.S2MError, match="BUSY"):
        a.debugIcpAlignPairsDevice([icp_scene(1500, 700, 2)[:2]])
    a.loopVerifyCollect()
    _fill(a, revisit)                                                                      # (the container as the twin's)
    assert raw.call(a, 0, prm) == 0
    _check_rows(raw, want)


def test_bad_arguments_and_an_empty_store(pair, revisit):
    a, _ = pair
    n = len(revisit[0])
    a.kfReset()
    got, best = a.loopVerifyMany([(5, [0, 1]), (6, []), (7, [2])], -1)
    assert [[(r.status, r.key_cur, r.key_pre) for r in row] for row in got] == [[(NONE, -1, -1)] * 2, [], [(NONE, -1, -1)]]
    assert best == [-1, -1, -1]
    _fill(a, revisit)
    ok = [(n - 1, [0, 1]), (n - 2, [2, 3])]
    cases = [
        Raw([(n - 1, [0, 1]), (n - 2, [2]), (n - 1, [3])]),       # a repeated key_cur
        Raw([(n - 2, [0]), (n, [1])]),                            # keys out of range
        Raw([(n - 2, [0]), (-1, [1])]),
        Raw([(n - 2, [0]), (n - 1, [1, n])]),
        Raw([(n - 2, [0]), (n - 1, [1, -1])]),
        Raw([(n - 2, [0]), (n - 1, [1, n - 1])]),                 # a candidate equal to its key_cur
        Raw([(n - 2, [0]), (n - 1, [1, 2, 1])]),                  # a candidate twice in a row
        Raw(ok, stride=0), Raw(ok, stride=9),
        Raw(ok, n_cand=[2, 3]),                                   # n_cand[r] > row_stride
        Raw(ok, n_cand=[2, -1]),
        Raw(ok, m=-1),
    ]
    for k, raw in enumerate(cases):
        for base_key in (-1, 0):
            assert raw.call(a, base_key, None) == -1 and raw.untouched(), k
            assert a.lib.s2m_loop_verify_many_check_args(n, raw.key_cur, raw.key_pre, raw.n_cand, raw.m, raw.stride, base_key, None) \
                == -1, k
    raw = Raw(ok)
    assert raw.call(a, n, None) == -1 and raw.untouched()              # base_key out of range
    assert a.lib.s2m_loop_verify_many(a.h, None, None, None, 2, 2, -1, None, raw.recs, raw.best) == -1
    assert a.lib.s2m_loop_verify_many(a.h, raw.key_cur, raw.key_pre, raw.n_cand, 2, 2, -1, None, None, None) == -1
    assert raw.untouched()
    assert a.lib.s2m_loop_verify_many(a.h, None, None, None, 0, 1, -1, None, None, None) == 0                  # m == 0
    assert s2m.loop_verify_many_check_args(n, ok) == 0
    prm = s2m.default_loop_params(**SC)
    for key_cur, _ in ok:                                         # nothing reached the container
        assert _closed(a, key_cur, [0], 0, dict_prm(prm, -1.0)) == [False]


def dict_prm(prm, fitness):
    p = s2m.default_loop_params()
    C.memmove(C.byref(p), C.byref(prm), C.sizeof(p))
    p.fitness_score = fitness
    return p


def test_the_synchronous_icp_agrees_after_the_call(pair, revisit):
    a, b = pair
    _fill(a, revisit)
    a.loopVerifyMany(ROWS, 0, s2m.default_loop_params(**SC))
    src, tgt, _ = icp_scene(1500, 700, 2)
    Ta, Tb = a.icpAlign(src, tgt), b.icpAlign(src, tgt)
    assert np.array_equal(Ta[0].view(np.uint32), Tb[0].view(np.uint32)) and Ta[1:] == Tb[1:]
    Ta, Tb = a.debugIcpAlignDevice(src, tgt), b.debugIcpAlignDevice(src, tgt)
    assert np.array_equal(Ta[0].view(np.uint32), Tb[0].view(np.uint32)) and Ta[1:] == Tb[1:]
