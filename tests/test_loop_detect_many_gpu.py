"""The loop detection by position for many keys (s2m_loop_detect_keys) on the device against its model
(tests/ref/loop_detect_many_ref.py): rows bit for bit over the fixed case list - store sizes at the tile's edges, query counts
at the block's, top_k 1, 3 and 8, without and with time_cur - the windows, the passes, the detector inside s2m_loop_closure_rs,
the call beside a pending closure, the end-to-end verification on the scripted revisit, the empty cases and the errors.
Stores are key frames of one point each: only poses and times matter."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import loop_detect_many_ref as M  # noqa: E402

from liorf_amd import s2m  # noqa: E402
from test_loop_closure_cpu import scripted_revisit  # noqa: E402
from test_loop_detect_many_cpu import argument_table  # noqa: E402
from test_loop_verify_gpu import ACCEPTED, CLOSED, NONE, PENDING, RS, _bytes, _fill  # noqa: E402

pytestmark = pytest.mark.gpu

T, B, S = s2m.loop_detect_shape()
KEY_MARK, N_MARK, D2_MARK = -77, -5, 0xDEADBEEF
ONE_POINT = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
i32p, f32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def model():
    """Per store size: the store and its cases with the model's rows, computed once and left unchanged."""
    stores, cases = {}, {}
    for name, N, keys, tc, kw in M.fixed_cases(T, B):
        if N not in stores:
            stores[N] = M.make_store(N)
        cases.setdefault(N, []).append((name, keys, tc, kw, M.detect_keys(*stores[N], keys, tc, **kw)))
    return stores, cases


@pytest.fixture(scope="module")
def revisit():
    return scripted_revisit()


def _store(g, P, t):
    g.kfReset()
    for k in range(len(t)):
        g.saveKeyFrame([P[k, 0], P[k, 1], P[k, 2], 0.0, 0.0, 0.0], t[k], ONE_POINT)
    assert g.kfSize() == len(t)


class Raw:
    """s2m_loop_detect_keys through the raw C call on outputs filled with marks."""

    def __init__(self, keys, time_cur=None, width=None, **kw):
        self.prm = s2m.default_loop_detect_params(**kw)
        self.keys = np.ascontiguousarray(keys, np.int32)
        self.tc = None if time_cur is None else np.ascontiguousarray(time_cur, np.float64)
        self.m = len(self.keys)
        self.K = max(self.prm.top_k, 1) if width is None else width
        self.key_pre = np.full((max(self.m, 1), self.K), KEY_MARK, np.int32)
        self.d2 = np.full((max(self.m, 1), self.K), D2_MARK, np.uint32)
        self.n = np.full(max(self.m, 1), N_MARK, np.int32)

    def call(self, g, m=None, keys=True, key_pre=True, d2=True, n=True, prm=True):
        return g.lib.s2m_loop_detect_keys(
            g.h, self.keys.ctypes.data_as(i32p) if keys else None, None if self.tc is None else self.tc.ctypes.data_as(f64p),
            self.m if m is None else m, C.byref(self.prm) if prm else None, self.key_pre.ctypes.data_as(i32p) if key_pre else None,
            self.d2.ctypes.data_as(f32p) if d2 else None, self.n.ctypes.data_as(i32p) if n else None)

    def untouched(self):
        return bool(np.all(self.key_pre == KEY_MARK) and np.all(self.d2 == D2_MARK) and np.all(self.n == N_MARK))

    def image(self):
        return self.key_pre.tobytes() + self.d2.tobytes() + self.n.tobytes()

    def check(self, want, name=""):
        """bit for bit the model's rows; the entries behind n_cand[i] keep their marks"""
        rows, d2rows, n = want
        assert np.array_equal(self.n[:self.m], n), (name, self.n[:self.m], n)
        for i in range(self.m):
            k = int(n[i])
            assert list(self.key_pre[i, :k]) == rows[i], (name, i, self.key_pre[i], rows[i])
            assert np.array_equal(self.d2[i, :k], d2rows[i].view(np.uint32)), (name, i)
            assert np.all(self.key_pre[i, k:] == KEY_MARK) and np.all(self.d2[i, k:] == D2_MARK), (name, i)


@pytest.mark.parametrize("N", M.store_sizes(T))
def test_rows_are_the_models_bit_for_bit(pair, model, N):
    a, _ = pair
    stores, cases = model
    _store(a, *stores[N])
    seen = 0
    for name, keys, tc, kw, want in cases[N]:
        if "window" in name:
            continue
        raw = Raw(keys, tc, **kw)
        assert raw.call(a) == 0, (name, a.lib.s2m_last_error(a.h))
        raw.check(want, name)
        seen += 1
    assert seen == 6 * len(M.query_counts(N, B))
    # d2 is optional: the keys and counts without it
    name, keys, tc, kw, want = cases[N][-1] if "window" not in cases[N][-1][0] else cases[N][0]
    raw = Raw(keys, tc, **kw)
    assert raw.call(a, d2=False) == 0
    assert np.array_equal(raw.n[:raw.m], want[2]) and np.all(raw.d2 == D2_MARK)
    # through the mirror: rows in the shape loopVerifyMany takes
    rows, d2 = a.loopDetectKeys(keys, tc, **kw)
    assert rows == [(int(k), r) for k, r in zip(keys, want[0])]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(d2, want[1]))


def test_windows_repeats_and_permutations(pair, model):
    a, _ = pair
    stores, cases = model
    N = 2 * T + 1
    P, t = stores[N]
    _store(a, P, t)
    seen = 0
    for name, keys, tc, kw, want in cases[N]:
        if "window" not in name:
            continue
        raw = Raw(keys, tc, **kw)
        assert raw.call(a) == 0, name
        raw.check(want, name)
        seen += 1
    assert seen == 2 * len(M.window_cases(N))
    # repeated and shuffled keys: permuting keys permutes rows and changes no row
    rng = np.random.default_rng(3)
    keys = np.concatenate([np.arange(N), rng.integers(0, N, 40)]).astype(np.int32)
    tc = M.time_cur_for(t, keys, seed=9)
    kw = dict(top_k=8, rel_lo=-29, rel_hi=M.INT32_MAX)
    first = Raw(keys, tc, **kw)
    assert first.call(a) == 0
    first.check(M.detect_keys(P, t, keys, tc, **kw), "repeats")
    perm = rng.permutation(len(keys))
    second = Raw(keys[perm], tc[perm], **kw)
    assert second.call(a) == 0
    assert np.array_equal(second.key_pre, first.key_pre[perm]) and np.array_equal(second.d2, first.d2[perm])
    assert np.array_equal(second.n, first.n[perm])


def test_passes_and_cuts(pair, model):
    a, _ = pair
    stores, cases = model
    N = 2 * T + 1
    P, t = stores[N]
    _store(a, P, t)
    keys = M.draw_keys(N, N)
    tc = M.time_cur_for(t, keys)
    for kw in (dict(top_k=3), dict(top_k=8, first=1, count=T)):             # (the second: a range of one tile, one split)
        a.debugLoopDetectPass(0)
        plain = Raw(keys, tc, **kw)
        assert plain.call(a) == 0
        plain.check(M.detect_keys(P, t, keys, tc, **kw), "default plan")
        passes, scratch = a.debugLoopDetectLast()
        assert passes == 1 and 0 < scratch <= 64 << 20
        for q in (1, 5, B + 1):
            a.debugLoopDetectPass(q)
            cut = Raw(keys, tc, **kw)
            assert cut.call(a) == 0
            assert cut.image() == plain.image(), q
            passes, scratch_q = a.debugLoopDetectLast()
            assert passes == -(-N // q) and 0 < scratch_q <= scratch, (q, passes)
        a.debugLoopDetectPass(0)
        for s in (1, 2):                                                    # fewer store splits: the same bytes
            a.debugLoopDetectSplits(s)
            cut = Raw(keys, tc, **kw)
            assert cut.call(a) == 0
            assert cut.image() == plain.image(), s
            assert a.debugLoopDetectLast()[1] <= scratch
        a.debugLoopDetectSplits(0)
    assert a.lib.s2m_debug_loop_detect_pass(a.h, -1) == -1 and a.lib.s2m_debug_loop_detect_splits(a.h, -1) == -1


def test_the_detector_inside_loop_closure_rs(pair, model):
    a, b = pair
    stores, _ = model
    P, t = stores[T + 1]
    P, t = P.copy(), t.copy()
    N = len(t)
    P[N - 1] = P[4] + np.float32(0.25)                                      # the newest key is back at the cluster
    _store(a, P, t)
    _store(b, P, t)
    near = np.flatnonzero(M.d2_to(P, P[N - 1]) < np.float32(100.0))
    assert len(near) > 8
    times = [t[N - 1], t[N - 1] + 30.5, t[N - 1] + 30.0, t[near[0]] + 30.0, t[near[0]] + 30.5, 1e6, -1e6, t[N - 1] - 25.0]
    reported = own = empty = 0
    for tc in times:
        rs = b.performRSLoopClosure(float(tc))
        raw = Raw([N - 1], [tc], top_k=1)
        assert raw.call(a) == 0
        raw.check(M.detect_keys(P, t, [N - 1], [tc], top_k=1), f"tc {tc}")
        if rs.status == NONE:
            assert raw.n[0] == 0 or raw.key_pre[0, 0] == N - 1, tc
            own += int(raw.n[0] == 1)
            empty += int(raw.n[0] == 0)
        else:
            assert rs.status != CLOSED and rs.key_cur == N - 1 and raw.n[0] == 1 and rs.key_pre == raw.key_pre[0, 0], tc
            reported += 1
    print("reported", reported, "N-1 itself", own, "empty", empty)
    assert reported >= 2 and own >= 1


def test_read_only_and_never_busy_beside_a_pending_closure(pair, revisit):
    a, b = pair
    _, poses, times, _ = revisit
    n = len(times)
    prm = s2m.default_loop_params(**RS)
    _fill(a, revisit)
    _fill(b, revisit)
    keys = np.arange(n, dtype=np.int32)
    kw = dict(search_radius=15.0, time_diff_s=20.0, top_k=4)
    want = M.detect_keys(poses[:, :3], times, keys, None, **kw)
    assert want[2].max() == 4 and want[2].min() == 0
    assert a.loopAlignLaunch(n - 2, 0, -1, prm).status == PENDING
    assert b.loopAlignLaunch(n - 2, 0, -1, prm).status == PENDING
    raw = Raw(keys, None, **kw)
    assert raw.call(a) == 0                                                 # not S2M_ERR_BUSY
    raw.check(want, "beside a pending closure")
    ra, rb = a.loopCollect(), b.loopCollect()
    assert _bytes(ra) == _bytes(rb) and ra.status in (ACCEPTED, s2m.S2M_LOOP_REJECTED)
    sa, sb = a.performRSLoopClosure(float(n), prm), b.performRSLoopClosure(float(n), prm)
    assert _bytes(sa) == _bytes(sb) and sa.key_pre == raw.key_pre[n - 1, 0] == 0


def test_end_to_end_on_the_revisit(pair, revisit):
    a, b = pair
    _, poses, times, _ = revisit
    n = len(times)
    prm = s2m.default_loop_params(**RS)
    keys = list(range(n - 4, n))
    _fill(a, revisit)
    _fill(b, revisit)
    found = a.findSessionLoopsByDistance(15.0, 20.0, 4, keys)
    rows, d2rows, _ = M.detect_keys(poses[:, :3], times, keys, None, search_radius=15.0, time_diff_s=20.0, top_k=4)
    assert found == [(k, c, float(d)) for k, r, ds in zip(keys, rows, d2rows) for c, d in zip(r, ds)]
    assert len(found) > 4 and {k for k, _, _ in found} == set(keys)
    won = a.verifySessionLoopsByDistance(15.0, 20.0, 4, keys, base_key=-1, params=prm, rows_per_call=3)
    twin = []
    for k, r in zip(keys, rows):
        recs, best = b.loopVerify(k, r, -1, prm)
        if best >= 0:
            twin.append(recs[best])
    print("accepted", [(w.key_cur, w.key_pre, w.icp.fitness_score) for w in won])
    assert won and len(won) == len(twin)
    for g, w in zip(won, twin):
        assert _bytes(g) == _bytes(w), (g.key_cur, g.key_pre, w.key_pre)
    for k, r in zip(keys, rows):                                            # the container: a winner's key is closed on both
        if k in {w.key_cur for w in won}:
            assert a.loopVerify(k, r[:1], -1, prm)[0][0].status == CLOSED and b.loopVerify(k, r[:1], -1, prm)[0][0].status == CLOSED


def test_empty_cases_and_errors_on_a_live_handle(pair, model):
    a, _ = pair
    stores, _ = model
    a.kfReset()
    raw = Raw([0, 5, -3], top_k=2)                                          # an empty store holds no key to be outside of
    assert raw.call(a) == 0 and list(raw.n) == [0, 0, 0] and np.all(raw.key_pre == KEY_MARK) and np.all(raw.d2 == D2_MARK)
    N = 50
    P, t = M.make_store(N)
    _store(a, P, t)
    raw = Raw([1, 2])
    assert raw.call(a, m=0) == 0 and raw.untouched()
    assert raw.call(a, m=0, keys=False, key_pre=False, n=False) == 0
    for kw in (dict(first=N), dict(count=0), dict(first=7, count=0)):       # an empty searched range
        raw = Raw([1, 2, 49], top_k=3, **kw)
        assert raw.call(a) == 0 and list(raw.n) == [0, 0, 0] and np.all(raw.key_pre == KEY_MARK)
    raw = Raw([1, 2, 49], top_k=3, exclude_lo=0, exclude_hi=N)              # a searched set that the window empties
    assert raw.call(a) == 0 and list(raw.n) == [0, 0, 0]
    raw = Raw([1, 2])
    assert raw.call(a, prm=False) == 0                                    # NULL parameters: the defaults
    assert np.array_equal(raw.n, M.detect_keys(P, t, [1, 2])[2])
    bad = 0
    for name, n_stored, keys, m, fields, verdict in argument_table(N):
        if n_stored != N or keys is None:
            continue
        raw = Raw(keys if len(keys) else [0], **(fields or {}))
        rc = raw.call(a, m=len(keys) if m is None else m, prm=fields is not None)
        assert (rc == 0) == (verdict == 0), (name, rc)
        if rc != 0:
            assert rc == -1 and raw.untouched(), name
            bad += 1
    assert bad >= 15
    for off in (dict(keys=False), dict(key_pre=False), dict(n=False)):      # null arrays with m > 0
        raw = Raw([1, 2])
        assert raw.call(a, **off) == -1 and raw.untouched(), off
    for v in (float("nan"), float("inf"), -float("inf")):                   # a time_cur that is not finite
        raw = Raw([1, 2], [0.0, v])
        assert raw.call(a) == -1 and raw.untouched()
    assert a.lib.s2m_loop_detect_keys(None, None, None, 0, None, None, None, None) == -1
