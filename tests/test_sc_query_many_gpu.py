"""GPU tests of the many-query form of the ScanContext place query (s2m_sc_query_keys / _descriptors, s2m_sc_get_descriptors;
DESIGN.md section 20): every row against the single query with the same searched set and against the model
(tests/ref/sc_query_many_ref.py, on the oracle).  The bar everywhere is Q.same_hits: keys and shifts equal, dist equal as
uint64, yaw_diff_rad equal as uint32.  No tolerance is involved.  T and B are the kernel's tile and query block."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import sc_query_many_ref as M  # noqa: E402
import sc_query_ref as Q  # noqa: E402

from liorf_amd import s2m, synth  # noqa: E402
from test_scancontext_cpu import make_descriptors, revisit, sequence_340  # noqa: E402

pytestmark = pytest.mark.gpu
SK, FULL = s2m.S2M_SC_ALIGN_SECTOR_KEY, s2m.S2M_SC_ALIGN_FULL
BIG = 10000000.0
INT32_MAX = 2**31 - 1
T, B = s2m.sc_query_many_shape()


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def fill(g, descs):
    g.scReset()
    for d in descs:
        g.scAddDescriptor(d)
    assert g.scSize() == len(descs)


def check_rows(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert Q.same_hits(a, b), (what, i, a, b)


def raw_many(g, queries, fill_byte=0xAB, **kw):
    """The call through ctypes on buffers filled with a sentinel: (status, hits as bytes (m, top_k * 24), n_hits (m,))."""
    p = s2m.default_sc_query_many_params(**kw)
    q = np.asarray(queries)
    by_key = q.ndim == 1
    m = len(q)
    hits = np.full((max(m, 1), p.q.top_k * 24), fill_byte, np.uint8)
    n = np.full(max(m, 1), -7, np.int32)
    hp, npp = hits.ctypes.data_as(C.POINTER(s2m.ScHit)), n.ctypes.data_as(C.POINTER(C.c_int32))
    if by_key:
        k = np.ascontiguousarray(q, np.int32)
        rc = g.lib.s2m_sc_query_keys(g.h, k.ctypes.data_as(C.POINTER(C.c_int32)), m, C.byref(p), hp, npp)
    else:
        d = np.ascontiguousarray(q, np.float64)
        rc = g.lib.s2m_sc_query_descriptors(g.h, d.ctypes.data_as(C.POINTER(C.c_double)), m, C.byref(p), hp, npp)
    return rc, hits, n


def test_rows_equal_single_queries(gpu):
    """sequence_340, all 340 keys as queries: every row is scQueryKey's answer; on a 48-key store every row is also the model's."""
    descs = sequence_340()
    fill(gpu, descs)
    keys = np.arange(340)
    n_hits = 0
    for align in (SK, FULL):
        for k in (1, 3, 32):
            for max_dist in (0.3, BIG):
                kw = dict(top_k=k, align=align, max_dist=max_dist)
                got = gpu.scQueryKeys(keys, **kw)
                check_rows(got, [gpu.scQueryKey(int(q), **kw) for q in keys], ("340", kw))
                n_hits += sum(len(r) for r in got)
    assert n_hits > 340 * 32 and gpu.scSize() == 340
    small = descs[100:148]
    fill(gpu, small)
    for align in (SK, FULL):
        dists = {}
        for k, max_dist in ((1, 0.3), (3, BIG), (32, 0.3), (32, BIG)):
            kw = dict(top_k=k, align=align, max_dist=max_dist)
            check_rows(gpu.scQueryKeys(np.arange(48), **kw), M.query_many(small, list(range(48)), dists=dists, **kw), ("48, model", kw))


def test_edges_of_the_tiling(gpu):
    """Stores of 1, T-1, T, T+1, 2T+1 keys, m of 1, B-1, B, B+1 queries, keys descending and repeated, a range that starts and
    ends inside a tile: against the single query and the model."""
    all_descs = make_descriptors(2 * T + 1, seed=41)
    all_descs[2 * T] = revisit(all_descs[1], 13, 0.03, 4)
    for n in sorted({1, max(T - 1, 1), T, T + 1, 2 * T + 1}):
        descs = all_descs[:n] if n < 2 * T + 1 else all_descs
        if n < 2 * T + 1 and n > 1:
            descs = descs[:-1] + [revisit(descs[0], 7, 0.03, n)]
        fill(gpu, descs)
        dists = {SK: {}, FULL: {}}
        for m in sorted({1, max(B - 1, 1), B, B + 1}):
            keys = [(n - 1 - i) % n for i in range(m)]                       # descending, repeated once m > n
            for align in (SK, FULL):
                kw = dict(top_k=3, align=align, max_dist=BIG)
                got = gpu.scQueryKeys(keys, **kw)
                check_rows(got, [gpu.scQueryKey(q, **kw) for q in keys], ("single", n, m, align))
                check_rows(got, M.query_many(descs, keys, dists=dists[align], **kw), ("model", n, m, align))
        if n == 2 * T + 1:
            keys = list(range(n - 1, -1, -1)) + [0, 0, n - 1]
            for sub in (dict(first=1, count=T + 2), dict(first=T - 1, count=2), dict(first=T + 1, count=T - 1 if T > 1 else 1), dict(first=n, count=0),
                        dict(first=2, count=-1)):
                for align in (SK, FULL):
                    kw = dict(top_k=32, align=align, max_dist=BIG, **sub)
                    got = gpu.scQueryKeys(keys, **kw)
                    check_rows(got, M.query_many(descs, keys, dists=dists[align], **kw), ("range", sub, align))
                    check_rows(got, [gpu.scQueryKey(q, **kw) for q in keys], ("range, single", sub, align))


def test_windows(gpu):
    """Fixed and relative windows together; queries with an empty set between neighbours that have one (their rows untouched); a
    window over the whole range; a window outside it."""
    descs = make_descriptors(14, seed=14)
    descs[5] = revisit(descs[1], 9, 0.03, 2)
    descs[11] = revisit(descs[1], 40, 0.03, 3)
    fill(gpu, descs)
    keys = [0, 13, 6, 7, 1, 12, 5, 11, 3]
    dists = {SK: {}, FULL: {}}
    windows = [dict(exclude_lo=2, exclude_hi=5, rel_lo=-1, rel_hi=2), dict(exclude_lo=6, exclude_hi=8, rel_lo=-3, rel_hi=INT32_MAX),
               dict(rel_lo=-29, rel_hi=INT32_MAX), dict(rel_lo=-5, rel_hi=INT32_MAX), dict(first=3, count=8, rel_lo=-2**31, rel_hi=1),
               dict(rel_lo=-2**31, rel_hi=0), dict(rel_lo=0, rel_hi=1), dict(rel_lo=-1, rel_hi=0),
               dict(first=3, count=8, exclude_lo=4, exclude_hi=6, rel_lo=-2, rel_hi=3), dict(first=3, count=8, rel_lo=-6, rel_hi=1),
               dict(exclude_lo=0, exclude_hi=14), dict(rel_lo=-2**31, rel_hi=INT32_MAX), dict(first=2, count=6, exclude_lo=-9, exclude_hi=99),
               dict(exclude_lo=20, exclude_hi=30, rel_lo=40, rel_hi=50), dict(exclude_lo=-9, exclude_hi=0, rel_lo=-60, rel_hi=-20), dict(rel_lo=5, rel_hi=-5)]
    some_empty = 0
    for w in windows:
        for align in (SK, FULL):
            kw = dict(top_k=32, align=align, max_dist=BIG, **w)
            want = M.query_many(descs, keys, dists=dists[align], **kw)
            check_rows(gpu.scQueryKeys(keys, **kw), want, (w, align))
            rc, hits, n = raw_many(gpu, keys, **kw)
            assert rc == 0 and n.tolist() == [len(r) for r in want]
            for i, row in enumerate(want):                                   # behind the valid records the caller's bytes stay
                assert np.all(hits[i, 24 * len(row):] == 0xAB), (w, align, i)
                assert hits[i, :24 * len(row)].tobytes() == row.tobytes()
            lens = [len(M.searched_keys(14, q, **w)) for q in keys]
            some_empty += 0 in lens and max(lens) > 0
    assert some_empty >= 4
    # first=3, count=8, rel -6..1: key 3, 6, 7 have nothing before them in the range but keys behind; 13 sees 3..6
    assert M.searched_keys(14, 13, first=3, count=8, rel_lo=-6, rel_hi=1) == [3, 4, 5, 6]


def test_ties_and_empty_descriptors(gpu):
    """Exact duplicates across a tile edge rank by key; an all-zero stored descriptor and an all-zero query never hit; top_k = 32
    with fewer than 32 hits."""
    n = 4 * T + 3
    descs = make_descriptors(n, seed=9)
    for k in (T - 1, T, 2 * T, 3 * T + 1):
        descs[k] = descs[0].copy()
    z1, z2 = 2 * T + 1, 4 * T + 2                          # (never one of the copies)
    descs[z1] = np.zeros((20, 60))
    descs[z2] = np.zeros((20, 60))
    fill(gpu, descs)
    keys = list(range(n))
    for align in (SK, FULL):
        kw = dict(top_k=32, align=align, max_dist=BIG)
        dists = {}
        got = gpu.scQueryKeys(keys, **kw)
        check_rows(got, M.query_many(descs, keys, dists=dists, **kw), ("ties", align))
        dup = sorted({0, T - 1, T, 2 * T, 3 * T + 1})
        assert got[T]["key"][:len(dup)].tolist() == dup and len(set(got[T]["dist"][:len(dup)].tolist())) == 1
        assert len(got[z1]) == 0 and len(got[z2]) == 0                        # an all-zero query
        assert all(len(r) == min(n - 2, 32) for i, r in enumerate(got) if i not in (z1, z2))   # fewer than 32: never the empty ones
        ext = gpu.scQueryDescriptors([np.zeros((20, 60)), descs[0]], **kw)
        assert len(ext[0]) == 0 and Q.same_hits(ext[1], got[0])
        few = gpu.scQueryKeys(keys, top_k=32, align=align, max_dist=0.3)
        check_rows(few, M.query_many(descs, keys, dists=dists, top_k=32, align=align, max_dist=0.3), ("ties under 0.3", align))
        assert few[0]["key"][:len(dup)].tolist() == dup and len(few[0]) < n - 2


def test_passes(gpu):
    """s2m_debug_sc_query_many_pass at 1, 3 and the default: identical bytes in hits and n_hits."""
    descs = sequence_340()[:23]
    fill(gpu, descs)
    keys = [22, 0, 5, 5, 17, 3, 21, 9, 10, 11, 1]
    ext = np.stack([revisit(descs[k], 11 + k, 0.04, k) for k in (2, 9, 14, 20, 20, 6, 7)])
    try:
        for queries, kw in ((keys, dict(rel_lo=-2, rel_hi=3)), (ext, {})):
            for align in (SK, FULL):
                out = {}
                for per_pass in (1, 3, 0):
                    gpu.scQueryManyPass(per_pass)
                    rc, hits, n = raw_many(gpu, queries, top_k=5, align=align, max_dist=BIG, **kw)
                    assert rc == 0
                    out[per_pass] = (hits.tobytes(), n.tobytes(), gpu.scQueryManyLast()[0])
                assert out[1][:2] == out[3][:2] == out[0][:2]
                m = len(queries)
                assert (out[1][2], out[3][2], out[0][2]) == (m, (m + 2) // 3, 1)
                assert gpu.scQueryManyLast()[1] <= 64 << 20
        with pytest.raises(s2m.S2MError):
            gpu.scQueryManyPass(-1)
    finally:
        gpu.scQueryManyPass(0)


def test_external_descriptors(gpu):
    descs = sequence_340()[:40]
    fill(gpu, descs)
    ext = [revisit(descs[k], 3 * k + 1, 0.05, k) for k in (0, 7, 19, 33, 39)] + [descs[12], make_descriptors(1, seed=77)[0]]
    for align in (SK, FULL):
        for kw in (dict(top_k=4, align=align), dict(top_k=32, align=align, max_dist=BIG, first=3, count=30, exclude_lo=10, exclude_hi=14)):
            check_rows(gpu.scQueryDescriptors(ext, **kw), [gpu.scQueryDescriptor(d, **kw) for d in ext], ("ext", kw))
    # what went in comes out, as 64-bit patterns
    out = gpu.scGetDescriptors()
    assert out.shape == (40, 20, 60) and np.array_equal(out.view(np.uint64), np.stack(descs).view(np.uint64))
    assert np.array_equal(gpu.scGetDescriptors(7, 5).view(np.uint64), np.stack(descs[7:12]).view(np.uint64))
    assert gpu.scGetDescriptors(40, 0).shape == (0, 20, 60)
    for first, count in ((-1, 1), (0, 41), (40, 1), (0, -1)):
        with pytest.raises(s2m.S2MError):
            gpu.scGetDescriptors(first, count)
    # one handle's descriptors queried in a second handle: the rows of scQueryKeys in the first
    other = s2m.MapOptimizationS2M()
    fill(other, descs)
    kw = dict(top_k=6, align=FULL, max_dist=BIG)
    check_rows(other.scQueryDescriptors(out[5:25], **kw), gpu.scQueryKeys(np.arange(5, 25), **kw), "carried over")
    # a relative window needs a stored key
    for w in (dict(rel_lo=0, rel_hi=1), dict(rel_lo=-29, rel_hi=INT32_MAX)):
        with pytest.raises(s2m.S2MError):
            other.scQueryDescriptors(ext, **w)
        rc, hits, n = raw_many(other, np.stack(ext), **w)
        assert rc == -1 and np.all(hits == 0xAB)
    assert len(other.scQueryDescriptors(ext, rel_lo=4, rel_hi=4)) == len(ext)
    # the descriptor s2m_sc_add_scan stores is the one s2m_make_scancontext returns
    scene = synth.make_scene(seed=21, half=35.0, n_boxes=14)
    clouds = [synth.to_xyzi(synth.make_scan(scene, np.array([0, 0, 0.2 * k, 2.0 * k, 0.0, 0.0]), "velodyne64", 6000, seed=50 + k)) for k in range(3)]
    other.scReset()
    for c in clouds:
        other.makeAndSaveScancontextAndKeys(c)
    want = np.stack([other.makeScancontext(c)[0] for c in clouds])
    assert np.array_equal(other.scGetDescriptors().view(np.uint64), want.view(np.uint64)) and other.scSize() == 3
    other.close()


def test_errors_and_empty_cases(gpu):
    descs = make_descriptors(6, seed=3)
    fill(gpu, descs)
    lib = gpu.lib
    p = s2m.default_sc_query_many_params(top_k=2)
    keys = (C.c_int32 * 3)(0, 5, 2)
    hits, n = (s2m.ScHit * 6)(), (C.c_int32 * 3)(9, 9, 9)
    assert lib.s2m_sc_query_keys(gpu.h, keys, 3, C.byref(p), hits, n) == 0 and all(1 <= x <= 2 for x in n)
    assert lib.s2m_sc_query_keys(gpu.h, keys, 3, None, hits, n) == 0 and [hits[0].key, hits[1].key, hits[2].key] == [0, 5, 2]   # p == NULL: top_k 1
    assert lib.s2m_sc_query_keys(gpu.h, None, 0, C.byref(p), None, None) == 0                    # m == 0 writes nothing
    assert lib.s2m_sc_query_descriptors(gpu.h, None, 0, None, None, None) == 0
    assert lib.s2m_sc_query_keys(gpu.h, keys, -1, C.byref(p), hits, n) == -1
    assert lib.s2m_sc_query_keys(gpu.h, None, 3, C.byref(p), hits, n) == -1
    assert lib.s2m_sc_query_keys(gpu.h, keys, 3, C.byref(p), None, n) == -1
    assert lib.s2m_sc_query_keys(gpu.h, keys, 3, C.byref(p), hits, None) == -1
    assert lib.s2m_sc_query_descriptors(gpu.h, None, 3, C.byref(p), hits, n) == -1
    for bad in ([0, 6, 1], [-1], [2, 3, INT32_MAX]):
        with pytest.raises(s2m.S2MError):
            gpu.scQueryKeys(bad)
    for bad in (dict(top_k=0), dict(top_k=33), dict(align=2), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(first=7), dict(count=7)):
        with pytest.raises(s2m.S2MError):
            gpu.scQueryKeys([0, 1], **bad)
        with pytest.raises(s2m.S2MError):
            gpu.scQueryDescriptors(descs[:2], **bad)
    assert [len(r) for r in gpu.scQueryKeys([0, 1, 2], count=0, max_dist=BIG)] == [0, 0, 0]
    assert gpu.scQueryKeys([]) == [] and gpu.scSize() == 6
    # an empty store: no hits from descriptors; any stored key is outside it
    gpu.scReset()
    assert [len(r) for r in gpu.scQueryDescriptors(descs[:3], top_k=32, max_dist=BIG)] == [0, 0, 0]
    with pytest.raises(s2m.S2MError):
        gpu.scQueryKeys([0])


def test_many_queries_leave_the_detector_alone():
    """The first 60 steps of the sequence_340 add-and-detect loop on two handles; one issues many-queries before every detection.
    Every (loop_id, yaw, ScMatch) and scSize() is equal."""
    descs = sequence_340()[:60]
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    for i, d in enumerate(descs):
        for g in (a, b):
            g.scAddDescriptor(d)
        a.scQueryKeys(np.arange(i, -1, -1), top_k=3, align=FULL if i % 2 else SK, **M.DETECTOR_WINDOW)
        a.scQueryDescriptors(descs[(7 * i) % 60:(7 * i) % 60 + 3], top_k=32, align=SK if i % 2 else FULL, max_dist=BIG)
        if i % 5 == 0:
            a.scGetDescriptors(0, i + 1)
        ra, rb = a.detectLoopClosureID(), b.detectLoopClosureID()
        assert ra[:2] == rb[:2] and C.string_at(C.addressof(ra[2]), C.sizeof(ra[2])) == C.string_at(C.addressof(rb[2]), C.sizeof(rb[2])), i
        assert a.scSize() == b.scSize() == i + 1
    a.close(); b.close()


def test_ring_key_case_on_the_device(gpu):
    """The detector finds nothing for key 96; the session-wide query names (96, 60) at shift 23, and so does findSessionLoops."""
    descs = Q.ring_key_case()
    fill(gpu, descs)
    lid, _, m = gpu.detectLoopClosureID()
    assert lid == -1 and 60 not in list(m.cand_idx)
    rows = gpu.scQueryKeys(np.arange(97), top_k=4, align=FULL, **M.DETECTOR_WINDOW)
    assert len(rows[96]) == 1 and rows[96][0]["key"] == 60 and rows[96][0]["shift"] == 23
    assert all(len(rows[k]) == 0 for k in range(30)) and all(h["key"] <= cur - 30 for cur, r in enumerate(rows) for h in r)
    check_rows([rows[96]], [gpu.scQueryKey(96, exclude_lo=67, exclude_hi=97, top_k=4, align=FULL)], "key 96")
    loops = gpu.findSessionLoops(gap=30, max_dist=0.3, top_k=4, align=FULL)
    mine = [x for x in loops if x[0] == 96]
    assert len(mine) == 1 and mine[0][:2] == (96, 60) and mine[0][2] == rows[96][0]["dist"] and mine[0][3] == float(Q.yaw_of_shift(23))
    assert [(c, p) for c, p, _, _ in loops] == [(cur, int(h["key"])) for cur, r in enumerate(rows) for h in r]
