"""GPU tests of the ring-key prefilter of the ScanContext place query (s2m_sc_ring_neighbours_* / s2m_sc_query_*_ring;
DESIGN.md section 22): the neighbour lists against the model (tests/ref/sc_ring_ref.py), the rows against the model and
against the calls that exist already.  Every comparison is on bytes: d2 as uint32 (R.same_neighbours), dist as uint64
(Q.same_hits).  No tolerance is involved.  T, B and W are the selection kernel's tile, query block and buffer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import sc_query_many_ref as M  # noqa: E402
import sc_query_ref as Q  # noqa: E402
import sc_ring_ref as R  # noqa: E402

from liorf_amd import s2m  # noqa: E402
from test_scancontext_cpu import make_descriptors, revisit, sequence_340  # noqa: E402

pytestmark = pytest.mark.gpu
SK, FULL = s2m.S2M_SC_ALIGN_SECTOR_KEY, s2m.S2M_SC_ALIGN_FULL
BIG = 10000000.0
INT32_MAX = 2**31 - 1
T, B, W = s2m.sc_ring_shape()
CANDS = (1, 3, 64, 256)
FILL = 0xAB


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    g.ring_store = None
    yield g
    g.close()


@pytest.fixture(scope="module")
def big():
    """2T + 2 random descriptors and their fp32 ring keys: ranges of one key fewer / exactly / one key more than one and two tiles."""
    descs = make_descriptors(2 * T + 2, seed=21)
    return descs, R.ring_keys(descs)


def fill(g, descs, tag=None):
    """The store holds `descs`; a tagged store that is there already is kept."""
    if tag is not None and g.ring_store == tag:
        return
    g.scReset()
    for d in descs:
        g.scAddDescriptor(d)
    assert g.scSize() == len(descs)
    g.ring_store = tag


def check_nb(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert R.same_neighbours(a, b), (what, i, a, b)


def check_rows(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert Q.same_hits(a, b), (what, i, a, b)


def raw_ring(g, queries, both, **kw):
    """The call through ctypes on buffers filled with FILL: (status, rows as bytes (m, width * record), counts (m,), record bytes)."""
    p = s2m.default_sc_ring_params(**kw)
    q = np.asarray(queries)
    by_key = q.ndim == 1
    m = len(q)
    rec, width = (24, p.m.q.top_k) if both else (8, p.n_candidates)
    rows = np.full((max(m, 1), max(width, 1) * rec), FILL, np.uint8)
    n = np.full(max(m, 1), -7, np.int32)
    rp = rows.ctypes.data_as(C.POINTER(s2m.ScHit if both else s2m.ScRingNeighbour))
    npp = n.ctypes.data_as(C.POINTER(C.c_int32))
    if by_key:
        k = np.ascontiguousarray(q, np.int32)
        fn = g.lib.s2m_sc_query_keys_ring if both else g.lib.s2m_sc_ring_neighbours_keys
        rc = fn(g.h, k.ctypes.data_as(C.POINTER(C.c_int32)), m, C.byref(p), rp, npp)
    else:
        d = np.ascontiguousarray(q, np.float64)
        fn = g.lib.s2m_sc_query_descriptors_ring if both else g.lib.s2m_sc_ring_neighbours_descriptors
        rc = fn(g.h, d.ctypes.data_as(C.POINTER(C.c_double)), m, C.byref(p), rp, npp)
    return rc, rows, n, rec


# ---- stage one against the model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CANDS)
def test_neighbours_equal_the_model_at_the_tile_edges(gpu, big, c):
    """Ranges of 1, 2, C-1, C, C+1 keys and of one key fewer / exactly / one more than one and two tiles, from key 1 on; m of 1,
    B-1 and B+1 with repeated and unordered keys; two external descriptors, one of them a stored one."""
    descs, keys32 = big
    fill(gpu, descs, "big")
    n = len(descs)
    key_lists = [[n - 1], [0, n - 1, 7, 7, n // 2, 2, 300][:B - 1], [0, n - 1, 7, 7, n // 2, 2, 300, 5, 5][:B + 1]]
    ext = [descs[10], make_descriptors(1, seed=77)[0]]
    counts = sorted({x for x in (1, 2, c - 1, c, c + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1) if 1 <= x <= n - 1})
    for count in counts:
        kw = dict(first=1, count=count)
        for keys in key_lists:
            check_nb(gpu.scRingNeighboursKeys(keys, n_candidates=c, **kw), R.neighbours_many(descs, keys, c, keys32=keys32, **kw), (c, count, keys))
        got = gpu.scRingNeighboursDescriptors(ext, n_candidates=c, **kw)
        check_nb(got, R.neighbours_many(descs, ext, c, keys32=keys32, **kw), (c, count, "ext"))
        check_nb(got[:1], gpu.scRingNeighboursKeys([10], n_candidates=c, **kw), (c, count, "a descriptor query is its key's query"))


def test_neighbours_across_the_stores_first_growth(gpu, big):
    descs, keys32 = big
    fill(gpu, descs[:255])
    for n in (255, 256, 257):
        if n > 255:
            gpu.scAddDescriptor(descs[n - 1])
        assert gpu.scSize() == n
        for c in (3, 256):
            keys = [n - 1, 0, 128]
            check_nb(gpu.scRingNeighboursKeys(keys, n_candidates=c), R.neighbours_many(descs[:n], keys, c, keys32=keys32[:n]), (n, c))
    gpu.ring_store = None


def test_neighbours_when_every_key_beats_the_threshold(gpu):
    """Constant images whose value falls with the key: seen from the last key d2 falls with every key, so every key is appended
    and the buffer of W words is pruned over and over; seen from key 0 it rises and nothing is appended after the first C."""
    n = 2 * T + 1
    descs = [np.full((20, 60), 0.01 * (n - k) + 1.0) for k in range(n)]
    keys32 = R.ring_keys(descs)
    assert np.all(np.diff(R.d2_all(keys32[n - 1], keys32)) < 0) and n > W
    fill(gpu, descs)
    gpu.ring_store = None
    for c in CANDS:
        keys = [n - 1, 0, n // 2, n - 1, 1]
        check_nb(gpu.scRingNeighboursKeys(keys, n_candidates=c, rel_lo=0, rel_hi=1), R.neighbours_many(descs, keys, c, keys32=keys32, rel_lo=0, rel_hi=1), c)


# ---- ties and non-finite keys ------------------------------------------------------------------------------------------------

def test_ties_in_the_ring_key_case(gpu):
    """Seven keys tie the nearest d2 (3 .. 8 and 60): the cut falls inside the group for C = 3 .. 6, at its end for 7, past it for 8."""
    descs = Q.ring_key_case()
    keys32 = R.ring_keys(descs)
    fill(gpu, descs, "ring_key_case")
    for c in range(3, 9):
        got = gpu.scRingNeighboursKeys([96, 60, 96], n_candidates=c, **M.DETECTOR_WINDOW)
        check_nb(got, R.neighbours_many(descs, [96, 60, 96], c, keys32=keys32, **M.DETECTOR_WINDOW), c)
        assert got[0]["key"].tolist() == [3, 4, 5, 6, 7, 8, 60, 42][:c]
        for align in (SK, FULL):
            kw = dict(top_k=4, align=align, **M.DETECTOR_WINDOW)
            rows = gpu.scQueryKeysRing([96, 50], n_candidates=c, **kw)
            check_rows(rows, R.query_many_ring(descs, [96, 50], c, keys32=keys32, **kw), (c, align))
            assert len(rows[0]) == (1 if c >= 7 else 0)
            if c >= 7:
                assert rows[0][0]["key"] == 60 and rows[0][0]["shift"] == 23


def test_all_zero_store(gpu):
    """Every d2 is 0: the lowest keys win; an empty descriptor has no comparable sector, so nothing is a hit."""
    n = 70
    descs = [np.zeros((20, 60)) for _ in range(n)]
    fill(gpu, descs)
    gpu.ring_store = None
    for c in (3, 64, 256):
        got = gpu.scRingNeighboursKeys([69, 0], n_candidates=c)
        for row in got:
            assert row["key"].tolist() == list(range(min(c, n))) and not np.any(row["d2"].view(np.uint32))
        assert gpu.scRingNeighboursKeys([40], n_candidates=c, first=10, rel_lo=-5, rel_hi=6)[0]["key"].tolist() == [k for k in range(10, n) if not 35 <= k < 46][:c]
        for align in (SK, FULL):
            assert [len(r) for r in gpu.scQueryKeysRing([69, 0], n_candidates=c, top_k=8, align=align, max_dist=BIG)] == [0, 0]


def test_non_finite_ring_keys(gpu):
    descs = make_descriptors(40, seed=13)
    descs[13] = descs[13].copy()
    descs[13][4, 9] = np.nan
    keys32 = R.ring_keys(descs)
    fill(gpu, descs)
    gpu.ring_store = None
    with_inf = descs[2].copy()
    with_inf[7, 3] = np.inf
    for c in (3, 256):
        assert [len(r) for r in gpu.scRingNeighboursDescriptors([with_inf], n_candidates=c)] == [0]
        assert [len(r) for r in gpu.scQueryDescriptorsRing([with_inf], n_candidates=c, top_k=8, max_dist=BIG)] == [0]
        keys = [0, 13, 39, 12]
        got = gpu.scRingNeighboursKeys(keys, n_candidates=c)
        check_nb(got, R.neighbours_many(descs, keys, c, keys32=keys32), c)
        assert len(got[1]) == 0 and all(13 not in r["key"].tolist() for r in got)
        assert [len(r) for r in got] == [min(c, 39), 0, min(c, 39), min(c, 39)]
        assert len(gpu.scQueryKeysRing([13], n_candidates=c, top_k=8, max_dist=BIG)[0]) == 0


# ---- both stages against the model --------------------------------------------------------------------------------------------

def small_store():
    """48 descriptors; keys 40 .. 47 revisit keys 0 .. 7 rotated, so that rows hold hits under 0.3."""
    descs = make_descriptors(48, seed=9)
    for k in range(40, 48):
        descs[k] = revisit(descs[k - 40], (7 * k) % 60, 0.05, k)
    return descs


WINDOWS = [dict(), dict(first=3, count=40, exclude_lo=10, exclude_hi=14), dict(rel_lo=-3, rel_hi=4),
           dict(first=2, exclude_lo=20, exclude_hi=25, rel_lo=-6, rel_hi=2), dict(M.DETECTOR_WINDOW), dict(first=48), dict(first=5, count=2)]


@pytest.mark.parametrize("align", [SK, FULL])
def test_rows_equal_the_model(gpu, align):
    """Fixed, relative and combined windows, the detector's, an empty set and a set smaller than n_candidates."""
    descs = small_store()
    keys32 = R.ring_keys(descs)
    fill(gpu, descs, "small")
    keys = [47, 40, 3, 31, 47, 44]
    ext = [revisit(descs[20], 11, 0.05, 3), descs[45]]
    n_hits = 0
    for window in WINDOWS:
        for c, top_k, max_dist in ((3, 1, 0.3), (10, 4, BIG)):
            kw = dict(top_k=top_k, align=align, max_dist=max_dist, **window)
            got = gpu.scQueryKeysRing(keys, n_candidates=c, **kw)
            check_rows(got, R.query_many_ring(descs, keys, c, keys32=keys32, **kw), ("keys", c, kw))
            n_hits += sum(len(r) for r in got)
            if "rel_lo" not in window:
                check_rows(gpu.scQueryDescriptorsRing(ext, n_candidates=c, **kw), R.query_many_ring(descs, ext, c, keys32=keys32, **kw), ("ext", c, kw))
    assert n_hits > 40
    assert [len(r) for r in gpu.scQueryKeysRing(keys, n_candidates=10, first=48)] == [0] * len(keys)
    assert [len(r) for r in gpu.scRingNeighboursKeys(keys, n_candidates=10, first=5, count=2)] == [2] * len(keys)


def test_full_alignment_on_short_rows(gpu):
    """n_candidates = 10 and windows that leave |R_i| = 1, 2, 4, 5: the last triple of a row holds one or two candidates, and a
    row ends exactly on a triple plus one.  Each row is s2m_sc_query_keys' / _descriptors' row for the same window as bytes, and
    the model's."""
    descs = small_store()
    keys32 = R.ring_keys(descs)
    fill(gpu, descs, "small")
    keys = [47, 6, 3, 31, 40]
    ext = [revisit(descs[20], 11, 0.05, 3)]
    for count in (1, 2, 4, 5):
        kw = dict(top_k=5, align=FULL, max_dist=BIG, first=5, count=count)
        for what, got, exhaustive, want in (
                ("keys", gpu.scQueryKeysRing(keys, n_candidates=10, **kw), gpu.scQueryKeys(keys, **kw), R.query_many_ring(descs, keys, 10, keys32=keys32, **kw)),
                ("ext", gpu.scQueryDescriptorsRing(ext, n_candidates=10, **kw), gpu.scQueryDescriptors(ext, **kw), R.query_many_ring(descs, ext, 10, keys32=keys32, **kw))):
            assert [len(r) for r in got] == [count] * len(got), (what, count)
            assert [r.tobytes() for r in got] == [r.tobytes() for r in exhaustive], (what, count, got, exhaustive)
            check_rows(got, want, (what, count))


# ---- equality with the calls that exist ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [SK, FULL])
def test_enough_candidates_give_the_exhaustive_rows(gpu, big, align):
    """n_candidates >= |S_i|: every row is s2m_sc_query_keys' / _descriptors' row, as bytes; at sector-key alignment every hit is
    s2m_sc_distance's (dist, shift)."""
    descs, _ = big
    for n in (48, 256):
        fill(gpu, descs[:n], ("big", n))
        keys = np.arange(n)[::-1].copy()
        ext = [descs[300], descs[7]]
        for window in (dict(), dict(M.DETECTOR_WINDOW), dict(first=3, count=n - 5, exclude_lo=10, exclude_hi=14, rel_lo=-2, rel_hi=9)):
            kw = dict(top_k=5, align=align, max_dist=BIG if n == 48 else 0.9, **window)
            got = gpu.scQueryKeysRing(keys, n_candidates=256, **kw)
            check_rows(got, gpu.scQueryKeys(keys, **kw), (n, kw))
            assert sum(len(r) for r in got) > n
            if "rel_lo" not in window:
                check_rows(gpu.scQueryDescriptorsRing(ext, n_candidates=256, **kw), gpu.scQueryDescriptors(ext, **kw), (n, "ext", kw))
            if align == SK and n == 48:
                for q, row in zip(keys, got):
                    d, s = gpu.distanceBtnScanContext(int(q), row["key"])
                    assert np.array_equal(d.view(np.uint64), row["dist"].view(np.uint64)) and np.array_equal(s, row["shift"])


def test_the_detectors_candidates_are_the_neighbours(gpu):
    """66 keys of sequence_340: key 65 revisits key 15.  The first detection searches [0, 36): its candidates are the three
    neighbours of key 65 there, and its match is the top-1 sector-key row of the ring query over the same set."""
    descs = sequence_340()[:66]
    n = len(descs)
    keys32 = R.ring_keys(descs)
    kw = dict(first=0, count=n - 30)
    model = R.query_many_ring(descs, [n - 1], 3, top_k=3, align=Q.ALIGN_SECTOR_KEY, max_dist=BIG, keys32=keys32, **kw)[0]
    assert len(model) == 3 and len(set(model["dist"].tolist())) == 3 and model[0]["key"] == 15 and model[0]["dist"] < 0.3
    fill(gpu, descs)
    gpu.ring_store = None
    nb = gpu.scRingNeighboursKeys([n - 1], n_candidates=3, **kw)[0]
    row = gpu.scQueryKeysRing([n - 1], n_candidates=3, top_k=1, align=SK, **kw)[0]
    lid, yaw, m = gpu.detectLoopClosureID()
    assert list(m.cand_idx) == nb["key"].tolist()
    assert np.array_equal(np.array(list(m.cand_d2), np.float32).view(np.uint32), nb["d2"].view(np.uint32))
    assert lid == 15 and len(row) == 1
    assert (m.nn_idx, m.nn_align) == (int(row[0]["key"]), int(row[0]["shift"]))
    assert np.float64(m.min_dist).view(np.uint64) == row["dist"].view(np.uint64)[0]
    assert np.float32(yaw).view(np.uint32) == row["yaw_diff_rad"].view(np.uint32)[0]


# ---- passes, read-only, the sentinel -------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_the_passes(gpu, big):
    descs, _ = big
    fill(gpu, descs, "big")
    keys = np.arange(0, len(descs), 13)
    ext = descs[100:109]
    kw = dict(n_candidates=256, top_k=8, align=SK, max_dist=BIG, first=1)
    want = None
    try:
        for per_pass in (0, 1, 7):
            gpu.scRingPass(per_pass)
            got = (gpu.scRingNeighboursKeys(keys, **kw), gpu.scQueryKeysRing(keys, **kw), gpu.scRingNeighboursDescriptors(ext, **kw),
                   gpu.scQueryDescriptorsRing(ext, **kw))
            passes, scratch = gpu.scRingLast()
            assert passes == (1 if per_pass == 0 else -(-len(ext) // per_pass)) and 0 < scratch <= 64 << 20
            if want is None:
                want = got
            check_nb(got[0], want[0], per_pass); check_rows(got[1], want[1], per_pass)
            check_nb(got[2], want[2], per_pass); check_rows(got[3], want[3], per_pass)
        gpu.scQueryKeysRing(keys, **kw)
        assert gpu.scRingLast()[0] == -(-len(keys) // 7) > 1
        with pytest.raises(s2m.S2MError):
            gpu.scRingPass(-1)
    finally:
        gpu.scRingPass(0)


def test_ring_queries_leave_the_detector_alone():
    """The first 45 steps of the sequence_340 add-and-detect loop on two handles; one issues ring queries before every detection.
    Every (loop_id, yaw, ScMatch) and scSize() is equal."""
    descs = sequence_340()[:45]
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    for i, d in enumerate(descs):
        for g in (a, b):
            g.scAddDescriptor(d)
        a.scQueryKeysRing(np.arange(i, -1, -1), n_candidates=3 + i % 5, top_k=3, align=FULL if i % 2 else SK, **M.DETECTOR_WINDOW)
        a.scRingNeighboursDescriptors(descs[(7 * i) % 40:(7 * i) % 40 + 3], n_candidates=256)
        a.scQueryDescriptorsRing(descs[:2], n_candidates=10, top_k=32, align=SK if i % 2 else FULL, max_dist=BIG)
        ra, rb = a.detectLoopClosureID(), b.detectLoopClosureID()
        assert ra[:2] == rb[:2] and C.string_at(C.addressof(ra[2]), C.sizeof(ra[2])) == C.string_at(C.addressof(rb[2]), C.sizeof(rb[2])), i
        assert a.scSize() == b.scSize() == i + 1
    a.close(); b.close()


def test_records_behind_the_counts_stay_the_callers(gpu):
    descs = small_store()
    fill(gpu, descs, "small")
    for both in (False, True):
        for queries in ([47, 3, 20], np.stack([descs[45], descs[1]])):
            rc, rows, n, rec = raw_ring(gpu, queries, both, n_candidates=10, top_k=6, first=4, count=7, max_dist=0.3)
            assert rc == s2m.S2M_OK and np.all(n >= 0) and np.all(n <= 7)
            for i in range(len(queries)):
                assert np.all(rows[i, n[i] * rec:] == FILL), (both, i)
                assert n[i] == 0 or not np.all(rows[i, :n[i] * rec] == FILL)
            if not both:
                assert n.tolist() == [7] * len(queries)


# ---- the Python mirror, errors, empty cases --------------------------------------------------------------------------------------

def test_find_session_loops_with_the_prefilter(gpu):
    descs = Q.ring_key_case()
    fill(gpu, descs, "ring_key_case")
    pairs = lambda loops: [(c, p) for c, p, _, _ in loops]
    assert (96, 60) in pairs(gpu.findSessionLoops(ring_candidates=8, top_k=4, align=FULL))
    assert (96, 60) not in pairs(gpu.findSessionLoops(ring_candidates=3, top_k=4, align=FULL))
    rows = gpu.scQueryKeys(np.arange(97), top_k=4, align=FULL, max_dist=0.3, rel_lo=-29, rel_hi=INT32_MAX)
    want = [(cur, int(h["key"]), float(h["dist"]), float(h["yaw_diff_rad"])) for cur, row in enumerate(rows) for h in row]
    assert gpu.findSessionLoops(top_k=4, align=FULL, ring_candidates=None) == want == gpu.findSessionLoops(30, 0.3, 4, FULL) and (96, 60) in pairs(want)
    assert set(gpu.findSessionLoops(ring_candidates=256, top_k=4, align=FULL)) == set(want)


def test_errors_leave_the_outputs_untouched(gpu):
    descs = small_store()
    fill(gpu, descs, "small")
    ext = np.stack([descs[1], descs[2]])
    bad = [([0, 1], dict(n_candidates=0)), ([0, 1], dict(n_candidates=257)), ([0, 1], dict(reserved=1)), ([0, 48], dict()), ([-1], dict()),
           ([0, 1], dict(top_k=33)), ([0], dict(align=2)), ([0], dict(max_dist=0.0)), ([0], dict(first=49)), (ext, dict(rel_lo=0, rel_hi=1))]
    for both in (False, True):
        for queries, kw in bad:
            rc, rows, n, _ = raw_ring(gpu, queries, both, **kw)
            assert rc == -1 and np.all(rows == FILL) and np.all(n == -7), (both, kw)
    p = s2m.default_sc_ring_params()
    k = np.zeros(2, np.int32)
    kp = k.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros(6, s2m.SC_RING_NEIGHBOUR_DTYPE)
    n = np.zeros(2, np.int32)
    assert gpu.lib.s2m_sc_ring_neighbours_keys(gpu.h, kp, 2, C.byref(p), None, n.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert gpu.lib.s2m_sc_ring_neighbours_keys(gpu.h, kp, 2, C.byref(p), out.ctypes.data_as(C.POINTER(s2m.ScRingNeighbour)), None) == -1
    assert gpu.lib.s2m_sc_query_keys_ring(gpu.h, None, 2, C.byref(p), None, None) == -1
    # m == 0 writes nothing, whatever the pointers; p == NULL means the defaults
    assert gpu.lib.s2m_sc_query_keys_ring(gpu.h, None, 0, None, None, None) == s2m.S2M_OK
    rc, rows, counts, _ = raw_ring(gpu, np.zeros(0, np.int32), False)
    assert rc == s2m.S2M_OK and np.all(rows == FILL) and np.all(counts == -7)
    assert gpu.lib.s2m_sc_ring_neighbours_keys(gpu.h, kp, 2, None, out.ctypes.data_as(C.POINTER(s2m.ScRingNeighbour)), n.ctypes.data_as(C.POINTER(C.c_int32))) == s2m.S2M_OK
    assert n.tolist() == [3, 3] and gpu.scSize() == 48
    # an empty store: nothing from descriptors; any stored key is outside it
    gpu.scReset()
    gpu.ring_store = None
    assert [len(r) for r in gpu.scRingNeighboursDescriptors(ext, n_candidates=256)] == [0, 0]
    assert [len(r) for r in gpu.scQueryDescriptorsRing(ext, n_candidates=256, top_k=32, max_dist=BIG)] == [0, 0]
    with pytest.raises(s2m.S2MError):
        gpu.scQueryKeysRing([0])
