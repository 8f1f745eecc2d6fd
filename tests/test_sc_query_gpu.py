"""GPU tests of the ScanContext place query (s2m_sc_query_*) against the model of its semantics
(tests/ref/sc_query_ref.py, on the oracle).  The bar everywhere: keys and shifts equal, dist equal as uint64, yaw_diff_rad
equal as uint32 (Q.same_hits).  No tolerance is involved."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import sc_query_ref as Q  # noqa: E402

from liorf_amd import s2m, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_scancontext_cpu import make_descriptors, revisit, sequence_340  # noqa: E402

pytestmark = pytest.mark.gpu
SK, FULL = s2m.S2M_SC_ALIGN_SECTOR_KEY, s2m.S2M_SC_ALIGN_FULL
BIG = 10000000.0


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def fill(g, descs):
    g.sc_query_store = None
    g.scReset()
    for d in descs:
        g.scAddDescriptor(d)
    assert g.scSize() == len(descs)


def check(got, want, what):
    assert Q.same_hits(got, want), (what, got, want)


def test_base_store(gpu):
    """sequence_340 (crosses the store's first growth at 256): stored keys and an external descriptor, the full range, K in
    1, 3, 32, both alignments; a stored sector-key query also equals s2m_sc_distance hit by hit."""
    descs = sequence_340()
    fill(gpu, descs)
    keys = range(340)
    ext = revisit(descs[17], 41, 0.05, 1)
    n_hits = 0
    for align in (SK, FULL):
        for q in (0, 255, 256, 339, "ext"):
            qd = ext if q == "ext" else descs[q]
            dists = Q.all_distances(descs, qd, align)
            for k in (1, 3, 32):
                for max_dist in (0.3, BIG):
                    want = Q.rank(dists, keys, k, max_dist)
                    kw = dict(top_k=k, align=align, max_dist=max_dist)
                    got = gpu.scQueryDescriptor(qd, **kw) if q == "ext" else gpu.scQueryKey(q, **kw)
                    check(got, want, (align, q, k, max_dist))
                    if q != "ext":
                        check(gpu.scQueryDescriptor(qd, **kw), want, ("as descriptor", align, q, k, max_dist))
                        if align == SK:
                            for h in got:
                                d, s = gpu.distanceBtnScanContext(q, [int(h["key"])])
                                assert d.view(np.uint64)[0] == h["dist"].view(np.uint64) and s[0] == h["shift"]
                    n_hits += len(got)
            # a stored query finds itself first, at distance 0 to rounding; the external one finds key 17 at shift 41
            first = gpu.scQueryKey(q, align=align)[0] if q != "ext" else gpu.scQueryDescriptor(ext, align=align)[0]
            assert (first["key"], first["shift"]) == ((17, 41) if q == "ext" else (q, 0))
    assert n_hits > 300
    assert gpu.scSize() == 340


def test_edges_of_the_searched_set(gpu):
    descs = make_descriptors(12, seed=14)
    descs[5] = revisit(descs[1], 9, 0.03, 2)
    q = revisit(descs[1], 30, 0.03, 3)
    # an empty store: no hits from a descriptor; any stored key is outside it
    gpu.scReset()
    assert len(gpu.scQueryDescriptor(q)) == 0 and len(gpu.scQueryDescriptor(q, count=0, top_k=32, align=FULL)) == 0
    with pytest.raises(s2m.S2MError):
        gpu.scQueryKey(0)
    # 1..7 keys: the three-at-a-time walk and its tail; K larger than |S|
    for n in (1, 2, 3, 4, 5, 7):
        fill(gpu, descs[:n])
        for align in (SK, FULL):
            dists = Q.all_distances(descs[:n], q, align)
            for k in (1, 32):
                check(gpu.scQueryDescriptor(q, top_k=k, align=align, max_dist=BIG), Q.rank(dists, range(n), k, BIG), (n, align, k))
            check(gpu.scQueryKey(n - 1, top_k=32, align=align, max_dist=BIG), Q.query(descs[:n], descs[n - 1], top_k=32, align=align, max_dist=BIG), (n, align))
    # windows and sub-ranges on 12 keys
    fill(gpu, descs)
    dists = {a: Q.all_distances(descs, q, a) for a in (SK, FULL)}
    ranges = [dict(exclude_lo=0, exclude_hi=12), dict(exclude_lo=-5, exclude_hi=40),                  # removes everything
              dict(exclude_lo=0, exclude_hi=4), dict(exclude_lo=-3, exclude_hi=2), dict(exclude_lo=8, exclude_hi=12), dict(exclude_lo=9, exclude_hi=99),
              dict(exclude_lo=4, exclude_hi=7), dict(exclude_lo=1, exclude_hi=2), dict(exclude_lo=7, exclude_hi=3),
              dict(first=3), dict(first=12), dict(first=0, count=0), dict(first=0, count=5), dict(first=2, count=10), dict(first=11, count=1),
              dict(first=2, count=9, exclude_lo=4, exclude_hi=6), dict(first=4, count=4, exclude_lo=0, exclude_hi=6),
              dict(first=4, count=4, exclude_lo=6, exclude_hi=12), dict(first=4, count=4, exclude_lo=0, exclude_hi=12)]
    for r in ranges:
        keys = Q.searched_keys(12, **r)
        for align in (SK, FULL):
            for max_dist in (0.05, 0.3, BIG):
                got = gpu.scQueryDescriptor(q, top_k=32, align=align, max_dist=max_dist, **r)
                check(got, Q.rank(dists[align], keys, 32, max_dist), (r, align, max_dist))
        if not keys:
            assert len(gpu.scQueryDescriptor(q, top_k=32, max_dist=BIG, **r)) == 0
    assert len(gpu.scQueryDescriptor(q, top_k=32, max_dist=0.3)) == 2 and len(gpu.scQueryDescriptor(q, top_k=32, max_dist=BIG)) == 12
    # each invalid argument
    for bad in (dict(top_k=0), dict(top_k=33), dict(align=2), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=2e7),
                dict(first=-1), dict(first=13), dict(count=-2), dict(count=13), dict(first=6, count=7)):
        with pytest.raises(s2m.S2MError):
            gpu.scQueryDescriptor(q, **bad)
        with pytest.raises(s2m.S2MError):
            gpu.scQueryKey(0, **bad)
    for key in (-1, 12):
        with pytest.raises(s2m.S2MError):
            gpu.scQueryKey(key)
    lib, d = gpu.lib, np.ascontiguousarray(q, np.float64)
    hits, n = (s2m.ScHit * 32)(), C.c_int32(7)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.s2m_sc_query_descriptor(None, dp, None, hits, C.byref(n)) == -1
    assert lib.s2m_sc_query_descriptor(gpu.h, None, None, hits, C.byref(n)) == -1
    assert lib.s2m_sc_query_descriptor(gpu.h, dp, None, None, C.byref(n)) == -1
    assert lib.s2m_sc_query_descriptor(gpu.h, dp, None, hits, None) == -1
    assert lib.s2m_sc_query_key(gpu.h, 0, None, None, None) == -1
    assert lib.s2m_sc_query_descriptor(gpu.h, dp, None, hits, C.byref(n)) == 0 and n.value == 1 and hits[0].key == 1    # p == NULL: the defaults
    assert gpu.scSize() == 12


def test_ties_and_empty_descriptors(gpu):
    """The 700-key store of test_detect_with_duplicated_key_frames_in_a_large_store (exact copies spread over workgroups) with
    two all-zero descriptors: equal distances come out in key order, an empty descriptor is never a hit and finds nothing."""
    rng = np.random.default_rng(23)
    base = make_descriptors(60, seed=9)
    descs = []
    for k in range(700):
        if k % 7 in (3, 4) or 250 <= k < 262 or 505 <= k < 512:
            descs.append(base[(k // 64) % 60].copy())
        else:
            d = base[int(rng.integers(0, 60))].copy()
            descs.append(revisit(d, int(rng.integers(0, 60)), float(rng.uniform(0.0, 0.05)), int(rng.integers(0, 1 << 30))))
    descs[40] = np.zeros((20, 60))
    descs[300] = np.zeros((20, 60))
    fill(gpu, descs)
    dup = 255                                              # 250 <= k < 262: base[3], as the keys of 192..255 with k % 7 in (3, 4)
    assert np.array_equal(descs[dup], descs[192])
    for align in (SK, FULL):
        dists = Q.all_distances(descs, descs[dup], align)
        for k, max_dist in ((32, 0.3), (32, BIG), (5, 0.3)):
            want = Q.rank(dists, range(700), k, max_dist)
            check(gpu.scQueryKey(dup, top_k=k, align=align, max_dist=max_dist), want, (align, k, max_dist))
            check(gpu.scQueryDescriptor(descs[dup], top_k=k, align=align, max_dist=max_dist), want, (align, k, max_dist))
        want = Q.rank(dists, range(700), 32, BIG)
        ties = sum(want["dist"][i] == want["dist"][i + 1] for i in range(31))
        assert ties >= 10 and all(want["key"][i] < want["key"][i + 1] for i in range(31) if want["dist"][i] == want["dist"][i + 1])
        # the empty descriptors are never a hit: a window of only them, and the whole store at the largest threshold
        assert len(gpu.scQueryKey(dup, first=40, count=1, align=align, max_dist=BIG)) == 0
        assert len(gpu.scQueryKey(dup, first=300, count=1, align=align, max_dist=BIG)) == 0
        tail = Q.rank(dists, range(280, 320), 32, BIG)
        assert 300 not in tail["key"]
        check(gpu.scQueryKey(dup, first=280, count=40, top_k=32, align=align, max_dist=BIG), tail, ("around 300", align))
        # an all-zero query compares with nothing
        assert len(gpu.scQueryKey(40, top_k=32, align=align, max_dist=BIG)) == 0
        assert len(gpu.scQueryDescriptor(np.zeros((20, 60)), top_k=32, align=align, max_dist=BIG)) == 0


@functools.lru_cache(maxsize=None)
def store_3100():
    """(descs, place): 3 x kScQueryMaxGroups + 28 descriptors with revisits of `place` at keys 5, 3071, 3072, 3099 and exact copies
    at 1000 and 3090."""
    n = 3 * s2m.SC_QUERY_MAX_GROUPS + 28
    assert n == 3100
    descs = make_descriptors(n, seed=31)
    place = make_descriptors(1, seed=32)[0]
    for i, k in enumerate((5, 3071, 3072, 3099)):
        descs[k] = revisit(place, 7 * i + 3, 0.04, 40 + i)
    descs[1000] = place.copy()
    descs[3090] = place.copy()
    return descs, place


def fill_3100(g):
    """The store holds store_3100(); one that is there already is kept (the queries leave the store alone)."""
    descs, place = store_3100()
    if getattr(g, "sc_query_store", None) != 3100:
        fill(g, descs)
    g.sc_query_store = 3100
    return descs, place


def test_more_than_one_pass_of_the_grid(gpu):
    """3 x kScQueryMaxGroups + 28 keys: the workgroups walk a second pass, the last one with a tail of one key.  Revisits of
    the query at keys 5, 3071, 3072, 3099 and exact copies at 1000 and 3090."""
    descs, place = fill_3100(gpu)
    want = Q.query(descs, place, top_k=8, align=SK)
    assert sorted(want["key"].tolist()) == [5, 1000, 3071, 3072, 3090, 3099] and want["key"][:2].tolist() == [1000, 3090]
    check(gpu.scQueryDescriptor(place, top_k=8, align=SK), want, "3100 keys")
    check(gpu.scQueryKey(1000, top_k=8, align=SK), want, "3100 keys, stored query")
    check(gpu.scQueryKey(1000, top_k=8, align=SK, exclude_lo=1000, exclude_hi=3072),
          Q.rank(Q.all_distances(descs, place, SK, want["key"].tolist()), [5, 3072, 3090, 3099], 8, 0.3), "3100 keys, window")
    sub = dict(first=2500, count=600)
    want = Q.query(descs, place, top_k=8, align=FULL, max_dist=BIG, **sub)
    assert want["key"][0] == 3090 and set(want["key"][:4].tolist()) == {3071, 3072, 3090, 3099}
    check(gpu.scQueryDescriptor(place, top_k=8, align=FULL, max_dist=BIG, **sub), want, "600 keys, full")


# the model's top 8 of store_3100()'s place at full alignment over the whole store and any threshold: the six planted keys (distance
# below 1e-4) and the two nearest random descriptors (0.4268, 0.4337; the next is 0.4388), from one run of
# Q.rank(Q.all_distances(descs, place, FULL), range(3100), 8, BIG) on the CPU
TOP8_FULL_3100 = [5, 1000, 1584, 3069, 3071, 3072, 3090, 3099]


def test_full_alignment_on_a_second_pass_of_the_grid(gpu):
    """Full alignment over all 3100 keys: 1024 workgroups, of which the first ten compare a second triple (the last a tail of one
    key) in the LDS the first one used.  The single query's row is the many-query's row for the same set as bytes - another
    kernel - and the model's over its top 8."""
    descs, place = fill_3100(gpu)
    kw = dict(top_k=8, align=FULL, max_dist=BIG)
    want = Q.rank(Q.all_distances(descs, place, FULL, TOP8_FULL_3100), TOP8_FULL_3100, 8, BIG)
    assert want["key"][:2].tolist() == [1000, 3090] and sorted(want["key"].tolist()) == TOP8_FULL_3100
    many = gpu.scQueryKeys([1000], **kw)[0]
    for what, got in (("stored query", gpu.scQueryKey(1000, **kw)), ("descriptor", gpu.scQueryDescriptor(place, **kw))):
        assert got.tobytes() == many.tobytes(), (what, got, many)
        check(got, want, what)


def test_ring_key_case_on_the_device(gpu):
    descs = Q.ring_key_case()
    fill(gpu, descs)
    lid, yaw, m = gpu.detectLoopClosureID()
    assert lid == -1 and list(m.cand_idx) == [3, 4, 5]
    hits = gpu.scQueryKey(96, exclude_lo=67, exclude_hi=97, top_k=32)
    assert len(hits) == 1 and hits[0]["key"] == 60 and hits[0]["shift"] == 23
    check(hits, Q.query(descs, descs[96], exclude_lo=67, exclude_hi=97, top_k=32), "ring-key case")


def test_sector_key_blind_case_on_the_device(gpu):
    blind, queries = Q.blind_case()
    fill(gpu, [blind])
    for sh, q in zip(Q.BLIND_SHIFTS, queries):
        got = gpu.scQueryDescriptor(q, align=SK, max_dist=BIG)
        assert len(got) == 1 and got[0]["shift"] != sh and got[0]["dist"] > 0.1
        check(got, Q.query([blind], q, align=SK, max_dist=BIG), ("blind, sector key", sh))
        got = gpu.scQueryDescriptor(q, align=FULL)
        assert len(got) == 1 and got[0]["shift"] == sh and got[0]["dist"] < 1e-3
        check(got, Q.query([blind], q, align=FULL), ("blind, full", sh))


def test_query_sources(gpu):
    """_scan builds the descriptor of s2m_make_scancontext; _projected the one of the deskewed cloud on the device."""
    scene = synth.make_scene(seed=21, half=35.0, n_boxes=14)
    poses = [np.array([0, 0, 0.2 * k, 2.0 * np.cos(0.2 * k), 2.0 * np.sin(0.2 * k), 0.0]) for k in range(5)]
    clouds = [synth.to_xyzi(synth.make_scan(scene, p, "velodyne64", 6000, seed=50 + k)) for k, p in enumerate(poses)]
    gpu.scReset()
    for c in clouds[:4]:
        gpu.makeAndSaveScancontextAndKeys(c)
    kw = dict(top_k=32, max_dist=BIG)
    for align in (SK, FULL):
        for c in (clouds[4], clouds[1]):
            a = gpu.scQueryScan(c, align=align, **kw)
            b = gpu.scQueryDescriptor(gpu.makeScancontext(c)[0], align=align, **kw)
            assert len(a) == 4 and Q.same_hits(a, b)
            check(a, Q.query([O.make_scancontext(x)[0] for x in clouds[:4]], O.make_scancontext(c)[0], align=align, **kw), ("scan", align))
        assert gpu.scQueryScan(clouds[1], align=align)[0]["key"] == 1
    assert gpu.scSize() == 4
    # the projected cloud, on a handle of its own
    g = s2m.MapOptimizationS2M()
    for c in clouds[:4]:
        g.makeAndSaveScancontextAndKeys(c)
    with pytest.raises(s2m.S2MError, match="NO_SCAN"):
        g.scQueryProjected()
    raw = synth.make_raw_scan(scene, synth.POSE_GT, "ouster", n_rings=32, n_az=512, angular_velocity=lambda t: np.array([0.1, -0.2, 0.8]),
                              imu_rate=400.0, stamp=12.5, keep_misses=True)
    proj = s2m.ImageProjectionS2M(g, s2m.S2M_SENSOR_OUSTER, n_scan=32, downsample_rate=1, point_filter_num=2)
    proj.cachePointCloud(raw["raw"], 12.5)
    assert proj.imuDeskewInfo(raw["imu"])
    full = proj.projectPointCloud()
    assert full.shape[0] > 4000
    for align in (SK, FULL):
        a = g.scQueryProjected(align=align, **kw)
        assert len(a) == 4 and Q.same_hits(a, g.scQueryScan(full, align=align, **kw))
    assert g.scSize() == 4
    g.close()


def test_queries_leave_the_detector_alone():
    """The first 60 steps of the sequence_340 add-and-detect loop on two handles; one issues a query of each kind before every
    detection.  Every (loop_id, yaw, ScMatch) and scSize() is equal."""
    descs = sequence_340()[:60]
    cloud = synth.to_xyzi(synth.make_scan(synth.make_scene(seed=21, half=35.0, n_boxes=14), np.zeros(6), "velodyne64", 6000, seed=50))
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    raw = synth.make_raw_scan(synth.make_scene(half=30.0, n_boxes=10), synth.POSE_GT, "ouster", n_rings=32, n_az=512, stamp=12.5, keep_misses=True)
    proj = s2m.ImageProjectionS2M(a, s2m.S2M_SENSOR_OUSTER, n_scan=32, downsample_rate=1, point_filter_num=2)
    proj.cachePointCloud(raw["raw"], 12.5)
    proj.imuDeskewInfo(raw["imu"])
    proj.projectPointCloud(readback=False)                # (leaves the rest of the handle alone: test_project_gpu.py)
    for i, d in enumerate(descs):
        for g in (a, b):
            g.scAddDescriptor(d)
        a.scQueryKey(i, top_k=3, exclude_lo=i - 29, exclude_hi=i + 1)
        a.scQueryDescriptor(descs[(7 * i) % 60], top_k=32, align=FULL, max_dist=BIG)
        a.scQueryScan(cloud, top_k=2, align=FULL if i % 2 else SK)
        a.scQueryProjected(top_k=32, align=SK if i % 2 else FULL, max_dist=BIG)
        ra, rb = a.detectLoopClosureID(), b.detectLoopClosureID()
        assert ra[:2] == rb[:2] and C.string_at(C.addressof(ra[2]), C.sizeof(ra[2])) == C.string_at(C.addressof(rb[2]), C.sizeof(rb[2])), i
        assert a.scSize() == b.scSize() == i + 1
    a.close(); b.close()
