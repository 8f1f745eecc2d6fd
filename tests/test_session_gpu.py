"""Saving and loading a session on the GPU (include/liorf_s2m.h, "Saving and loading a session"), held
against the model of tests/ref/session_ref.py: a scripted session is built through the per-key calls into handle A, saved, and
loaded into fresh handles - one with the default staging chunk, one with a chunk of 4 KiB - which then have to answer every call
bit for bit as A does, and to continue as A does.

The store: nine keys whose cloud sizes sit on the kernels' edges (0 - s2m_kf_add accepts an empty cloud -, 1, 63, 64, 65, 255,
256, 257, 1000 records, with bits in all eight words and one NaN coordinate) in a cluster of their own, then the 32 keys of the
scripted revisit (tests/test_loop_closure_cpu.py), whose clouds let loop closures and the relocalisation run for real.
With 128 records to a chunk the edge keys' offsets 0, 0, 1, 64, 128, 193, 448, 704, 961, 1961 give a chunk edge on a key
boundary (128), edges inside record runs, and a key (255 records from 193) across three chunks; test_the_small_chunk_meets_
its_three_conditions holds that arithmetic.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import relocalize_ref as R
import session_ref as M

from liorf_amd import s2m
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, BUSY, FORMAT, CHECKSUM, IO = -1, s2m.S2M_ERR_BUSY, s2m.S2M_ERR_FORMAT, s2m.S2M_ERR_CHECKSUM, s2m.S2M_ERR_IO
EDGE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
SMALL_CHUNK = 4096
N_DESC = 35
LOOP = dict(search_radius=15.0, search_num=2, icp_leaf=0.5)
PAIRS = [(40, 9), (39, 10), (38, 11)]                   # the revisit's last keys against its first (store keys = revisit + 9)


def code_of(fn):
    """The status a call fails with (0: it did not fail)."""
    try:
        fn()
        return 0
    except s2m.S2MError as e:
        return e.code


def raw(x):
    """Anything a call returns, as bytes: bit-for-bit comparisons of arrays (NaNs included), ctypes records and tuples of them."""
    if isinstance(x, np.ndarray):
        return repr((x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, C.Structure):                      # field by field: a record's padding is nobody's promise
        return b"{" + b"|".join(raw(getattr(x, f[0])) for f in x._fields_) + b"}"
    if isinstance(x, C.Array):
        return b"|".join(raw(v) for v in x) if issubclass(x._type_, C.Structure) else bytes(x)
    if isinstance(x, (tuple, list)):
        return b"|".join(raw(v) for v in x)
    return repr(x).encode()


def edge_clouds():
    rng = np.random.default_rng(5)
    out = []
    for n in EDGE_SIZES:
        c = rng.normal(0, 3, (n, 8)).astype(F)
        c[:, 3] = 1.0
        w = c.view(np.uint32)
        w[:, 5:] = rng.integers(0, 1 << 32, (n, 3), dtype=np.uint64).astype(np.uint32)     # bits in words 5..7, any pattern
        w[::2, 3] = rng.integers(0, 1 << 32, w[::2, 3].shape, dtype=np.uint64).astype(np.uint32)
        out.append(c)
    out[5].view(np.uint32)[100, 1] = 0x7FC00123         # one NaN coordinate, with a payload
    return out


def script():
    """(clouds, poses, times, descriptors) of the 41 keys."""
    rc, rp, rt, _, rd = R.revisit()
    ec = edge_clouds()
    ep = np.array([[300.0 + 2.0 * k, -100.0, 0.5, 0.01 * k, -0.02, 0.3 * k] for k in range(len(ec))], F)
    et = -100.0 + np.arange(len(ec))
    descs = [O.make_scancontext(c)[0] if len(c) else np.zeros((20, 60)) for c in ec] + list(rd)
    return ec + list(rc), np.vstack([ep, rp]).astype(F), np.concatenate([et, rt]), descs


def build(g):
    """The scripted session through the per-key calls; returns the model of what the handle then holds."""
    clouds, poses, times, descs = script()
    m, graph = M.Session(), M.Graph()
    for k in range(len(clouds)):
        g.saveKeyFrame(poses[k], times[k], clouds[k])
        g.addOdomFactor(poses[k])
        m.add_key(poses[k], times[k], clouds[k])
        graph.add_odometry(poses[k])
        if k < N_DESC:
            g.scAddDescriptor(descs[k])
    m.desc = np.array([np.asarray(d, np.float64).reshape(1200) for d in descs[:N_DESC]])
    for _ in range(3):                                   # the detector has been called: the kd-tree's age goes into the blob
        g.detectLoopClosureID()
    m.n_search, m.counter = N_DESC - 30, 3
    var, k = [0.04, 0.04, 0.04, 0.09, 0.09, 0.09], 0.0
    for cur, pre in PAIRS:
        r = g.loopAlign(cur, pre, -1, s2m.default_loop_params(fitness_score=np.inf, **LOOP))
        assert r.status == s2m.S2M_LOOP_ACCEPTED, (cur, pre, r.status, r.icp.converged, r.icp.fitness_score)
        rel = s2m.between_xyzrpy(r.pose_from, r.pose_to)
        g.pgAddBetween(cur, pre, rel, var, k)
        graph.add_between(cur, pre, rel, var, k)
        m.pairs.append((cur, pre))
        k = 1.0                                          # the later ones robust (Cauchy), as an SC closure's factor
    m.pairs.sort()
    g.pgAddGps(20, [-1.0, 3.0, 0.2], [1.0, 1.0, 4.0])
    graph.add_gps(20, [-1.0, 3.0, 0.2], [1.0, 1.0, 4.0])
    m.set_graph(graph)
    return m


@pytest.fixture(scope="module")
def saved():
    """(A, the model, A's blob) - saved before anything is optimised, so that the model knows every bit of it."""
    a = s2m.MapOptimizationS2M()
    m = build(a)
    blob = a.session_save()
    yield a, m, blob
    a.close()


@pytest.fixture(scope="module")
def trio(saved):
    """A and two handles loaded from its blob: default chunk, small chunk. Every test applies the same calls to all three."""
    a, _, blob = saved
    b0, b1 = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    b1.sessionChunk(SMALL_CHUNK)
    for b in (b0, b1):
        info = b.session_load(blob)
        assert (info.n_keys, info.n_descriptors, info.n_loop_pairs, info.n_variables, info.n_factors, info.bytes) == (41, N_DESC, 3, 41, 45, len(blob))
    yield [a, b0, b1]
    b0.close()
    b1.close()


def same(trio, fn, what):
    """fn on A and on both loaded handles, in lockstep; the results are the same bits. Returns a loaded handle's."""
    vals = [fn(g) for g in trio]
    got = [raw(v) for v in vals]
    assert got[0] == got[1], what + ": default chunk"
    assert got[0] == got[2], what + ": small chunk"
    return vals[1]


# ---- 1. the blob is the model's --------------------------------------------------------------------------------

def test_the_small_chunk_meets_its_three_conditions():
    off = np.concatenate([[0], np.cumsum(EDGE_SIZES)])
    per = SMALL_CHUNK // 32
    edges = set(range(per, int(off[-1]), per))
    assert any(e in set(off[1:-1].tolist()) for e in edges)                                  # an edge exactly on a key boundary
    assert any(off[k] < e < off[k + 1] for e in edges for k in range(len(EDGE_SIZES)))      # an edge inside a record run
    assert any(len([e for e in edges if off[k] < e < off[k + 1]]) >= 2 for k in range(len(EDGE_SIZES)))   # a key across three chunks


def test_the_blob_is_byte_for_byte_the_models(saved):
    a, m, blob = saved
    want = M.write(m)
    assert len(blob) == len(want) == a.session_info().bytes
    if blob != want:                                     # name the first section that differs
        _, got_secs, _ = M.split(blob)
        for name, x, y in zip(M.SECTIONS, got_secs, m.sections()):
            assert x == y, name
    assert blob == want
    assert M.write(M.parse(blob)) == blob
    info = s2m.session_check(blob)
    assert (info.n_keys, info.n_points) == (41, sum(EDGE_SIZES) + sum(len(c) for c in R.revisit()[0]))


def test_a_blob_the_model_wrote_loads_and_saves_back(saved):
    _, m, _ = saved
    want = M.write(m)
    g = s2m.MapOptimizationS2M()
    g.sessionChunk(SMALL_CHUNK)
    g.session_load(want)
    assert g.session_save() == want
    # and the model's own scripted session (empty clouds, a ScanContext store shorter than the key-frame store)
    blob = M.write(M.scripted())
    for chunk in (0, 1024):
        g.kfReset(); g.scReset(); g.pgReset()
        g.sessionChunk(chunk)
        g.session_load(blob)
        assert g.session_save() == blob
    g.close()


# ---- 2. round trip, 3. derived state ----------------------------------------------------------------------------

def test_round_trip_at_both_chunk_sizes(saved, trio):
    _, _, blob = saved
    for g in trio:
        for chunk in (0, SMALL_CHUNK, 1024):
            g.sessionChunk(chunk)
            assert g.session_save() == blob, chunk
    trio[0].sessionChunk(0); trio[1].sessionChunk(0); trio[2].sessionChunk(SMALL_CHUNK)
    chunks = []
    trio[2].session_save(write=lambda c: chunks.append(len(c)) and None)
    big = [c for c in chunks if c > SMALL_CHUNK]             # (the small sections are written whole: here the factors)
    assert len(big) <= 2 and len(chunks) > 1000 and sum(chunks) == len(blob)


def test_derived_state_is_bit_equal(trio):
    same(trio, lambda g: g.scKeys(), "ring and sector keys")
    ring, sector = trio[1].scKeys()
    desc = np.array(script()[3][:N_DESC], np.float64).reshape(N_DESC, 20, 60)
    assert np.allclose(ring, desc.mean(axis=2), rtol=1e-6) and np.allclose(sector, desc.mean(axis=1), rtol=1e-12)
    for k in range(41):
        same(trio, lambda g: g.kfFrame(k), f"frame of key {k}")
        th, td, pos, n = trio[2].kfFrame(k)
        assert np.array_equal(th.view(np.uint32), td.view(np.uint32)) and n == len(script()[0][k])
        assert np.array_equal(pos[:3], script()[1][k, :3])


# ---- 4. behaviour ------------------------------------------------------------------------------------------------

def test_extraction_and_maps_are_bit_equal(trio):
    times = script()[2]
    same(trio, lambda g: g.extractSurroundingKeyFrames(times[-1] + 0.5, return_map=True), "extractSurroundingKeyFrames")
    keys, cloud = same(trio, lambda g: g.extractSurroundingKeyFramesAt([305.0, -99.0, 0.0], s2m.default_kf_params(density=0.5), return_map=True),
                       "extractSurroundingKeyFramesAt the edge cluster")
    assert set(keys.tolist()) <= set(range(9)) and len(keys) >= 5 and len(cloud) > 100
    same(trio, lambda g: g.extractSurroundingKeyFramesAt([-20.0, 3.0, 0.0], return_map=True), "extractSurroundingKeyFramesAt the circle")
    got = same(trio, lambda g: g.globalMapCloud(), "s2m_kf_map_cloud over all keys")
    assert got.shape[0] == sum(len(c) for c in script()[0])
    # what the saved map shows of the stored words: the transform passes word 4 (the intensity) through and writes 1 and zeros
    # into the others, so words 3 and 5 .. 7 are held by the blobs alone (save(B) == save(A), test_round_trip_at_both_chunk_sizes)
    edge = np.concatenate(edge_clouds()).view(np.uint32)
    assert np.array_equal(got[:edge.shape[0]].view(np.uint32)[:, 4], edge[:, 4])
    assert np.isnan(got[:edge.shape[0], :3]).any()
    same(trio, lambda g: g.publishGlobalMap(return_keys=True), "s2m_global_map")


def test_scancontext_calls_are_bit_equal(trio):
    for align in (s2m.S2M_SC_ALIGN_SECTOR_KEY, s2m.S2M_SC_ALIGN_FULL):
        for key in (0, 17, N_DESC - 1):
            hits = same(trio, lambda g: g.scQueryKey(key, top_k=8, align=align, max_dist=10.0), f"scQueryKey {key} {align}")
            assert len(hits) == 8 or key != 17
    # the detector: the fourth call since the tree was made searches the 5 keys it held then; six more calls rebuild it
    _, _, detail = same(trio, lambda g: g.detectLoopClosureID(), "detectLoopClosureID")
    assert max(detail.cand_idx) < N_DESC - 30
    for _ in range(7):
        _, _, detail = same(trio, lambda g: g.detectLoopClosureID(), "detectLoopClosureID")
    assert max(detail.cand_idx) < N_DESC - 30 + 1        # (the rebuild at the tenth call saw the same 35 descriptors)
    same(trio, lambda g: g.session_info(), "session_info after the detector ran")
    same(trio, lambda g: g.distanceBtnScanContext(20, [1, 9, 21, 34]), "distanceBtnScanContext")


def test_loop_closure_and_relocalisation_are_bit_equal(trio):
    times = script()[2]
    prm = s2m.default_loop_params(fitness_score=0.3, **LOOP)
    r = same(trio, lambda g: g.performRSLoopClosure(times[-1], prm), "performRSLoopClosure, closed")
    assert (r.status, r.key_cur) == (s2m.S2M_LOOP_ALREADY_CLOSED, 40)      # the container came along: the pair is not reported again
    assert same(trio, lambda g: g.loopAlign(39, 10, -1, prm), "loopAlign of a stored pair").status == s2m.S2M_LOOP_ALREADY_CLOSED
    fresh = same(trio, lambda g: g.loopAlign(36, 12, -1, prm), "loopAlign of a new pair")
    assert fresh.status in (s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_REJECTED) and fresh.icp.iterations > 0
    same(trio, lambda g: g.loopFindNearKeyframes(12, 2, -1, 0.5), "loopFindNearKeyframes")
    scan, _ = R.query_scan("Q1")
    rp = s2m.default_reloc_params(loop_search_radius=R.R, loop_search_num=R.SEARCH_NUM, loop_icp_leaf=R.LEAF, loop_fitness_score=R.FITNESS)
    recs, best = same(trio, lambda g: g.relocalizeScan(scan, rp), "relocalizeScan")
    assert best >= 0 and recs[best].hit.key in (R.TRUE_KEY + 9 - 1, R.TRUE_KEY + 9)
    same(trio, lambda g: g.session_save(), "the blob after the closures")


def test_pose_graph_calls_are_bit_equal(trio):
    same(trio, lambda g: g.pgPoses(), "pgPoses")
    res = same(trio, lambda g: g.pgOptimize(), "pgOptimize")
    assert res.n_factors >= 45 and res.n_variables == 41 and res.iterations > 0
    same(trio, lambda g: g.pgPoses(), "pgPoses after the optimise")
    same(trio, lambda g: g.pgMarginal(23), "pgMarginal")
    same(trio, lambda g: g.pgMarginals([0, 40]), "pgMarginals")
    same(trio, lambda g: g.session_save(), "the blob after the optimise")


# ---- 5. continuation -----------------------------------------------------------------------------------------------

def test_three_further_keys_continue_alike(trio):
    clouds, poses, times, descs = script()
    prm = s2m.default_loop_params(fitness_score=0.3, **LOOP)
    for j in (1, 2, 3):                                  # a second lap: the revisit's keys 1 .. 3 again, a little off
        pose = poses[9 + j] + np.array([0.2, -0.1, 0.0, 0.0, 0.0, 0.02], F)
        t = times[-1] + j
        for g in trio:
            g.saveKeyFrame(pose, t, clouds[9 + j])
            g.scAddDescriptor(descs[9 + j])
            g.addOdomFactor(pose)
    same(trio, lambda g: g.performRSLoopClosure(times[-1] + 3, prm), "performRSLoopClosure from the new newest key")
    r = same(trio, lambda g: g.loopAlign(43, 12, -1, s2m.default_loop_params(fitness_score=np.inf, **LOOP)), "loopAlign of the newest key")
    assert r.status in (s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_ALREADY_CLOSED)      # (closed: the RS closure above took key 43)
    rel = s2m.between_xyzrpy(r.pose_from, r.pose_to) if r.status == s2m.S2M_LOOP_ACCEPTED else np.array([-0.2, 0.1, 0, 0, 0, -0.02], F)
    for g in trio:
        g.pgAddBetween(43, 12, rel, [0.05] * 6, 1.0)
    same(trio, lambda g: g.pgOptimize(), "pgOptimize of the grown graph")
    for g in trio:
        g.pgApplyToStore(0, 44)
    same(trio, lambda g: g.pgPoses(), "poses")
    same(trio, lambda g: g.extractSurroundingKeyFrames(times[-1] + 3.5, return_map=True), "extraction after correctPoses")
    same(trio, lambda g: g.detectLoopClosureID(), "detection")
    same(trio, lambda g: [g.kfFrame(k) for k in (0, 9, 43)], "frames after correctPoses")
    same(trio, lambda g: g.globalMapCloud(40, 4), "the new keys' clouds")
    same(trio, lambda g: g.session_save(), "the blob of the grown session")
    info = s2m.session_check(trio[0].session_save())
    assert (info.n_keys, info.n_descriptors, info.n_variables) == (44, N_DESC + 3, 44)
    # and once more round: what was loaded, grown and saved loads again
    g = s2m.MapOptimizationS2M()
    g.session_load(trio[2].session_save())
    assert g.session_save() == trio[0].session_save()
    assert raw(g.pgPoses()) == raw(trio[0].pgPoses())
    g.close()


# ---- 6. the arena -------------------------------------------------------------------------------------------------

def test_clouds_beyond_one_arena_block():
    rng = np.random.default_rng(9)
    cloud = rng.normal(0, 20, (1_100_000, 8)).astype(F)        # 35.2 MB a key: each of the three needs a 64 MB block of its own
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    for k in range(3):
        a.saveKeyFrame([k, 0, 0, 0, 0, 0.1 * k], float(k), cloud)
    small = np.ones((5, 8), F)
    a.saveKeyFrame([9, 0, 0, 0, 0, 0], 9.0, small)              # and a small one behind them
    blob = a.session_save()
    assert len(blob) == 224 + 4 * 40 + 32 * (3 * 1_100_000 + 5)
    b.session_load(blob)
    assert b.session_save() == blob
    assert raw(a.globalMapCloud()) == raw(b.globalMapCloud())
    b.saveKeyFrame([10, 0, 0, 0, 0, 0], 10.0, small)            # the arena goes on from a valid state
    a.saveKeyFrame([10, 0, 0, 0, 0, 0], 10.0, small)
    assert raw(a.globalMapCloud(3, 2)) == raw(b.globalMapCloud(3, 2)) and a.session_save() == b.session_save()
    a.close()
    b.close()


# ---- 7. contracts ---------------------------------------------------------------------------------------------------

def sizes(g):
    return g.kfSize(), g.scSize(), g.pgSize(), g.session_info().n_loop_pairs


def test_load_into_a_handle_that_is_not_empty_is_refused(saved):
    _, _, blob = saved
    g = s2m.MapOptimizationS2M()
    g.session_load(blob)
    before = g.session_save()
    with pytest.raises(s2m.S2MError, match="reset") as e:
        g.session_load(blob)
    assert e.value.code == INVALID and g.session_save() == before == blob
    for part in ("kf", "sc", "pg"):                      # each store alone is enough to refuse
        h = s2m.MapOptimizationS2M()
        if part == "kf":
            h.saveKeyFrame([0] * 6, 0.0, np.ones((3, 8), F))
        elif part == "sc":
            h.scAddDescriptor(np.ones((20, 60)))
        else:
            h.pgSetInitial(0, [0] * 6)
        assert code_of(lambda: h.session_load(blob)) == INVALID, part
        h.close()
    g.kfReset(); g.scReset(); g.pgReset()
    assert sizes(g) == (0, 0, (0, 0), 0)
    g.session_load(blob)
    assert g.session_save() == blob
    g.close()


def test_corruption_and_failing_callbacks_leave_the_stores_empty(saved):
    a, _, blob = saved
    hd, secs, _ = M.split(blob)
    cloud_at = M.HEADER + len(secs[0])
    desc_at = cloud_at + len(secs[1])
    g = s2m.MapOptimizationS2M()
    for chunk in (0, SMALL_CHUNK):
        g.sessionChunk(chunk)
        for at in (cloud_at + 32 * 700 + 5, desc_at + 9600 * 20 + 3):
            bad = bytearray(blob)
            bad[at] ^= 0x10
            assert code_of(lambda: g.session_load(bytes(bad))) == CHECKSUM, (chunk, at)
            assert sizes(g) == (0, 0, (0, 0), 0)
        for cut in (50, M.HEADER + 100, cloud_at + 32 * 1000 + 7, desc_at + 5000, len(blob) - 10):
            assert code_of(lambda: g.session_load(blob[:cut])) == FORMAT, cut       # the stream ends early
            assert sizes(g) == (0, 0, (0, 0), 0)
        # a read callback that fails halfway
        left = [len(blob) // 2]
        pos = [0]

        def read(n):
            if left[0] < n:
                raise OSError("the disk went away")
            left[0] -= n
            pos[0] += n
            return blob[pos[0] - n:pos[0]]
        assert code_of(lambda: g.session_load(read=read)) == IO
        assert sizes(g) == (0, 0, (0, 0), 0)
        g.session_load(blob)                             # and a good load after all that
        assert g.session_save() == blob
        g.kfReset(); g.scReset(); g.pgReset()
    # content that the checksums cover but the checks refuse: a loop pair that names no stored key
    m = M.parse(blob)
    m.pairs[-1] = (40, 41)
    assert code_of(lambda: g.session_load(M.write(m))) == FORMAT and sizes(g) == (0, 0, (0, 0), 0)
    # a write callback that fails: the handle that saves is unchanged
    n = [0]

    def write(chunk):
        n[0] += 1
        return n[0] == 40
    before = sizes(a)
    a.sessionChunk(SMALL_CHUNK)
    assert code_of(lambda: a.session_save(write=write)) == IO and n[0] == 40
    a.sessionChunk(0)
    assert sizes(a) == before and a.session_info().bytes >= len(blob)
    g.close()


def test_busy_while_a_closure_or_an_optimise_is_pending_and_the_estimates_a_save_writes(saved):
    _, _, blob = saved
    d, e = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    d.session_load(blob)
    e.session_load(blob)
    r = d.loopAlignLaunch(37, 12, -1, s2m.default_loop_params(fitness_score=0.3, **LOOP))
    assert r.status == s2m.S2M_LOOP_PENDING
    assert code_of(d.session_save) == BUSY and code_of(lambda: d.session_load(blob)) == BUSY
    d.loopCollect()
    e.loopAlign(37, 12, -1, s2m.default_loop_params(fitness_score=0.3, **LOOP))
    assert d.session_save() == e.session_save()
    # a launched optimise
    rc, _ = d.pgOptimizeLaunch()
    assert rc == s2m.S2M_PG_PENDING
    assert code_of(d.session_save) == BUSY and code_of(lambda: d.session_load(blob)) == BUSY
    rc, res = d.pgOptimizeCollect()
    assert rc == s2m.S2M_OK and res.iterations > 0
    got = d.session_save()                               # the device's estimates are newer than the mirror: the save fetches them
    want = e.pgOptimize()
    assert got == e.session_save() and bytes(want) == bytes(res)
    x0, x1 = M.parse(blob).X, M.parse(got).X
    assert not np.array_equal(x0, x1) and np.abs(x1 - x0).max() > 1e-4
    d.close()
    e.close()


# ---- 8. the file forms -------------------------------------------------------------------------------------------------

def test_files_round_trip(saved, tmp_path):
    a, _, blob = saved
    p = str(tmp_path / "session.s2m")
    g = s2m.MapOptimizationS2M()
    g.session_load(blob)
    g.session_save_file(p)
    assert open(p, "rb").read() == blob
    h = s2m.MapOptimizationS2M()
    info = h.session_load_file(p)
    assert info.bytes == len(blob) and h.session_save() == blob
    h.kfReset(); h.scReset(); h.pgReset()
    open(p, "wb").write(blob[:len(blob) // 3])
    assert code_of(lambda: h.session_load_file(p)) == FORMAT and sizes(h) == (0, 0, (0, 0), 0)
    assert code_of(lambda: h.session_load_file(str(tmp_path / "none.s2m"))) == IO
    assert code_of(lambda: g.session_save_file(str(tmp_path / "no" / "such" / "dir.s2m"))) == IO
    g.close()
    h.close()
