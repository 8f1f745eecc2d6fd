"""GPU tests of localising a scan in the stored map: ICP with an initial guess (s2m_icp_align_guess, the per-slot guesses of the
device loop), s2m_relocalize_scan on the scripted revisit against the model of tests/ref/relocalize_ref.py and against a twin
handle, and s2m_extract_surrounding_at against the existing extraction, the restated selection and the host composition.
See tests/test_relocalize_cpu.py for the model's figures and for why the best record of Q2 is key 7 at position 3.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import relocalize_ref as M

from liorf_amd import s2m, synth
from test_icp_cpu import icp_scene
from test_relocalize_cpu import POS_BAR, YAW_BAR, free_centre_store
from test_global_map_cpu import BOUNDARY_D, BOUNDARY_R

pytestmark = pytest.mark.gpu

F = np.float32
A, RJ, FEW = s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_REJECTED, s2m.S2M_LOOP_TOO_FEW_POINTS
FIX = dict(loop_search_radius=M.R, loop_search_num=M.SEARCH_NUM, loop_icp_leaf=M.LEAF, loop_fitness_score=M.FITNESS)   # top_k 4, all 60 shifts
# Largest entry of |T - oracle_T @ G| (float64 product) measured on an MI355X for the guess of the second test: 9.6e-7, in the
# translation column: the device chains its float 4x4 products from G, the model chains them from I and
# multiplies by G once. The bar is four times that; it is below the README's ICP bar (2e-4) and a hundredth of what tells
# T_true * G from the identity.
T_GUESS_MEASURED = 9.6e-7
T_GUESS_BAR = 4 * T_GUESS_MEASURED


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _same_icp(a, b):
    """Two (T, converged, fitness, iterations): the same bits."""
    assert np.array_equal(np.asarray(a[0], F).view(np.uint32), np.asarray(b[0], F).view(np.uint32)), (a, b)
    assert a[1] == b[1] and a[3] == b[3] and np.float64(a[2]).view(np.uint64) == np.float64(b[2]).view(np.uint64), (a[1:], b[1:])


def _icp_of(rec):
    return np.array(rec.icp.T, F).reshape(4, 4), bool(rec.icp.converged), rec.icp.fitness_score, rec.icp.iterations


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


@pytest.fixture(scope="module")
def twin():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


# ---- part A: ICP with an initial guess ----------------------------------------------------------------------

def _guess_case():
    """icp_scene with its source pre-moved by G^-1 (float64, stored as fp32), so that the guess G puts it back where
    icp_scene left it: (src', tgt, G float32 4x4, T_true)."""
    src, tgt, T_true = icp_scene(6000, 1500, 5)
    G = np.eye(4)
    G[:3, :3] = synth.rotation_rpy(0.02, -0.01, 0.7)
    G[:3, 3] = (3.0, -2.0, 0.5)
    G = G.astype(F)
    Gi = np.linalg.inv(G.astype(np.float64))
    moved = src.copy()
    moved[:, :3] = (src[:, :3].astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]).astype(F)
    return moved, tgt, G, T_true


def test_identity_guess_is_icp_align(gpu):
    src, tgt, _ = icp_scene(6000, 1500, 5)
    want = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    _same_icp(gpu.icpAlignGuess(src, tgt, None, max_correspondence_distance=30.0), want)
    _same_icp(gpu.icpAlignGuess(src, tgt, np.eye(4, dtype=F), max_correspondence_distance=30.0), want)
    neg0 = np.eye(4, dtype=F)
    neg0[0, 1] = -0.0                                    # equal to the identity as `guess != Identity` compares
    _same_icp(gpu.icpAlignGuess(src, tgt, neg0, max_correspondence_distance=30.0), want)


def test_a_real_guess_against_the_oracle(gpu):
    src, tgt, G, T_true = _guess_case()
    T, conv, fit, its = gpu.icpAlignGuess(src, tgt, G, max_correspondence_distance=30.0)
    To, convo, fito, itso, _ = M.icp_guess(src, tgt, G, max_corr_dist=30.0)
    dev = float(np.abs(T.astype(np.float64) - To).max())
    print("guessed ICP: iterations", its, itso, "fitness", fit, fito, "max |T - oracle_T @ G|", dev)
    assert conv == convo and conv and its == itso
    assert abs(fit - fito) <= 1e-6
    assert T_GUESS_BAR <= 2e-4 and T_GUESS_BAR < np.abs(T_true @ G.astype(np.float64) - np.eye(4)).max() / 100
    assert dev <= T_GUESS_BAR
    # T includes the guess: it takes the pre-moved source onto the target, as T_true * G does
    assert np.abs(T.astype(np.float64) - T_true @ G.astype(np.float64))[:3, 3].max() < 0.03
    # and the guess was used: from the identity the same source ends elsewhere
    T0, _, fit0, its0 = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    print("from the identity: iterations", its0, "fitness", fit0)
    assert its0 != its or np.abs(T0 - T).max() > 1e-3


def test_host_loop_and_device_loop_agree_for_three_guesses_in_lockstep(gpu):
    src, tgt, G, _ = _guess_case()
    G2 = np.eye(4)
    G2[:3, :3] = synth.rotation_rpy(0.02, -0.01, 1.0)
    G2[:3, 3] = (3.0, -2.0, 0.5)
    guesses = [G, G2.astype(F), np.eye(4, dtype=F)]
    kw = dict(max_correspondence_distance=30.0)
    got = gpu.debugIcpAlignGuessManyDevice(src, [tgt, tgt, tgt], guesses, **kw)
    its = [g[3] for g in got]
    print("iterations per slot", its, "fitness", [g[2] for g in got])
    assert len({(i - 1) // s2m.S2M_ICP_RANGE for i in its}) > 1          # the slots end in different ranges: not vacuous
    for k, g in enumerate(guesses):
        _same_icp(got[k], gpu.debugIcpAlignGuessManyDevice(src, [tgt], [g], **kw)[0])     # slot k of 3 = slot 0 of 1
        _same_icp(got[k], gpu.icpAlignGuess(src, tgt, g, **kw))                           # the device loop = the host loop
    _same_icp(got[2], gpu.icpAlign(src, tgt, **kw))
    # the guesses in another order land in other slots and give the same results
    back = gpu.debugIcpAlignGuessManyDevice(src, [tgt, tgt, tgt], guesses[::-1], **kw)
    for k in range(3):
        _same_icp(back[2 - k], got[k])
    # no guesses: the call it stands beside
    _same_icp(gpu.debugIcpAlignGuessManyDevice(src, [tgt], None, **kw)[0], gpu.icpAlign(src, tgt, **kw))


def test_bad_guesses_are_rejected(gpu):
    src, tgt, G, _ = _guess_case()
    r = s2m.IcpResult()
    for bad in ("nan", "row"):
        g = G.copy()
        if bad == "nan":
            g[1, 2] = np.nan
        else:
            g[3, 3] = 2.0
        gp = g.ctypes.data_as(C.POINTER(C.c_float))
        assert gpu.lib.s2m_icp_align_guess(gpu.h, src.ctypes.data, len(src), tgt.ctypes.data, len(tgt), 32, gp, None, C.byref(r)) == -1, bad
        with pytest.raises(s2m.S2MError):
            gpu.debugIcpAlignGuessManyDevice(src, [tgt, tgt], [G, g], max_correspondence_distance=30.0)
    g = G.copy()
    g[0, 3] = np.inf
    with pytest.raises(s2m.S2MError):
        gpu.icpAlignGuess(src, tgt, g)


# ---- part B: relocalisation ---------------------------------------------------------------------------------

def _fill(g, extra=False, extra_sc=False):
    """The scripted revisit as a stored map: every key's cloud into the key-frame store and the ScanContext store."""
    clouds, poses, times, _, _ = M.revisit()
    g.kfReset()
    g.scReset()
    for k in range(len(clouds)):
        g.saveKeyFrame(poses[k], times[k], clouds[k])
        g.makeAndSaveScancontextAndKeys(clouds[k])
    if extra:                                            # a 33rd key: the first 600 records of key 5's cloud, in both stores
        g.saveKeyFrame(poses[5], times[-1] + 1.0, clouds[5][:600])
        g.makeAndSaveScancontextAndKeys(clouds[5][:600])
    if extra_sc:                                         # the ScanContext store one key longer than the key-frame store
        g.makeAndSaveScancontextAndKeys(clouds[5][:600])


def _hit_bytes(hits):
    return [h.tobytes() for h in hits]


@pytest.mark.parametrize("name", ["Q1", "Q2"])
def test_relocalize_against_the_model_and_the_twin(gpu, twin, name):
    scan, true = M.query_scan(name)
    m = M.model(name)
    _fill(gpu)
    _fill(twin)
    prm = s2m.default_reloc_params(**FIX)
    recs, best = gpu.relocalizeScan(scan, prm)
    hits = gpu.scQueryScan(scan, top_k=M.TOP_K, align=s2m.S2M_SC_ALIGN_FULL)
    assert [_bytes(r.hit) for r in recs] == _hit_bytes(hits) and len(recs) == len(m["records"]) == 4
    assert [r.hit.key for r in recs] == [w["key"] for w in m["records"]]
    src = twin.voxelGrid(scan, M.LEAF)
    for r, w in zip(recs, m["records"]):
        pe = M.pose_error(r.pose_xyzrpy, true) if r.status == A else None
        print(name, "key", r.hit.key, "status", r.status, "fitness", r.icp.fitness_score, w["fitness"], "iterations", r.icp.iterations, w["iterations"],
              "pose error", pe)
        assert (r.status, r.n_src, r.n_tgt) == (w["status"], w["n_src"], w["n_tgt"])
        assert np.abs(np.array(r.guess, np.float64).reshape(4, 4) - w["guess"]).max() <= 1e-6
        # the record's icp: what a twin handle gives through s2m_icp_align_guess on the same source, target and guess
        tgt = twin.loopFindNearKeyframes(r.hit.key, M.SEARCH_NUM, -1, M.LEAF)
        assert src.shape[0] == r.n_src and tgt.shape[0] == r.n_tgt
        want = twin.icpAlignGuess(src, tgt, np.array(r.guess, F).reshape(4, 4), max_correspondence_distance=M.MAX_CORR)
        _same_icp(_icp_of(r), want)
        if r.status == A:
            assert list(r.pose_tobemapped) == [r.pose_xyzrpy[k] for k in (3, 4, 5, 0, 1, 2)]
            assert np.allclose(np.array(r.pose_xyzrpy), M.translation_and_euler64(np.array(r.icp.T, np.float64).reshape(4, 4)), atol=1e-6)
        else:
            assert list(r.pose_xyzrpy) == [0.0] * 6 and list(r.pose_tobemapped) == [0.0] * 6
    assert best == m["best"]
    ranked = sorted((r.icp.fitness_score, i) for i, r in enumerate(recs) if r.status == A)
    assert best == ranked[0][1]                                        # the rule: least (fitness, position)
    if name == "Q2":
        assert best != 0 and recs[0].hit.key == 23 and recs[0].status == A    # not the descriptor's first hit, the mirror place
    assert recs[best].hit.key in (7, 8)
    pe, ye = M.pose_error(recs[best].pose_xyzrpy, true)
    assert pe < POS_BAR and ye < YAW_BAR, (pe, ye)
    k8 = [r for r in recs if r.hit.key == 8][0]
    pe, ye = M.pose_error(k8.pose_xyzrpy, true)
    assert k8.status == A and pe < POS_BAR and ye < YAW_BAR, (pe, ye)


def test_without_the_yaw_the_true_place_is_rejected(gpu):
    scan, _ = M.query_scan("Q2")
    m = M.model("Q2", use_yaw=False)
    _fill(gpu)
    recs, best = gpu.relocalizeScan(scan, s2m.default_reloc_params(use_yaw=0, **FIX))
    print("use_yaw 0:", [(r.hit.key, r.status, r.icp.fitness_score, r.icp.iterations) for r in recs], "best", best)
    assert [r.status for r in recs] == [w["status"] for w in m["records"]]
    k8 = [r for r in recs if r.hit.key == 8][0]
    assert k8.status == RJ
    assert best == m["best"] and (best == -1 or recs[best].hit.key != 8)
    poses = M.revisit()[1]
    for r in recs:                                                     # the guess is the key's stored transform, nothing else
        assert np.abs(np.array(r.guess, np.float64).reshape(4, 4) - M.transformation64(poses[r.hit.key])).max() <= 1e-6


def test_gates_and_errors(gpu):
    clouds = M.revisit()[0]
    scan, _ = M.query_scan("Q1")
    prm = s2m.default_reloc_params(**FIX)
    # a 33rd key of 600 points, queried directly: it is the first hit (distance 0), takes no slot, and the others are aligned
    _fill(gpu, extra=True)
    recs, best = gpu.relocalizeScan(clouds[5][:600], s2m.default_reloc_params(query_max_dist=10000000.0, **dict(FIX, loop_search_num=0)))
    assert recs[0].hit.key == 32 and recs[0].hit.dist == 0.0
    assert (recs[0].status, recs[0].n_tgt < 1000, recs[0].icp.iterations) == (FEW, True, 0)
    assert all(r.status in (A, RJ) and r.icp.iterations > 0 for r in recs[1:]) and len(recs) > 1
    # a scan of 200 points: every record TOO_FEW_POINTS
    recs, best = gpu.relocalizeScan(scan[:: max(1, len(scan) // 200)][:200], s2m.default_reloc_params(query_max_dist=10000000.0, **FIX))
    assert len(recs) == 4 and best == -1 and all(r.status == FEW and r.n_src <= 200 and r.n_tgt == 0 for r in recs)
    # no hits
    assert gpu.relocalizeScan(scan, s2m.default_reloc_params(query_max_dist=1e-9, **FIX)) == ([], -1)
    # an empty scan: no records
    assert gpu.relocalizeScan(np.zeros((0, 8), F), prm) == ([], -1)
    # bad parameters
    for bad in (dict(query_top_k=9), dict(query_top_k=0), dict(loop_icp_leaf=0.0), dict(loop_search_radius=-1.0)):
        with pytest.raises(s2m.S2MError):
            gpu.relocalizeScan(scan, s2m.default_reloc_params(**dict(FIX, **bad)))
    # the ScanContext store one key longer than the key-frame store: a hit on the extra key is an error
    _fill(gpu, extra_sc=True)
    out = (s2m.RelocCandidate * 8)()
    n, b = C.c_int32(7), C.c_int32(7)
    q = np.ascontiguousarray(clouds[5][:600], F)
    assert gpu.lib.s2m_relocalize_scan(gpu.h, q.ctypes.data, len(q), 32, 0, C.byref(prm), out, C.byref(n), C.byref(b)) == -1
    assert (n.value, b.value) == (0, -1) and b"out of step" in gpu.lib.s2m_last_error(gpu.h)
    recs, best = gpu.relocalizeScan(scan, s2m.default_reloc_params(query_count=32, **FIX))     # the keys both stores hold still work
    assert best == 0 and recs[0].hit.key == 8


def test_busy_while_a_verification_is_pending(gpu):
    scan, _ = M.query_scan("Q1")
    _fill(gpu)
    prm = s2m.default_reloc_params(**FIX)
    lp = s2m.default_loop_params(search_radius=15.0, search_num=2, icp_leaf=0.5)
    early, _ = gpu.loopVerifyLaunch(31, [0, 16], -1, lp)
    assert [e.status for e in early] == [s2m.S2M_LOOP_PENDING] * 2
    out = (s2m.RelocCandidate * 8)()
    n, b = C.c_int32(7), C.c_int32(7)
    a = np.ascontiguousarray(scan, F)
    assert gpu.lib.s2m_relocalize_scan(gpu.h, a.ctypes.data, len(a), 32, 0, C.byref(prm), out, C.byref(n), C.byref(b)) == s2m.S2M_ERR_BUSY
    assert (n.value, b.value) == (7, 7)                    # touched nothing
    got, best = gpu.loopVerifyCollect()
    assert len(got) == 2
    recs, best = gpu.relocalizeScan(scan, prm)
    assert best == 0 and recs[0].hit.key == 8 and recs[0].status == A


def test_relocalisation_is_read_only(gpu, twin, cfg_small):
    scan, _ = M.query_scan("Q2")
    prm = s2m.default_reloc_params(**FIX)
    lp = s2m.default_loop_params(search_radius=15.0, search_num=2, icp_leaf=0.5)
    out = []
    for g, with_call in ((twin, False), (gpu, True)):
        _fill(g)
        if with_call:
            recs, best = g.relocalizeScan(scan, prm)
            assert best >= 0
        lid, yaw, match = g.detectLoopClosureID()
        ver, vbest = g.loopVerify(31, [16, 0, 2], -1, lp)
        out.append((lid, yaw, _bytes(match), [_bytes(v) for v in ver], vbest, g.kfSize(), g.scSize()))
    assert out[0] == out[1] and out[0][4] >= 0
    # a registration beside it, on the fixture of test_registration_after_the_map_calls_is_unchanged (tests/test_global_map_gpu.py)
    rng = np.random.default_rng(13)
    sc = synth.to_xyzi(cfg_small["scan"])
    mp = synth.to_xyzi(cfg_small["map"])
    k = 6
    parts = np.array_split(mp, k)
    results = []
    for with_call in (False, True):
        g = s2m.MapOptimizationS2M()
        try:
            for i in range(k):
                g.saveKeyFrame(np.zeros(6, F), float(i), parts[i])
                g.makeAndSaveScancontextAndKeys(parts[i])
            g.extractSurroundingKeyFrames(float(k), s2m.default_kf_params(map_leaf=0.4))
            g.downsampleCurrentScan(sc, 0.4)
            if with_call:
                recs, best = g.relocalizeScan(sc, s2m.default_reloc_params(query_max_dist=10000000.0, loop_search_num=k, loop_icp_leaf=0.4))
                print("beside the registration:", [(r.hit.key, r.status, r.n_src, r.n_tgt, r.icp.iterations) for r in recs], best)
                assert len(recs) == 4 and any(r.icp.iterations > 0 for r in recs)       # the alignment ran
                assert g.kfSize() == k and g.scSize() == k
            g.transformTobeMapped = cfg_small["pose_init"].copy()
            r = g.scan2MapOptimization()
            g.saveKeyFrame(np.zeros(6, F), float(k), None)                # scan_ds as the downsample left it
            results.append((_bytes(r), g.extractSurroundingKeyFrames(float(k)).tolist(), g.globalMapCloud(k, 1, 0.0).tobytes()))
        finally:
            g.close()
    assert results[0] == results[1]


# ---- part C: the local map around a given position ---------------------------------------------------------

def _cloud(rng, n):
    c = synth.to_xyzi(rng.uniform(-30, 30, (n, 3)).astype(F))
    c[:, 4] = rng.uniform(0, 100, n).astype(F)
    return c


def _circle(n, seed=0):
    """n keys on a 20 m circle driven round and round (the store of tests/test_global_map_gpu.py)."""
    rng = np.random.default_rng(seed)
    a = np.arange(n) * 0.05
    xyz = np.c_[20 * np.cos(a), 20 * np.sin(a), 0.2 * np.sin(3 * a)] + rng.normal(0, 0.3, (n, 3))
    return np.c_[xyz, rng.normal(0, 0.05, (n, 3))].astype(F)


def _line(n=6000):
    """The line store of test_extract_surrounding_big_store_few_candidates: more keys than the tile, few of them near any point."""
    poses = np.zeros((n, 6), F)
    poses[:, 0] = (np.arange(n, dtype=F) - F(n - 1)) * F(0.5)
    poses[:, 1] = 0.2 * np.sin(0.1 * np.arange(n))
    return poses


def _store(g, poses, clouds):
    g.kfReset()
    for k in range(poses.shape[0]):
        g.saveKeyFrame(poses[k], float(k), clouds[k % len(clouds)])


def _compose(g, poses, clouds, keys, leaf):
    parts = [g.transformPointCloud(clouds[k % len(clouds)], poses[k]) for k in keys]
    cat = np.concatenate(parts) if parts else np.zeros((0, 8), F)
    return g.voxelGrid(cat, leaf) if cat.shape[0] else cat


@pytest.fixture(scope="module")
def stores():
    rng = np.random.default_rng(1)
    clouds = [_cloud(rng, 40) for _ in range(5)]
    return {"circle300": (_circle(300, seed=300), clouds), "circle6000": (_circle(6000, seed=6000), clouds), "line6000": (_line(), clouds[:1])}


@pytest.mark.parametrize("which", ["circle300", "circle6000"])
def test_at_the_newest_key_is_the_existing_extraction(gpu, stores, which):
    poses, clouds = stores[which]
    n = poses.shape[0]
    _store(gpu, poses, clouds)
    if n > 4096:
        assert (np.linalg.norm(poses[:, :3] - poses[-1, :3], axis=1) < 50).sum() > 4096        # the device-wide sort
    for D in (2.0, 1.0):
        prm = s2m.default_kf_params(density=D, map_leaf=0.5, recent_window_s=0.0)
        keys, m = gpu.extractSurroundingKeyFrames(float(n - 1), prm, return_map=True)
        keys_at, m_at = gpu.extractSurroundingKeyFramesAt(poses[-1, :3], prm, return_map=True)
        assert keys_at.tolist() == keys.tolist() and len(keys) > 0
        assert keys_at.tolist() == M.select_at(poses[:, :3], poses[-1, :3], 50.0, D)
        _same(m_at, m)


@pytest.mark.parametrize("which", ["circle300", "line6000", "circle6000"])
def test_a_centre_that_is_no_key(gpu, stores, which):
    poses, clouds = stores[which]
    n = poses.shape[0]
    _store(gpu, poses, clouds)
    if which == "line6000":
        c = np.array([poses[3000, 0] + 0.13, 10.0, 0.0], F)           # 10 m off the line, mid-way: wide scan, few candidates
    elif which == "circle300":
        c = np.zeros(3, F)                                            # the centre of the circle
    else:
        c = np.array([1.5, -2.5, 0.1], F)                             # every key a candidate: wide scan, device-wide sort
    assert np.linalg.norm(poses[:, :3] - c, axis=1).min() > 5.0
    for D in (2.0, 1.0):
        prm = s2m.default_kf_params(density=D, map_leaf=0.5)
        keys, m = gpu.extractSurroundingKeyFramesAt(c, prm, return_map=True)
        want = M.select_at(poses[:, :3], c, 50.0, D)
        assert keys.tolist() == want and len(want) > 0, (which, D)
        if which == "line6000":                                       # (on the circles every key is a candidate from anywhere inside)
            assert keys.tolist() != M.select_at(poses[:, :3], poses[-1, :3], 50.0, D)
        _same(m, _compose(gpu, poses, clouds, want, 0.5))
    # installed as the local map with its index: the next extraction around the newest key replaces it
    assert gpu.laserCloudSurfFromMapDSNum == m.shape[0]


def test_boundary_store_capacity_and_errors(gpu):
    P, c = free_centre_store()
    cloud = _cloud(np.random.default_rng(4), 30)
    gpu.kfReset()
    n_out, n_keys = C.c_size_t(5), C.c_size_t(5)
    cp = c.ctypes.data_as(C.POINTER(C.c_float))
    kk = np.zeros(8, np.int32)
    kp = kk.ctypes.data_as(C.POINTER(C.c_int32))
    # the empty store: S2M_OK, nothing changes
    assert gpu.lib.s2m_extract_surrounding_at(gpu.h, cp, None, None, 32, 0, C.byref(n_out), kp, 8, C.byref(n_keys)) == s2m.S2M_OK
    assert (n_out.value, n_keys.value) == (0, 0)
    for k in range(P.shape[0]):
        gpu.saveKeyFrame(np.r_[P[k], 0, 0, 0].astype(F), 0.0, cloud)
    prm = s2m.default_kf_params(search_radius=BOUNDARY_R, density=BOUNDARY_D, map_leaf=0.5)
    keys = gpu.extractSurroundingKeyFramesAt(c, prm)
    assert keys.tolist() == M.select_at(P, c, BOUNDARY_R, BOUNDARY_D) and sorted(keys.tolist()) == [0, 1, 6]
    # capacity: the first cap records / keys and S2M_ERR_CAPACITY, the full counts, the map installed
    keys, full = gpu.extractSurroundingKeyFramesAt(c, prm, return_map=True)
    out = np.zeros((full.shape[0] - 1, 8), F)
    rc = gpu.lib.s2m_extract_surrounding_at(gpu.h, cp, C.byref(prm), out.ctypes.data, 32, out.shape[0], C.byref(n_out), kp, 8, C.byref(n_keys))
    assert rc == s2m.S2M_ERR_CAPACITY and n_out.value == full.shape[0] and n_keys.value == 3
    _same(out, full[:-1])
    rc = gpu.lib.s2m_extract_surrounding_at(gpu.h, cp, C.byref(prm), None, 32, 0, C.byref(n_out), kp, 2, C.byref(n_keys))
    assert rc == s2m.S2M_ERR_CAPACITY and kk[:2].tolist() == keys[:2].tolist() and n_keys.value == 3
    # a map leaf far too small for the extent: PCL hands the concatenation through
    tiny = s2m.default_kf_params(search_radius=BOUNDARY_R, density=BOUNDARY_D, map_leaf=1e-6)
    k2, m2 = gpu.extractSurroundingKeyFramesAt(c, tiny, return_map=True)
    assert gpu.leaf_too_small and m2.shape[0] == 30 * len(k2)
    # errors: a centre that is not finite, a null centre, bad parameters
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        b = np.array(bad, F)
        assert gpu.lib.s2m_extract_surrounding_at(gpu.h, b.ctypes.data_as(C.POINTER(C.c_float)), None, None, 32, 0, C.byref(n_out), None, 0, None) == -1
    assert gpu.lib.s2m_extract_surrounding_at(gpu.h, None, None, None, 32, 0, C.byref(n_out), None, 0, None) == -1
    badp = s2m.default_kf_params(density=0.0)
    assert gpu.lib.s2m_extract_surrounding_at(gpu.h, cp, C.byref(badp), None, 32, 0, C.byref(n_out), None, 0, None) == -1
    # recent_window_s is ignored, whatever it holds
    odd = s2m.default_kf_params(search_radius=BOUNDARY_R, density=BOUNDARY_D, map_leaf=0.5, recent_window_s=float("nan"))
    assert gpu.extractSurroundingKeyFramesAt(c, odd).tolist() == keys.tolist()


# ---- end to end -------------------------------------------------------------------------------------------------

def test_localize_in_the_stored_map_then_register(gpu):
    scan, true = M.query_scan("Q1")
    _fill(gpu)
    pose, recs, best = gpu.localizeInStoredMap(scan, s2m.default_reloc_params(**FIX))
    assert best == 0 and recs[best].hit.key == 8
    assert list(pose) == list(recs[best].pose_tobemapped) and list(gpu.transformTobeMapped) == list(pose)
    assert gpu.laserCloudSurfFromMapDSNum > 1000
    gpu.downsampleCurrentScan(scan, 0.4)
    r = gpu.scan2MapOptimization()
    final = np.r_[gpu.transformTobeMapped[3:6], gpu.transformTobeMapped[0:3]]
    pe, ye = M.pose_error(final, true)
    print("registration from the relocalised pose: iters", r.iters_run, "converged", r.converged, "skipped", r.skipped, "pose error", pe, ye)
    assert r.skipped == 0 and r.iters_run > 0 and r.converged
    assert pe < POS_BAR and ye < YAW_BAR
