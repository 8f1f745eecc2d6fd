"""The stage between the plane fit and the LM close on the device - residual weight, Jacobian row (:1216-1234), the 28
products, the wave reduction (permlane swaps, two batches of 14, entries with fewer than 64 live lanes) and the workgroup's
partial row - held sum by sum against the float statement of tests/ref/lm_rows_ref.py, at attitudes of tens of degrees.

s2m_debug_lm_rows hands back the partial rows one registration launch wrote and the wave table it read.  Every sum of every
row has to lie within `bound` of `exact` (expected_rows: the exactly rounded sum of the kept points' products, and the worst
case of the row's fp64 additions in any order, doubled - derived, about 1 000 times below what one fp32 ulp in one Jacobian
entry does to a sum), computed from the device's own flag / coeff4, so that only this stage is under test; the counts are equal
as integers.  tests/test_lm_rows_cpu.py shows that every single-term mutation of the Jacobian breaks this bar, and that the
allclose bar of test_parity_gpu.py::test_normal_equations does not see a sign flip at the suite's one attitude.

Shapes seen on the MI355X (asserted from what the hook reports; active rows x waves per workgroup, entries at launch 0):
  tiny 2 000 points                    32 x 8, 256 entries of 8 lanes
  small 12 000 points                  188 x 8, 1 504 entries of 8 lanes, the last ones empty (188 chunks are still cut in
                                       eight; launches 1, 2, 5 read the same 1 504 after the density re-split)
  20 000 points                        168 x 8, 1 344 entries: 1 158 of 16 lanes (a chunk is cut in four from 16 385 points
                                       on), 184 of 8, 2 empty
  140 037 points                       140 x 16, 2 240 entries: full ones, and the last one 140 037 mod 64 = 5 lanes
  140 037 points, S2M_BIG_BLOCKS=0     256 x 8, the same 2 240 entries: several per wave
Largest |got - exact| / bound observed: 0.12 on tiny, 0.04 on small (all launches and switches), 0.004 at 140 037 points
(a record, not a tolerance).
"""
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import lm_close_cases as LC  # noqa: E402
import lm_rows_ref as LR  # noqa: E402
from test_tiers_gpu import _check  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(LR.ATTITUDES)
RECORD = {}                                                # shape -> largest |got - exact| / bound seen, printed at the end


def _handle(cfg, **params):
    g = s2m.MapOptimizationS2M(**params)
    g.setInputCloud(synth.to_xyzi(cfg["map"]))
    g.setScan(synth.to_xyzi(cfg["scan"]))
    return g


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_rows(g, scan, rows, out, table, pose, trig=None, what=""):
    """The rows of one launch against the statement at `pose` (the pose the launch ran with), from the device's own flag and
    coeff4 there.  Returns (largest |got - exact| / bound, counts per row)."""
    n = scan.shape[0]
    _, _, flag, coeff = g.surfOptimization(pose)
    qperm = g.scanPrep(s2m.S2M_DEBUG_PREP_READ)["qperm"]
    assert sorted(qperm.tolist()) == list(range(n))
    assert rows.shape == (out.n_rows_active, 28) and table.shape == (out.n_waves, 2)
    assert out.n_rows_active == LR.active_rows(out.n_waves, out.wpb, out.nblocks) and out.done == 0
    mem = LR.row_members(table, out.n_waves, out.n_rows_active, n)
    assert sorted(np.concatenate(mem).tolist()) == list(range(n)), "the wave table does not cover the scan once"
    exact, bound, counts = LR.expected_rows(scan, coeff, flag, mem, qperm, pose=pose, trig=trig)
    kept = int(np.count_nonzero(flag))
    assert kept >= 0.2 * n, (what, kept)                   # a case without correspondences checks nothing: it fails
    ratio = LR.worst_ratio(rows, exact, bound)
    print(what, "rows", out.n_rows_active, "wpb", out.wpb, "nblocks", out.nblocks, "n_waves", out.n_waves, "kept", kept,
          "max |got - exact| / bound", ratio)
    assert np.array_equal(rows[:, 27], counts.astype(np.float64)), (what, "counts differ")
    assert int(counts.sum()) == kept
    assert np.all(np.abs(rows - exact) <= bound), (what, ratio)
    return ratio, counts


def check_launch0(g, scan, pose, what):
    """Test a on one pose: the rows of the first launch of a scan, and the close of s2m_normal_eq on those rows."""
    g.surfOptimization(pose)
    rows, out, table = g.lmRows(pose, 0)
    assert np.array_equal(np.array(out.pose_used, F32).view(np.uint32), np.asarray(pose, F32).view(np.uint32))
    ratio, counts = check_rows(g, scan, rows, out, table, pose, what=what)
    AtA, AtB, n_sel = g.normal_eq(pose)
    assert n_sel == int(counts.sum())
    lo, hi = LC.inexact_bounds(rows)
    iAtA, iAtB, _ = LC.intended(rows)
    got = np.array([AtA[a, b] for a, b in LC.UT] + list(AtB), F32)
    want = np.array([iAtA[a, b] for a, b in LC.UT] + list(iAtB), F32)
    exact = lo.view(np.uint32) == hi.view(np.uint32)       # the fp64 order of the close cannot move the fp32 value
    assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), what
    assert np.all(got >= lo) and np.all(got <= hi), what
    assert np.array_equal(AtA.view(np.uint32), AtA.T.copy().view(np.uint32))
    return ratio, out, table


def _note(shape, ratio):
    RECORD[shape] = max(RECORD.get(shape, 0.0), ratio)
    print("RECORD", shape, RECORD[shape])


# ---- a. rows of launch 0 at every attitude ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_of_launch_0(cfg_tiny, name):
    """Per attitude at the start pose (attitude + POSE_DELTA) and at the attitude itself (the two edge attitudes put
    pitch within 1e-3 of pi / 2 and yaw at nextafter(pi, 0) into sinf / cosf as they stand)."""
    cfg = LR.at_attitude(cfg_tiny, LR.ATTITUDES[name])
    g = _handle(cfg)
    try:
        for which in ("pose_init", "pose_gt"):
            ratio, out, table = check_launch0(g, cfg["scan"], cfg[which], f"tiny/{name}/{which}")
            _note("tiny", ratio)
    finally:
        g.close()
    if name == "pitch_edge":
        assert abs(float(cfg["pose_gt"][1]) - np.pi / 2) < 1e-3
    if name == "yaw_edge":
        assert cfg["pose_gt"][2] == np.nextafter(F32(np.pi), F32(0))


# ---- b. shapes ----------------------------------------------------------------------------------------------------------
def test_shape_tiny_eight_lane_entries(cfg_tiny):
    g = _handle(cfg_tiny)
    try:
        _, out, table = check_launch0(g, cfg_tiny["scan"], cfg_tiny["pose_init"], "shape/tiny")
        assert out.wpb == 8 and table[:, 1].max() == 8 and out.n_waves <= out.n_rows_active * out.wpb
    finally:
        g.close()


@pytest.mark.parametrize("name", ["gt", "a"])
def test_shape_small_empty_entries(cfg_small, name):
    """12 000 points are 188 chunks, still cut in eight: 8-lane entries again, and behind the half-filled last chunk
    entries without a lane."""
    cfg = LR.at_attitude(cfg_small, LR.ATTITUDES[name])
    g = _handle(cfg)
    try:
        ratio, out, table = check_launch0(g, cfg["scan"], cfg["pose_init"], f"shape/small/{name}")
        _note("small", ratio)
        assert out.wpb == 8 and table[:, 1].max() == 8 and np.count_nonzero(table[:, 1] == 0) > 0
        assert out.n_waves <= out.n_rows_active * out.wpb
    finally:
        g.close()


@pytest.mark.parametrize("name", ["gt", "a"])
def test_shape_sixteen_lane_entries(cfg_small, name):
    """Between 16 385 and 32 768 points a chunk is cut in four: small's scan plus 8 000 of its points jittered by a
    millimetre, its map."""
    rng = np.random.default_rng(20000)
    s = cfg_small["scan"]
    extra = s[rng.choice(len(s), 8000, replace=False)] + rng.normal(0.0, 1e-3, (8000, 3))
    cfg = dict(cfg_small)
    cfg["scan"] = np.concatenate([s, extra.astype(F32)]).astype(F32)
    cfg = LR.at_attitude(cfg, LR.ATTITUDES[name])
    g = _handle(cfg)
    try:
        ratio, out, table = check_launch0(g, cfg["scan"], cfg["pose_init"], f"shape/20000/{name}")
        _note("20000", ratio)
        print("entry sizes", np.unique(table[:, 1], return_counts=True))
        assert out.wpb == 8 and table[:, 1].max() == 16 and np.count_nonzero(table[:, 1] == 16) > out.n_waves // 2
    finally:
        g.close()


@pytest.fixture(scope="module")
def cfg_140037(cfg_kitti64):
    """kitti64's scan plus 20 037 of its points jittered by a millimetre, its map."""
    rng = np.random.default_rng(140037)
    s = cfg_kitti64["scan"]
    extra = s[rng.choice(len(s), 20037, replace=False)] + rng.normal(0.0, 1e-3, (20037, 3))
    cfg = dict(cfg_kitti64)
    cfg["scan"] = np.concatenate([s, extra.astype(F32)]).astype(F32)
    assert cfg["scan"].shape[0] == 140037
    return cfg


@pytest.mark.parametrize("name", ["gt", "a"])
@pytest.mark.parametrize("big", ["1", "0"])
def test_shape_large(cfg_140037, monkeypatch, big, name):
    """Above 2 048 wave-table entries: 16-wave workgroups, full entries and a short last one; with S2M_BIG_BLOCKS=0 the same
    scan on 8-wave workgroups, where a wave walks several entries."""
    monkeypatch.setenv("S2M_BIG_BLOCKS", big)
    cfg = LR.at_attitude(cfg_140037, LR.ATTITUDES[name])
    n = cfg["scan"].shape[0]
    g = _handle(cfg)
    try:
        ratio, out, table = check_launch0(g, cfg["scan"], cfg["pose_init"], f"shape/140037/big{big}/{name}")
        _note("140037 big" + big, ratio)
        last = table[np.argmax(table[:, 0] + table[:, 1])]
        assert np.count_nonzero(table[:, 1] == 64) > 1000 and last[0] + last[1] >= n and 0 < n - last[0] < 64
        if big == "1":
            assert out.wpb == 16 and out.n_waves > 2048
        else:
            assert out.wpb == 8 and out.n_waves > out.n_rows_active * out.wpb
    finally:
        g.close()


# ---- c. roles -----------------------------------------------------------------------------------------------------------
SWITCHES = [{"S2M_SPLIT": "0"}, {"S2M_SPLIT": "1"}, {"S2M_SPLIT": "2"}, {"S2M_NO_FUSE": "1"}, {"S2M_SPLIT": "1", "S2M_NO_FUSE": "1"}]


@pytest.mark.parametrize("name", ["gt", "a"])
def test_rows_of_later_launches_under_every_role(cfg_small, monkeypatch, name):
    """Launches 1, 2 and 5 of a real loop: written by the fused kernel, by certify + search, closed in the prologue or by
    k_finalize - against the statement at the pose the launch ran with and the device's own trig, and the same bits under
    every switch."""
    cfg = LR.at_attitude(cfg_small, LR.ATTITUDES[name])
    first = None
    for env in SWITCHES:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            g = _handle(cfg, early_exit=0)               # a fresh handle: the switches are read at s2m_create
        try:
            got = {}
            for launch in (1, 2, 5):
                rows, out, table = g.lmRows(cfg["pose_init"], launch)
                used = np.array(out.pose_used, F32)
                assert np.all(np.isfinite(used)) and not np.array_equal(used, cfg["pose_init"])
                ratio, _ = check_rows(g, cfg["scan"], rows, out, table, used, trig=LR.device_trig(g, used), what=f"roles/{name}/{env}/launch{launch}")
                _note("roles", ratio)
                got[launch] = (_bits(rows), _bits(used), _bits(table))
            if first is None:
                first = got
            assert got == first, env
        finally:
            g.close()


# ---- d. the oracle at attitude --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tiny", "small"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_at_attitude(request, name, scene):
    """Search and plane fit bit for bit (test_tiers_gpu._check), cold and warm, and the whole loop with the bars of
    test_parity_gpu.py::test_lm_loop_pose_delta_per_iteration, unchanged, at every attitude.  (On the MI355X every bar held
    at every attitude - the deltas were the oracle's to the bit - so no pose needed a float64 recomputation.)"""
    cfg = LR.at_attitude(request.getfixturevalue("cfg_" + scene), LR.ATTITUDES[name])
    m, s = synth.to_xyzi(cfg["map"]), synth.to_xyzi(cfg["scan"])
    g = _handle(cfg)
    orc = O.Oracle(knn_backend=1, num_threads=8)
    try:
        orc.set_map(m)
        orc.set_scan(s)
        assert _check(g, orc, cfg["pose_init"]) > 0.5 * len(s)     # cold
        _check(g, orc, cfg["pose_gt"])                             # warm: certificates from the pose before
        _check(g, orc, cfg["pose_init"])
        g.setScan(s)                                               # the loop starts like a fresh scan
        g.transformTobeMapped = cfg["pose_init"].copy()
        r = g.scan2MapOptimization()
        ro = orc.scan2MapOptimization(cfg["pose_init"])
        tg, to = g.trace(), orc.trace()
        worst = [float(np.abs(np.array(a.delta) - np.array(b.delta)).max()) for a, b in zip(tg, to)]
        print(scene, name, "iters", r.iters_run, ro.iters_run, "n_sel", [(a.n_sel, b.n_sel) for a, b in zip(tg, to)], "max |delta - oracle|",
              worst, "max |pose - oracle|", float(np.abs(np.array(r.pose) - np.array(ro.pose)).max()))
        assert (r.iters_run, r.converged, r.is_degenerate) == (ro.iters_run, ro.converged, ro.is_degenerate)
        assert len(tg) == len(to) == r.iters_run
        for a, b in zip(tg, to):
            assert abs(a.n_sel - b.n_sel) <= max(3, int(2e-4 * b.n_sel))
            da, db = np.array(a.delta), np.array(b.delta)
            assert np.abs(da[:3] - db[:3]).max() <= 1e-4
            assert np.abs(da[3:] - db[3:]).max() <= 1e-4
        assert np.abs(np.array(r.pose) - np.array(ro.pose)).max() <= 1e-4
    finally:
        g.close()
        orc.close()


# ---- e. handle state ------------------------------------------------------------------------------------------------------
def test_the_handle_stays_usable(cfg_small):
    """The hook twice gives the same bits, and a registration after it - launch 0, later launches, another pose whose density
    re-split the hook's loop consumed - is the registration of a handle that never saw the hook, byte for byte."""
    m, s = synth.to_xyzi(cfg_small["map"]), synth.to_xyzi(cfg_small["scan"])
    other = LR.at_attitude(cfg_small, LR.ATTITUDES["a"])["pose_init"]     # (far from the map: another density picture)

    def register(g):
        g.transformTobeMapped = cfg_small["pose_init"].copy()
        r = g.scan2MapOptimization()
        return bytes(r), [bytes(t) for t in g.trace()]

    used, fresh = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        for g in (used, fresh):
            g.setInputCloud(m)
            g.setScan(s)
        used.setParams(early_exit=0)
        for pose, launch in ((cfg_small["pose_init"], 0), (cfg_small["pose_init"], 2), (other, 1), (cfg_small["pose_gt"], 5)):
            a, b = used.lmRows(pose, launch), used.lmRows(pose, launch)
            assert _bits(a[0]) == _bits(b[0]) and bytes(a[1]) == bytes(b[1]) and _bits(a[2]) == _bits(b[2]), launch
            assert np.count_nonzero(a[0][:, 27]) > 0 or launch > 0
        used.setParams(early_exit=1)
        assert register(used) == register(fresh)
        assert register(used) == register(fresh)
    finally:
        used.close()
        fresh.close()


def test_hook_refuses_what_it_cannot_observe(cfg_tiny):
    g = s2m.MapOptimizationS2M()
    try:
        with pytest.raises(s2m.S2MError, match="NO_SCAN"):
            g.lmRows(cfg_tiny["pose_init"], 0)
        g.setInputCloud(synth.to_xyzi(cfg_tiny["map"]))
        g.setScan(synth.to_xyzi(cfg_tiny["scan"]))
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):        # early_exit is on: the loop may end before launch 1
            g.lmRows(cfg_tiny["pose_init"], 1)
        g.setParams(early_exit=0, max_iter=5)
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):        # launch outside 0 .. max_iter-1 of the CURRENT parameters
            g.lmRows(cfg_tiny["pose_init"], 5)
        assert g.lmRows(cfg_tiny["pose_init"], 4)[1].n_rows_active > 0
        g.launch(cfg_tiny["pose_init"])
        with pytest.raises(s2m.S2MError, match="INVALID_ARG"):        # an optimise is pending
            g.lmRows(cfg_tiny["pose_init"], 0)
        g.collect()
        assert g.lmRows(cfg_tiny["pose_init"], 0)[1].n_rows_active > 0
    finally:
        g.close()
