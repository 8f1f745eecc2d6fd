"""The registration path (k_register, k_certify_lean, the map index, plane_fit_5x3) at its edges, against the oracle: the
scenes of tests/test_register_edges_cpu.py, whose companions show that each scene has its edge and that the oracle there
is the numpy statement.  The comparison is _check of tests/test_tiers_gpu.py: gate decision, indices, d2 bits, flag and
coeff bits.  Scenes with ties run on two fresh handles (the order inside a cell of map_sorted comes from atomics).
PARITY UNPINNED beyond the kNN (oracle/s2m_oracle.h)."""
import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O
from test_register_edges_cpu import (FACE_OFFSETS, FLIP_STEPS, GATES, NEAR_K, NONDEFAULT_GATES, OUTLIERS, clump_scene, coarse_scene,
                                     face_scene, flip_poses, flip_scene, gate_scene, near_tie_scene, plane_scene, room_scene,
                                     tie_scene)
from test_tiers_gpu import _check

pytestmark = pytest.mark.gpu

ABLATE = ["0", "1", "2", "3", "64", "128"]


def _pair(sc, knn_backend=0):
    gpu = s2m.MapOptimizationS2M(gate_sq=sc["gate_sq"])
    gpu.setInputCloud(sc["map"])
    gpu.setScan(sc["scan"])
    orc = O.Oracle(knn_backend=knn_backend, num_threads=8, gate_sq=sc["gate_sq"])
    orc.set_map(sc["map"])
    orc.set_scan(sc["scan"])
    return gpu, orc


def _walk(sc, poses, handles=2, knn_backend=0):
    """Every pose on `handles` fresh handles: cold, then warm (the same pose again), then the rest of the walk."""
    for _ in range(handles):
        gpu, orc = _pair(sc, knn_backend)
        _check(gpu, orc, poses[0])
        for p in poses:
            _check(gpu, orc, p)
        gpu.close()
        orc.close()


def _shift(dx, base=None):
    p = np.zeros(6, np.float32) if base is None else np.asarray(base, np.float32).copy()
    p[3] = np.float32(p[3] + np.float32(dx))
    return p


@pytest.mark.parametrize("ablate", ABLATE)
@pytest.mark.parametrize("gate_sq", GATES)
def test_fifth_neighbour_on_the_gate(monkeypatch, gate_sq, ablate):
    """The 5th at prev(g), g, next(g); then the walk that moves it across the gate in 1-ulp, 1 um and 1 mm steps."""
    monkeypatch.setenv("S2M_ABLATE", ablate)
    sc = gate_scene(gate_sq)
    ulp = 2.0 ** -18
    poses = [_shift(0.0)] + [_shift(k * ulp) for k in (1, 2, -1, -2, 3, 0)] + \
            [_shift(k * 1e-6) for k in (1, 3, -2, 5)] + [_shift(k * 1e-3) for k in (1, -1, 2, 0)]
    _walk(sc, poses)


@pytest.mark.parametrize("gate_sq", NONDEFAULT_GATES)
def test_non_default_gate_pose_walk(cfg_small, monkeypatch, gate_sq):
    for ablate in ("0", "3", "64", "128"):
        monkeypatch.setenv("S2M_ABLATE", ablate)
        sc = dict(map=cfg_small["map"], scan=cfg_small["scan"][:4000], gate_sq=gate_sq)
        rng = np.random.default_rng(3)
        p = cfg_small["pose_init"].astype(np.float32)
        poses = [p]
        for scale in (0.0, 0.02, 1e-3, 1e-5, 0.3, 1e-4):
            d = rng.normal(0, 1, 6).astype(np.float32) * np.float32(scale) * np.array([0.03, 0.03, 0.03, 1, 1, 1], np.float32)
            poses.append((poses[-1] + d).astype(np.float32))
        _walk(sc, poses, handles=1, knn_backend=1)


@pytest.mark.parametrize("gate_sq", NONDEFAULT_GATES)
def test_non_default_gate_dense_clump(cfg_small, monkeypatch, gate_sq):
    """The scene of test_dense_clump_and_scattered_queries_under_every_path under other gates (100: 10 m cells, every
    search overflows its tile)."""
    sc = clump_scene(cfg_small, gate_sq)
    for ablate in ("0", "64", "128", "3"):
        monkeypatch.setenv("S2M_ABLATE", ablate)
        p = sc["pose"]
        poses = []
        for step in (0.0, 1e-3, 0.05, 1e-5, 0.5):
            p = (p + np.float32(step)).astype(np.float32)
            poses.append(p)
        _walk(sc, poses, handles=1, knn_backend=1)


def _loop(cfg, ablate, monkeypatch, gate_sq):
    monkeypatch.setenv("S2M_ABLATE", ablate)
    g = s2m.MapOptimizationS2M(gate_sq=gate_sq)
    g.setInputCloud(cfg["map"])
    r = g.optimize(cfg["scan"], cfg["pose"] if "pose" in cfg else cfg["pose_init"])
    tr = g.trace()
    out = (r.iters_run, r.converged, r.n_sel_last, np.array(r.pose, np.float32),
           np.array([t.n_sel for t in tr]), np.array([t.pose[:] for t in tr], np.float32),
           np.array([t.delta[:] for t in tr], np.float32), tr, r.is_degenerate)
    g.close()
    return out


def _loop_bars(cfg, monkeypatch, gate_sq):
    """Across ablate 0/1/2 bitwise the loop of ablate 3; against the oracle by the bars of
    test_lm_loop_pose_delta_per_iteration."""
    ref = _loop(cfg, "3", monkeypatch, gate_sq)
    for ablate in ("0", "1", "2"):
        got = _loop(cfg, ablate, monkeypatch, gate_sq)
        assert got[:3] == ref[:3] and got[8] == ref[8], (ablate, got[:3], ref[:3])
        assert np.array_equal(got[4], ref[4]), ablate
        for k in (3, 5, 6):
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (ablate, k)
    orc = O.Oracle(knn_backend=1, num_threads=8, gate_sq=gate_sq)
    orc.set_map(cfg["map"])
    orc.set_scan(cfg["scan"])
    ro = orc.scan2MapOptimization(cfg["pose"] if "pose" in cfg else cfg["pose_init"])
    assert (ref[0], ref[1], ref[8]) == (ro.iters_run, ro.converged, ro.is_degenerate)
    to = orc.trace()
    assert len(to) == len(ref[7]) == ref[0]
    for a, b in zip(ref[7], to):
        assert abs(a.n_sel - b.n_sel) <= max(3, int(2e-4 * b.n_sel))
        da, db = np.array(a.delta), np.array(b.delta)
        assert np.abs(da[:3] - db[:3]).max() <= 1e-4
        assert np.abs(da[3:] - db[3:]).max() <= 1e-4
    assert np.abs(ref[3] - np.array(ro.pose)).max() <= 1e-4
    orc.close()


@pytest.mark.parametrize("gate_sq", [0.25, 4.0])
def test_non_default_gate_lm_loop(cfg_small, monkeypatch, gate_sq):
    _loop_bars(cfg_small, monkeypatch, gate_sq)


@pytest.mark.parametrize("k", NEAR_K)
def test_near_ties_below_the_key_resolution(monkeypatch, k):
    sc = near_tie_scene(k)
    poses = [_shift(0.0), _shift(2.0 ** -18), _shift(1e-4), _shift(0.0)]
    for ablate in ABLATE:
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, poses)


def test_exact_ties_and_duplicates(monkeypatch):
    sc = tie_scene()
    poses = [_shift(0.0), _shift(2.0 ** -18), _shift(0.003), _shift(0.0)]
    for ablate in ABLATE:
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, poses)
    gpu, orc = _pair(sc)                               # the same map installed again on one handle
    for rep in range(2):
        gpu.setInputCloud(sc["map"])
        for p in poses:
            _check(gpu, orc, p)
    gpu.close()
    orc.close()


def test_plane_fit_degeneracies(monkeypatch):
    """Hundreds of crafted 5-point tuples, one query each: flag and coeff bit for bit (x86 and the device agree on
    subnormals, rank threshold, pivot ties)."""
    sc = plane_scene()
    for ablate in ("0", "3"):
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, [np.zeros(6, np.float32), _shift(2.0 ** -30)], handles=1)


@pytest.mark.parametrize("offset", FACE_OFFSETS)
def test_cell_faces(monkeypatch, offset):
    sc = face_scene(offset)
    ulp = 2.0 ** -17 if offset[0] == 0 else 2.0 ** -9
    poses = [_shift(0.0), _shift(ulp), _shift(-ulp), _shift(1e-3), _shift(0.0)]
    for ablate in ABLATE:
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, poses, handles=1)


@pytest.mark.parametrize("far", OUTLIERS)
def test_grid_coarsening(cfg_tiny, monkeypatch, far):
    sc = coarse_scene(cfg_tiny, far)
    p = sc["pose"]
    poses = [p, _shift(1e-4, p), _shift(0.02, p)]
    for ablate in ("0", "3", "64"):
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, poses, handles=1, knn_backend=1)


def test_map_that_cannot_be_gridded(cfg_tiny):
    """A finite point at 1e30: S2M_ERR_CAPACITY, the handle then has no map (skipped == 1), and a good map after that
    gives the oracle's results again."""
    m = synth.to_xyzi(cfg_tiny["map"])
    bad = np.concatenate([m, np.array([[1e30] + [0.0] * (m.shape[1] - 1)], np.float32)])
    gpu = s2m.MapOptimizationS2M()
    gpu.setInputCloud(m)
    gpu.setScan(synth.to_xyzi(cfg_tiny["scan"]))
    with pytest.raises(s2m.S2MError, match="S2M_ERR_CAPACITY"):
        gpu.setInputCloud(bad)
    gpu.transformTobeMapped = cfg_tiny["pose_init"].copy()
    r = gpu.scan2MapOptimization()
    assert r.skipped == 1 and r.iters_run == 0
    gpu.setInputCloud(m)
    orc = O.Oracle(knn_backend=0, num_threads=8)
    orc.set_map(m)
    orc.set_scan(synth.to_xyzi(cfg_tiny["scan"]))
    _check(gpu, orc, cfg_tiny["pose_init"])
    gpu.close()
    orc.close()


@pytest.mark.parametrize("step", FLIP_STEPS)
def test_certificate_flip_flop(monkeypatch, step):
    sc = flip_scene()
    poses = flip_poses(step)
    for ablate in ("0", "1", "2", "3"):
        monkeypatch.setenv("S2M_ABLATE", ablate)
        _walk(sc, poses)


def test_lattice_room_loop(monkeypatch):
    _loop_bars(room_scene(), monkeypatch, 1.0)
