"""The preparation of a single scan in fewer launches: the cell scan inside the scatter, the density
wishes chunk by chunk without a wave table in front of them, the state upload in the density kernel's launch.  Bar: what the
new chain leaves - qperm, qx/qy/qz, chunk_parts, chunk_factor before it is consumed, the final wave table and its length -
is BYTE FOR BYTE what the six-kernel chain (the one a scan slot of a batch still runs) leaves, through the observation hook
s2m_debug_scan_prep, which runs either chain on the resident scan."""
import numpy as np
import pytest

from liorf_amd import s2m, synth

pytestmark = pytest.mark.gpu

FIELDS = ("qperm", "qxyz", "chunk_parts", "chunk_factor", "wave_table")


def _same(a: dict, b: dict, what):
    assert a["n_waves"] == b["n_waves"] and a["n_waves"] > 0, (what, a["n_waves"], b["n_waves"])
    for k in FIELDS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _second_pose(pose):
    p = np.array(pose, np.float32).copy()
    p[2] += np.float32(np.deg2rad(1.0))       # yaw
    p[3] += np.float32(0.5)
    return p


def _both_chains(gpu, scan, poses, what):
    """Either chain on the resident scan, with and without the density pass; returns the new chain's last result."""
    gpu.setScan(scan)
    as_set = gpu.scanPrep(s2m.S2M_DEBUG_PREP_READ)                  # what s2m_set_scan itself left
    new0 = gpu.scanPrep(s2m.S2M_DEBUG_PREP_NEW)                     # ordering only; the table is built on demand for the read-out
    old0 = gpu.scanPrep(s2m.S2M_DEBUG_PREP_LEGACY)
    _same(new0, old0, (what, "ordering"))
    assert as_set["n_waves"] == -1                                  # no table until something needs one
    for k in ("qperm", "qxyz", "chunk_parts"):
        assert as_set[k].tobytes() == old0[k].tobytes(), (what, "set_scan", k)
    assert not old0["chunk_factor"].any()
    new = None
    for j, pose in enumerate(poses):
        new = gpu.scanPrep(s2m.S2M_DEBUG_PREP_NEW, pose)
        old = gpu.scanPrep(s2m.S2M_DEBUG_PREP_LEGACY, pose)
        _same(new, old, (what, "pose", j))
        # a permutation, and a table that covers every point once
        assert np.array_equal(np.sort(new["qperm"]), np.arange(scan.shape[0], dtype=np.int32)), what
        t = new["wave_table"]
        assert t[:, 1].sum() == scan.shape[0] and (np.diff(t[:, 0]) > 0).all() and t[0, 0] == 0, what
        assert not gpu.scanPrep(s2m.S2M_DEBUG_PREP_READ)["chunk_factor"].any(), what      # consumed: zero between uses
    return new


@pytest.fixture(scope="module")
def small():
    cfg = synth.make_config("small")
    gpu = s2m.MapOptimizationS2M()
    gpu.setInputCloud(synth.to_xyzi(cfg["map"]))
    yield gpu, synth.to_xyzi(cfg["scan"]), (np.array(cfg["pose_init"], np.float32), _second_pose(cfg["pose_init"]))
    gpu.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 12000])
def test_new_chain_equals_the_six_kernels(small, n):
    gpu, scan, poses = small
    _both_chains(gpu, scan[:n], poses, n)


def test_non_finite_records(small):
    gpu, scan, poses = small
    s = scan[:4097].copy()
    s[0, 0] = np.nan
    s[1023, 1] = np.inf
    s[1024, :3] = (-np.inf, np.nan, 1.0)
    s[-1, 2] = np.nan
    _both_chains(gpu, s, poses, "non-finite")


def test_one_polar_cell(small):
    gpu, scan, poses = small
    rng = np.random.default_rng(5)
    s = np.zeros((2000, scan.shape[1]), np.float32)
    s[:, 0] = 10.0 + 0.01 * rng.random(2000)
    s[:, 1] = 0.01 * rng.random(2000)
    s[:, 2] = rng.uniform(-1.0, 1.0, 2000)
    r = _both_chains(gpu, s, poses, "one cell")
    assert np.unique(r["qperm"][:64]).size == 64


def _far_field(rng, n, width):
    """n points between 100 and 280 m, all around: every 64 of them span a box that asks for 4 parts"""
    rho, az = rng.uniform(100.0, 280.0, n), rng.uniform(-np.pi, np.pi, n)
    s = np.zeros((n, width), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = rho * np.cos(az), rho * np.sin(az), rng.uniform(-20.0, 20.0, n)
    return s


def test_far_field_cells(small):
    """16 000 points scattered over the far-field cells: a small scan, every chunk cut as finely as it goes (8 parts; a scan
    large enough for such chunks to ask for 4 is the first case of test_wishes_beyond_the_table_capacity)"""
    gpu, scan, poses = small
    r = _both_chains(gpu, _far_field(np.random.default_rng(6), 16000, scan.shape[1]), poses, "far field")
    assert r["chunk_parts"].min() == 8 and (r["wave_table"][:-1, 1] == 8).all()


# The wishes CAN exceed the table: scan_slot_prepare gives a scan of more than 65 536 points (base_parts 1) 1.5 entries per chunk,
# and k_chunk_parts asks for 4 where a chunk's box is large; with base_parts 2 the table has 2.5 entries per chunk and the wishes
# go up to 8.  far: the share of far-field points; the cap the extent-only table then takes is 8, 4, 2 or 1.
@pytest.mark.parametrize("n,far,cap", [(70000, 1.0, 1), (70000, 0.3, 2), (40000, 0.2, 4), (70000, 0.1, 8)])
def test_wishes_beyond_the_table_capacity(small, n, far, cap):
    gpu, scan, poses = small
    rng = np.random.default_rng(7)
    s = np.concatenate([scan[rng.integers(0, scan.shape[0], n - int(n * far))] + np.float32(0.001) * rng.standard_normal((n - int(n * far), scan.shape[1])).astype(np.float32),
                        _far_field(rng, int(n * far), scan.shape[1])])
    s = np.ascontiguousarray(s[rng.permutation(n)])
    r = _both_chains(gpu, s, poses[:1], ("capacity", n, far))
    parts = r["chunk_parts"]
    nc, base = parts.size, (1 if n > 65536 else 2)
    up = lambda a, b: (a + b - 1) // b
    capacity = up(up(nc * base + nc // 2, 8), 8) * 8 * 8                # scan_slot_prepare: workgroups of 8 waves, in steps of 8
    totals = {c: int(np.minimum(parts, c).sum()) for c in (8, 4, 2, 1)}
    want = next((c for c in (8, 4, 2) if totals[c] <= capacity), 1)
    assert want == cap, (totals, capacity)                              # the case is the one it claims to be
    if cap < 8:
        assert totals[8] > capacity
    if far == 1.0:
        assert (parts == 4).all()                                       # every chunk asks for p = 4


def test_dense_map_asks_for_finer_cuts():
    """a compact scan inside a small dense map: the boxes of its entries hold thousands of map points, chunk_factor > 1"""
    rng = np.random.default_rng(8)
    m = np.zeros((30000, 4), np.float32)
    m[:, :3] = rng.uniform((-3.0, -3.0, -1.0), (3.0, 3.0, 1.0), (30000, 3))
    s = np.zeros((40000, 4), np.float32)
    s[:, :3] = rng.uniform((-2.5, -2.5, -0.8), (2.5, 2.5, 0.8), (40000, 3))
    pose = np.array([0.0, 0.0, 0.01, 0.05, -0.03, 0.0], np.float32)
    gpu = s2m.MapOptimizationS2M()
    gpu.setInputCloud(m)
    r = _both_chains(gpu, s, (pose, _second_pose(pose)), "dense")
    assert r["chunk_factor"].max() > 1
    gpu.close()


def test_empty_scan_stays_a_no_op(small):
    gpu, scan, poses = small
    gpu.setScan(scan[:0])
    assert gpu.scanPrep(s2m.S2M_DEBUG_PREP_NEW, poses[0])["n_waves"] == 0
    gpu.transformTobeMapped = poses[0].copy()
    r = gpu.scan2MapOptimization()
    assert r.skipped == 2 and r.iters_run == 0
