"""CPU companions of tests/test_voxel_edges_gpu.py: the clouds those tests build (run lengths, radix tiles, key bits,
the INT32_MAX index range, voxel faces, the map frame) and the float64 numpy statement (numpy_voxel_grid,
tests/test_voxel_cpu.py) checked against the oracle on them.  PARITY UNPINNED."""
import numpy as np
import pytest

from liorf_amd import synth
from oracle import oracle as O
from test_voxel_cpu import numpy_voxel_grid, raw_cloud

RUN_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 39, 40, 41, 47, 48, 63, 64, 65, 96, 97, 255, 256, 257, 272, 511, 512, 513, 1023, 1024,
               1025, 1040, 2048, 2049]
MAP_OFFSETS = [(5000.0, -3000.0, 20.0), (20000.0, 8000.0, -50.0), (100000.0, 60000.0, 30.0)]


def blob_cloud(lengths, leaf, offset=(0.0, 0.0, 0.0), seed=3, n_background=3000):
    """(n, 8) records: for every m in `lengths` a voxel holding exactly m points (inside the middle 80 % of the voxel,
    so fp32 rounding cannot move one out), every other voxel 1-8 apart in z so that long runs sit at low and high
    output positions, among n_background points spread 1-3 per voxel over a box of their own; shuffled."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    base = np.floor(o / leaf)
    parts = []
    for k, m in enumerate(lengths):
        cell = base + np.array([4 + 2 * (k % 6), 4 + 2 * (k // 6), 2 + 9 * (k % 2)])
        p = (cell + rng.uniform(0.1, 0.9, (m, 3))) * leaf
        parts.append(p)
    bg = (base + np.array([-60, -60, -3]) + rng.uniform(0, [40, 40, 6], (n_background, 3))) * leaf
    xyz = np.concatenate(parts + [bg], 0).astype(np.float32)
    rec = synth.to_xyzi(xyz)
    rec[:, 4] = rng.uniform(0, 255, rec.shape[0]).astype(np.float32)
    return rec[rng.permutation(rec.shape[0])]


def with_stride(rec, stride):
    """The same points as contiguous records of `stride` bytes (12: xyz, 16: xyz + 1, 20: + intensity, 32: PointXYZI)."""
    return np.ascontiguousarray(rec[:, : stride // 4])


def tile_cloud(n, bad_at=(), seed=5):
    """raw_cloud(n) with NaN / +-inf records at the given positions (radix tiles are 4 096 keys, histogram rounds 1 024)."""
    rec = raw_cloud(n, seed=seed, with_bad=False)
    for k, i in enumerate(i for i in bad_at if i < n):
        rec[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    return rec


def sweep_cloud(n=200000, half=80.0, seed=7):
    """A +-80 m sweep, z in [-3, 12] m: at leaf 0.2 the index range is 800 x 800 x 75 = 4.8e7 > 2^22, at 0.4
    400 x 400 x 38 = 6.1e6 > 2^22, so the third radix pass (bits 22..31) sorts real digits."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-half, -half, -3.0], [half, half, 12.0], (n, 3)).astype(np.float32)
    xyz[: n // 3] = (xyz[: n // 3] * np.float32(0.05)).astype(np.float32)              # dense near field: longer runs
    rec = synth.to_xyzi(xyz)
    rec[:, 4] = rng.uniform(0, 255, n).astype(np.float32)
    return rec


def range_cloud(ext, n=4000, seed=9):
    """Leaf 1.0 and coordinates k + 0.5 (exact in fp32): each axis has (int64)((max - min) * 1) + 1 = ext[d] voxels,
    and the voxel indices floor(max) - floor(min) + 1 are the same numbers, so the largest key is
    ext0 * ext1 * ext2 - 1 (no int overflow in the oracle's index arithmetic when the product is <= INT32_MAX)."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(ext)
    xyz = (rng.integers(0, ext, (n, 3)) + 0.5).astype(np.float32)
    xyz[0] = 0.5
    xyz[1] = ext - 0.5
    return synth.to_xyzi(xyz)


def index_range(rec, leaf):
    """PCL's size check: prod((int64)((max - min) * inv) + 1) over the finite points, fp32 arithmetic as published."""
    p = rec[np.isfinite(rec[:, :3]).all(1), :3]
    inv = np.float32(1.0) / np.float32(leaf)
    return int(np.prod(((p.max(0) - p.min(0)) * inv).astype(np.int64) + 1))


def numpy_keys(rec, leaf):
    ok = np.isfinite(rec[:, :3]).all(1)
    p = rec[ok, :3]
    inv = np.float32(1.0) / np.float32(leaf)
    min_b = np.floor(p.min(0) * inv).astype(np.int64)
    div = np.floor(p.max(0) * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(p * inv) - min_b.astype(np.float32)).astype(np.int64)
    return ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


def face_cloud(leaf, offset=(0.0, 0.0, 0.0), seed=2):
    """Points exactly on voxel faces: coordinates offset + k * leaf (k = -12 .. 12, every sign), -0.0 in each axis, and
    a second point per face voxel 0.3 leaf inside it."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    k = rng.integers(-12, 13, (1500, 3)).astype(np.float64)
    on = (o + k * leaf).astype(np.float32)
    inside = (o + (k + 0.3) * leaf).astype(np.float32)
    zero = np.array([[-0.0, 1.0, 1.0], [1.0, -0.0, 1.0], [1.0, 1.0, -0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], np.float32)
    xyz = np.concatenate([on, inside] + ([zero] if not np.any(o) else []), 0)
    rec = synth.to_xyzi(xyz)
    rec[:, 4] = rng.uniform(0, 255, rec.shape[0]).astype(np.float32)
    return rec[rng.permutation(rec.shape[0])]


def check_numpy(rec, leaf, out):
    """out (device or oracle records) against numpy_voxel_grid: same voxels in the same order, equal counts where the
    statement can tell them (the voxel's point count is not in the record: equal voxel number and centroids within
    the fp32 rounding bound of a sequential sum of m values, (m + 1) * 2^-24 * max |coordinate| of the voxel)."""
    if rec.shape[1] < 8:                      # (records under 20 bytes carry no intensity: it reads as 0)
        keep = 5 if rec.shape[1] >= 5 else 3
        rec = np.concatenate([rec[:, :keep], np.zeros((rec.shape[0], 8 - keep), np.float32)], 1)
    ref, counts = numpy_voxel_grid(rec, leaf)
    assert out.shape[0] == ref.shape[0]
    ok = np.isfinite(rec[:, :3]).all(1)
    p = rec[ok]
    keys = numpy_keys(rec, leaf)
    order = np.argsort(keys, kind="stable")
    heads = np.flatnonzero(np.r_[True, keys[order][1:] != keys[order][:-1]])
    vmax = np.maximum.reduceat(np.abs(p[order][:, [0, 1, 2, 4]].astype(np.float64)), heads, axis=0)
    bound = (counts[:, None] + 1) * 2.0 ** -24 * vmax + 1e-30
    got = out[:, [0, 1, 2, 4]].astype(np.float64) if out.shape[1] >= 5 else out[:, :3].astype(np.float64)
    assert np.all(np.abs(got - ref[:, : got.shape[1]]) <= bound[:, : got.shape[1]])
    return counts


def test_numpy_check_of_narrow_records():
    rec = blob_cloud([41, 97], 0.4, n_background=300)
    for stride in (12, 16, 20):
        out, _ = O.voxel_grid(with_stride(rec, stride), 0.4)
        check_numpy(with_stride(rec, stride), 0.4, out)


@pytest.mark.parametrize("leaf,offset", [(0.4, (0.0, 0.0, 0.0))] + [(lf, o) for o in MAP_OFFSETS for lf in (0.2, 0.4, 0.5)])
def test_blob_clouds_hold_the_run_lengths(leaf, offset):
    rec = blob_cloud(RUN_LENGTHS, leaf, offset)
    out, small = O.voxel_grid(rec, leaf)
    assert not small
    counts = check_numpy(rec, leaf, out)
    for m in RUN_LENGTHS:
        assert (counts == m).sum() >= 1, m
    assert counts.max() == 2049


def test_sweeps_reach_the_third_digit_pass():
    rec = sweep_cloud()
    for leaf in (0.2, 0.4):
        keys = numpy_keys(rec, leaf)
        assert keys.max() >= 2 ** 22 and len(np.unique(keys >> 22)) >= 2
        out, small = O.voxel_grid(rec, leaf)
        assert not small
        check_numpy(rec, leaf, out)


def test_index_range_on_both_sides_of_int32_max():
    below, above = range_cloud((1290, 1290, 1290)), range_cloud((1291, 1290, 1290))
    assert index_range(below, 1.0) == 1290 ** 3 <= 2 ** 31 - 1 < index_range(above, 1.0) == 1291 * 1290 ** 2
    assert numpy_keys(below, 1.0).max() <= 2 ** 31 - 1 and numpy_keys(below, 1.0).max() >= 2 ** 30
    out, small = O.voxel_grid(below, 1.0)
    assert not small
    check_numpy(below, 1.0, out)
    out, small = O.voxel_grid(above, 1.0)
    assert small and np.array_equal(out[:, :3], above[:, :3])


@pytest.mark.parametrize("leaf", [0.25, 0.5, 2.0])
def test_face_clouds(leaf):
    rec = face_cloud(leaf)
    out, _ = O.voxel_grid(rec, leaf)
    check_numpy(rec, leaf, out)


@pytest.mark.parametrize("out_stride", [12, 16, 20, 32, 48])
def test_oracle_output_strides(out_stride):
    rec = blob_cloud([41, 1025], 0.4, n_background=500)
    ref, _ = O.voxel_grid(rec, 0.4)
    out, _ = O.voxel_grid(rec, 0.4, out_stride=out_stride)
    w = min(out_stride // 4, 5)
    assert out.shape == (ref.shape[0], out_stride // 4)
    assert np.array_equal(out[:, :w].view(np.uint32), ref[:, :w].view(np.uint32)) and np.all(out[:, w:] == 0)
