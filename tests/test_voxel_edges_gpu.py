"""The voxel-grid filter (s2m_voxel.hip) where its code paths switch, and extractCloud's frame table, against the oracle
(bit-exact records in ascending voxel-index order) and the float64 numpy statement (tests/test_voxel_edges_cpu.py).
PARITY UNPINNED."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m, synth
from oracle import oracle as O
from test_voxel_cpu import raw_cloud
from test_voxel_edges_cpu import (MAP_OFFSETS, RUN_LENGTHS, blob_cloud, check_numpy, face_cloud, numpy_keys, range_cloud,
                                  sweep_cloud, tile_cloud, with_stride)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _same(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(gpu, rec, leaf):
    out = gpu.voxelGrid(rec, leaf)
    ref, small = O.voxel_grid(rec, leaf)
    assert not small and not gpu.leaf_too_small
    _same(out, ref)
    check_numpy(rec, leaf, out)
    return out


@pytest.mark.parametrize("stride", [12, 16, 20, 32])
def test_run_lengths_at_every_hand_over(gpu, stride):
    """Voxels of exactly 1, 7, 8, 9, 15, 16, 17 points (k_vox_centroid's 8-record batches), 39, 40 | 41 (kLongRun:
    above 40 points a wave takes the voxel), 47, 48, 63, 64, 65, 96, 97, 255, 256, 257, 272 (centroid_wave_role's
    256-record chunks, add_run's 32 / 16 / 1 tails), 511 .. 1023, 1024 | 1025 (kVeryLongRun: a workgroup), 1040,
    2048, 2049 (1 024-record rounds, both buffers), with 12-, 16-, 20- and 32-byte input records (intensity read only
    from 20 bytes on)."""
    _check(gpu, with_stride(blob_cloud(RUN_LENGTHS, 0.4), stride), 0.4)


@pytest.mark.parametrize("offset", MAP_OFFSETS)
@pytest.mark.parametrize("leaf", [0.2, 0.4, 0.5])
def test_run_lengths_and_faces_in_the_map_frame(gpu, offset, leaf):
    """The run-length cloud and a face cloud at 5 km, 20 km and 100 km from the origin (where loopFindNearKeyframes
    filters the ICP submaps): the same hand-overs with large minimum voxel indices (floor(1e5 / 0.2) = 5e5)."""
    _check(gpu, blob_cloud(RUN_LENGTHS, leaf, offset), leaf)
    _check(gpu, face_cloud(leaf, offset), leaf)


def test_many_long_and_very_long_runs(gpu):
    """4 200 voxels of 41 .. 60 points (more than the 4 096 long runs at which k_vox_centroid_long's wave grid is capped
    at 1 024 workgroups and its item loop strides) and 264 voxels of 1 025 .. 1 030 points (more than the 256 very long
    runs its workgroup role is capped at)."""
    rng = np.random.default_rng(1)
    rec = blob_cloud(list(rng.integers(41, 61, 4200)), 0.4, n_background=2000)
    assert 4200 <= (check_numpy(rec, 0.4, O.voxel_grid(rec, 0.4)[0]) > 40).sum()
    _check(gpu, rec, 0.4)
    rec = blob_cloud(list(rng.integers(1025, 1031, 264)), 0.4, n_background=2000)
    _check(gpu, rec, 0.4)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193])
def test_radix_tile_edges(gpu, n):
    """n around the sort's 4 096-key tiles and 1 024-key rounds, NaN / +-inf records at positions 0, 1023, 1024, 4095,
    4096 and n - 1 (their key 0xffffffff sorts behind every voxel); and a cloud that is all non-finite but one point,
    placed at the last position of a tile (4095) or the first of the next (4096)."""
    _check(gpu, tile_cloud(n, (0, 1023, 1024, 4095, 4096, n - 1)), 0.4)
    if n > 4096:
        for i in (4095, 4096):
            rec = np.full((n, 8), np.nan, np.float32)
            rec[i] = raw_cloud(1, with_bad=False)[0]
            _same(gpu.voxelGrid(rec, 0.4), O.voxel_grid(rec, 0.4)[0])


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_keys_above_2_22(gpu, leaf):
    """A +-80 m sweep: the largest voxel index is >= 2^22 and keys differ in bits 22..31, so all three 11-bit passes
    of the radix sort move real digits."""
    rec = sweep_cloud()
    keys = numpy_keys(rec, leaf)
    assert keys.max() >= 2 ** 22 and len(np.unique(keys >> 22)) >= 2
    _check(gpu, rec, leaf)


def test_index_range_at_int32_max(gpu):
    """Leaf 1, extents 1290^3 = 2 146 689 000 voxels (just below INT32_MAX: filtered, keys up to 2^31 - 2^20) and
    1291 x 1290^2 = 2 148 353 100 (just above: PCL's "leaf size is too small", the input handed through)."""
    below, above = range_cloud((1290, 1290, 1290)), range_cloud((1291, 1290, 1290))
    _check(gpu, below, 1.0)
    out = gpu.voxelGrid(above, 1.0)
    assert gpu.leaf_too_small and np.array_equal(out.view(np.uint32), above.view(np.uint32))


@pytest.mark.parametrize("leaf", [0.25, 0.5, 2.0])
def test_points_on_voxel_faces(gpu, leaf):
    """Coordinates exactly k * leaf (k = -12 .. 12; leaf exact in binary, so x * (1 / leaf) = k exactly and the point
    belongs to voxel k, not k - 1) and -0.0 in each axis."""
    _check(gpu, face_cloud(leaf), leaf)


SENTINEL = np.float32(-7.25e33)


def _host_call(gpu, rec, leaf, out_stride, cap, guard=8):
    words = out_stride // 4
    buf = np.full(((cap + guard) * words,), SENTINEL, np.float32)
    m = C.c_size_t(0)
    rc = gpu.lib.s2m_voxel_downsample(gpu.h, rec.ctypes.data, rec.shape[0], rec.shape[1] * 4, leaf, buf.ctypes.data, out_stride,
                                      cap, C.byref(m))
    return rc, m.value, buf


@pytest.mark.parametrize("out_stride", [12, 16, 20, 32, 48])
def test_output_strides(gpu, out_stride):
    """Output records of 12, 16, 20, 32 and 48 bytes through the C ABI: the oracle's records of the same stride (xyz,
    1.0, mean intensity, zeros), nothing written past the last record."""
    rec = blob_cloud([41, 97, 1025, 2049], 0.4, n_background=1500)
    ref, _ = O.voxel_grid(rec, 0.4, out_stride=out_stride)
    rc, m, buf = _host_call(gpu, rec, 0.4, out_stride, ref.shape[0])
    words = out_stride // 4
    assert rc == 0 and m == ref.shape[0]
    _same(buf[: m * words].reshape(m, words), ref)
    assert np.all(buf[m * words:] == SENTINEL)


@pytest.mark.parametrize("which", ["host", "device"])
def test_capacity_with_long_runs(gpu, which):
    """cap = 1, n_out - 1 and n_out with long (41, 97 points) and very long (1 025, 2 049 points) runs at low and at high
    output positions, so that some of them lie below cap and some at or above it: the first min(cap, n_out) records
    are the oracle's, S2M_ERR_CAPACITY with the needed size when cap < n_out, and a guard region after
    cap * out_stride keeps its sentinel (host ABI and s2m_voxel_downsample_device)."""
    rec = blob_cloud([41, 97, 1025, 2049, 41, 97, 1025, 2049], 0.4, n_background=600)
    ref, _ = O.voxel_grid(rec, 0.4)
    n_out = ref.shape[0]
    guard = n_out + 64                  # (an overrun of up to n_out records would still land inside the buffer, on the sentinel)
    for cap in (1, n_out - 1, n_out):
        if which == "host":
            rc, m, buf = _host_call(gpu, rec, 0.4, 32, cap, guard)
            got = buf.reshape(-1, 8)
        else:
            torch = pytest.importorskip("torch")
            d_in = torch.from_numpy(rec).cuda()
            d_out = torch.full(((cap + guard) * 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            mm = C.c_size_t(0)
            rc = gpu.lib.s2m_voxel_downsample_device(gpu.h, C.c_void_p(d_in.data_ptr()), rec.shape[0], 32, 0.4,
                                                     C.c_void_p(d_out.data_ptr()), 32, cap, C.byref(mm))
            m = mm.value
            got = d_out.cpu().numpy().reshape(-1, 8)
        assert m == n_out and rc == (0 if cap == n_out else -5), (cap, rc)
        _same(got[:cap], ref[:cap])
        assert np.all(got[cap:] == SENTINEL), cap


def _frames(n_frames, seed=4, far=False):
    rng = np.random.default_rng(seed)
    frames, poses = [], []
    for k in range(n_frames):
        n = int(rng.integers(20, 120))
        xyz = rng.uniform([-15, -15, -2], [15, 15, 4], (n, 3)).astype(np.float32)
        rec = synth.to_xyzi(xyz)
        rec[:, 4] = rng.uniform(0, 100, n).astype(np.float32)
        frames.append(rec)
        base = np.array([20000.0, -8000.0, 30.0]) if far else np.zeros(3)
        poses.append(np.r_[base + [2.0 * k, 0.5 * k, 0.01 * k], rng.uniform(-0.05, 0.05, 2), rng.uniform(-3, 3)].astype(np.float32))
    return frames, np.stack(poses) if poses else np.zeros((0, 6), np.float32)


def _oracle_extract(frames, poses, leaf):
    cat = np.concatenate([O.transform_point_cloud(f, p) for f, p in zip(frames, poses)], 0)
    return O.voxel_grid(cat, leaf)[0]


@pytest.mark.parametrize("n_frames", [1, 2, 37, 300])
@pytest.mark.parametrize("far", [False, True])
def test_extract_cloud_frame_table(gpu, n_frames, far):
    """k_transform_frames finds each point's frame by a binary search over the frame offsets: 1, 2, 37 and 300 key frames,
    empty frames at the front, in the middle and at the end, 1-point frames, key poses at the origin and ~21.5 km from
    it (the map frame of a long run), 32-byte records."""
    frames, poses = _frames(n_frames, seed=n_frames, far=far)
    if n_frames >= 37:
        for i in (0, 1, n_frames // 2, n_frames - 1):
            frames[i] = frames[i][:0]
        for i in (2, n_frames // 2 + 1, n_frames - 2):
            frames[i] = frames[i][:1]
    leaf = 0.4
    ref = _oracle_extract(frames, poses, leaf)
    _same(gpu.extractCloud(frames, poses, leaf), ref)
    if n_frames >= 37:
        ref12 = _oracle_extract([np.ascontiguousarray(f[:, :3]) for f in frames], poses, leaf)
        out12 = gpu.extractCloud([np.ascontiguousarray(f[:, :3]) for f in frames], poses, leaf)
        assert np.array_equal(out12[:, :3].view(np.uint32), ref12[:, :3].view(np.uint32))
