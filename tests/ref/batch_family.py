"""Two deterministic families of scans for the batch and slot tests beyond eight scans (tests/test_batch_slots_gpu.py), cut from
the `tiny` and `small` configurations of liorf_amd.synth so that nothing large is generated.  Pure numpy: the CPU test
(tests/test_batch_family_cpu.py) holds the families to what the oracle says about them, the GPU test runs them.

tiny_member(k), k = 0 .. 63: 2 000 down to 173 points of the tiny scan against the tiny map (6 000 points) - 32 down to 3
  64-point chunks, 40 down to 8 workgroups per slot, so the lockstep grid of every batch is ragged - from a guess of its own.
mid_member(k), k = 0 .. 8: 3 840 points (60 chunks, 64 workgroups as a batch slot) of the `small` scans 0 .. 2 against the
  small map of index 0: eight of them are the last grid that closes its iterations in the registration kernel (512 workgroups),
  nine the first that does not.
"""
import functools

import numpy as np

from liorf_amd import synth

N_TINY = 64
N_MID = 9
TIGHT = dict(conv_deg=2e-4, conv_cm=2e-4)            # the thresholds that spread the tiny family's iteration counts over both ranges

# the constants of scan_slot_prepare that blocks_of restates (liorf_amd/csrc/s2m_types.h)
WAVES_PER_BLOCK = 8                                  # kBlock / 64
BLOCKS_QUANTUM = 8                                   # kBlocksQuantum
MAX_BLOCKS = 512                                     # kMaxBlocks; also kFuseMaxBlocks (s2m_abi.hip), the largest grid with a fused close
SEG_ITERS = 8                                        # launches of the first range with early exit on (Tuning::seg_iters)
CTX_SLOTS, INIT_SLOTS, PREP_SLOTS, MAX_SLOTS = 8, 12, 16, 64     # kCtxSlots, kInitSlots, kPrepSlots, kMaxSlots


@functools.lru_cache(maxsize=None)
def _tiny():
    cfg = synth.make_config("tiny")
    return synth.to_xyzi(cfg["map"]), synth.to_xyzi(cfg["scan"]), cfg["pose_init"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _small(scan_index):
    cfg = synth.make_config("small", scan_index=scan_index)
    return synth.to_xyzi(cfg["map"]), synth.to_xyzi(cfg["scan"]), cfg["pose_init"].astype(np.float32)


def tiny_map():
    return _tiny()[0]


def mid_map():
    return _small(0)[0]


def tiny_member(k):
    """(scan records, pose guess) of member k = 0 .. 63."""
    assert 0 <= k < N_TINY
    _, scan, pose0 = _tiny()
    rng = np.random.default_rng(1000 + k)
    d = np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.05, 0.05, 3)]).astype(np.float32)
    return np.ascontiguousarray(scan[k % 3:][:2000 - 29 * k]), (pose0 + d).astype(np.float32)


def mid_member(k):
    """(scan records, pose guess) of member k = 0 .. 8."""
    assert 0 <= k < N_MID
    _, scan, pose0 = _small(k % 3)
    pose = pose0.copy()
    pose[3] += np.float32(0.01 * (k // 3))
    return np.ascontiguousarray(scan[k // 3::3][:3840]), pose


def blocks_of(n_points):
    """Workgroups of a batch slot that holds n_points records.  A restatement of scan_slot_prepare
    (liorf_amd/csrc/s2m_prep.hip:178-193) for the 8-wave workgroup shape and one wave-table entry per wave (the defaults)."""
    n_chunks = (n_points + 63) // 64
    base_parts = 1
    while base_parts < 8 and n_chunks * base_parts * 2 <= 2048:
        base_parts *= 2
    nblocks = (n_chunks * base_parts + n_chunks // 2 + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK
    nblocks = (nblocks + BLOCKS_QUANTUM - 1) // BLOCKS_QUANTUM * BLOCKS_QUANTUM
    return min(max(nblocks, BLOCKS_QUANTUM), MAX_BLOCKS)
