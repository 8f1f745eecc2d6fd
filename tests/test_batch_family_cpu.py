"""The scan families of the batch tests beyond eight scans (tests/ref/batch_family.py) under the oracle: which members are
degenerate, which converge inside the first range of launches, which sit on its last launch, which run all 30 iterations - and the
workgroup counts that put the batches on the slot-count edges.  tests/test_batch_slots_gpu.py relies on every one of these; a
change to liorf_amd.synth that moves a family off an edge fails here, not silently on the GPU.  The values are what the oracle
(knn_backend=1) gives for these inputs: properties of the inputs under the reference, not of the library."""
import functools
import os
import sys

import numpy as np

from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import batch_family as F  # noqa: E402


def _run(m, members, **kw):
    orc = O.Oracle(knn_backend=1, num_threads=8, **kw)
    orc.set_map(m)
    out = []
    for scan, pose in members:
        orc.set_scan(scan)
        r = orc.scan2MapOptimization(pose)
        out.append((r.iters_run, r.converged, r.is_degenerate, r.n_sel_last, r.skipped))
    orc.close()
    return out


@functools.lru_cache(maxsize=None)
def _tiny(tight):
    return _run(F.tiny_map(), [F.tiny_member(k) for k in range(F.N_TINY)], **(F.TIGHT if tight else {}))


@functools.lru_cache(maxsize=None)
def _mid():
    return _run(F.mid_map(), [F.mid_member(k) for k in range(F.N_MID)])


def _with_iters(rows, pred):
    return [k for k, r in enumerate(rows) if pred(r[0])]


def test_observation_hook_is_bound_and_checks_its_arguments():
    """s2m_debug_batch_last (include/liorf_s2m_debug.h): declared among the diagnostics, mirrored field by field, null-checked on
    the host without a device."""
    import ctypes as C
    from liorf_amd import s2m
    lib = s2m.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "s2m_debug_batch_last(" in open(os.path.join(root, "include", "liorf_s2m_debug.h")).read()
    assert "s2m_debug_batch_last" in s2m.ABI_SYMBOLS and len(lib.s2m_debug_batch_last.argtypes) == 2
    assert C.sizeof(s2m.BatchLoop) == 5 * 4 and C.sizeof(s2m.BatchLast) == 8 * 4 + 2 * C.sizeof(s2m.BatchLoop)
    out = s2m.BatchLast()
    assert lib.s2m_debug_batch_last(None, C.byref(out)) == -1 and lib.s2m_debug_batch_last(None, None) == -1


def test_members_are_cut_as_documented():
    m = F.tiny_map()
    assert m.shape == (6000, 8) and m.dtype == np.float32
    p0 = F.tiny_member(0)[1]
    for k in range(F.N_TINY):
        s, p = F.tiny_member(k)
        assert s.shape == (2000 - 29 * k, 8) and s.dtype == np.float32 and s.flags.c_contiguous and p.dtype == np.float32
        d = np.abs(p.astype(np.float64) - F._tiny()[2])
        assert d[:3].max() <= 0.01 + 1e-6 and d[3:].max() <= 0.05 + 1e-6
        assert k == 0 or not np.array_equal(p, p0)
    assert F.tiny_member(63)[0].shape[0] == 173
    assert np.array_equal(F.tiny_member(4)[0][0], F.tiny_member(1)[0][0]) and not np.array_equal(F.tiny_member(4)[0][0], F.tiny_member(0)[0][0])
    assert F.mid_map().shape == (30000, 8)
    for k in range(F.N_MID):
        s, p = F.mid_member(k)
        assert s.shape == (3840, 8) and s.flags.c_contiguous and p.dtype == np.float32
    assert F.mid_member(3)[1][3] == F.mid_member(0)[1][3] + np.float32(0.01)


def test_workgroups_per_slot_put_the_batches_on_the_edges():
    """blocks_of restates scan_slot_prepare (liorf_amd/csrc/s2m_prep.hip:178-193)."""
    tiny = [F.blocks_of(F.tiny_member(k)[0].shape[0]) for k in range(F.N_TINY)]
    chunks = [(F.tiny_member(k)[0].shape[0] + 63) // 64 for k in range(F.N_TINY)]
    assert (max(chunks), min(chunks)) == (32, 3)
    assert (tiny[0], max(tiny), min(tiny)) == (40, 40, 8) and len(set(tiny)) > 2          # ragged: the widest row is member 0's
    # 12 rows of 40 are the last fused grid of the tiny family, 13 the first that k_finalize closes
    assert 12 * max(tiny) <= F.MAX_BLOCKS < 13 * max(tiny)
    assert F.CTX_SLOTS < F.INIT_SLOTS <= 12 < 13 <= F.PREP_SLOTS                         # the fuse edge lies apart from the ctx and prep chunk edges
    mid = [F.blocks_of(F.mid_member(k)[0].shape[0]) for k in range(F.N_MID)]
    assert mid == [64] * F.N_MID
    assert 8 * 64 == F.MAX_BLOCKS and 9 * 64 > F.MAX_BLOCKS
    # every member is past the soft condition :1300 (more than min_feats = 30 records)
    assert min(F.tiny_member(k)[0].shape[0] for k in range(F.N_TINY)) > 30


def test_tiny_family_default_thresholds():
    rows = _tiny(False)
    assert all(r[4] == 0 for r in rows)                                   # none skipped
    n_sel = [r[3] for r in rows]
    assert (min(n_sel), max(n_sel)) == (66, 938) and min(n_sel) > 50      # (min_corr = 50)
    assert all(r[2] == 1 for r in rows)                                   # all degenerate: the matP projector path
    assert _with_iters(rows, lambda i: i == 30) == [24, 48]
    rest = [r for k, r in enumerate(rows) if k not in (24, 48)]
    assert len(rest) == 62 and all(2 <= r[0] <= 7 and r[1] == 1 for r in rest)
    # a batch of members 0 .. n-1 needs its second range from n = 25 on
    assert all(r[0] <= F.SEG_ITERS for r in rows[:24]) and rows[24][0] > F.SEG_ITERS


def test_tiny_family_tight_thresholds():
    rows = _tiny(True)
    assert all(r[4] == 0 for r in rows)
    assert _with_iters(rows, lambda i: i == 8) == [6, 47, 50]             # the last launch of the first range
    assert _with_iters(rows, lambda i: i == 9) == [7, 45]                 # the first of the second
    assert _with_iters(rows, lambda i: i == 11) == [21, 57]
    assert _with_iters(rows, lambda i: i == 30) == [5, 15, 24, 48, 49, 52, 53, 56]
    others = [r[0] for r in rows if r[0] not in (8, 9, 11, 30)]
    assert len(others) == 64 - 3 - 2 - 2 - 8 and all(3 <= i <= 7 for i in others)
    assert len(_with_iters(rows, lambda i: i < 8)) >= 30


def test_mid_family():
    rows = _mid()
    assert all(r[4] == 0 and r[2] == 0 for r in rows)                     # none skipped, none degenerate
    n_sel = [r[3] for r in rows]
    assert (min(n_sel), max(n_sel)) == (3560, 3609)
    assert _with_iters(rows, lambda i: i == 30) == [7]
    assert all(r[0] in (4, 5) and r[1] == 1 for k, r in enumerate(rows) if k != 7)
