"""The pending optimise of batches and slots (liorf_amd/csrc/s2m_abi_batch.hip, s2m_context::Registration::pending; DESIGN.md
"the pending optimise"): a refused launch marks nothing, a collect clears what it collects, a batch and a slot's own loop do
not cross, a batch collect matches its launch.  Every refusal is an argument check on the host; whatever is collected around
one has, for pose, result fields and trace, the bits of s2m_optimize on a handle of its own (tests/ref/solo_ref.py)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
from solo_ref import solo  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
INVALID_ARG = -1                                                    # S2M_ERR_INVALID_ARG (include/liorf_s2m.h)


@functools.lru_cache(maxsize=None)
def _scene():
    """Three `small` scans (12 000 points; the last one ragged) against the 30 000-point map of the first."""
    cfgs = [synth.make_config("small", scan_index=k) for k in range(N)]
    m = synth.to_xyzi(cfgs[0]["map"])
    scans = [synth.to_xyzi(c["scan"]) for c in cfgs]
    scans[2] = scans[2][:6001]
    poses = np.stack([c["pose_init"] for c in cfgs]).astype(np.float32)
    return m, scans, poses


@functools.lru_cache(maxsize=None)
def _solo(**kw):
    """The solo results of the three scans with the parameters `kw`: computed once, shared, never written to."""
    m, scans, poses = _scene()
    return [solo(m, s, p, **kw) for s, p in zip(scans, poses)]


def _handle(**kw):
    gpu = s2m.MapOptimizationS2M(**kw)
    gpu.setInputCloud(_scene()[0])
    return gpu


def _check(gpu, slot, pose, res, want, what):
    assert (res.iters_run, res.converged, res.is_degenerate, res.n_sel_last, res.skipped) == want[1], what
    assert np.array_equal(np.asarray(pose, np.float32).view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(np.array(res.affine, np.float32).view(np.uint32), want[2].view(np.uint32)), what
    tr = np.array([t.pose[:] for t in gpu.batchTrace(slot)], np.float32)
    assert tr.shape == want[3].shape and np.array_equal(tr.view(np.uint32), want[3].view(np.uint32)), what


def _batch_collect_rc(gpu, n):
    poses = np.zeros((n, 6), np.float32)
    res = (s2m.Result * n)()
    rc = gpu.lib.s2m_optimize_batch_collect(gpu.h, n, poses.ctypes.data_as(C.POINTER(C.c_float)), None, res)
    return rc, poses, res


def test_refused_batch_launch_leaves_nothing_pending():
    """A batch launch over a slot without a scan is refused - and must leave slots 0 and 1 unmarked: a collect of slot 0 is
    refused (nothing was launched), a parameter change on the parent still reaches the slots, and the next batch gives the solo
    bits.  (Before the single pending state the slots in front of the failing one stayed marked, and every later batch launch
    after a parameter change failed with "an optimize launch is pending".)"""
    m, scans, poses = _scene()
    gpu = _handle()
    gpu.batchSetScan(0, scans[0])
    gpu.batchSetScan(1, scans[1])
    s2 = scans[2]
    assert gpu.lib.s2m_batch_set_scan(gpu.h, 2, C.c_void_p(s2.ctypes.data), len(s2), 6, 0) != 0      # stride 6: slot 2 exists, without a scan
    with pytest.raises(s2m.S2MError):
        gpu.batchLaunch(poses[:3])
    with pytest.raises(s2m.S2MError):
        gpu.slotCollect(0)
    gpu.setParams(max_iter=12)
    out, res = gpu.optimizeBatch(scans[:2], poses[:2])
    want = _solo(max_iter=12)
    for b in range(2):
        _check(gpu, b, out[b], res[b], want[b], b)
    gpu.close()


def test_slot_and_batch_do_not_cross():
    """No batch launch over a slot whose own loop is in flight; no slot launch and no s2m_set_params under a pending batch.
    The refused calls change nothing: what was in flight is collected with the solo bits.  (Slot 1 holds a scan too, so that
    the batch launch is refused for the slot in flight and not for a missing scan.)"""
    m, scans, poses = _scene()
    want = _solo(early_exit=1)                                      # (the default)
    gpu = _handle()
    gpu.slotSetScan(0, scans[0])
    gpu.slotSetScan(1, scans[1])
    gpu.slotLaunch(0, poses[0])
    with pytest.raises(s2m.S2MError, match="slot launch is pending"):
        gpu.batchLaunch(poses[:2])
    p, r = gpu.slotCollect(0)
    _check(gpu, 0, p, r, want[0], "slot 0")
    gpu.batchSetScans(scans[:2])
    gpu.batchLaunch(poses[:2])
    with pytest.raises(s2m.S2MError, match="batch launch is pending"):
        gpu.slotLaunch(0, poses[0])
    with pytest.raises(s2m.S2MError, match="pending"):
        gpu.setParams(plane_tol=0.05)
    out, res = gpu.batchCollect()
    for b in range(2):
        _check(gpu, b, out[b], res[b], want[b], b)
    gpu.close()


def test_batch_collect_must_match_its_launch():
    m, scans, poses = _scene()
    want = _solo(early_exit=1)                                      # (the default)
    gpu = _handle()
    gpu.batchSetScans(scans[:2])
    gpu.batchLaunch(poses[:2])
    for n in (1, 3):
        assert _batch_collect_rc(gpu, n)[0] == INVALID_ARG, n
    rc, out, res = _batch_collect_rc(gpu, 2)
    assert rc == s2m.S2M_OK
    for b in range(2):
        _check(gpu, b, out[b], res[b], want[b], b)
    assert _batch_collect_rc(gpu, 2)[0] == INVALID_ARG          # collected already
    gpu.close()
    fresh = _handle()
    assert _batch_collect_rc(fresh, 2)[0] == INVALID_ARG
    fresh.close()


@pytest.mark.parametrize("early", (1, 0))
def test_slot_after_batch_and_batch_after_slot(early):
    """On one handle: a batch of two, the two-slot stream of scans over three scans, the batch again.  Every result and trace
    has the solo bits: no kind (row of a batch / loop of its own) and no range flag survives its collect."""
    m, scans, poses = _scene()
    want = _solo(early_exit=early)
    gpu = _handle(early_exit=early)

    def batch():
        out, res = gpu.optimizeBatch(scans[:2], poses[:2])
        for b in range(2):
            _check(gpu, b, out[b], res[b], want[b], ("batch", b))

    batch()
    gpu.slotSetScan(0, scans[0])
    for i in range(N):
        gpu.slotLaunch(i & 1, poses[i])
        if i + 1 < N:
            gpu.slotSetScan((i + 1) & 1, scans[i + 1])
        p, r = gpu.slotCollect(i & 1)
        _check(gpu, i & 1, p, r, want[i], ("stream", i))
    batch()
    gpu.close()
