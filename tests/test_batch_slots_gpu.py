"""Batches of 9 to 64 scans and slot indices up to 63 (liorf_amd/csrc/s2m_abi_batch.hip): everything that depends on the slot
count changes behaviour beyond the eight scans the other batch tests stop at - the tables that travel as kernel arguments in
chunks of 8 (CtxTable), 12 (StateInitTable) and 16 (PrepTable) slots, the 512-workgroup threshold between the fused close and
k_finalize, entries 8 .. 63 of the SlotTable, the graph cache keyed by the list of live slots.

The bar is the header's promise (include/liorf_s2m.h): every live row of a batch has, for pose, result fields, affine and trace
poses, the BITS of s2m_optimize on a fresh handle of its own (tests/ref/solo_ref.py) - no tolerance.  s2m_debug_batch_last only
proves that the intended path ran (how many table launches, which loop, which range).  The scans are the two families of
tests/ref/batch_family.py, held to the oracle's account of them by tests/test_batch_family_cpu.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from liorf_amd import s2m
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import batch_family as F  # noqa: E402
from solo_ref import solo  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARG = -1                                                    # S2M_ERR_INVALID_ARG (include/liorf_s2m.h)
MAP_SHIFT = 0.02                                                    # metres in x, test_reinstall_a_few_slots_of_many
# launches of k_set_ctxs / k_init_states / scan-ordering tables for a batch of n freshly installed scans, all live
TABLE_LAUNCHES = {1: (1, 1, 1), 8: (1, 1, 1), 9: (2, 1, 1), 12: (2, 1, 1), 13: (2, 2, 1), 16: (2, 2, 1), 17: (3, 2, 2), 33: (5, 3, 3),
                  64: (8, 6, 4)}


def _map(family, shifted=False):
    m = F.tiny_map() if family == "tiny" else F.mid_map()
    if shifted:
        m = m.copy()
        m[:, 0] += np.float32(MAP_SHIFT)
    return m


def _member(family, k):
    return F.tiny_member(k) if family == "tiny" else F.mid_member(k)


@functools.lru_cache(maxsize=None)
def _solo(family, k, shifted=False, **kw):
    """The reference of a row: member k on a fresh handle of its own with the parameters `kw`.  Computed once per (member,
    parameter set), shared, never written to."""
    scan, pose = _member(family, k)
    return solo(_map(family, shifted), scan, pose, **kw)


def _handle(family="tiny", **kw):
    gpu = s2m.MapOptimizationS2M(**kw)
    gpu.setInputCloud(_map(family))
    return gpu


def _check(gpu, slot, pose, res, want, what):
    """tests/test_batch_state_gpu._check: result fields, pose, affine and trace poses of `slot` equal the solo bits."""
    assert (res.iters_run, res.converged, res.is_degenerate, res.n_sel_last, res.skipped) == want[1], what
    assert np.array_equal(np.asarray(pose, np.float32).view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(np.array(res.affine, np.float32).view(np.uint32), want[2].view(np.uint32)), what
    tr = np.array([t.pose[:] for t in gpu.batchTrace(slot)], np.float32).reshape(-1, 6)
    assert tr.shape == want[3].reshape(-1, 6).shape and np.array_equal(tr.view(np.uint32), want[3].reshape(-1, 6).view(np.uint32)), what


def _batch(gpu, family, members, what, install=True, shifted=False, **kw):
    """Members `members` in slots 0 .. n-1 (installed from host records, or the resident ones launched again): every row bitwise solo."""
    sp = [_member(family, k) for k in members]
    poses = np.stack([p for _, p in sp])
    if install:
        out, res = gpu.optimizeBatch([s for s, _ in sp], poses)
    else:
        gpu.batchLaunch(poses)
        out, res = gpu.batchCollect()
    for b, k in enumerate(members):
        _check(gpu, b, out[b], res[b], _solo(family, k, shifted, **kw), (what, "slot", b, "member", k))
    return out, res


def _loop(last, j=0):
    lp = last.loop[j]
    return dict(wpb=lp.wpb, nslots=lp.nslots, nblocks=lp.nblocks, fused=lp.fused, first_split=lp.first_split)


def test_batch_sizes_at_every_chunk_edge_growing_then_shrinking():
    """One handle, default parameters (early exit on: two ranges where a row needs them), tiny members 0 .. n-1 for n at and
    just past every chunk edge (8 | 9, 12 | 13, 16 | 17), at 33 and at the limit, then back down over graphs already captured."""
    gpu = _handle()
    seen = set()
    for n in (1, 8, 9, 12, 13, 16, 17, 33, 64, 17, 9, 1):
        _batch(gpu, "tiny", range(n), n)
        last = gpu.batchLast()
        assert (last.n_scans, last.n_live) == (n, n), n
        assert (last.ctx_launches, last.init_launches, last.prep_launches) == TABLE_LAUNCHES[n], n
        lp = _loop(last)
        assert last.n_loops == 1 and (lp["wpb"], lp["nslots"], lp["nblocks"]) == (8, n, 40), (n, lp)
        assert lp["fused"] == (1 if n <= 12 else 0), (n, lp)          # 12 x 40 = 480 <= 512 < 13 x 40
        needs_second = max(_solo("tiny", k)[1][0] for k in range(n)) > F.SEG_ITERS
        assert needs_second == (n >= 25), n                          # members 24 and 48 run all 30 iterations
        assert last.ranges_issued == (2 if needs_second else 1), n
        # launches 0 .. 7 are fused launches whatever closes them; certify + search start with the second range of an unfused loop
        assert lp["first_split"] == (8 if needs_second else -1), (n, lp)
        assert last.graph_cached == (1 if n in seen else 0), n
        if n == 17 and n in seen:
            # the same 17 resident scans launched again: no DevCtx block changed, so no k_set_ctxs launch; still the solo bits
            _batch(gpu, "tiny", range(n), (n, "again"), install=False)
            last = gpu.batchLast()
            assert (last.ctx_launches, last.init_launches, last.graph_cached, last.n_live) == (0, 2, 1, n)
        seen.add(n)
    gpu.close()


def test_rows_past_eight_against_the_oracle():
    """Tiny members 8, 12, 16 and 63 - the first rows behind the three chunk sizes and the last slot, fixed before any GPU run - as
    rows of a batch of 64, held to the oracle with the bar of tests/test_batch_gpu.py: equal iterations, pose within 1e-5.  The
    solo result's distance is printed beside the row's."""
    gpu = _handle()
    out, res = _batch(gpu, "tiny", range(64), "oracle")
    gpu.close()
    orc = O.Oracle(knn_backend=1, num_threads=8)
    orc.set_map(F.tiny_map())
    rows = []
    for k in (8, 12, 16, 63):
        scan, pose = F.tiny_member(k)
        orc.set_scan(scan)
        ro = orc.scan2MapOptimization(pose)
        d_row = float(np.abs(np.array(ro.pose) - out[k]).max())
        d_solo = float(np.abs(np.array(ro.pose) - _solo("tiny", k)[0]).max())
        print(f"member {k}: iters row {res[k].iters_run} solo {_solo('tiny', k)[1][0]} oracle {ro.iters_run}; "
              f"max |pose - oracle| row {d_row:.3g} solo {d_solo:.3g}")
        rows.append((k, res[k].iters_run, ro.iters_run, d_row))
    orc.close()
    for k, it, it_o, d in rows:
        assert it == it_o and d <= 1e-5, (k, it, it_o, d)


def test_sixty_four_rows_with_tight_thresholds_in_two_ranges_and_in_one():
    """conv_deg = conv_cm = 2e-4 spreads the 64 rows over both ranges: rows done inside the first, on its last launch (8), on the
    first of the second (9), and rows that run all 30.  Then early exit off: 30 launches for every row in one range - fused up to
    launch 7, the lean certify kernel + search + k_finalize over 64 grid rows from launch 8."""
    its = [_solo("tiny", k, **F.TIGHT)[1][0] for k in range(64)]
    assert 8 in its and 9 in its and 30 in its and sum(i < 8 for i in its) >= 30, its     # the families' account (test_batch_family_cpu.py)
    gpu = _handle(**F.TIGHT)
    for rep in range(2):
        _batch(gpu, "tiny", range(64), ("tight", rep), **F.TIGHT)
        last = gpu.batchLast()
        lp = _loop(last)
        assert last.ranges_issued == 2 and last.n_live == 64 and last.graph_cached == rep, rep
        assert (lp["nslots"], lp["nblocks"], lp["fused"], lp["first_split"]) == (64, 40, 0, 8), lp
    gpu.setParams(early_exit=0, max_iter=30)
    kw = dict(early_exit=0, max_iter=30, **F.TIGHT)
    for rep in range(2):
        out, res = _batch(gpu, "tiny", range(64), ("all thirty", rep), **kw)
        assert all(r.iters_run == 30 for r in res)
        last = gpu.batchLast()
        lp = _loop(last)
        assert last.ranges_issued == 1 and last.graph_cached == rep, rep
        assert (lp["nslots"], lp["nblocks"], lp["fused"], lp["first_split"]) == (64, 40, 0, 8), lp
    gpu.close()


@pytest.mark.parametrize("early", (0, 1))
def test_fuse_boundary_by_slot_count_alone(early):
    """Mid members have 64 workgroups each: eight rows are exactly the last grid whose iterations close inside the registration
    kernel (512 workgroups), nine the first that k_finalize closes, with certify + search from launch 8 on.  Nothing but the slot
    count differs.  With early exit on, member 7 runs all 30 iterations and forces the second range at either size."""
    gpu = _handle("mid", early_exit=early)
    for visit, n in enumerate((8, 9, 8)):
        out, res = _batch(gpu, "mid", range(n), (early, n), early_exit=early)
        last = gpu.batchLast()
        lp = _loop(last)
        assert (lp["wpb"], lp["nblocks"], lp["nslots"]) == (8, 64, n), lp
        assert (lp["fused"], lp["first_split"]) == ((1, -1) if n == 8 else (0, 8)), lp
        assert last.ranges_issued == (2 if early else 1) and last.graph_cached == (1 if visit == 2 else 0), (n, visit)
        if not early:
            assert all(r.iters_run == 30 for r in res) and all(len(gpu.batchTrace(b)) == 30 for b in range(n))
        else:
            assert res[7].iters_run == 30 and min(r.iters_run for r in res) < F.SEG_ITERS      # a row done in the first range beside one that is not
    gpu.close()


def test_holes_across_the_chunk_edges():
    """17 slots with 0, 7, 8, 12 and 16 - the first and last rows of the chunks - holding no usable scan: no records at all (0,
    8, 16), or 30 records, not more than min_feats (7, 12; the reference's :1300).  12 live rows: exactly one full StateInitTable
    and nothing behind it; the second ordering table would hold the empty slot 16 alone and is not issued."""
    gpu = _handle()
    empty = np.zeros((0, 8), np.float32)
    holes = {0: empty, 8: empty, 16: empty, 7: F.tiny_member(7)[0][:30], 12: F.tiny_member(12)[0][:30]}
    sp = [F.tiny_member(k) for k in range(17)]
    poses = np.stack([p for _, p in sp])
    out, res = gpu.optimizeBatch([holes.get(b, sp[b][0]) for b in range(17)], poses)
    for b in range(17):
        if b in holes:
            assert (res[b].skipped, res[b].iters_run) == (2, 0) and np.array_equal(out[b].view(np.uint32), poses[b].view(np.uint32)), b
        else:
            _check(gpu, b, out[b], res[b], _solo("tiny", b), ("holes", b))
    last = gpu.batchLast()
    lp = _loop(last)
    assert (last.n_scans, last.n_live) == (17, 12)
    assert (last.ctx_launches, last.init_launches, last.prep_launches) == (3, 1, 1)
    assert (lp["nslots"], lp["nblocks"], lp["fused"]) == (12, 40, 1), lp
    # every slot empty: nothing to run, and nothing wrong with that
    out, res = gpu.optimizeBatch([empty] * 17, poses)
    for b in range(17):
        assert (res[b].skipped, res[b].iters_run) == (2, 0) and np.array_equal(out[b].view(np.uint32), poses[b].view(np.uint32)), b
    last = gpu.batchLast()
    assert (last.n_scans, last.n_live, last.ranges_issued, last.n_loops) == (17, 0, 0, 0)
    assert (last.init_launches, last.prep_launches) == (0, 0)
    # and the full 17 on the same handle
    _batch(gpu, "tiny", range(17), "full after holes")
    assert gpu.batchLast().n_live == 17
    gpu.close()


def test_reinstall_a_few_slots_of_many():
    """After a batch of 17: three slots (one per CtxTable chunk) get another scan through s2m_batch_set_scan, then the parent's
    max_iter changes, then its map - each time the 17 resident scans are launched again, and each row has the solo bits of what
    its slot holds now, under the parent's parameters, against the parent's map."""
    gpu = _handle()
    members = list(range(17))
    _batch(gpu, "tiny", members, "first")
    for slot, k in ((3, 40), (11, 41), (16, 42)):
        gpu.batchSetScan(slot, F.tiny_member(k)[0])
        members[slot] = k
    _batch(gpu, "tiny", members, "three reinstalled", install=False)
    last = gpu.batchLast()
    assert (last.ctx_launches, last.init_launches, last.n_live) == (1, 2, 17)    # three changed DevCtx blocks: one table
    gpu.setParams(max_iter=12)                                       # sync_slot over 17 children; the captured loops are dropped
    _batch(gpu, "tiny", members, "max_iter 12", install=False, max_iter=12)
    last = gpu.batchLast()
    assert (last.ctx_launches, last.graph_cached) == (3, 0)
    gpu.setInputCloud(_map("tiny", shifted=True))                    # adopt_map over 17 children: their certificates are void
    _batch(gpu, "tiny", members, "shifted map", install=False, shifted=True, max_iter=12)
    assert gpu.batchLast().ctx_launches == 3
    gpu.close()


def test_high_slot_indices_and_limits():
    """Slot 63 asked for first (64 child contexts and streams made at once) runs a loop of its own; slot 64 and 65 scans are
    refused by every entry point with nothing changed; the handle then runs the largest batch."""
    gpu = _handle()
    scan, pose = F.tiny_member(5)
    gpu.slotSetScan(63, scan)
    gpu.slotLaunch(63, pose)
    p, r = gpu.slotCollect(63)
    _check(gpu, 63, p, r, _solo("tiny", 5), "slot 63")
    assert len(gpu.batchTrace(63)) == r.iters_run > 0
    assert gpu.lib.s2m_batch_set_scan(gpu.h, 64, C.c_void_p(scan.ctypes.data), len(scan), 32, 0) == INVALID_ARG
    assert gpu.lib.s2m_batch_set_scan(gpu.h, -1, C.c_void_p(scan.ctypes.data), len(scan), 32, 0) == INVALID_ARG
    n = 65
    ptrs = (C.c_void_p * n)(*[C.c_void_p(scan.ctypes.data)] * n)
    sizes = (C.c_size_t * n)(*[len(scan)] * n)
    poses = np.tile(pose, (n, 1)).astype(np.float32)
    before = poses.copy()
    fp = poses.ctypes.data_as(C.POINTER(C.c_float))
    res = (s2m.Result * n)()
    assert gpu.lib.s2m_batch_set_scans(gpu.h, n, ptrs, sizes, 32, 0) == INVALID_ARG
    assert gpu.lib.s2m_optimize_batch_launch(gpu.h, n, fp) == INVALID_ARG
    assert gpu.lib.s2m_optimize_batch(gpu.h, n, ptrs, sizes, 32, fp, None, res) == INVALID_ARG
    for m in (n, 64, 1):
        assert gpu.lib.s2m_optimize_batch_collect(gpu.h, m, fp, None, res) == INVALID_ARG, m      # nothing pending
    assert np.array_equal(poses, before)
    gpu.slotLaunch(63, pose)                                        # slot 63 still holds its scan
    p, r = gpu.slotCollect(63)
    _check(gpu, 63, p, r, _solo("tiny", 5), "slot 63 after the refusals")
    _batch(gpu, "tiny", range(64), "64 after the refusals")
    gpu.close()


@pytest.fixture(scope="module")
def torch_on_device():
    """torch with its device context made: the first use of the device in a process takes torch seconds, which belong to no test."""
    import torch
    torch.zeros(1).cuda()
    torch.cuda.synchronize()
    return torch


def test_host_and_device_sources_at_seventeen(torch_on_device):
    """s2m_batch_set_scans from device records (torch tensors of the same bytes): the rows of the host-source batch, bit for bit."""
    torch = torch_on_device
    sp = [F.tiny_member(k) for k in range(17)]
    poses = np.stack([p for _, p in sp])
    gpu = _handle()
    host_out, host_res = _batch(gpu, "tiny", range(17), "host source")
    d_scans = [torch.from_numpy(s).cuda() for s, _ in sp]
    torch.cuda.synchronize()
    for g in (gpu, _handle()):                                       # slots that held the scans before, and fresh ones
        g.batchSetScans(device_ptrs=[(t.data_ptr(), t.shape[0], 32) for t in d_scans])
        assert g.batchLast().prep_launches == 2
        g.batchLaunch(poses)
        out, res = g.batchCollect()
        for b in range(17):
            _check(g, b, out[b], res[b], _solo("tiny", b), ("device source", b))
            assert np.array_equal(out[b].view(np.uint32), host_out[b].view(np.uint32)) and res[b].iters_run == host_res[b].iters_run
        g.close()
    del d_scans
