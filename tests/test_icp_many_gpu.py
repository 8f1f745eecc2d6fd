"""The slotted device loop (s2m_debug_icp_align_many_device: what s2m_loop_verify_launch queues): one source against several
targets, the alignments advanced in lockstep through shared launches. Every out[i] must be byte for byte s2m_icp_align(src,
tgt_i) on the same handle - the contract that makes the feature checkable without a new oracle."""
import numpy as np
import pytest

from liorf_amd import s2m
from test_icp_cpu import icp_scene
from test_icp_device_loop_gpu import _moved, _same
from test_icp_edges_cpu import edge_scene, tie_scene

pytestmark = pytest.mark.gpu

R = s2m.S2M_ICP_RANGE


@pytest.fixture(scope="module")
def gpu():
    g = s2m.MapOptimizationS2M()
    yield g
    g.close()


def _many(gpu, src, tgts, many_first=False, **kw):
    """The slotted call against the single alignments, called before or after it."""
    got = gpu.debugIcpAlignManyDevice(src, tgts, **kw) if many_first else None
    want = [gpu.icpAlign(src, t, **kw) for t in tgts]
    if got is None:
        got = gpu.debugIcpAlignManyDevice(src, tgts, **kw)
    assert len(got) == len(want) == len(tgts)
    for g, w in zip(got, want):
        _same(g, w)
    return want


@pytest.mark.parametrize("reach", [30.0, 1.0])
@pytest.mark.parametrize("n_src", [3, 257])
def test_targets_of_every_size_in_one_call(gpu, n_src, reach):
    """Targets of 1, 2, 3, 1023, 1025 and 4097 points: grids sized by the largest slot, workgroups beyond a slot's extent, one
    tile and one block more than a multiple. With a reach of 1 m the one-point target has fewer than 3 correspondences among 257
    sources: that slot ends unconverged in its first iteration while the others run on."""
    src, tgt = edge_scene(4097, n_src, seed=4097 + n_src)
    want = _many(gpu, src, [tgt[:n] for n in (1, 2, 3, 1023, 1025, 4097)], max_correspondence_distance=reach)
    print("iterations per slot", [w[3] for w in want])
    if n_src == 257:
        assert want[5][3] > 1                                    # the full target needs several iterations
        if reach == 1.0:
            assert (want[0][1], want[0][3]) == (False, 0)
            assert np.array_equal(want[0][0], np.eye(4, dtype=np.float32))


def test_a_slot_with_non_finite_targets(gpu):
    src, tgt = edge_scene(4097, 700, seed=11)
    bad = tgt.copy()
    for k, j in enumerate(range(0, bad.shape[0], 7)):
        bad[j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    bad[1023, :3] = np.nan; bad[1024, 0] = np.inf; bad[4096, 2] = -np.inf
    none = tgt[:64].copy()
    none[:, :3] = np.nan                                         # no finite target at all: no source has a match
    want = _many(gpu, src, [tgt, bad, tgt[:1500], none], max_correspondence_distance=30.0)
    assert want[1][1] and np.isfinite(want[1][2]) and not want[3][1]
    src[5, 0] = np.nan; src[9, 2] = np.inf
    _many(gpu, src, [bad, tgt], many_first=True, max_correspondence_distance=30.0)


def test_a_slot_with_exact_ties(gpu):
    src, tgt = tie_scene(n_src=257)
    shifted = tgt.copy()
    shifted[:, 0] += np.float32(0.25)                            # no ties in this slot
    want = _many(gpu, src, [shifted, tgt, tgt[:2048]], max_correspondence_distance=30.0, max_iterations=1)
    assert want[1][3] == 1 and abs(want[1][0][0, 3] - 0.5) < 1e-5
    _many(gpu, src, [shifted, tgt, tgt[:2048]], max_correspondence_distance=30.0)


@pytest.mark.parametrize("k", [1, 8])
def test_one_slot_and_eight(gpu, k):
    src, tgt, _ = icp_scene(1500, 700, 2)
    _many(gpu, src, [tgt[:1500 - 97 * i] for i in range(k)], max_correspondence_distance=30.0)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignManyDevice(src, [tgt] * (s2m.S2M_LOOP_MAX_CANDIDATES + 1))
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignManyDevice(src, [])


def test_the_same_target_twice(gpu):
    src, tgt, _ = icp_scene(1500, 700, 2)
    got = gpu.debugIcpAlignManyDevice(src, [tgt, tgt[:800], tgt], max_correspondence_distance=30.0)
    _same(got[0], got[2])
    _same(got[0], gpu.icpAlign(src, tgt, max_correspondence_distance=30.0))
    _same(got[1], gpu.icpAlign(src, tgt[:800], max_correspondence_distance=30.0))


def test_slots_that_end_in_different_ranges(gpu):
    """Iteration limits of R - 1, R and R + 1 on a scene that needs more, beside a slot that converges inside the first range
    (the target is the source itself): the slot that has ended idles while the other goes on to the limit."""
    src0, tgt, _ = icp_scene(6000, 1500, 5)
    src = _moved(src0, 2.0)
    kw = dict(max_correspondence_distance=30.0, transformation_epsilon=1e-12, euclidean_fitness_epsilon=1e-14)
    for m in (R - 1, R, R + 1):
        want = _many(gpu, src, [tgt, src.copy(), tgt[:3000]], max_iterations=m, **kw)
        assert want[0][3] == m and want[1][3] < R - 1, (m, want[0][3], want[1][3])
    # by PCL's own criteria: the slots end in different ranges
    want = _many(gpu, src, [tgt, src.copy(), tgt[:3000], tgt[:1000]], **kw)
    print("iterations per slot", [w[3] for w in want])
    assert want[0][3] > R + 1 and want[1][3] < R


@pytest.mark.parametrize("tuning", [(0.5, 1, 1), (0.0, 0, 0)])
def test_fallback_lists_and_brute_force(gpu, tuning):
    """Small cells and one shell, so that every slot has a non-empty fallback list; and the brute force alone."""
    src, tgt, _ = icp_scene(1500, 700, 2)
    edge_src, edge_tgt = edge_scene(1025, 700, seed=1725)
    try:
        gpu.debugIcpTuning(*tuning)
        if tuning[2]:
            for t in (tgt, tgt[:1023]):
                assert gpu.debugIcpNearest(src, t, 1)[1] > 0      # the list is not empty
        _many(gpu, src, [tgt, tgt[:1023], edge_tgt, tgt[:5]], max_correspondence_distance=30.0)
    finally:
        gpu.debugIcpTuning()


def test_two_calls_in_a_row_regrow_and_leave_nothing_behind():
    """A small call, a larger one with more slots (the buffers grow), the small one again (stale per-slot state), on one handle."""
    g = s2m.MapOptimizationS2M()
    try:
        src_a, tgt_a = edge_scene(1025, 257, seed=1282)
        src_b, tgt_b, _ = icp_scene(6000, 1500, 5)
        first = _many(g, src_a, [tgt_a, tgt_a[:3]], many_first=True, max_correspondence_distance=30.0)
        _many(g, src_b, [tgt_b[:4097], tgt_b, tgt_b[:1023], tgt_b[:2000], tgt_b[:300]], many_first=True, max_correspondence_distance=30.0)
        again = g.debugIcpAlignManyDevice(src_a, [tgt_a, tgt_a[:3]], max_correspondence_distance=30.0)
        for a, b in zip(again, first):
            _same(a, b)
        one = g.debugIcpAlignManyDevice(src_a, [tgt_a[:3]], max_correspondence_distance=30.0)
        _same(one[0], first[1])
        _same(g.debugIcpAlignDevice(src_a, tgt_a, max_correspondence_distance=30.0), first[0])
    finally:
        g.close()
