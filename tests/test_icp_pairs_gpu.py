"""The table form of the device loop (s2m_debug_icp_align_pairs_device: what s2m_loop_verify_many queues): P pairs, each with its
own source, target and guess, advanced in lockstep through the kernels of the slotted loop, their descriptions in a table in
device memory. Every out[k] must be byte for byte s2m_icp_align(src_k, tgt_k) on the same handle: a pair's partial rows, its
stride over the source, its search shape and its fallback list are those of the single alignment of its sizes, whatever the
other pairs of the call are."""
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


def _pairs(gpu, pairs, pairs_first=False, **kw):
    """The table call against the single alignments, called before or after it."""
    got = gpu.debugIcpAlignPairsDevice(pairs, **kw) if pairs_first else None
    want = [gpu.icpAlign(s, t, **kw) for s, t in pairs]
    if got is None:
        got = gpu.debugIcpAlignPairsDevice(pairs, **kw)
    assert len(got) == len(want) == len(pairs)
    for k, (g, w) in enumerate(zip(got, want)):
        try:
            _same(g, w)
        except AssertionError as e:
            raise AssertionError(f"pair {k} (n_src {len(pairs[k][0])}, n_tgt {len(pairs[k][1])}): {e}") from None
    return want


# ---- sources of every size in one call: the per-pair row count and stride ----------------------------------------------------
N_SRC = (3, 255, 256, 257, 1500, 65537)     # rows: 1, 1, 1, 2, 6 and 257 -> the cap of 256, whose rows stride twice
N_TGT = (1025, 4097)
_sized = {}


def _sized_pairs(gpu, reach):
    """The twelve pairs and their single alignments, computed once per reach and left alone."""
    if reach not in _sized:
        pairs = []
        for n_src in N_SRC:
            src, tgt = edge_scene(4097, n_src, seed=4097 + n_src)
            pairs += [(src, tgt[:n]) for n in N_TGT]
        _sized[reach] = (pairs, [gpu.icpAlign(s, t, max_correspondence_distance=reach) for s, t in pairs])
    return _sized[reach]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("reach", [30.0, 1.0])
def test_sources_of_every_size_in_one_call(gpu, reach, reverse):
    """A grid sized by the largest pair's rows must not change what a smaller pair sums: its surplus workgroups return at entry
    (they would write rows into the next pair's stretch), the fold takes its own rows, the stride is its own rows * 256. (The
    stride alone cannot show here: a launch has the most rows of any pair and only a pair at the cap of 256 rows strides, see
    DESIGN.md section 12.)"""
    pairs, want = _sized_pairs(gpu, reach)
    order = list(range(len(pairs)))[::-1] if reverse else list(range(len(pairs)))
    got = gpu.debugIcpAlignPairsDevice([pairs[k] for k in order], max_correspondence_distance=reach)
    print("iterations per pair", [want[k][3] for k in order])
    for g, k in zip(got, order):
        try:
            _same(g, want[k])
        except AssertionError as e:
            raise AssertionError(f"n_src {len(pairs[k][0])}, n_tgt {len(pairs[k][1])}: {e}") from None
    if reach == 30.0:
        assert want[-1][3] > 1 and want[-4][3] > 1                  # the large pairs need several iterations


# ---- the number of pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 9, 64])
def test_one_pair_nine_and_sixty_four(gpu, P):
    src, tgt, _ = icp_scene(1500, 700, 2)
    _pairs(gpu, [(src[:700 - 7 * k], tgt[:1500 - 11 * k]) for k in range(P)], max_correspondence_distance=30.0)


def test_no_pair_and_sixty_five(gpu):
    src, tgt, _ = icp_scene(1500, 700, 2)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignPairsDevice([(src, tgt)] * 65)
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignPairsDevice([])
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignPairsDevice([(src, tgt)], max_iterations=0)
    got = gpu.debugIcpAlignPairsDevice([(src[:0], tgt), (src, tgt[:0]), (src, tgt)], max_correspondence_distance=30.0)
    assert not got[0][1] and got[0][3] == 0 and np.array_equal(got[0][0], np.eye(4, dtype=np.float32))
    _same(got[1], gpu.icpAlign(src, tgt[:0]))
    _same(got[2], gpu.icpAlign(src, tgt, max_correspondence_distance=30.0))


def test_the_same_source_in_several_pairs(gpu):
    src, tgt, _ = icp_scene(1500, 700, 2)
    tgts = [tgt, tgt[:800], tgt[:1023], tgt]
    slots = gpu.debugIcpAlignManyDevice(src, tgts, max_correspondence_distance=30.0)
    got = gpu.debugIcpAlignPairsDevice([(src, t) for t in tgts], max_correspondence_distance=30.0)
    for g, w in zip(got, slots):
        _same(g, w)
    _same(got[0], got[3])


# ---- pairs that end in different ranges -------------------------------------------------------------------------------------
def test_pairs_that_end_in_different_ranges(gpu):
    """Iteration limits of R - 1, R and R + 1 on a scene that needs more, beside a pair that converges inside the first range (its
    target is its source) and a pair with two correspondences (a one-point target, all but two sources out of reach) that ends
    unconverged in its first iteration with the identity: the pairs that have ended idle while the others go on."""
    src0, tgt, _ = icp_scene(6000, 1500, 5)
    src = _moved(src0, 2.0)
    few = src[:300].copy()
    few[2:, :3] += np.float32(1000.0)                             # two sources within 30 m of tgt[:1]
    few[:2, :3] = tgt[0, :3] + np.array([[0.5, 0, 0], [0, 0.25, 0]], np.float32)
    kw = dict(max_correspondence_distance=30.0, transformation_epsilon=1e-12, euclidean_fitness_epsilon=1e-14)
    for m in (R - 1, R, R + 1):
        want = _pairs(gpu, [(src, tgt), (src[:900], src[:900].copy()), (few, tgt[:1]), (src[:1200], tgt[:3000])], max_iterations=m, **kw)
        assert want[0][3] == m and want[1][3] < R - 1, (m, want[0][3], want[1][3])
        assert (want[2][1], want[2][3]) == (False, 0) and np.array_equal(want[2][0], np.eye(4, dtype=np.float32))
    want = _pairs(gpu, [(src, tgt), (src[:900], src[:900].copy()), (few, tgt[:1]), (src[:1200], tgt[:3000]), (src, tgt[:1000])], **kw)
    print("iterations per pair", [w[3] for w in want])
    assert want[0][3] > R + 1 and want[1][3] < R
    assert len({(w[3] - 1) // R for w in want if w[3] > 0}) > 1   # the pairs end in different ranges


def test_a_one_point_target_at_a_reach_of_one_metre(gpu):
    """The pair of test_targets_of_every_size_in_one_call that has fewer than 3 correspondences: it ends in its first iteration
    while the pairs beside it run on."""
    src, tgt = edge_scene(4097, 257, seed=4097 + 257)
    src3, _ = edge_scene(4097, 3, seed=4097 + 3)
    want = _pairs(gpu, [(src, tgt), (src, tgt[:1]), (src3, tgt[:1025]), (src[:100], tgt[:2])], max_correspondence_distance=1.0)
    assert (want[1][1], want[1][3]) == (False, 0) and np.array_equal(want[1][0], np.eye(4, dtype=np.float32))
    assert want[0][3] > 1


# ---- non-finite input, ties, fallback lists, guesses ---------------------------------------------------------------------
def test_pairs_with_non_finite_points(gpu):
    src, tgt = edge_scene(4097, 700, seed=11)
    bad = tgt.copy()
    for k, j in enumerate(range(0, bad.shape[0], 7)):
        bad[j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    bad[1023, :3] = np.nan; bad[1024, 0] = np.inf; bad[4096, 2] = -np.inf
    none = tgt[:64].copy()
    none[:, :3] = np.nan                                         # no finite target at all: no source has a match
    bad_src = src[:513].copy()
    bad_src[5, 0] = np.nan; bad_src[9, 2] = np.inf; bad_src[512, 1] = -np.inf
    want = _pairs(gpu, [(src, tgt), (src[:300], bad), (bad_src, tgt[:1500]), (src[:257], none), (bad_src, bad)],
                  max_correspondence_distance=30.0)
    assert want[1][1] and np.isfinite(want[1][2]) and not want[3][1]
    assert want[4][1] and np.isfinite(want[4][2])


def test_a_pair_with_exact_ties(gpu):
    src, tgt = tie_scene(n_src=257)
    shifted = tgt.copy()
    shifted[:, 0] += np.float32(0.25)                            # no ties in this pair
    src256, _ = tie_scene(n_src=256)
    pairs = [(src, shifted), (src, tgt), (src256, tgt), (src[:100], tgt[:2048])]
    want = _pairs(gpu, pairs, max_correspondence_distance=30.0, max_iterations=1)
    assert want[1][3] == 1 and abs(want[1][0][0, 3] - 0.5) < 1e-5
    _pairs(gpu, pairs, max_correspondence_distance=30.0)


@pytest.mark.parametrize("tuning", [(0.5, 1, 1), (0.0, 0, 0)])
def test_fallback_lists_and_brute_force(gpu, tuning):
    """Small cells and one shell, so that every pair has a non-empty fallback list of its own length; and the brute force alone."""
    src, tgt, _ = icp_scene(1500, 700, 2)
    edge_src, edge_tgt = edge_scene(1025, 300, seed=1325)
    try:
        gpu.debugIcpTuning(*tuning)
        if tuning[2]:
            for s, t in ((src, tgt), (edge_src, edge_tgt), (src[:257], tgt[:1023])):
                assert gpu.debugIcpNearest(s, t, 1)[1] > 0        # the list is not empty
        _pairs(gpu, [(src, tgt), (edge_src, edge_tgt), (src[:257], tgt[:1023]), (src[:3], tgt[:5])], max_correspondence_distance=30.0)
    finally:
        gpu.debugIcpTuning()


def test_one_pair_with_a_guess(gpu):
    src, tgt, T_true = icp_scene(1500, 700, 2)
    edge_src, edge_tgt = edge_scene(1025, 257, seed=1282)
    G = T_true.astype(np.float32)
    G[:3, 3] += np.array([0.05, -0.02, 0.01], np.float32)
    pairs = [(edge_src, edge_tgt), (src, tgt), (src[:500], tgt[:1023])]
    guesses = [None, G, np.eye(4, dtype=np.float32)]              # (the identity is no guess, as PCL tests it)
    got = gpu.debugIcpAlignPairsDevice(pairs, guesses=guesses, max_correspondence_distance=30.0)
    _same(got[0], gpu.icpAlign(edge_src, edge_tgt, max_correspondence_distance=30.0))
    guessed = gpu.icpAlignGuess(src, tgt, G, max_correspondence_distance=30.0)
    _same(got[1], guessed)
    _same(got[2], gpu.icpAlign(src[:500], tgt[:1023], max_correspondence_distance=30.0))
    plain = gpu.icpAlign(src, tgt, max_correspondence_distance=30.0)
    assert guessed[3] != plain[3] or not np.array_equal(guessed[0], plain[0])      # the guess changed the alignment's course
    bad = G.copy()
    bad[3, 3] = 2.0
    with pytest.raises(s2m.S2MError, match="INVALID_ARG"):
        gpu.debugIcpAlignPairsDevice(pairs, guesses=[None, bad, None])


# ---- stale state -----------------------------------------------------------------------------------------------------------
def test_calls_in_a_row_regrow_and_leave_nothing_behind():
    """A small call, a larger one with more pairs and larger clouds (the buffers grow), the small one again (stale per-pair state:
    the list counts, the done flags, the cell counts), then the slotted and the single device loop on the same handle."""
    g = s2m.MapOptimizationS2M()
    try:
        src_a, tgt_a = edge_scene(1025, 257, seed=1282)
        src_b, tgt_b, _ = icp_scene(6000, 1500, 5)
        small = [(src_a, tgt_a), (src_a[:100], tgt_a[:3])]
        first = _pairs(g, small, pairs_first=True, max_correspondence_distance=30.0)
        _pairs(g, [(src_b, tgt_b[:4097]), (src_b[:700], tgt_b), (src_a, tgt_b[:1023]), (src_b[:3], tgt_b[:2000]), (src_b, tgt_b[:300])],
               pairs_first=True, max_correspondence_distance=30.0)
        again = g.debugIcpAlignPairsDevice(small, max_correspondence_distance=30.0)
        for a, b in zip(again, first):
            _same(a, b)
        one = g.debugIcpAlignPairsDevice(small[1:], max_correspondence_distance=30.0)
        _same(one[0], first[1])
        many = g.debugIcpAlignManyDevice(src_a, [tgt_a, tgt_a[:3]], max_correspondence_distance=30.0)
        _same(many[0], first[0])
        _same(many[1], g.icpAlign(src_a, tgt_a[:3], max_correspondence_distance=30.0))
        _same(g.debugIcpAlignDevice(src_a, tgt_a, max_correspondence_distance=30.0), first[0])
        _same(g.debugIcpAlignPairsDevice(small, max_correspondence_distance=30.0)[0], first[0])
    finally:
        g.close()
