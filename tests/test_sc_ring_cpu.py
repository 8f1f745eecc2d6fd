"""The ring-key prefilter of the ScanContext place query without a GPU (include/liorf_s2m.h, "The place query behind a
ring-key prefilter"): defaults and layout, s2m_sc_ring_check_args against the many-query's table and its
own rows, the model (tests/ref/sc_ring_ref.py) against the reference's nanoflann, on the store in which the detector misses
the only loop, and against the exhaustive model when every searched key is a candidate."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import sc_query_many_ref as M
import sc_query_ref as Q
import sc_ring_ref as R

from liorf_amd import s2m
from oracle import oracle as O
from test_sc_query_many_cpu import ARG_TABLE
from test_scancontext_cpu import make_descriptors, sequence_340

OK, INVALID = s2m.S2M_OK, -1
INT32_MAX = 2**31 - 1


def test_defaults_and_layout():
    p = s2m.default_sc_ring_params()
    assert (p.m.q.first, p.m.q.count, p.m.q.exclude_lo, p.m.q.exclude_hi, p.m.q.top_k, p.m.q.align, p.m.q.max_dist) == (0, -1, 0, 0, 1, s2m.S2M_SC_ALIGN_SECTOR_KEY, 0.3)
    assert (p.m.rel_lo, p.m.rel_hi, p.n_candidates, p.reserved) == (0, 0, 3, 0)
    assert s2m.load_library().s2m_sc_ring_default_params(None) == INVALID
    assert C.sizeof(s2m.ScRingParams) == C.sizeof(s2m.ScQueryManyParams) + 8 == 48
    assert C.sizeof(s2m.ScRingNeighbour) == 8 == s2m.SC_RING_NEIGHBOUR_DTYPE.itemsize == R.NEIGHBOUR_DTYPE.itemsize
    assert s2m.ScRingNeighbour.d2.offset == 0 and s2m.ScRingNeighbour.key.offset == 4
    assert s2m.S2M_SC_RING_MAX_CAND == 256 == R.MAX_CAND
    q = s2m.default_sc_ring_params(n_candidates=8, top_k=4, rel_lo=-29, first=2)
    assert (q.n_candidates, q.m.q.top_k, q.m.rel_lo, q.m.q.first) == (8, 4, -29, 2)
    tile, block, words = s2m.sc_ring_shape()
    assert tile >= 64 and block >= 1 and words >= 256 + 64
    assert s2m.load_library().s2m_debug_sc_ring_shape(None, None, None) == INVALID


@pytest.mark.parametrize("n_stored,m,fields,descriptor_query,status", ARG_TABLE)
def test_many_query_table_passes_through(n_stored, m, fields, descriptor_query, status):
    for c in (1, 3, 256):
        assert s2m.sc_ring_check_args(n_stored, m, s2m.default_sc_ring_params(n_candidates=c, **fields), descriptor_query) == status


@pytest.mark.parametrize("fields,descriptor_query,status", [
    ({"n_candidates": 0}, False, INVALID), ({"n_candidates": 1}, False, OK), ({"n_candidates": 256}, True, OK),
    ({"n_candidates": 257}, False, INVALID), ({"n_candidates": -1}, True, INVALID), ({"reserved": 1}, False, INVALID),
    ({"reserved": 1}, True, INVALID), ({"rel_lo": -29, "rel_hi": INT32_MAX}, True, INVALID), ({"rel_lo": -29, "rel_hi": INT32_MAX}, False, OK),
])
def test_ring_rows_of_the_table(fields, descriptor_query, status):
    assert s2m.sc_ring_check_args(100, 3, s2m.default_sc_ring_params(**fields), descriptor_query) == status


def test_null_params_are_the_defaults():
    assert s2m.sc_ring_check_args(100, 4, None) == OK and s2m.sc_ring_check_args(100, 4, None, True) == OK
    assert s2m.sc_ring_check_args(100, -4, None) == INVALID and s2m.sc_ring_check_args(-1, 4, None) == INVALID


def test_null_handle():
    lib = s2m.load_library()
    assert lib.s2m_sc_ring_neighbours_keys(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_sc_ring_neighbours_descriptors(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_sc_query_keys_ring(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_sc_query_descriptors_ring(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_debug_sc_ring_pass(None, 0) == INVALID
    assert lib.s2m_debug_sc_ring_last(None, None, None) == INVALID


def test_d2_is_the_detectors_statement():
    """On sequence_340 the model's three neighbours over the detector's searched set are the oracle detector's candidates, d2 as
    bits (the oracle restates nanoflann's L2_Adaptor order; tests/golden/sc_ringkey_ref_golden.npz pins it to the reference)."""
    descs = sequence_340()
    keys32 = R.ring_keys(descs)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sc_ringkey_ref_golden.npz"))
    checked = 0
    for i in range(30, 340):
        ns = int(g["n_search"][i])
        nb = R.neighbours(keys32, keys32[i], range(ns), 3)
        assert nb["key"].tolist() == g["cand_idx"][i].tolist()[:len(nb)], i
        assert np.array_equal(nb["d2"].view(np.uint32), g["cand_d2"][i].view(np.uint32)[:len(nb)]), i
        checked += len(nb) == 3
    assert checked == 300                                   # (the first ten detections search a tree of one key)


@pytest.mark.parametrize("k", [3, 16])
def test_model_equals_the_references_nanoflann(k):
    descs = sequence_340()
    keys32 = R.ring_keys(descs)
    if O.nanoflann_ringkey_knn(keys32[:5], keys32[5], 3) is None:
        pytest.skip("oracle/_ref is absent: the reference's nanoflann was not built")
    for i in range(30, 340, 7):
        searched = M.searched_keys(340, i, **M.DETECTOR_WINDOW)
        if not searched:
            continue
        idx, d2, found = O.nanoflann_ringkey_knn(keys32[:len(searched)], keys32[i], k)
        nb = R.neighbours(keys32, keys32[i], searched, k)
        assert found == len(nb) == min(k, len(searched))
        assert idx[:found].tolist() == nb["key"].tolist(), i
        assert np.array_equal(d2[:found].view(np.uint32), nb["d2"].view(np.uint32)), i


def test_ring_key_case():
    """Six keys tie the revisited place's ring key and take the detector's three slots: C = 3 misses the loop as the detector
    does, C = 8 names (96, 60) at shift 23 in both alignments."""
    descs = Q.ring_key_case()
    keys32 = R.ring_keys(descs)
    nb3 = R.neighbours_many(descs, [96], 3, keys32=keys32, **M.DETECTOR_WINDOW)[0]
    nb8 = R.neighbours_many(descs, [96], 8, keys32=keys32, **M.DETECTOR_WINDOW)[0]
    assert nb3["key"].tolist() == [3, 4, 5] and nb8["key"].tolist() == [3, 4, 5, 6, 7, 8, 60, 42]
    assert len(set(nb8["d2"][:7].view(np.uint32).tolist())) == 1 and nb8["d2"][7] > nb8["d2"][6]   # seven tie: the key decides
    for align in (Q.ALIGN_SECTOR_KEY, Q.ALIGN_FULL):
        kw = dict(top_k=4, align=align, max_dist=0.3, keys32=keys32, **M.DETECTOR_WINDOW)
        assert len(R.query_many_ring(descs, [96], 3, **kw)[0]) == 0
        row = R.query_many_ring(descs, [96], 8, **kw)[0]
        assert len(row) == 1 and row[0]["key"] == 60 and row[0]["shift"] == 23
        assert abs(row[0]["dist"] - 9.78742063e-05) < 1e-13      # (the issue states it to nine digits)
    m = O.SCManager()
    for d in descs:
        m.add_descriptor(d)
    lid, _, det = m.detectLoopClosureID()
    m.close()
    assert lid == -1 and 60 not in det["cand_idx"] and det["cand_idx"] == [3, 4, 5]


def test_enough_candidates_give_the_exhaustive_rows():
    descs = make_descriptors(40, seed=11)
    queries = [0, 17, 39, 17] + [descs[5] * 0.5]
    for window in (dict(), dict(first=3, count=30, exclude_lo=10, exclude_hi=14), dict(rel_lo=-4, rel_hi=5)):
        stored_only = "rel_lo" in window
        qs = queries[:4] if stored_only else queries
        for align in (Q.ALIGN_SECTOR_KEY, Q.ALIGN_FULL):
            kw = dict(top_k=5, align=align, max_dist=Q.BIG, **window)
            want = M.query_many(descs, qs, **kw)
            assert M.same_rows(R.query_many_ring(descs, qs, 40, **kw), want)
            assert M.same_rows(R.query_many_ring(descs, qs, 256, **kw), want)
            assert not M.same_rows(R.query_many_ring(descs, qs, 2, **kw), want)
