"""The many-query form of the ScanContext place query without a GPU (include/liorf_s2m.h, "The place query for many queries at
once"): the model's searched set with both windows, s2m_sc_query_many_check_args against every row of
the header's error table, and the session-wide query on the store in which the reference's detector misses the only loop."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import sc_query_many_ref as M
import sc_query_ref as Q

from liorf_amd import s2m
from oracle import oracle as O

OK, INVALID = s2m.S2M_OK, -1
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


def test_defaults_and_layout():
    p = s2m.default_sc_query_many_params()
    assert (p.q.first, p.q.count, p.q.exclude_lo, p.q.exclude_hi, p.q.top_k, p.q.align, p.q.max_dist) == (0, -1, 0, 0, 1, s2m.S2M_SC_ALIGN_SECTOR_KEY, 0.3)
    assert (p.rel_lo, p.rel_hi) == (0, 0)
    assert s2m.load_library().s2m_sc_query_many_default_params(None) == INVALID
    import ctypes as C
    assert C.sizeof(s2m.ScQueryManyParams) == C.sizeof(s2m.ScQueryParams) + 8
    t, b = s2m.sc_query_many_shape()
    assert t >= 1 and b >= 1
    assert s2m.load_library().s2m_debug_sc_query_many_shape(None, None) == INVALID


def test_relative_window_clipped_at_both_ends_of_the_range():
    # range [10, 30): a window around key 12 reaches below the range, one around key 28 above it
    assert M.searched_keys(40, 12, first=10, count=20, rel_lo=-5, rel_hi=3) == list(range(15, 30))
    assert M.searched_keys(40, 28, first=10, count=20, rel_lo=-3, rel_hi=9) == list(range(10, 25))
    assert M.searched_keys(40, 20, first=10, count=20, rel_lo=-100, rel_hi=100) == []
    # a window that lies outside the range, an empty and a reversed one: the single query's set
    assert M.searched_keys(40, 2, first=10, count=20, rel_lo=-2, rel_hi=3) == list(range(10, 30))
    assert M.searched_keys(40, 20, first=10, count=20, rel_lo=4, rel_hi=4) == list(range(10, 30))
    assert M.searched_keys(40, 20, first=10, count=20, rel_lo=5, rel_hi=-5) == list(range(10, 30))
    # the query's own key is in the set unless a window takes it out
    assert 20 in M.searched_keys(40, 20) and 20 not in M.searched_keys(40, 20, rel_lo=0, rel_hi=1)
    # a descriptor query has no relative window
    assert M.searched_keys(40, None, rel_lo=-100, rel_hi=100) == list(range(40))


def test_union_with_the_fixed_window():
    got = M.searched_keys(40, 20, exclude_lo=5, exclude_hi=12, rel_lo=-2, rel_hi=3)
    assert got == [c for c in range(40) if not (5 <= c < 12) and not (18 <= c < 23)]
    # overlapping and nested windows
    assert M.searched_keys(40, 10, exclude_lo=5, exclude_hi=12, rel_lo=-2, rel_hi=8) == [c for c in range(40) if not (5 <= c < 18)]
    assert M.searched_keys(40, 8, exclude_lo=5, exclude_hi=12, rel_lo=-1, rel_hi=1) == [c for c in range(40) if not (5 <= c < 12)]


def test_rel_hi_int32_max_and_the_detectors_exclusion():
    n = 100
    for key in (0, 29, 30, 31, 99):
        assert M.searched_keys(n, key, **M.DETECTOR_WINDOW) == list(range(0, max(key - 29, 0)))
    # no overflow: the largest key of an int32 store with the largest window
    assert M.searched_keys(5, INT32_MAX - 1, rel_lo=INT32_MIN, rel_hi=INT32_MAX) == []
    assert M.searched_keys(5, 3, rel_lo=INT32_MAX, rel_hi=INT32_MAX) == list(range(5))
    assert M.searched_keys(5, 3, rel_lo=1, rel_hi=INT32_MAX) == [0, 1, 2, 3]


# (n_stored, m, fields, descriptor_query, status): one row of the header's error table per group
ARG_TABLE = [
    (100, 1, {}, False, OK), (100, 1, {}, True, OK), (0, 5, {}, False, OK), (0, 0, {}, True, OK),
    (100, 0, {}, False, OK), (100, -1, {}, False, INVALID), (100, -1, {}, True, INVALID), (100, INT32_MAX, {}, False, OK),
    # what the single query rejects
    (100, 3, {"top_k": 0}, False, INVALID), (100, 3, {"top_k": 32}, False, OK), (100, 3, {"top_k": 33}, False, INVALID),
    (100, 3, {"align": 1}, False, OK), (100, 3, {"align": 2}, False, INVALID), (100, 3, {"align": -1}, True, INVALID),
    (100, 3, {"max_dist": 0.0}, False, INVALID), (100, 3, {"max_dist": float("nan")}, False, INVALID), (100, 3, {"max_dist": 10000000.0}, False, OK),
    (100, 3, {"max_dist": 2e7}, True, INVALID),
    (100, 3, {"first": -1}, False, INVALID), (100, 3, {"first": 100}, False, OK), (100, 3, {"first": 101}, False, INVALID),
    (100, 3, {"count": -2}, False, INVALID), (100, 3, {"count": 101}, False, INVALID), (100, 3, {"first": 40, "count": 61}, True, INVALID),
    (100, 3, {"first": INT32_MAX, "count": INT32_MAX}, False, INVALID), (-1, 3, {}, False, INVALID),
    (100, 3, {"exclude_lo": INT32_MIN, "exclude_hi": INT32_MAX}, True, OK),
    # the relative window: any values for stored keys; on a descriptor query only an empty one
    (100, 3, {"rel_lo": -29, "rel_hi": INT32_MAX}, False, OK), (100, 3, {"rel_lo": INT32_MIN, "rel_hi": INT32_MAX}, False, OK),
    (100, 3, {"rel_lo": 5, "rel_hi": -5}, False, OK),
    (100, 3, {"rel_lo": -29, "rel_hi": INT32_MAX}, True, INVALID), (100, 3, {"rel_lo": 0, "rel_hi": 1}, True, INVALID),
    (100, 3, {"rel_lo": 0, "rel_hi": 0}, True, OK), (100, 3, {"rel_lo": 7, "rel_hi": 7}, True, OK), (100, 3, {"rel_lo": 5, "rel_hi": -5}, True, OK),
    (100, 0, {"rel_lo": 0, "rel_hi": 1}, True, INVALID),
]


@pytest.mark.parametrize("n_stored,m,fields,descriptor_query,status", ARG_TABLE)
def test_argument_table(n_stored, m, fields, descriptor_query, status):
    assert s2m.sc_query_many_check_args(n_stored, m, s2m.default_sc_query_many_params(**fields), descriptor_query) == status


def test_null_params_are_the_defaults():
    assert s2m.sc_query_many_check_args(100, 4, None) == OK and s2m.sc_query_many_check_args(100, 4, None, True) == OK
    assert s2m.sc_query_many_check_args(100, -4, None) == INVALID and s2m.sc_query_many_check_args(-1, 4, None) == INVALID


def test_null_handle():
    lib = s2m.load_library()
    assert lib.s2m_sc_query_keys(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_sc_query_descriptors(None, None, 0, None, None, None) == INVALID
    assert lib.s2m_sc_get_descriptors(None, 0, 0, None) == INVALID
    assert lib.s2m_debug_sc_query_many_pass(None, 0) == INVALID


def test_ring_key_case_over_the_whole_session():
    """All 97 keys with the detector's exclusion, all 60 shifts, 0.3: the session-wide query names (96, 60), the pair the
    oracle's detector does not report."""
    descs = Q.ring_key_case()
    rows = M.query_many(descs, list(range(97)), top_k=4, align=Q.ALIGN_FULL, max_dist=0.3, **M.DETECTOR_WINDOW)
    assert len(rows) == 97 and all(len(rows[k]) == 0 for k in range(30))
    pairs = [(cur, int(h["key"])) for cur, row in enumerate(rows) for h in row]
    assert (96, 60) in pairs and all(pre <= cur - 30 for cur, pre in pairs)
    assert rows[96][0]["key"] == 60 and rows[96][0]["shift"] == 23
    m = O.SCManager()
    for d in descs:
        m.add_descriptor(d)
    lid, _, det = m.detectLoopClosureID()
    m.close()
    assert lid == -1 and 60 not in det["cand_idx"]
