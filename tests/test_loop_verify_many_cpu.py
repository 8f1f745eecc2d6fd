"""The host-only parts of s2m_loop_verify_many: the argument checks (s2m_loop_verify_many_check_args, the verdict the call gives
before any device work) and the plan of its passes (s2m_debug_loop_verify_many_plan) against a ten-line model."""
import ctypes as C

import numpy as np
import pytest

from liorf_amd import s2m

N = 32
OK, BAD = 0, -1                   # S2M_OK, S2M_ERR_INVALID_ARG
GOOD = [(N - 1, [0, 1]), (N - 2, [2, 3])]


@pytest.mark.parametrize("base_key", [-1, 0])
@pytest.mark.parametrize("rows,kw,want", [
    (GOOD, {}, OK),
    ([(31, [16, 4, 0, 24, 2]), (30, [0, 1, 14]), (29, [2]), (20, []), (28, [3, 12])], {}, OK),
    ([(N - 1, [0, 1]), (N - 2, [2]), (N - 1, [3])], {}, BAD),            # a repeated key_cur
    ([(N - 1, [0, 1]), (N - 1, []), (N - 2, [3])], {}, OK),              # ... but not in a row without candidates
    ([(N - 2, [0]), (N, [1])], {}, BAD),                                 # keys out of range
    ([(N - 2, [0]), (-1, [1])], {}, BAD),
    ([(N - 2, [0]), (N - 1, [1, N])], {}, BAD),
    ([(N - 2, [0]), (N - 1, [1, -1])], {}, BAD),
    ([(N - 2, [0]), (N, [])], {}, OK),                                   # (a row without candidates names no key)
    ([(N - 2, [0]), (N - 1, [1, N - 1])], {}, BAD),                      # a candidate equal to its key_cur
    ([(N - 2, [0]), (N - 1, [1, 2, 1])], {}, BAD),                       # a candidate twice in a row
    ([(N - 2, [1]), (N - 1, [1])], {}, OK),                              # ... but the same candidate in two rows
    (GOOD, dict(row_stride=0), BAD),
    (GOOD, dict(row_stride=9), BAD),
    ([(N - 1, list(range(8)))], {}, OK),
    ([(N - 1, list(range(9)))], {}, BAD),
    (GOOD, dict(n_cand=[2, 3]), BAD),                                    # n_cand[r] > row_stride
    (GOOD, dict(n_cand=[2, -1]), BAD),
    (GOOD, dict(n_cand=[0, 0]), OK),
    (GOOD, dict(m=-1), BAD),
    (GOOD, dict(m=0), OK),
    (None, dict(m=0), OK),
    (None, dict(m=2, row_stride=2), BAD),                                # null arrays with m > 0
])
def test_argument_table(rows, kw, want, base_key):
    assert s2m.loop_verify_many_check_args(N, rows, base_key, **kw) == want


def test_arguments_that_do_not_depend_on_the_rows():
    assert s2m.loop_verify_many_check_args(N, GOOD, N) == BAD                              # base_key out of range
    assert s2m.loop_verify_many_check_args(N, GOOD, -2) == BAD
    assert s2m.loop_verify_many_check_args(-1, GOOD) == BAD
    assert s2m.loop_verify_many_check_args(0, [(5, [0, 1]), (5, [7])]) == BAD              # an empty store: a repeat is still one
    assert s2m.loop_verify_many_check_args(0, [(5, [0, 1]), (6, [7])]) == OK               # ... and keys are not looked at
    assert s2m.loop_verify_many_check_args(N, GOOD, -1, s2m.default_loop_params(search_radius=-1.0)) == BAD
    assert s2m.loop_verify_many_check_args(N, GOOD, -1, s2m.default_loop_params(search_num=2)) == OK
    lib = s2m.load_library()
    kc, kp, nc, stride = s2m._verify_many_rows(GOOD)
    for arrays in ((None, kp, nc), (kc, None, nc), (kc, kp, None)):
        assert lib.s2m_loop_verify_many_check_args(N, *arrays, 2, stride, -1, None) == BAD


def _model(n_cand, per_pass):
    """Passes are filled in order; a row goes to the next pass when it does not fit; a row is never split."""
    first, used = [], 0
    for r, n in enumerate(n_cand):
        if r == 0 or used + n > per_pass:
            first.append(r)
            used = 0
        used += n
    return first + [len(n_cand)]


def _clamped(per_pass):
    return s2m.S2M_LOOP_MANY_MAX_PAIRS if per_pass == 0 else min(max(per_pass, s2m.S2M_LOOP_MAX_CANDIDATES), s2m.S2M_LOOP_MANY_MAX_PAIRS)


@pytest.mark.parametrize("per_pass", [0, 1, 8, 9, 13, 63, 64, 1000])
def test_plan_against_the_model(per_pass):
    rng = np.random.default_rng(per_pass)
    cases = [[], [0], [0, 0, 0], [8], [8] * 20, [5, 3, 1, 0, 2], [1] * 200, [0, 8, 0, 8, 0], [7, 2, 7, 2], [4] * 33]
    cases += [list(rng.integers(0, 9, int(m))) for m in (1, 2, 17, 64, 65, 300)]
    for n_cand in cases:
        plan = s2m.loop_verify_many_plan(n_cand, per_pass)
        cap = _clamped(per_pass)
        assert plan == _model(n_cand, cap), (n_cand, per_pass)
        assert plan[0] == 0 if n_cand else plan == [0]
        assert plan[-1] == len(n_cand) and all(a < b for a, b in zip(plan, plan[1:]))      # in order, no empty pass, every row once
        for a, b in zip(plan, plan[1:]):
            assert sum(n_cand[a:b]) <= cap                                                 # a pass holds whole rows within its room
            if b < len(n_cand):
                assert sum(n_cand[a:b + 1]) > cap                                          # ... and is full: the next row did not fit


def test_plan_edges():
    assert s2m.loop_verify_many_plan([], 8) == [0]                                         # m = 0: no pass
    assert s2m.loop_verify_many_plan([8], 1) == [0, 1]                                     # a row of 8 fits at the smallest pass size
    assert s2m.loop_verify_many_plan([8, 8, 8], 8) == [0, 1, 2, 3]
    assert s2m.loop_verify_many_plan([0, 0, 8, 0, 0, 8], 8) == [0, 5, 6]                   # rows without candidates take no room
    assert s2m.loop_verify_many_plan([8] * 8 + [1], 0) == [0, 8, 9]
    lib = s2m.load_library()
    first, n_pass = (C.c_int32 * 4)(), C.c_int32(7)
    bad = (C.c_int32 * 3)(1, 9, 1)
    assert lib.s2m_debug_loop_verify_many_plan(bad, 3, 8, first, C.byref(n_pass)) == BAD and n_pass.value == 7
    assert lib.s2m_debug_loop_verify_many_plan(bad, -1, 8, first, C.byref(n_pass)) == BAD
    assert lib.s2m_debug_loop_verify_many_plan(None, 3, 8, first, C.byref(n_pass)) == BAD
    assert lib.s2m_debug_loop_verify_many_plan(bad, 3, 8, None, C.byref(n_pass)) == BAD
