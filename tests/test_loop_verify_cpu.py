"""CPU checks of the loop-closure verification (include/liorf_s2m.h, "Verification: one key against several candidates"): the
argument table of s2m_loop_verify_check_args (host code of the library, no handle, no GPU) and the model of *best - the accepted
record with the least (icp.fitness_score, position) - pinned on hand-made records."""
import pytest

from liorf_amd import s2m

OK, INVALID = s2m.S2M_OK, -1
NEW = ["s2m_loop_verify_check_args", "s2m_loop_verify_launch", "s2m_loop_verify_poll", "s2m_loop_verify_collect", "s2m_loop_verify",
       "s2m_debug_icp_align_many_device"]


def test_symbols_are_exported_and_listed():
    lib = s2m.load_library()
    for name in NEW:
        assert name in s2m.ABI_SYMBOLS and hasattr(lib, name), name
    assert s2m.S2M_LOOP_MAX_CANDIDATES == 8
    for name in ("loopVerify", "loopVerifyLaunch", "loopVerifyPoll", "loopVerifyCollect", "performSCLoopClosureVerified",
                 "debugIcpAlignManyDevice"):
        assert callable(getattr(s2m.MapOptimizationS2M, name)), name


# (n_stored, key_cur, candidates, base_key, status)
ARG_TABLE = [
    (32, 31, [0], -1, OK), (32, 31, [16, 4, 0, 24, 2], -1, OK), (32, 31, [0, 1, 16, 2], 0, OK),
    (32, 31, list(range(8)), -1, OK), (32, 31, list(range(9)), -1, INVALID), (32, 31, [], -1, INVALID),      # n_cand in [1, 8]
    (32, 31, [32], -1, INVALID), (32, 31, [-1], -1, INVALID), (32, 31, [0, 5, 32], -1, INVALID),             # a key outside the store
    (32, 32, [0], -1, INVALID), (32, -1, [0], -1, INVALID), (32, 31, [0], 32, INVALID), (32, 31, [0], -2, INVALID),
    (32, 31, [0], 31, OK), (32, 0, [31, 30], -1, OK),
    (32, 31, [4, 4], -1, INVALID), (32, 31, [0, 1, 2, 0], -1, INVALID), (32, 31, [7, 6, 5, 4, 3, 2, 1, 7], 0, INVALID),   # listed twice
    (32, 31, [31], -1, INVALID), (32, 31, [0, 31], 0, INVALID), (32, 5, [4, 6, 5], -1, INVALID),              # key_cur among them
    (1, 0, [0], -1, INVALID),                                                                                # (its only key is key_cur)
    (0, 31, [0, 1], -1, OK), (0, 0, [0, 0], -1, OK), (0, 31, list(range(9)), -1, INVALID), (0, 31, [], -1, INVALID),   # an empty store
    (-1, 0, [0], -1, INVALID),
]


@pytest.mark.parametrize("n_stored,key_cur,cand,base_key,status", ARG_TABLE)
def test_argument_table(n_stored, key_cur, cand, base_key, status):
    assert s2m.loop_verify_check_args(n_stored, key_cur, cand, base_key) == status


def test_null_list_and_parameters():
    assert s2m.loop_verify_check_args(32, 31, None, -1, n_cand=1) == INVALID
    assert s2m.loop_verify_check_args(32, 31, [0], -1, s2m.default_loop_params()) == OK
    for bad in (dict(search_radius=0.0), dict(search_num=-1), dict(icp_leaf=0.0), dict(fitness_score=float("nan"))):
        assert s2m.loop_verify_check_args(32, 31, [0], -1, s2m.default_loop_params(**bad)) == INVALID, bad
    assert s2m.loop_verify_check_args(32, 31, [0], -1, s2m.default_loop_params(fitness_score=-1.0)) == OK


def _rec(status, fitness):
    r = s2m.LoopResult()
    r.status, r.icp.fitness_score = status, fitness
    return r


A, RJ, FEW, CLOSED = s2m.S2M_LOOP_ACCEPTED, s2m.S2M_LOOP_REJECTED, s2m.S2M_LOOP_TOO_FEW_POINTS, s2m.S2M_LOOP_ALREADY_CLOSED


@pytest.mark.parametrize("records,best", [
    ([(A, 0.2)], 0), ([(RJ, 0.2)], -1), ([], -1),
    ([(RJ, 12.1), (RJ, 0.65), (A, 0.0089), (RJ, 0.65), (A, 0.0088)], 4),
    ([(A, 0.25), (A, 0.1), (A, 0.1), (A, 0.3)], 1),                  # a tie at equal fitness: the earlier position
    ([(A, 0.0), (A, 0.0)], 0),
    ([(RJ, 0.001), (A, 0.29)], 1),                                  # a rejected record (not converged) never wins, whatever its fitness
    ([(FEW, 0.0), (A, 0.2), (FEW, 0.0)], 1), ([(CLOSED, 0.0)] * 3, -1),
    ([(RJ, 0.4), (FEW, 0.0), (s2m.S2M_LOOP_PENDING, 0.0), (s2m.S2M_LOOP_NONE, 0.0)], -1),   # none accepted
])
def test_model_of_best(records, best):
    assert s2m.loop_verify_best([_rec(s, f) for s, f in records]) == best
