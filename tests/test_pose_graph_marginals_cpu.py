"""CPU tests of the block marginals' host side (include/liorf_s2m.h, s2m_pg_marginals / s2m_pg_joint_marginal): the exported
symbols, s2m_pg_marginals_check_args, the pass size the Python mirror states, and the golden bounds file."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_marginals_ref as M  # noqa: E402
from liorf_amd import s2m  # noqa: E402

SYMBOLS = ["s2m_pg_marginals_check_args", "s2m_pg_marginals", "s2m_pg_joint_marginal"]


def test_symbols_are_declared_bound_and_exported():
    lib = s2m.load_library()
    header = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in s2m.ABI_SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(lib, name).argtypes, name
    for name in ("pgMarginals", "pgJointMarginal"):
        assert callable(getattr(s2m.MapOptimizationS2M, name))
    assert callable(s2m.pg_marginals_check_args)


def test_pass_size_matches_the_header_and_holds_a_joint_marginal():
    header = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    cols = int(re.search(r"#define\s+S2M_PG_BLOCK_COLUMNS\s+(\d+)", header).group(1))
    assert cols == s2m.S2M_PG_BLOCK_COLUMNS and cols >= 12 and cols % 6 == 0
    assert s2m.PG_MARGINALS_KEYS_PER_PASS == cols // 6


def test_check_args_verdicts():
    chk = s2m.pg_marginals_check_args
    n, bad = 7, -1
    assert chk(n, None, 0) == 0 and chk(n, [], 0) == 0 and chk(0, None, 0) == 0      # n_keys == 0
    assert chk(n, [3, 3, 3]) == 0                                                    # repeats
    assert chk(n, [0]) == 0 and chk(n, [n - 1]) == 0 and chk(n, [0, n - 1, 0]) == 0
    assert chk(n, None, 2) == bad                                                    # null keys with n_keys > 0
    assert chk(n, [1, 2], -1) == bad and chk(n, None, -1) == bad
    assert chk(n, [-1]) == bad and chk(n, [n]) == bad
    assert chk(n, [0, 1, -1]) == bad and chk(n, [0, n, 1]) == bad                    # wherever the bad key stands
    assert chk(0, [0]) == bad                                                        # an empty graph has no key


def test_bounds_file_has_a_bound_for_every_floor():
    b = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_marginals_bounds.json")))
    assert set(b) == {M.case_id(*c) for c in M.CASES}
    for name, a, k in M.CASES:
        c = b[M.case_id(name, a, k)]
        assert c["keys"] == [a, k]
        assert set(c["floor"]) == {"joint_" + t for t in M.TYPES} == set(c["bound"])
        for key, v in c["bound"].items():
            assert v == pytest.approx(10 * c["floor"][key], rel=1e-12, abs=0.0)      # a hand-edited bound is caught
