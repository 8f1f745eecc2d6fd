"""CPU side of the loop detection by position for many keys (include/liorf_s2m.h, s2m_loop_detect_keys): the model
(tests/ref/loop_detect_many_ref.py) against the numpy restatement of detectLoopClosureDistance() in test_loop_closure_cpu.py,
the visibility of every wrong reading on the fixed case list the GPU tests run, the conditions on the generated stores, and the
argument table through s2m_loop_detect_keys_check_args, which needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import loop_detect_many_ref as M  # noqa: E402

from liorf_amd import s2m  # noqa: E402
from test_loop_closure_cpu import detect_loop, scripted_revisit  # noqa: E402

OK, BAD = s2m.S2M_OK, -1                                                    # S2M_ERR_INVALID_ARG
INT32_MAX = M.INT32_MAX


@pytest.fixture(scope="module")
def shape():
    t, b, s = s2m.loop_detect_shape()
    assert t >= 2 and b >= 2 and 1 <= s
    return t, b, s


@pytest.fixture(scope="module")
def cases(shape):
    """The fixed case list with the model's rows, computed once."""
    stores = {}
    out = []
    for name, N, keys, tc, kw in M.fixed_cases(shape[0], shape[1]):
        if N not in stores:
            stores[N] = M.make_store(N)
        P, t = stores[N]
        out.append((name, N, keys, tc, kw, M.detect_keys(P, t, keys, tc, **kw)))
    return stores, out


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1], b[1])) and np.array_equal(a[2], b[2])


def _as_detector(P, t, time_cur, R, W):
    """What s2m_loop_closure_rs reports from the row of {N-1}: (N-1, key_pre) or (-1, -1)."""
    N = len(t)
    rows, _, n = M.detect_keys(P, t, [N - 1], [time_cur], search_radius=R, time_diff_s=W, top_k=1)
    if n[0] == 0 or rows[0][0] == N - 1:
        return -1, -1
    return N - 1, rows[0][0]


def test_the_model_is_the_detector_on_the_scripted_revisit():
    _, poses, times, _ = scripted_revisit()
    found = set()
    for R in (10.0, 15.0, 25.0):
        for W in (30.0, 20.0, 5.0):
            for tc in (31.0, 31.5, 40.0, 0.0):
                want = detect_loop(poses[:, :3], times, tc, R, W)
                assert _as_detector(poses[:, :3], times, tc, R, W) == want, (R, W, tc)
                found.add(want[1])
    assert {-1, 0} <= found                                                 # (the revisit's loop and the empty case)


def test_the_model_is_the_detector_on_random_lattice_stores():
    rng = np.random.default_rng(11)
    own = loops = none = 0
    for case in range(300):
        N = int(rng.integers(1, 90))
        P = (rng.integers(-24, 25, (N, 3)) * 0.25).astype(np.float32)
        if N > 1 and case % 3 == 0:
            P[N - 1] = P[int(rng.integers(0, N - 1))] + np.float32(0.25) * rng.integers(-1, 2, 3).astype(np.float32)
        t = 0.5 * rng.integers(0, 160, N).astype(np.float64)
        tc = float(t[N - 1] + rng.choice([0.0, 0.5, 4.0, 4.5, 30.0, 80.0]))
        R, W = float(rng.choice([2.0, 5.0, 10.0])), float(rng.choice([4.0, 30.0]))
        want = detect_loop(P, t, tc, R, W)
        assert _as_detector(P, t, tc, R, W) == want, case
        rows, _, n = M.detect_keys(P, t, [N - 1], [tc], search_radius=R, time_diff_s=W, top_k=1)
        own += int(n[0] == 1 and rows[0][0] == N - 1)
        loops += int(want[1] >= 0)
        none += int(n[0] == 0)
    print("nearest passing candidate is N-1 itself:", own, "loops:", loops, "empty rows:", none)
    assert own >= 10 and loops >= 30 and none >= 10


def test_every_store_has_full_partial_and_empty_rows(cases):
    """No test may skip or mask rows: over the cases of every generated store there is a row with n_cand == top_k, one with
    0 < n_cand < top_k and an empty one; the planted edges are there - exact ties in d2, d2 == r2, |dt| == W, more than 8
    candidates in the radius."""
    stores, listed = cases
    for N, (P, t) in stores.items():
        full = part = empty = False
        for name, n_store, keys, tc, kw, (rows, d2, n) in listed:
            if n_store != N:
                continue
            k = kw["top_k"]
            full |= bool(np.any(n == k))
            part |= bool(np.any((n > 0) & (n < k)))
            empty |= bool(np.any(n == 0))
        assert full and part and empty, (N, full, part, empty)
    P, t = stores[max(stores)]
    N = len(t)
    r2 = np.float32(100.0)
    ties = at_r2 = at_w = crowded = 0
    for q in range(N):
        d2 = M.d2_to(P, P[q])
        late = np.abs(t - t[q]) > 30.0
        near = np.flatnonzero((d2 < r2) & late)
        ties += int(len(np.unique(d2[near])) < len(near))
        at_r2 += int(np.any((d2 == r2) & late))
        at_w += int(np.any((d2 < r2) & (np.abs(t - t[q]) == 30.0)))
        crowded += int(len(near) > 8)
    print("queries with ties:", ties, "with d2 == r2:", at_r2, "with |dt| == W:", at_w, "with more than 8 candidates:", crowded)
    assert ties and at_r2 and at_w and crowded


def test_every_variant_is_visible_on_the_fixed_case_list(cases):
    stores, listed = cases
    for v in M.VARIANTS:
        seen = [name for name, N, keys, tc, kw, want in listed if not _same(M.detect_keys(*stores[N], keys, tc, variant=v, **kw), want)]
        print(v, "differs on", len(seen), "of", len(listed), "cases")
        assert seen, v


def test_rows_depend_on_their_own_query_alone(cases):
    stores, _ = cases
    N = max(stores)
    P, t = stores[N]
    keys = M.draw_keys(N, 40, seed=5)
    tc = M.time_cur_for(t, keys, seed=5)
    rows, d2, n = M.detect_keys(P, t, keys, tc, top_k=3)
    for i in (0, 7, 39):
        r1, d1, n1 = M.detect_keys(P, t, keys[i:i + 1], tc[i:i + 1], top_k=3)
        assert r1[0] == rows[i] and n1[0] == n[i]


def test_the_models_rows_are_rows_of_loop_verify_many(cases):
    stores, listed = cases
    checked = 0
    for name, N, keys, tc, kw, (rows, d2, n) in listed:
        if tc is not None or len(set(int(k) for k in keys)) != len(keys):
            continue                                                        # verify_many asks for distinct key_cur, no key against itself
        as_rows = [(int(k), r) for k, r in zip(keys, rows)]
        assert s2m.loop_verify_many_check_args(N, as_rows, base_key=-1, row_stride=kw["top_k"]) == OK, name
        checked += 1
    assert checked >= 10


def test_default_params():
    p = s2m.default_loop_detect_params()
    assert C.sizeof(p) == 40
    assert (p.search_radius, p.time_diff_s, p.first, p.count) == (10.0, 30.0, 0, -1)
    assert (p.exclude_lo, p.exclude_hi, p.rel_lo, p.rel_hi, p.top_k, p.reserved) == (0, 0, 0, 0, 1, 0)
    lp = s2m.default_loop_params()
    assert (p.search_radius, p.time_diff_s) == (lp.search_radius, lp.time_diff_s)
    assert s2m.load_library().s2m_loop_detect_default_params(None) == BAD
    with pytest.raises(AttributeError):
        s2m.default_loop_detect_params(no_such_field=1)


def argument_table(N=50):
    """(name, n_stored, keys, m or None, parameter fields or None for a null pointer, verdict)."""
    return [
        ("defaults", N, [0, N - 1, 3, 3], None, None, OK),
        ("m == 0", N, [], None, {}, OK),
        ("m == 0, null keys", N, None, 0, {}, OK),
        ("m < 0", N, [1], -1, {}, BAD),
        ("null keys, m > 0", N, None, 2, {}, BAD),
        ("key -1", N, [0, -1], None, {}, BAD),
        ("key N", N, [N], None, {}, BAD),
        ("key N - 1", N, [N - 1], None, {}, OK),
        ("n_stored < 0", -1, [], None, {}, BAD),
        ("empty store, any keys", 0, [5, -3], None, {}, OK),
        ("empty store, first 1", 0, [], None, dict(first=1), BAD),
        ("top_k 0", N, [1], None, dict(top_k=0), BAD),
        ("top_k 8", N, [1], None, dict(top_k=s2m.S2M_LOOP_MAX_CANDIDATES), OK),
        ("top_k 9", N, [1], None, dict(top_k=s2m.S2M_LOOP_MAX_CANDIDATES + 1), BAD),
        ("reserved", N, [1], None, dict(reserved=1), BAD),
        ("first < 0", N, [1], None, dict(first=-1), BAD),
        ("first == N", N, [1], None, dict(first=N), OK),
        ("first > N", N, [1], None, dict(first=N + 1), BAD),
        ("count -2", N, [1], None, dict(count=-2), BAD),
        ("count 0", N, [1], None, dict(count=0), OK),
        ("range to the end", N, [1], None, dict(first=10, count=N - 10), OK),
        ("range past the store", N, [1], None, dict(first=10, count=N - 9), BAD),
        ("range sum past int32", N, [1], None, dict(first=10, count=INT32_MAX), BAD),
        ("windows of any kind", N, [1], None, dict(exclude_lo=-5, exclude_hi=10**9, rel_lo=-INT32_MAX, rel_hi=INT32_MAX), OK),
        ("windows lo >= hi", N, [1], None, dict(exclude_lo=9, exclude_hi=3, rel_lo=4, rel_hi=4), OK),
        ("radius 0", N, [1], None, dict(search_radius=0.0), BAD),
        ("radius < 0", N, [1], None, dict(search_radius=-1.0), BAD),
        ("radius inf", N, [1], None, dict(search_radius=float("inf")), BAD),
        ("radius nan", N, [1], None, dict(search_radius=float("nan")), BAD),
        ("time_diff inf", N, [1], None, dict(time_diff_s=float("inf")), BAD),
        ("time_diff nan", N, [1], None, dict(time_diff_s=float("nan")), BAD),
        ("time_diff 0", N, [1], None, dict(time_diff_s=0.0), OK),
    ]


def test_argument_table_through_check_args():
    for name, n, keys, m, fields, want in argument_table():
        prm = None if fields is None else s2m.default_loop_detect_params(**fields)
        for has_tc in (False, True):
            assert s2m.loop_detect_keys_check_args(n, keys, prm, m=m, has_time_cur=has_tc) == want, name
    # what s2m_loop_params rejects in the radius and the time difference is what this call rejects
    for r, w in ((0.0, 30.0), (-1.0, 30.0), (float("nan"), 30.0), (float("inf"), 30.0), (10.0, float("nan")), (10.0, float("inf")), (10.0, -1.0),
                 (1e-3, 0.0), (1e19, 30.0)):
        loop = s2m.loop_verify_check_args(10, 5, [1], -1, s2m.default_loop_params(search_radius=r, time_diff_s=w))
        mine = s2m.loop_detect_keys_check_args(10, [5], s2m.default_loop_detect_params(search_radius=r, time_diff_s=w))
        assert loop == mine, (r, w, loop, mine)


def test_argument_table_and_plan_stand_alone_under_sanitizers(tmp_path):
    """The checker and the pass planner are plain host code (s2m_loop_detect_plan.hpp): a program of its own, built with
    -fsanitize=address,undefined by the host compiler, walks the table and the plans."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "loop_detect_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",               # the runtimes are part of the program
                           "-I", os.path.join(root, "liorf_amd", "csrc"), "-o", exe, os.path.join(root, "tests", "ref", "loop_detect_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_symbols_and_headers():
    lib = s2m.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "liorf_s2m.h")).read()
    dbg = open(os.path.join(root, "include", "liorf_s2m_debug.h")).read()
    for n in ("s2m_loop_detect_default_params", "s2m_loop_detect_keys_check_args", "s2m_loop_detect_keys"):
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n) and n + "(" in main and n + "(" not in dbg
    for n in ("s2m_debug_loop_detect_pass", "s2m_debug_loop_detect_shape", "s2m_debug_loop_detect_last", "s2m_debug_loop_detect_splits"):
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n) and n + "(" in dbg and n + "(" not in main
    assert lib.s2m_loop_detect_keys(None, None, None, 0, None, None, None, None) == BAD                 # a null handle
    assert lib.s2m_debug_loop_detect_shape(None, None, None) == BAD
    # kf_d2 is one statement in a shared header: no unit restates it
    csrc = os.path.join(root, "liorf_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".h")) and "float kf_d2(" in open(os.path.join(csrc, f)).read()]
    assert holders == ["s2m_kf_d2.hpp"]
