"""GPU tests of the key-frame selection stage by stage (kf_select, liorf_amd/csrc/s2m_voxel.hip), read back through
s2m_debug_kf_select_last and held to tests/ref/kf_select_ref.py: the path taken, the candidate count, the centroids (bit for
bit: they are fp32 sums in rank order), the nearest key of each, the frame table's keys and offsets, the point count - at every
store size and candidate count where one code path hands over to the next, and the three paths against each other.

One handle is filled once, key by key, from kf_select_ref.store(); the fixture stops at the sizes of kf_select_ref.SIZES, runs
the selections of that size and notes what the hook and the call returned. The tests compare the notes with the reference.
Every comparison is exact: integers equal, floats equal as 32-bit words.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import kf_select_ref as K
from liorf_amd import s2m

pytestmark = pytest.mark.gpu

F = np.float32
DS = (2.0, 0.5)
MAP_LEAF = 0.4
RECENT_SIZES = (1025, 4097, 8193)
RECENTS = (0, 1, 1500)                       # keys the recent window takes (at most the store)
GMAP_SIZES = (4096, 4097)
PATH_COUNTS = (1025, 2048, 4096)             # candidates of the narrow-against-pre comparison
FAR_KEY = np.array([1e4, 0.0, 0.0, 0.0, 0.0, 0.0], F)
TINY = 1e-6


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _prm(R, D):
    return s2m.default_kf_params(search_radius=float(R), density=float(D), map_leaf=MAP_LEAF)


def _add(g, P, sizes, k, pose=None):
    g.saveKeyFrame(K.key_pose(P, k) if pose is None else pose, float(k), K.frame_cloud(k, sizes[k]))


def _at(g, centre, R, D):
    """One selection around `centre`: the keys the call returned and the hook's copy of the stages."""
    keys = g.extractSurroundingKeyFramesAt(centre, _prm(R, D))
    return {"keys": keys, "hook": g.kfSelectLast()}


def _time_cur(n, n_recent):
    """Key k was saved at time k: the window (time_cur - t < 10) takes exactly the n_recent newest keys."""
    return float(n - 1) + 10.0 - n_recent + 0.5 if n_recent else float(n - 1) + 10.0


@pytest.fixture(scope="module")
def notes():
    P, sizes, _ = K.store()
    out = {}
    g, g2 = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    try:
        with pytest.raises(s2m.S2MError) as e:               # before any selection: nothing to observe
            g.kfSelectLast()
        out["before"] = e.value.code
        g.extractSurroundingKeyFramesAt(K.CENTRE, _prm(50.0, 2.0))      # (an empty store runs no selection)
        with pytest.raises(s2m.S2MError) as e:
            g.kfSelectLast()
        out["before_empty"] = e.value.code
        for n in K.SIZES:
            while g.kfSize() < n:
                k = g.kfSize()
                if k == 4096:
                    # the three paths give one result: narrow on 4 096 keys, then pre on the same keys and one more at 1e4 m,
                    # which is no candidate and no nearest key; it is then moved to where the store has key 4 096
                    for m in PATH_COUNTS:
                        for D in DS:
                            out["narrow", m, D] = _at(g, K.CENTRE, K.radius_for(P[:4096], K.CENTRE, m), D)
                    _add(g, P, sizes, k, pose=FAR_KEY)
                    for m in PATH_COUNTS:
                        for D in DS:
                            out["pre", m, D] = _at(g, K.CENTRE, K.radius_for(P[:4096], K.CENTRE, m), D)
                    g.correctPoses(K.key_pose(P, k)[None], first=k)
                else:
                    _add(g, P, sizes, k)
            assert g.kfSize() == n
            for D in DS:                                       # the hand-over sizes
                out["size", n, D] = _at(g, K.CENTRE, 50.0, D)
            if n in RECENT_SIZES:                              # around the newest key, with recent keys
                for r in RECENTS:
                    r = min(r, n)
                    keys = g.extractSurroundingKeyFrames(_time_cur(n, r), _prm(50.0, 2.0))
                    out["recent", n, r] = {"keys": keys, "hook": g.kfSelectLast()}
                r = min(RECENTS[-1], n)
                keys, cloud = g.extractSurroundingKeyFrames(_time_cur(n, r), _prm(50.0, 2.0), return_map=True)
                want = g2.extractCloud([K.frame_cloud(k, sizes[k]) for k in keys], np.stack([K.key_pose(P, k) for k in keys]), MAP_LEAF)
                out["map", n] = {"keys": keys, "map": cloud, "want": want}
            if n in GMAP_SIZES:
                _, keys = g.publishGlobalMap(s2m.default_gmap_params(pose_density=3.0), return_keys=True)
                out["gmap", n] = {"keys": keys, "hook": g.kfSelectLast()}
            if n == 4096:
                out["tiny", "narrow"] = _at(g, K.CENTRE, 50.0, TINY)
        # the full store: exact candidate counts, the leaf-too-small case in the other two paths, two calls in a row
        for m in K.COUNTS:
            for D in DS:
                out["count", m, D] = _at(g, K.CENTRE, K.radius_for(P, K.CENTRE, m), D)
        out["tiny", "pre"] = _at(g, K.CENTRE, K.radius_for(P, K.CENTRE, 2048), TINY)
        out["tiny", "wide"] = _at(g, K.CENTRE, K.radius_for(P, K.CENTRE, 4097), TINY)
        out["again"] = [_at(g, K.CENTRE, K.radius_for(P, K.CENTRE, 4097), 2.0) for _ in range(2)]
        # a short buffer: the counts and what fits, then S2M_ERR_CAPACITY
        cent, nn, keys, off = np.zeros((1, 3), F), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int32)
        i32 = C.POINTER(C.c_int32)
        o = s2m.KfSelectOut(cent_cap=1, cent=s2m._fp(cent), nn=nn.ctypes.data_as(i32), frames_cap=1, keys=keys.ctypes.data_as(i32),
                            offsets=off.ctypes.data_as(i32))
        rc = g.lib.s2m_debug_kf_select_last(g.h, C.byref(o))
        out["short"] = (rc, o.path, o.n_cand, o.n_cent, o.n_frames, o.n_points, cent.copy(), int(nn[0]), int(keys[0]))
    finally:
        g.close(); g2.close()
    return out


def _check_stages(note, ref, n_keys):
    """The hook's stages and the returned keys against the reference, everything exact."""
    h = note["hook"]
    assert h["path"] == ref["path"] == K.expected_path(n_keys, ref["n_cand"])
    assert (h["n_cand"], h["n_cent"], h["n_frames"]) == (ref["n_cand"], ref["n_cent"], ref["n_frames"])
    assert np.array_equal(_bits(h["cent"]), _bits(ref["cent"]))
    assert np.array_equal(h["nn"], ref["nn"])
    assert np.array_equal(h["keys"], ref["keys"]) and np.array_equal(note["keys"], ref["keys"])
    assert np.array_equal(h["offsets"], ref["offsets"]) and h["n_points"] == ref["n_points"]


def test_no_selection_yet_is_an_error(notes):
    assert notes["before"] == notes["before_empty"] == -4               # S2M_ERR_NO_SCAN


@pytest.mark.parametrize("n", K.SIZES)
def test_stages_at_every_hand_over(notes, n):
    for D in DS:
        ref = K.store_stages(n, 50.0, D)
        _check_stages(notes["size", n, D], ref, n)
        assert notes["size", n, D]["hook"]["path"] == (K.PATH_NARROW if n <= 4096 else (K.PATH_PRE if ref["n_cand"] <= 4096 else K.PATH_WIDE))


@pytest.mark.parametrize("m", K.COUNTS)
def test_candidate_counts_on_the_full_store(notes, m):
    P, _, _ = K.store()
    for D in DS:
        ref = K.store_stages(K.N_KEYS, K.radius_for(P, K.CENTRE, m), D)
        assert ref["n_cand"] == m
        _check_stages(notes["count", m, D], ref, K.N_KEYS)
        assert notes["count", m, D]["hook"]["path"] == (K.PATH_PRE if m <= 4096 else K.PATH_WIDE)


@pytest.mark.parametrize("m", PATH_COUNTS)
def test_narrow_and_pre_give_one_result(notes, m):
    P, _, _ = K.store()
    for D in DS:
        a, b = notes["narrow", m, D], notes["pre", m, D]
        assert (a["hook"]["path"], b["hook"]["path"]) == (K.PATH_NARROW, K.PATH_PRE)
        assert a["hook"]["n_cand"] == b["hook"]["n_cand"] == m
        for f in ("cent", "nn", "keys", "offsets"):
            assert np.array_equal(_bits(a["hook"][f]) if f == "cent" else a["hook"][f], _bits(b["hook"][f]) if f == "cent" else b["hook"][f]), f
        assert np.array_equal(a["keys"], b["keys"])
        _check_stages(a, K.store_stages(4096, K.radius_for(P[:4096], K.CENTRE, m), D), 4096)


def test_pre_and_wide_share_their_centroids(notes):
    """4 096 candidates on the full store go through the single workgroup, 4 097 through the radix sorts; the one candidate more sits
    in a voxel of its own (test_kf_select_cpu), so every other centroid keeps its bits and its nearest key."""
    P, _, _ = K.store()
    for D in DS:
        a, b = notes["count", 4096, D]["hook"], notes["count", 4097, D]["hook"]
        assert (a["path"], b["path"]) == (K.PATH_PRE, K.PATH_WIDE) and b["n_cent"] == a["n_cent"] + 1
        new = P[K.store_stages(K.N_KEYS, K.radius_for(P, K.CENTRE, 4097), D)["order"][-1]]
        rest = ~(_bits(b["cent"]) == _bits(new)).all(axis=1)
        assert rest.sum() == a["n_cent"]
        assert np.array_equal(_bits(b["cent"][rest]), _bits(a["cent"])) and np.array_equal(b["nn"][rest], a["nn"])


@pytest.mark.parametrize("n", RECENT_SIZES)
def test_around_the_newest_key_with_recent_keys(notes, n):
    P, sizes, _ = K.store()
    for r in RECENTS:
        r = min(r, n)
        ref = K.store_stages(n, 50.0, 2.0, n_recent=r, centre=tuple(P[n - 1].tolist()))
        assert len(ref["entry_keys"]) == ref["n_cent"] + r
        _check_stages(notes["recent", n, r], ref, n)
    assert K.store_stages(n, 50.0, 2.0, n_recent=min(1500, n), centre=tuple(P[n - 1].tolist()))["entry_keys"].size > 1024   # a second round of k_kf_select_frames
    m = notes["map", n]
    assert np.array_equal(m["keys"], notes["recent", n, min(1500, n)]["keys"])
    assert m["map"].shape == m["want"].shape and m["map"].shape[0] > 0 and np.array_equal(_bits(m["map"]), _bits(m["want"]))


@pytest.mark.parametrize("n", GMAP_SIZES)
def test_global_map_selection(notes, n):
    P, _, _ = K.store()
    ref = K.store_stages(n, 1e3, 3.0, centre=tuple(P[n - 1].tolist()))
    assert ref["n_cand"] == n and ref["path"] == (K.PATH_NARROW if n == 4096 else K.PATH_WIDE)
    _check_stages(notes["gmap", n], ref, n)


@pytest.mark.parametrize("path", ["narrow", "pre", "wide"])
def test_leaf_too_small_in_each_path(notes, path):
    P, _, _ = K.store()
    n, R = {"narrow": (4096, 50.0), "pre": (K.N_KEYS, K.radius_for(P, K.CENTRE, 2048)), "wide": (K.N_KEYS, K.radius_for(P, K.CENTRE, 4097))}[path]
    ref = K.store_stages(n, R, TINY)
    h = notes["tiny", path]["hook"]
    assert ref["leaf_too_small"] and h["path"] == {"narrow": 0, "pre": 1, "wide": 2}[path]
    assert h["n_cent"] == h["n_cand"] == ref["n_cand"]
    assert np.array_equal(_bits(h["cent"]), _bits(P[:n][ref["order"]]))          # the candidate positions in rank order
    _check_stages(notes["tiny", path], ref, n)


def test_far_centre():
    """The same keys 100 km out, where the fp32 subtraction of kf_d2 cancels most of the significand: a store of its own."""
    P, sizes, _ = K.store()
    n = 4097
    Pf = (P[:n] + K.FAR_SHIFT).astype(F)
    c = (K.CENTRE + K.FAR_SHIFT).astype(F)
    g = s2m.MapOptimizationS2M()
    try:
        for k in range(n):
            _add(g, Pf, sizes, k)
        for R in (K.radius_for(Pf, c, 2048), F(1e3)):
            for D in DS:
                ref = K.stages(Pf, c, R, D, sizes=sizes[:n])
                assert ref["n_cand"] == (2048 if R < 1e3 else n)
                _check_stages(_at(g, c, R, D), ref, n)
    finally:
        g.close()


def test_two_calls_and_a_fresh_handle_give_identical_stages(notes):
    P, sizes, _ = K.store()
    a, b = notes["again"]
    for f in ("path", "n_cand", "n_cent", "n_frames", "n_points"):
        assert a["hook"][f] == b["hook"][f]
    for f in ("cent", "nn", "keys", "offsets"):
        assert np.array_equal(a["hook"][f].view(np.uint32), b["hook"][f].view(np.uint32)), f
    n = 4097
    g = s2m.MapOptimizationS2M()
    try:
        for k in range(n):
            _add(g, P, sizes, k)
        for D in DS:
            fresh, first = _at(g, K.CENTRE, 50.0, D)["hook"], notes["size", n, D]["hook"]
            assert {f: fresh[f] for f in ("path", "n_cand", "n_cent", "n_frames", "n_points")} == {f: first[f] for f in ("path", "n_cand", "n_cent", "n_frames", "n_points")}
            for f in ("cent", "nn", "keys", "offsets"):
                assert np.array_equal(fresh[f].view(np.uint32), first[f].view(np.uint32)), (D, f)
    finally:
        g.close()


def test_short_buffers_get_the_counts_and_what_fits(notes):
    rc, path, n_cand, n_cent, n_frames, n_points, cent, nn0, key0 = notes["short"]
    full = notes["again"][1]["hook"]
    assert rc == -5 and n_cent > 1 and n_frames > 1                      # S2M_ERR_CAPACITY
    assert (path, n_cand, n_cent, n_frames, n_points) == tuple(full[f] for f in ("path", "n_cand", "n_cent", "n_frames", "n_points"))
    assert np.array_equal(_bits(cent[0]), _bits(full["cent"][0])) and nn0 == full["nn"][0] and key0 == full["keys"][0]
