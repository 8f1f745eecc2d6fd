"""CPU side of saving and loading a session (include/liorf_s2m.h, "Saving and loading a session"): the model
of the blob (tests/ref/session_ref.py) with its pins, and s2m_session_check - structure, checksums, content - held against it.
Nothing here needs a GPU; the GPU tests (test_session_gpu.py) hold the library's save and load against the same model.
"""
import ctypes as C
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import session_ref as M

from liorf_amd import s2m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT, CHECKSUM, IO = -7, -8, -9
NEW = ["s2m_session_info_of", "s2m_session_save", "s2m_session_load", "s2m_session_save_file", "s2m_session_load_file", "s2m_session_check"]
NEW_DEBUG = ["s2m_debug_session_chunk", "s2m_debug_sc_keys", "s2m_debug_kf_frame"]


def status(blob):
    """The status of s2m_session_check."""
    try:
        s2m.session_check(blob)
        return 0
    except s2m.S2MError as e:
        return e.code


def flip(blob, byte, bit=0):
    b = bytearray(blob)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.fixture(scope="module")
def scripted():
    s = M.scripted()
    return s, M.write(s)


def section_spans(blob):
    hd, secs, _ = M.split(blob)
    spans, at = [], M.HEADER
    for n in hd["sizes"]:
        spans.append((at, at + n))
        at += n
    return spans


# ---- the ABI ------------------------------------------------------------------------------------------------

def test_symbols_statuses_and_struct():
    lib = s2m.load_library()
    main = open(os.path.join(ROOT, "include", "liorf_s2m.h")).read()
    dbg = open(os.path.join(ROOT, "include", "liorf_s2m_debug.h")).read()
    for n in NEW + NEW_DEBUG:
        assert n in s2m.ABI_SYMBOLS and hasattr(lib, n) and getattr(lib, n).argtypes, n
        assert (n + "(" in dbg and n not in main) if n in NEW_DEBUG else (n + "(" in main), n
    for name, val in (("S2M_ERR_FORMAT", FORMAT), ("S2M_ERR_CHECKSUM", CHECKSUM), ("S2M_ERR_IO", IO)):
        assert int(re.search(r"#define " + name + r"\s+(-?\d+)", main).group(1)) == val == getattr(s2m, name)
        assert s2m.ERRORS[val] == name
    assert int(re.search(r"#define S2M_SESSION_VERSION\s+(\d+)", main).group(1)) == s2m.S2M_SESSION_VERSION == M.VERSION
    assert C.sizeof(s2m.SessionInfo) == 40               # u32, 5 x i32, 2 x u64
    assert "not a security measure" in main.lower()
    for name in ("session_save", "session_load", "session_save_file", "session_load_file", "session_info"):
        assert hasattr(s2m.MapOptimizationS2M, name), name
    assert lib.s2m_session_check(None, 0, None) == -1


# ---- the model ----------------------------------------------------------------------------------------------

def test_checksum_of_five_words_by_hand():
    words = [1, 2, 3, 0xFFFFFFFF, 5]
    # s1 = 1 + 2 + 3 + 4294967295 + 5; s2 = 1*1 + 2*2 + 3*3 + 4*4294967295 + 5*5
    assert M.checksum(struct.pack("<5I", *words)) == (4294967306, 17179869219)
    assert M.checksum_fast(struct.pack("<5I", *words)) == (4294967306, 17179869219)
    # and mod 2^64: 2^32 words of 0xffffffff would wrap; a first-word index near 2^64 does so in five
    s1, s2 = M.checksum(struct.pack("<5I", *words), first=(1 << 64) - 3)
    assert s1 == 4294967306 and s2 == sum(((1 << 64) - 3 + i + 1) * w for i, w in enumerate(words)) % (1 << 64)


def test_checksum_combines_at_every_split_of_64_words():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype("<u4").tobytes()
    whole = M.checksum(data)
    assert whole == M.checksum_fast(data)
    for cut in range(65):
        a, b = M.checksum(data[:4 * cut]), M.checksum(data[4 * cut:])
        assert M.combine(a, b, cut) == whole, cut
        assert M.combine(a, (0, 0), cut) == a
        # three chunks, the way a staging pipeline meets them
        for cut2 in range(cut, 65, 7):
            c = M.checksum(data[4 * cut2:])
            mid = M.checksum(data[4 * cut:4 * cut2])
            assert M.combine(M.combine(a, mid, cut), c, cut2) == whole


def test_the_parser_returns_what_was_written(scripted):
    s, blob = scripted
    p = M.parse(blob)
    assert M.write(p) == blob
    assert p.counts() == s.counts() and (p.n_search, p.counter) == (s.n_search, s.counter) == (5, 7)
    assert np.array_equal(p.poses.view(np.uint32), s.poses.view(np.uint32)) and np.array_equal(p.times, s.times)
    assert all(np.array_equal(a, b) for a, b in zip(p.clouds, s.clouds))
    assert np.array_equal(p.desc, s.desc) and p.pairs == s.pairs and p.factors == s.factors
    assert np.array_equal(p.X, s.X) and np.array_equal(p.has_init, s.has_init)
    c = s.counts()
    assert (c["n_keys"], c["n_descriptors"], c["n_loop_pairs"], c["n_variables"], c["n_factors"]) == (40, 35, 3, 40, 44)
    kinds = [(f["type"], f["k"] > 0) for f in s.factors]
    assert kinds.count((M.PRIOR, False)) == 1 and kinds.count((M.GPS, False)) == 1 and kinds.count((M.BETWEEN, True)) == 1
    assert kinds.count((M.BETWEEN, False)) == 39 + 2
    words = np.concatenate(s.clouds)
    assert np.isnan(words.view(np.float32)[:, :3]).any() and words[:, 3].any() and words[:, 5:].any()


def test_the_library_accepts_the_model_and_reports_its_counts(scripted):
    s, blob = scripted
    info = s2m.session_check(blob)
    c = s.counts()
    assert info.version == 1 and info.bytes == len(blob)
    assert {k: getattr(info, k) for k in c} == c
    assert len(blob) == 112 + 40 * 40 + 32 * c["n_points"] + 9600 * 35 + 8 * 3 + 168 * 44 + 100 * 40 + 112
    with pytest.raises(ValueError):
        M.parse(flip(blob, len(blob) // 2))


# ---- rejections -----------------------------------------------------------------------------------------------

def reheader(blob, patch):
    """The blob with header bytes patched by patch(bytearray) and the header's checksum made to match again."""
    hdr = bytearray(blob[:M.HEADER])
    patch(hdr)
    foot = blob[-M.FOOTER:-16]
    return bytes(hdr) + blob[M.HEADER:-M.FOOTER] + foot + struct.pack("<QQ", *M.checksum(bytes(hdr) + foot))


def test_wrong_magic_and_version_2_are_format_errors(scripted):
    _, blob = scripted
    assert status(reheader(blob, lambda h: h.__setitem__(0, ord("X")))) == FORMAT
    assert status(reheader(blob, lambda h: h.__setitem__(slice(8, 12), struct.pack("<I", 2)))) == FORMAT
    assert status(reheader(blob, lambda h: None)) == 0      # (the helper itself leaves a valid blob)
    assert status(b"") == FORMAT and status(blob[:50]) == FORMAT


def test_truncation_at_every_boundary_and_inside_every_section_is_a_format_error(scripted):
    _, blob = scripted
    cuts = {M.HEADER // 2, M.HEADER, len(blob) - M.FOOTER, len(blob) - M.FOOTER // 2, len(blob) - 4, len(blob) - 1}
    for a, b in section_spans(blob):
        assert b > a
        cuts |= {a, (a + b) // 2 // 4 * 4, (a + b) // 2 // 4 * 4 + 1, b}
    for cut in sorted(cuts):
        assert status(blob[:cut]) == FORMAT, cut
    assert status(blob + b"\0\0\0\0") == FORMAT             # and bytes behind the footer


def test_a_flipped_bit_in_each_section_is_a_checksum_error(scripted):
    _, blob = scripted
    for (a, b), name in zip(section_spans(blob), M.SECTIONS):
        for at in (a, (a + b) // 2, b - 1):
            for bit in (0, 7):
                assert status(flip(blob, at, bit)) == CHECKSUM, (name, at, bit)
    for at in range(len(blob) - M.FOOTER, len(blob), 8):    # and in the footer's own words
        assert status(flip(blob, at, 3)) == CHECKSUM, at


def test_a_flipped_header_bit_with_a_stale_checksum_is_a_checksum_error(scripted):
    _, blob = scripted
    # the counts (n_keys .. n_factors), the reserved word, n_points and a section size: everything behind magic, version,
    # header size, and before the total the structure is located by
    for at in list(range(16, 48, 4)) + [48, 56, 64, 96]:
        assert status(flip(blob, at, 1)) == CHECKSUM, at
    assert status(flip(blob, 3, 0)) == FORMAT and status(flip(blob, 8, 1)) == FORMAT and status(flip(blob, 104, 2)) == FORMAT


def rewritten(s, blob, **patch):
    """The scripted blob with whole sections replaced (by name) or header counts changed (n_search=...), every checksum
    recomputed: structurally valid, so that only the content is left to object to."""
    hd, secs, _ = M.split(blob)
    for k, name in enumerate(M.SECTIONS):
        if name in patch:
            secs[k] = patch[name]
    counts = [patch.get(k, hd[k]) for k in ("n_keys", "n_descriptors", "n_search", "counter", "n_loop_pairs", "n_variables", "n_factors")]
    sizes = [len(x) for x in secs]
    hdr = M.header_bytes(counts, patch.get("n_points", hd["n_points"]), sizes, M.HEADER + sum(sizes) + M.FOOTER)
    return M.assemble(hdr, secs)


def test_valid_structure_and_checksums_but_bad_content_is_a_format_error(scripted):
    s, blob = scripted
    _, secs, _ = M.split(blob)
    keys, loops, factors, var = bytearray(secs[0]), bytearray(secs[3]), bytearray(secs[4]), bytearray(secs[5])
    assert status(rewritten(s, blob)) == 0

    def with_bytes(sec, at, data):
        b = bytearray(sec)
        b[at:at + len(data)] = data
        return bytes(b)
    k5 = 5 * M.KEY_BYTES
    n5 = struct.unpack("<i", keys[k5 + 32:k5 + 36])[0]
    cases = {
        "a NaN pose": dict(keys=with_bytes(keys, k5 + 8, struct.pack("<f", np.nan))),
        "an infinite time": dict(keys=with_bytes(keys, k5 + 24, struct.pack("<d", np.inf))),
        "a negative point count": dict(keys=with_bytes(keys, k5 + 32, struct.pack("<i", -1))),
        "point counts that do not sum to the section": dict(keys=with_bytes(keys, k5 + 32, struct.pack("<i", n5 + 1))),
        "n_points that is not the section": dict(n_points=s.counts()["n_points"] + 1),
        "a loop pair naming key n_keys": dict(loops=with_bytes(loops, 8 * 2 + 4, struct.pack("<i", 40))),
        "a loop pair's key_cur naming key n_keys": dict(loops=with_bytes(loops, 8 * 2, struct.pack("<i", 40))),
        "loop pairs not ascending": dict(loops=bytes(loops[8:16] + loops[0:8] + loops[16:24])),
        "a factor naming variable n_variables": dict(factors=with_bytes(factors, 168 * 43 + 4, struct.pack("<i", 40))),
        "a between naming variable n_variables": dict(factors=with_bytes(factors, 168 * 40 + 8, struct.pack("<i", 40))),
        "a self loop": dict(factors=with_bytes(factors, 168 * 40 + 8, struct.pack("<i", 20))),
        "a factor of unknown type": dict(factors=with_bytes(factors, 168 * 43, struct.pack("<i", 3))),
        "a GPS factor with six rows": dict(factors=with_bytes(factors, 168 * 43 + 12, struct.pack("<i", 6))),
        "a weight that is no variance": dict(factors=with_bytes(factors, 168 * 41 + 112, struct.pack("<d", 0.0))),
        "a NaN measurement": dict(factors=with_bytes(factors, 168 * 41 + 16 + 8 * 4, struct.pack("<d", np.nan))),
        "a negative robust scale": dict(factors=with_bytes(factors, 168 * 42 + 160, struct.pack("<d", -1.0))),
        "n_search above n": dict(n_search=36),
        "a negative counter": dict(counter=-1),
        # (41 variables: the X block first, then the flags)
        "a variable without a value that no factor made": dict(vars=bytes(var[:96 * 40]) + bytes(96) + bytes(var[96 * 40:]) + struct.pack("<I", 0),
                                                               n_variables=41),
        "a has_init that is no flag": dict(vars=with_bytes(var, 96 * 40 + 4 * 7, struct.pack("<I", 2))),
        "a NaN estimate": dict(vars=with_bytes(var, 96 * 3 + 8, struct.pack("<d", np.nan))),
    }
    for name, patch in cases.items():
        assert status(rewritten(s, blob, **patch)) == FORMAT, name
    # a variable beyond the factors is fine when it holds a value (s2m_pg_set_initial makes such)
    v = bytes(var[:96 * 40]) + np.array(M.state_of([1, 2, 3, 0, 0, 0.5])).tobytes() + bytes(var[96 * 40:]) + struct.pack("<I", 1)
    assert status(rewritten(s, blob, vars=v, n_variables=41)) == 0


# ---- edge cases -----------------------------------------------------------------------------------------------

def test_an_empty_session_is_valid():
    blob = M.write(M.Session())
    assert len(blob) == 224
    info = s2m.session_check(blob)
    assert (info.n_keys, info.n_descriptors, info.n_loop_pairs, info.n_variables, info.n_factors, info.n_points, info.bytes) == (0, 0, 0, 0, 0, 0, 224)
    assert M.write(M.parse(blob)) == blob


def test_key_frames_without_descriptors_and_a_graph_without_key_frames_are_valid():
    full = M.scripted()
    a = M.Session()
    a.poses, a.times, a.clouds = full.poses, full.times, full.clouds
    info = s2m.session_check(M.write(a))
    assert (info.n_keys, info.n_descriptors, info.n_variables, info.n_points) == (40, 0, 0, full.counts()["n_points"])
    b = M.Session()
    b.factors, b.X, b.has_init = full.factors, full.X, full.has_init
    info = s2m.session_check(M.write(b))
    assert (info.n_keys, info.n_variables, info.n_factors) == (0, 40, 44)
    # descriptors alone, more of them than keys, and keys whose clouds are all empty
    c = M.Session()
    c.desc, c.n_search, c.counter = full.desc, 35, 0
    for k in range(3):
        c.add_key(full.poses[k], full.times[k], np.zeros((0, 8), np.float32))
    info = s2m.session_check(M.write(c))
    assert (info.n_keys, info.n_descriptors, info.n_points) == (3, 35, 0)
    # but loop pairs need their keys
    b.pairs = [(1, 0)]
    assert status(M.write(b)) == FORMAT
