"""Model of the ScanContext place query (include/liorf_s2m.h, "ScanContext place query"), written on the
oracle's distance_btn_scancontext and dist_direct_sc: the searched set, the two alignments, the threshold, the order of the
hits and the yaw.  Both test_sc_query_cpu.py and test_sc_query_gpu.py use it; it also builds the two stores of the issue's
cases (ring keys that tie, a descriptor the sector key cannot align)."""
import math

import numpy as np

from oracle import oracle as O

ALIGN_SECTOR_KEY, ALIGN_FULL = 0, 1
MAX_K = 32
BIG = 10000000.0
HIT_DTYPE = np.dtype([("dist", np.float64), ("key", np.int32), ("shift", np.int32), ("yaw_diff_rad", np.float32), ("reserved", np.int32)])


def full_distance(q, c):
    """From 10000000 / shift 0, s = 0..59 ascending: distDirectSC(q, circshift(c, s)) whenever strictly smaller (a NaN never is)."""
    best, shift = BIG, 0
    for s in range(60):
        d = O.dist_direct_sc(q, c, s)
        if d < best:
            best, shift = d, s
    return best, shift


def distance(q, c, align):
    return O.distance_btn_scancontext(q, c) if align == ALIGN_SECTOR_KEY else full_distance(q, c)


def yaw_of_shift(shift: int) -> np.float32:
    """deg2rad(float) of shift * PC_UNIT_SECTORANGLE, as the detector forms it (reference include/Scancontext.cpp:17-20, :338-339)."""
    return np.float32(float(np.float32(shift * (360.0 / 60.0))) * math.pi / 180.0)


def searched_keys(n, first=0, count=-1, exclude_lo=0, exclude_hi=0):
    end = n if count < 0 else first + count
    return [k for k in range(first, end) if not (exclude_lo <= k < exclude_hi)]


def all_distances(descs, q, align, keys=None):
    """{key: (dist, shift)} of q against descs[key]; compute once, rank many times."""
    keys = range(len(descs)) if keys is None else keys
    return {k: distance(q, descs[k], align) for k in keys}


def rank(dists, keys, top_k=1, max_dist=0.3):
    """The hits among `keys` given {key: (dist, shift)}: d < max_dist, ascending (d, key), the first top_k."""
    hits = sorted((dists[k][0], k, dists[k][1]) for k in keys if dists[k][0] < max_dist)[:top_k]
    out = np.zeros(len(hits), HIT_DTYPE)
    for i, (d, k, s) in enumerate(hits):
        out[i] = (d, k, s, yaw_of_shift(s), 0)
    return out


def query(descs, q, first=0, count=-1, exclude_lo=0, exclude_hi=0, top_k=1, align=ALIGN_SECTOR_KEY, max_dist=0.3):
    keys = searched_keys(len(descs), first, count, exclude_lo, exclude_hi)
    return rank(all_distances(descs, q, align, keys), keys, top_k, max_dist)


def same_hits(a, b) -> bool:
    """The bar of the GPU tests: keys and shifts equal, dist equal as uint64, yaw equal as uint32."""
    return (len(a) == len(b) and np.array_equal(a["key"], b["key"]) and np.array_equal(a["shift"], b["shift"])
            and np.array_equal(a["dist"].view(np.uint64), b["dist"].view(np.uint64))
            and np.array_equal(a["yaw_diff_rad"].view(np.uint32), b["yaw_diff_rad"].view(np.uint32))
            and not np.any(a["reserved"]))


# ---- the issue's two cases -------------------------------------------------------------------------------------------------

def ring_key_case():
    """97 descriptors: keys 3..8 are the place of key 60 with every ring rotated on its own (its exact ring key, like a corridor
    seen from elsewhere); key 96, the query, revisits key 60 rotated by 23 sectors.  The detector's three ring-key candidates
    are 3, 4, 5 (ties go to the lower index) and it finds no loop; the true key 60 is the only key under 0.3."""
    from test_scancontext_cpu import make_descriptors, revisit
    descs = make_descriptors(96, seed=5)
    base = descs[60]
    for k in range(3, 9):
        r = np.random.default_rng(100 + k)
        descs[k] = np.stack([np.roll(base[ring], int(r.integers(1, 60))) for ring in range(20)])
    descs.append(revisit(base, 23, 0.05, 7))
    return descs


BLIND_SHIFTS = (20, 31, 47)


def blind_case():
    """(blind, [query for sh in BLIND_SHIFTS]): every column of `blind` is a permutation of the same 20 values, so all column
    means are equal and fastAlignUsingVkey has nothing to align on; the queries revisit it rotated by 20, 31 and 47 sectors."""
    from test_scancontext_cpu import revisit
    r = np.random.default_rng(3)
    vals = r.uniform(0.5, 6.0, 20)
    blind = np.stack([r.permutation(vals) for _ in range(60)], axis=1)
    return blind, [revisit(blind, sh, 0.02, 5) for sh in BLIND_SHIFTS]
