"""Model of the ring-key prefilter of the ScanContext place query (include/liorf_s2m.h, "The place query behind a ring-key
prefilter"), on sc_query_ref / sc_query_many_ref: fp32 ring keys as the store holds them, the squared
distance in the order of nanoflann's L2_Adaptor with every intermediate rounded to fp32, the neighbour set R_i as the first
n_candidates of the searched set by (d2, key), and a row as the single query's ranking over R_i."""
import numpy as np

import sc_query_many_ref as M
import sc_query_ref as Q
from oracle import oracle as O

MAX_CAND = 256
NEIGHBOUR_DTYPE = np.dtype([("d2", np.float32), ("key", np.int32)])
INF_BITS = 0x7F800000


def ring_key(desc) -> np.ndarray:
    """The fp32 ring key the store holds for a descriptor: (float) of makeRingkeyFromScancontext."""
    return O.make_ringkey(desc).astype(np.float32)


def ring_keys(descs) -> np.ndarray:
    return np.stack([ring_key(d) for d in descs]) if len(descs) else np.zeros((0, 20), np.float32)


def d2_all(q, keys) -> np.ndarray:
    """d2(q, keys[c]) for every row c: five groups of four, result += d0*d0 + d1*d1 + d2*d2 + d3*d3, every sum and product an
    fp32 operation (numpy's float32 arithmetic rounds each one)."""
    q = np.asarray(q, np.float32)
    k = np.asarray(keys, np.float32).reshape(-1, 20)
    result = np.zeros(len(k), np.float32)
    with np.errstate(all="ignore"):
        for g in range(5):
            d = [q[4 * g + u] - k[:, 4 * g + u] for u in range(4)]
            result = result + (((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3])
    assert result.dtype == np.float32
    return result


def neighbours(keys32, q32, searched, n_candidates) -> np.ndarray:
    """R: the first n_candidates of {c in searched : d2(q, c) < +inf} in ascending (d2, key) order (NEIGHBOUR_DTYPE)."""
    searched = list(searched)
    out = np.zeros(0, NEIGHBOUR_DTYPE)
    if not searched:
        return out
    d2 = d2_all(q32, keys32[searched])
    pairs = sorted((int(np.float32(d).view(np.uint32)), int(c)) for d, c in zip(d2, searched) if d < np.inf)[:n_candidates]
    out = np.zeros(len(pairs), NEIGHBOUR_DTYPE)
    for i, (bits, c) in enumerate(pairs):
        out[i] = (np.uint32(bits).view(np.float32), c)
    return out


def _query_of(descs, keys32, q):
    stored = np.ndim(q) == 0
    key = int(q) if stored else None
    return key, (descs[key] if stored else np.asarray(q, np.float64).reshape(20, 60)), (keys32[key] if stored else ring_key(q))


def neighbours_many(descs, queries, n_candidates=3, keys32=None, **window):
    """One NEIGHBOUR_DTYPE array per query; a query is a stored key (int) or a descriptor."""
    keys32 = ring_keys(descs) if keys32 is None else keys32
    rows = []
    for q in queries:
        key, _, q32 = _query_of(descs, keys32, q)
        rows.append(neighbours(keys32, q32, M.searched_keys(len(descs), key, **window), n_candidates))
    return rows


def query_many_ring(descs, queries, n_candidates=3, top_k=1, align=Q.ALIGN_SECTOR_KEY, max_dist=0.3, keys32=None, **window):
    """One HIT_DTYPE array per query: the single query's ranking over R_i."""
    keys32 = ring_keys(descs) if keys32 is None else keys32
    rows = []
    for q in queries:
        key, qd, q32 = _query_of(descs, keys32, q)
        r = [int(c) for c in neighbours(keys32, q32, M.searched_keys(len(descs), key, **window), n_candidates)["key"]]
        rows.append(Q.rank(Q.all_distances(descs, qd, align, r), r, top_k, max_dist))
    return rows


def same_neighbours(a, b) -> bool:
    """The bar of the GPU tests: keys equal, d2 equal as uint32."""
    return len(a) == len(b) and np.array_equal(a["key"], b["key"]) and np.array_equal(a["d2"].view(np.uint32), b["d2"].view(np.uint32))
