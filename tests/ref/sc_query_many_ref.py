"""Model of the many-query form of the ScanContext place query (include/liorf_s2m.h, "The place query for many queries at
once"), on sc_query_ref: the searched set with the fixed and the relative window, and every row as the
single query's ranking over that set."""
import numpy as np

import sc_query_ref as Q

INT32_MAX = 2**31 - 1
DETECTOR_WINDOW = dict(rel_lo=-29, rel_hi=INT32_MAX)      # "nothing from the 30 most recent keys on": key i sees 0 .. i-30


def searched_keys(n, key=None, first=0, count=-1, exclude_lo=0, exclude_hi=0, rel_lo=0, rel_hi=0):
    """The single query's set minus [key + rel_lo, key + rel_hi) (Python integers: no overflow); key=None is a descriptor query,
    rel_lo >= rel_hi no relative window."""
    keys = Q.searched_keys(n, first, count, exclude_lo, exclude_hi)
    if key is None or rel_lo >= rel_hi:
        return keys
    return [c for c in keys if not (key + rel_lo <= c < key + rel_hi)]


def query_many(descs, queries, top_k=1, align=Q.ALIGN_SECTOR_KEY, max_dist=0.3, dists=None, **window):
    """One HIT_DTYPE array per query; a query is a stored key (int) or a descriptor.  `dists` caches {query position or key:
    all_distances} between calls that differ in the window, top_k or max_dist only."""
    rows = []
    for i, q in enumerate(queries):
        stored = np.ndim(q) == 0
        key = int(q) if stored else None
        keys = searched_keys(len(descs), key, **window)
        tag = (align, key if stored else ("ext", i))
        if dists is not None and tag in dists:
            d = dists[tag]
        else:
            d = Q.all_distances(descs, descs[key] if stored else q, align, keys if dists is None else None)
            if dists is not None:
                dists[tag] = d
        rows.append(Q.rank(d, keys, top_k, max_dist))
    return rows


def same_rows(a, b) -> bool:
    return len(a) == len(b) and all(Q.same_hits(x, y) for x, y in zip(a, b))
