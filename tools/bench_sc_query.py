"""Wall time of the ScanContext place query (s2m_sc_query_key) against what the library offered before it.

Stores of 2 000 and 20 000 random descriptors (20 x 60 max-height images with empty bins); the newest key revisits key n / 4,
rotated by 23 sectors with noise.  Medians of 20 calls after 3 warm-ups, every call ending with the library's own
synchronisation:
  detect_ms            s2m_sc_detect_loop: 3 ring-key candidates, 7 shifts each
  compose_ms           the exhaustive search as it could be composed before: s2m_sc_distance(newest, all other keys) - the
                       candidate list goes up, every distance and shift comes back - and the ranking by (distance, key)
                       under 0.3 with numpy on the host (compose_rank_ms of it)
  query_ms             s2m_sc_query_key(newest, all other keys) for both alignments and K = 1, 10; with it the bytes of
                       descriptors (and, for the sector-key alignment, sector keys) one query reads and bytes / time
The K = 10 hits of the sector-key query are compared with the composition's before anything is timed.

  python tools/bench_sc_query.py [--out profiles/sc_query_bench_line.json]     one JSON line, also written to --out
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (2000, 20000)
REPS, WARMUP = 20, 3


def _store(n, seed=0):
    rng = np.random.default_rng(seed)
    descs = rng.uniform(0.0, 6.0, (n, 20, 60)) * (rng.uniform(0, 1, (n, 20, 60)) > 0.35)
    place = descs[n // 4]
    q = np.roll(place, 23, axis=1)
    descs[n - 1] = np.where(q == 0, 0.0, q + rng.normal(0, 0.05, q.shape))
    return descs


def _median_ms(fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def _rank(dist, shift, keys, k, max_dist=0.3):
    ok = np.flatnonzero(dist < max_dist)
    order = ok[np.lexsort((keys[ok], dist[ok]))][:k]
    return keys[order], dist[order], shift[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc_query_bench_line.json"))
    args = ap.parse_args()
    from liorf_amd import s2m
    g = s2m.MapOptimizationS2M()
    line = {"workload": "random 20x60 descriptors; the newest key revisits key n/4 rotated by 23 sectors; query = newest against all other keys",
            "reps": REPS, "warmup": WARMUP, "sizes": {}}
    for n in SIZES:
        g.scReset()
        for d in _store(n):
            g.scAddDescriptor(d)
        others = np.arange(n - 1, dtype=np.int32)
        window = dict(exclude_lo=n - 1, exclude_hi=n)
        # the two paths agree before anything is timed
        dist, shift = g.distanceBtnScanContext(n - 1, others)
        keys, d10, s10 = _rank(dist, shift, others, 10)
        hits = g.scQueryKey(n - 1, top_k=10, **window)
        assert np.array_equal(hits["key"], keys) and np.array_equal(hits["dist"].view(np.uint64), d10.view(np.uint64)) and np.array_equal(hits["shift"], s10)
        assert len(hits) >= 1 and hits[0]["key"] == n // 4 and hits[0]["shift"] == 23
        row = {"hits_under_0.3": int(len(hits)), "detect_ms": _median_ms(g.detectLoopClosureID)}
        row["compose_ms"] = _median_ms(lambda: _rank(*g.distanceBtnScanContext(n - 1, others), others, 10))
        row["compose_rank_ms"] = _median_ms(lambda: _rank(dist, shift, others, 10))
        for align, name in ((s2m.S2M_SC_ALIGN_SECTOR_KEY, "sector_key"), (s2m.S2M_SC_ALIGN_FULL, "full")):
            nbytes = (n - 1) * 8 * (1200 + (60 if align == s2m.S2M_SC_ALIGN_SECTOR_KEY else 0))
            for k in (1, 10):
                p = s2m.default_sc_query_params(top_k=k, align=align, **window)
                ms = _median_ms(lambda: g.scQueryKey(n - 1, p))
                row[f"query_{name}_k{k}_ms"] = ms
                row[f"query_{name}_k{k}_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            row[f"query_{name}_bytes"] = nbytes
        full = g.scQueryKey(n - 1, top_k=1, align=s2m.S2M_SC_ALIGN_FULL, **window)
        assert full[0]["key"] == n // 4 and full[0]["shift"] == 23
        line["sizes"][str(n)] = row
    g.close()
    line["note"] = "wall clock, median; every call ends with the library's own synchronisation"
    txt = json.dumps(line)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
