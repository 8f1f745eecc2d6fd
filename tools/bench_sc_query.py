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

--many measures the many-query form (s2m_sc_query_keys) instead: all n keys of an n-key store as queries
against all n keys, both alignments, top_k = 8, against a loop of s2m_sc_query_key over the same keys in the same process (the
raw C call on buffers made once).  Medians of five after one warm-up; the passes the call used and the device bytes of one pass;
rows and loop are compared as bytes at the smallest size before anything is timed.
  python tools/bench_sc_query.py --many [--sizes 2000,5000,20000] [--kernel-stats kernel_stats.csv] [--out profiles/sc_query_many_bench_line.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_sc_query.py --many-only 2000
                                        only the two batch calls, for the per-kernel split that --kernel-stats folds in
"""
import argparse
import csv
import ctypes as C
import json
import re
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


MANY_SIZES = (2000, 5000, 20000)
MANY_REPS, MANY_WARMUP, MANY_K = 5, 1, 8


def _median_of(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def _kernel_stats(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"k_sc_many_\w+?(?=ILi|E|<|\(|$)", r.get("Name", ""))
            if m:
                name = m.group(0) + ("<full>" if "ILi1E" in r["Name"] or "<1>" in r["Name"] else "<sector_key>" if "dist" in m.group(0) else "")
                rows[name] = {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)}
    return rows


def many(args):
    from liorf_amd import s2m
    sizes = [args.many_only] if args.many_only else [int(x) for x in args.sizes.split(",")]
    g = s2m.MapOptimizationS2M()
    line = {"workload": "random 20x60 descriptors; all n keys of the store as queries against all n keys, top_k 8, max_dist 0.3; "
                        "batch = one s2m_sc_query_keys, loop = n x s2m_sc_query_key",
            "reps": MANY_REPS, "warmup": MANY_WARMUP, "shape": dict(zip(("tile_cands", "block_queries"), s2m.sc_query_many_shape())), "sizes": {}}
    hp, ip = C.POINTER(s2m.ScHit), C.POINTER(C.c_int32)
    for n in sizes:
        g.scReset()
        for d in _store(n):
            g.scAddDescriptor(d)
        keys = np.arange(n, dtype=np.int32)
        hits, cnt = np.zeros((n, MANY_K), s2m.SC_HIT_DTYPE), np.zeros(n, np.int32)
        lhits, lcnt = np.zeros((n, MANY_K), s2m.SC_HIT_DTYPE), np.zeros(n, np.int32)
        row = {}
        for align, name in ((s2m.S2M_SC_ALIGN_FULL, "full"), (s2m.S2M_SC_ALIGN_SECTOR_KEY, "sector_key")):
            pm = s2m.default_sc_query_many_params(top_k=MANY_K, align=align)
            ps = s2m.default_sc_query_params(top_k=MANY_K, align=align)

            def batch():
                rc = g.lib.s2m_sc_query_keys(g.h, keys.ctypes.data_as(ip), n, C.byref(pm), hits.ctypes.data_as(hp), cnt.ctypes.data_as(ip))
                assert rc == 0, g.lib.s2m_last_error(g.h)

            def loop():
                fn, h, base, cbase = g.lib.s2m_sc_query_key, g.h, lhits.ctypes.data, lcnt.ctypes.data
                for k in range(n):
                    fn(h, k, C.byref(ps), C.cast(base + k * MANY_K * 24, hp), C.cast(cbase + 4 * k, ip))

            if args.many_only:
                batch(); batch()
                continue
            if n == sizes[0]:                              # the two agree before anything is timed
                batch(); loop()
                assert np.array_equal(cnt, lcnt) and all(hits[i, :cnt[i]].tobytes() == lhits[i, :cnt[i]].tobytes() for i in range(n))
                assert cnt[n - 1] >= 2 and hits[n - 1, 1]["key"] == n // 4 and hits[n - 1, 1]["shift"] == 23
            row[f"{name}_batch_ms"] = _median_of(batch, MANY_REPS, MANY_WARMUP)
            passes, scratch = g.scQueryManyLast()
            row[f"{name}_passes"], row[f"{name}_scratch_bytes"] = passes, scratch
            row[f"{name}_loop_ms"] = _median_of(loop, MANY_REPS, MANY_WARMUP)
            row[f"{name}_speedup"] = round(row[f"{name}_loop_ms"] / row[f"{name}_batch_ms"], 2)
            row[f"{name}_batch_ns_per_pair"] = round(row[f"{name}_batch_ms"] * 1e6 / (n * n), 2)
        line["sizes"][f"{n}x{n}"] = row
    g.close()
    if args.many_only:
        return
    if args.kernel_stats:
        line["kernels_2000x2000"] = _kernel_stats(args.kernel_stats)
    line["note"] = "wall clock, median; every call ends with the library's own synchronisation; kernels_*: rocprofv3 --kernel-trace --stats of a --many-only run"
    txt = json.dumps(line)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--many", action="store_true", help="the many-query form against a loop of single queries")
    ap.add_argument("--many-only", type=int, default=0, help="store size: only two batch calls per alignment (under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--sizes", default=",".join(str(x) for x in MANY_SIZES), help="--many: store sizes")
    ap.add_argument("--kernel-stats", default="", help="--many: rocprofv3 kernel_stats.csv of a --many-only run")
    args = ap.parse_args()
    if args.many or args.many_only:
        args.out = args.out or os.path.join(ROOT, "profiles", "sc_query_many_bench_line.json")
        return many(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "sc_query_bench_line.json")
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
