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

--ring measures the ring-key prefilter (s2m_sc_query_keys_ring) on the --many stores: all n keys against
all n keys, top_k 8, max_dist 0.3, both alignments, n_candidates 3, 10, 32, 128 and 256, beside the exhaustive s2m_sc_query_keys
in the same process (the yardstick; the raw C calls on buffers made once).  Medians of five after one warm-up, time per call and
per query, the ratio exhaustive / ring and the passes.  Before anything is timed the n_candidates = 256 rows of a 256-key store
are compared with the exhaustive rows as bytes, and the neighbour lists of a sample of queries with the numpy model
(tests/ref/sc_ring_ref.py).  Recall: on the 5 000-key revisit store of tools/bench_loop.py, the share of the exhaustive query's
top-1 pairs (detector window, full alignment, 0.3) each n_candidates keeps.
  python tools/bench_sc_query.py --ring [--sizes 2000,5000,20000] [--kernel-stats kernel_stats.csv] [--out profiles/sc_ring_bench_line.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_sc_query.py --ring-only 20000
                                        one ring call per alignment at n_candidates = 32: the split between the two stages
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
            m = re.search(r"k_sc_(?:many|ring)_\w+?(?=ILi|E|<|\(|$)", r.get("Name", ""))
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


RING_CANDS = (3, 10, 32, 128, 256)
RECALL_KEYS = 5000


def _ring_checks(g, s2m):
    """Before anything is timed: n_candidates = 256 on a 256-key store gives the exhaustive rows as bytes; the neighbour lists of
    a sample of queries on a 2 000-key store are the numpy model's."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sc_ring_ref as R
    descs = _store(2000)
    g.scReset()
    for d in descs[:256]:
        g.scAddDescriptor(d)
    keys = np.arange(256, dtype=np.int32)
    for align in (s2m.S2M_SC_ALIGN_FULL, s2m.S2M_SC_ALIGN_SECTOR_KEY):
        a = g.scQueryKeysRing(keys, n_candidates=256, top_k=MANY_K, align=align)
        b = g.scQueryKeys(keys, top_k=MANY_K, align=align)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and sum(len(x) for x in a) >= 256
    for d in descs[256:]:
        g.scAddDescriptor(d)
    keys32 = R.ring_keys(descs)
    sample = list(range(0, 2000, 97))
    for c in RING_CANDS:
        got = g.scRingNeighboursKeys(sample, n_candidates=c)
        assert all(R.same_neighbours(x, y) for x, y in zip(got, R.neighbours_many(descs, sample, c, keys32=keys32)))


def _ring_recall(g, s2m):
    """The revisit store of tools/bench_loop.py (real frames at keys 0 .. 27 and the last key, one small cloud elsewhere): of the
    exhaustive query's top-1 pairs, the share the prefilter keeps."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_loop as BL
    n = RECALL_KEYS
    true = BL._true_poses(n)
    big = BL._clouds([true[k] for k in range(BL.N_BIG)] + [true[-1]])
    small = big[1][:BL.SMALL_PTS].copy()
    g.scReset()
    for k in range(n):
        g.makeAndSaveScancontextAndKeys(big[k] if k < BL.N_BIG else (big[-1] if k == n - 1 else small))
    keys = np.arange(n, dtype=np.int32)
    kw = dict(top_k=1, align=s2m.S2M_SC_ALIGN_FULL, max_dist=0.3, rel_lo=-29, rel_hi=2**31 - 1)
    want = g.scQueryKeys(keys, **kw)
    pairs = [(i, int(r[0]["key"])) for i, r in enumerate(want) if len(r)]
    out = {"keys": n, "exhaustive_top1_pairs": len(pairs), "last_key_pair": [p for p in pairs if p[0] == n - 1]}
    for c in RING_CANDS:
        got = g.scQueryKeysRing(keys, n_candidates=c, **kw)
        kept = sum(1 for i, k in pairs if len(got[i]) and int(got[i][0]["key"]) == k)
        out[f"kept_c{c}"] = round(kept / max(len(pairs), 1), 4)
        out[f"last_key_kept_c{c}"] = bool(len(got[n - 1]) and len(want[n - 1]) and got[n - 1][0]["key"] == want[n - 1][0]["key"])
    return out


def ring(args):
    from liorf_amd import s2m
    sizes = [args.ring_only] if args.ring_only else [int(x) for x in args.sizes.split(",")]
    g = s2m.MapOptimizationS2M()
    line = {"workload": "random 20x60 descriptors; all n keys of the store as queries against all n keys, top_k 8, max_dist 0.3; "
                        "ring = one s2m_sc_query_keys_ring with n_candidates C, exhaustive = one s2m_sc_query_keys (the yardstick)",
            "reps": MANY_REPS, "warmup": MANY_WARMUP, "shape": dict(zip(("tile_keys", "block_queries", "buffer_words"), s2m.sc_ring_shape())), "sizes": {}}
    hp, ip = C.POINTER(s2m.ScHit), C.POINTER(C.c_int32)
    if not args.ring_only:
        _ring_checks(g, s2m)
        line["checked"] = "C = 256 rows equal the exhaustive rows as bytes at n = 256; neighbour lists equal the numpy model on 21 queries at n = 2000"
    for n in sizes:
        g.scReset()
        for d in _store(n):
            g.scAddDescriptor(d)
        keys = np.arange(n, dtype=np.int32)
        hits, cnt = np.zeros((n, MANY_K), s2m.SC_HIT_DTYPE), np.zeros(n, np.int32)
        row = {}
        for align, name in ((s2m.S2M_SC_ALIGN_FULL, "full"), (s2m.S2M_SC_ALIGN_SECTOR_KEY, "sector_key")):
            pm = s2m.default_sc_query_many_params(top_k=MANY_K, align=align)

            def exhaustive():
                rc = g.lib.s2m_sc_query_keys(g.h, keys.ctypes.data_as(ip), n, C.byref(pm), hits.ctypes.data_as(hp), cnt.ctypes.data_as(ip))
                assert rc == 0, g.lib.s2m_last_error(g.h)

            def ring_call(c):
                pr = s2m.default_sc_ring_params(top_k=MANY_K, align=align, n_candidates=c)
                rc = g.lib.s2m_sc_query_keys_ring(g.h, keys.ctypes.data_as(ip), n, C.byref(pr), hits.ctypes.data_as(hp), cnt.ctypes.data_as(ip))
                assert rc == 0, g.lib.s2m_last_error(g.h)

            if args.ring_only:
                ring_call(32)
                continue
            row[f"{name}_exhaustive_ms"] = _median_of(exhaustive, MANY_REPS, MANY_WARMUP)
            for c in RING_CANDS:
                ms = _median_of(lambda: ring_call(c), MANY_REPS, MANY_WARMUP)
                row[f"{name}_ring_c{c}_ms"] = ms
                row[f"{name}_ring_c{c}_us_per_query"] = round(ms * 1e3 / n, 3)
                row[f"{name}_ring_c{c}_passes"] = g.scRingLast()[0]
                row[f"{name}_ring_c{c}_ratio"] = round(row[f"{name}_exhaustive_ms"] / ms, 1)
                assert cnt[n - 1] >= 1 and hits[n - 1, 0]["key"] == n - 1     # (a key is its own nearest ring key)
        line["sizes"][f"{n}x{n}"] = row
    if args.ring_only:
        g.close()
        return
    line["recall"] = _ring_recall(g, s2m)
    g.close()
    if args.kernel_stats:
        line["kernels_c32_20000x20000"] = _kernel_stats(args.kernel_stats)
    line["note"] = ("wall clock, median; every call ends with the library's own synchronisation; ratio = exhaustive_ms / ring_ms; "
                    "kernels_*: rocprofv3 --kernel-trace --stats of a --ring-only run (one call per alignment, n_candidates 32)")
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
    ap.add_argument("--sizes", default=",".join(str(x) for x in MANY_SIZES), help="--many / --ring: store sizes")
    ap.add_argument("--kernel-stats", default="", help="--many / --ring: rocprofv3 kernel_stats.csv of a --many-only / --ring-only run")
    ap.add_argument("--ring", action="store_true", help="the ring-key prefilter against the exhaustive many-query")
    ap.add_argument("--ring-only", type=int, default=0, help="store size: one ring call per alignment at 32 candidates (under rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if args.ring or args.ring_only:
        args.out = args.out or os.path.join(ROOT, "profiles", "sc_ring_bench_line.json")
        return ring(args)
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
