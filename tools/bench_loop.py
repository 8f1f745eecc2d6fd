"""Wall time of performRSLoopClosure() on the resident key-frame store against today's binding.

Stores of 5 000 and 50 000 keys on a circle of 0.5 m key spacing (1 s apart) that ends where it started; the last key's stored
pose carries a drift of (0.3, -0.2, 0) m and 0.02 rad of yaw. Keys 0 .. 27 and the last key hold 30 000-point ray-cast frames
of bench_keyframes.py's scene (cast at the keys' true poses), every other key a 1 000-point cloud. kitti.yaml settings:
search radius 15 m, search_num 25, ICP leaf 0.5, fitness 0.3, time window 30 s. Medians after warm-up of:
  loop_closure_rs_ms   s2m_loop_closure_rs: detection, both submaps, ICP. Timed with fitness_score = -1, so that every
                       repetition does the whole work and is rejected after ICP (an accepted closure is recorded and
                       the next call on the same key stops at S2M_LOOP_ALREADY_CLOSED); one accepted call follows,
                       reported as accepted_ms
  host_path_ms         the same pair as the binding does it today with this library: host key-frame clouds, per-frame
                       s2m_transform_cloud, concatenation, s2m_voxel_downsample of both submaps, s2m_icp_align
                       (the PCL kd-tree detection of the binding is not included)
  icp_ms               s2m_icp_align alone on the two submaps (host copies, upload included); icp_share = icp_ms /
                       loop_closure_rs_ms
  detect_ms            s2m_loop_closure_rs on a store whose newest key has no candidate (detection alone)

  python tools/bench_loop.py                           one JSON line
  python tools/bench_loop.py --async                   the same line, and profiles/loop_async_bench_line.json (--async-out) with
                                                       the launched closure on the same stores:
    held_ms              (a) time the handle is held: s2m_loop_closure_rs_launch plus every s2m_loop_poll until the result, polled
                         every --poll-us microseconds (launch_ms, polls, polls_ms), against loop_closure_rs_ms of the same run
    latency_ms           (b) launch to result, polled in that rhythm, and latency_tight_ms polled back to back
    search_us            (c) device time of one nearest-neighbour search of the two submaps (HIP events, s2m_debug_icp_time_nearest):
                         k_icp_nn against the grid at several cell edges and shell caps, with the grid's build time and n_fallback
    registration_ms      (d) the early-exit registration of bench.py's scans (set_scan + optimize on host records) on this
                         handle, with and without a closure pending
  python tools/bench_loop.py --verify                  only profiles/loop_verify_bench_line.json (--verify-out): on the same stores the
                                                       K = 1, 2, 4, 8 nearest of the RS detector's radius candidates of the last key,
    verify_collect_ms    (a) s2m_loop_verify_launch to the result of s2m_loop_verify_collect: the K alignments in lockstep
    held_ms              (b) time the handle is held: the launch plus every s2m_loop_verify_poll, polled every --poll-us microseconds
    sequential_ms        (c) the same K through K s2m_loop_align_launch + s2m_loop_collect pairs one after the other - the baseline;
                         (a) and (c) take turns in one process after warm-up, medians of at least 10 repetitions, with (c)'s
                         min-max spread; meets_bar: (a) is below (c) by more than that spread (K = 1: not above it by more)
  python tools/bench_loop.py --verify-many             only profiles/loop_verify_many_bench_line.json (--verify-many-out): on the first store of
                                                       --sizes (5 000 keys) the last m = 16, 64, 256 keys as rows, each against the K = 4
                                                       nearest of its RS radius candidates (a row may have fewer, or none), fitness -1;
                                                       and, as "first28", keys 0 .. 27 as rows - the keys that hold real frames, so
                                                       that every pair passes the size gates (--verify-many-cases picks the cases),
    many_ms              (a) s2m_loop_verify_many over the rows, one call
    loop_ms              (b) a loop of s2m_loop_verify over the same rows through the raw C call - the baseline; the rows of (a) and
                         (b) are compared as bytes before anything is timed; (a) and (b) take turns after two warm-up rounds,
                         medians of at least 5 repetitions with min .. max; meets_bar at m = 64: (a) below (b) by more than (b)'s own
                         min .. max spread, at m = 16: (a) not above (b)
  python tools/bench_loop.py --relocalize              only profiles/relocalize_bench_line.json (--relocalize-out): the first store of
                                                       --sizes (5 000 keys) with every key's descriptor in the ScanContext store, and a
                                                       30 000-point frame cast 0.7 m beside key 10 and turned by 0.5 rad as the query,
    relocalize_ms        s2m_relocalize_scan from host records at top_k = 1, 4, 8 (all 60 shifts, the K nearest of keys 0 .. 27 - the
                         keys that hold real frames - whatever their distance, search_num 25, leaf 0.5): the query, the source
                         filter, a submap per hit, the alignments in lockstep; with the hits, their statuses and iterations, the
                         best key and its distance from the true pose
    query_ms             s2m_sc_query_scan alone with the same parameters; query_ms_all_keys: over all keys, threshold 0.3
  python tools/bench_loop.py --detect-many             only profiles/loop_detect_many_bench_line.json (--detect-many-out): stores of
                                                       --sizes one-point key frames on two laps of a circle (only poses and times matter),
    detect_keys_ms       s2m_loop_detect_keys through the Python mirror, all keys against all keys and the last 64 keys against
                         all keys, top_k 1 and 8 (R 15 m, 30 s); c_call_ms the C call on numpy arrays; c_call_one_split_ms the 64
                         queries with the store splits switched off (s2m_debug_loop_detect_splits)
    host_numpy_ms        the same rows from a host copy of the poses by numpy brute force in chunks of 256 queries (some rows are
                         compared with the device's before anything is timed), host_ckdtree_ms by scipy's cKDTree if scipy is there
  python tools/bench_loop.py --kernel-stats stats.csv  folds the k_loop_detect* and k_icp* rows of a rocprofv3
                                                       --kernel-trace --stats run into the JSON line
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAME_PTS, SMALL_PTS, N_BIG = 30000, 1000, 28
DRIFT = np.array([0.3, -0.2, 0.0, 0.0, 0.0, 0.02])


def _true_poses(n):
    th = 2 * np.pi * np.arange(n) / (n - 1)
    r = 0.5 * (n - 1) / (2 * np.pi)
    p = np.zeros((n, 6))
    p[:, 0], p[:, 1], p[:, 5] = r * np.sin(th), r * (1 - np.cos(th)), th
    p[-1] = [0, 0, 0, 0, 0, 0]                                         # exactly back at the start
    return p


def _clouds(true_near):
    from liorf_amd import synth
    scene = synth.make_scene(seed=11, half=70.0, n_boxes=92)
    rng = np.random.default_rng(1)
    out = []
    for k, p in enumerate(true_near):
        rpyxyz = np.array([p[3], p[4], p[5], p[0], p[1], 0.1 + p[2]])
        c = synth.to_xyzi(synth.make_scan(scene, rpyxyz, "velodyne64", FRAME_PTS, seed=100 + k))
        c[:, 4] = rng.uniform(0, 100, FRAME_PTS).astype(np.float32)
        out.append(c)
    return out


def _median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t)), 4)


def _stats(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"k_loop_detect\w*|k_icp\w*", r.get("Name", ""))
            if m:                                                  # (the loop's kernels are templates: the table form apart)
                name = m.group(0) + ("<pairs>" if "IcpPair" in r.get("Name", "") else "")
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3)}
    return rows


def _async_row(eng, s2m, a, time_cur, rej, sync_ms, kc, kp, scans):
    """The launched closure on a filled store (fitness -1: every repetition runs the whole ICP and is rejected)."""
    r = s2m.LoopResult()
    lib, h = eng.lib, eng.h
    pending, rejected = s2m.S2M_LOOP_PENDING, s2m.S2M_LOOP_REJECTED

    def closure(poll_s):
        t0 = time.perf_counter()
        rc = lib.s2m_loop_closure_rs_launch(h, time_cur, C.byref(rej), C.byref(r))
        t1 = time.perf_counter()
        assert rc == 0 and r.status == pending, (rc, r.status)
        held, polls = t1 - t0, 0
        while r.status == pending:
            if poll_s > 0:
                time.sleep(poll_s)
            p0 = time.perf_counter()
            rc = lib.s2m_loop_poll(h, C.byref(r))
            held += time.perf_counter() - p0
            polls += 1
            assert rc == 0
        assert r.status == rejected
        return t1 - t0, held, polls, time.perf_counter() - t0

    rows = {"loop_closure_rs_ms": sync_ms, "poll_us": a.poll_us}
    for name, poll_s in (("paced", a.poll_us * 1e-6), ("tight", 0.0)):
        runs = [closure(poll_s) for _ in range(a.warmup + a.reps)][a.warmup:]
        med = lambda k: round(1e3 * float(np.median([x[k] for x in runs])), 4)
        if name == "paced":
            rows.update(launch_ms=med(0), held_ms=med(1), polls=int(np.median([x[2] for x in runs])), latency_ms=med(3))
            rows["polls_ms"] = round(rows["held_ms"] - rows["launch_ms"], 4)
        else:
            rows.update(latency_tight_ms=med(3), polls_tight=int(np.median([x[2] for x in runs])), held_tight_ms=med(1))
    rows["iterations"] = r.icp.iterations
    rows["ranges"] = -(-r.icp.iterations // s2m.S2M_ICP_RANGE)
    # (c) one search of the two submaps: the brute force, then the grid over cell edges (metres) and shell caps
    cur = eng.loopFindNearKeyframes(kc, 0, -1, 0.5)
    prev = eng.loopFindNearKeyframes(kp, 25, -1, 0.5)
    _, _, _, us0 = eng.debugIcpNearest(cur, prev, 0, reps=20)
    search = {"n_cur": int(cur.shape[0]), "n_prev": int(prev.shape[0]), "k_icp_nn_us": round(us0, 2), "grid": []}
    for cell_m in (0.5, 0.75, 1.0, 1.5, 2.0):
        for cap in (2, 3, 4):
            eng.debugIcpTuning(cell_m / 0.3, cap, 1)              # (the debug calls take the edge in units of the default leaf, 0.3)
            _, nf, ub, us = eng.debugIcpNearest(cur, prev, 1, reps=20)
            search["grid"].append({"cell_m": cell_m, "shell_cap": cap, "search_us": round(us, 2), "build_us": round(ub, 2), "n_fallback": nf})
    eng.debugIcpTuning()
    rows["search_us"] = search
    # (d) registration with and without a closure pending
    if scans:
        m, cfgs = scans
        eng.setInputCloud(m)
        reg = {}
        for name in ("no_closure", "closure_pending"):
            ts = []
            for j in range(3 + 4 * len(cfgs)):
                k = j % len(cfgs)
                if name == "closure_pending":
                    rc = lib.s2m_loop_closure_rs_launch(h, time_cur, C.byref(rej), C.byref(r))
                    assert rc == 0 and r.status == pending
                t0 = time.perf_counter()
                eng.setScan(cfgs[k][0])
                eng.transformTobeMapped = cfgs[k][1].copy()
                eng.scan2MapOptimization()
                ts.append(time.perf_counter() - t0)
                if name == "closure_pending":
                    still = lib.s2m_loop_poll(h, C.byref(r)) == 0 and r.status == pending
                    reg["still_pending_after_registration"] = reg.get("still_pending_after_registration", 0) + int(still)
                    eng.loopCollect()
            reg[name + "_ms"] = round(1e3 * float(np.median(ts[3:])), 4)
        reg["registrations"] = 4 * len(cfgs)
        rows["registration_ms"] = reg
    return rows


def _verify_row(eng, s2m, a, stored, times, rej):
    """K candidates verified in lockstep against the same K through sequential launch + collect pairs (fitness -1: every
    alignment runs to its end and is rejected, so the container stays empty and every repetition does the whole work)."""
    lib, h = eng.lib, eng.h
    n = len(times)
    kc = n - 1
    d = np.linalg.norm(stored[:, :3].astype(np.float64) - stored[kc, :3].astype(np.float64), axis=1)
    near = [int(k) for k in np.argsort(d, kind="stable") if k != kc and d[k] <= 15.0 and abs(times[k] - times[kc]) > 30.0]
    recs = (s2m.LoopResult * s2m.S2M_LOOP_MAX_CANDIDATES)()
    one = s2m.LoopResult()
    nn, best = C.c_int32(0), C.c_int32(-1)
    pending, rejected = s2m.S2M_LOOP_PENDING, s2m.S2M_LOOP_REJECTED
    row = {"radius_candidates": len(near), "poll_us": a.poll_us, "K": {}}

    def lockstep(keys, poll_s):
        K = len(keys)
        t0 = time.perf_counter()
        rc = lib.s2m_loop_verify_launch(h, kc, keys, K, -1, C.byref(rej), recs, C.byref(best))
        held = time.perf_counter() - t0
        assert rc == 0 and all(recs[i].status == pending for i in range(K)), (rc, [recs[i].status for i in range(K)])
        if poll_s is None:
            rc = lib.s2m_loop_verify_collect(h, recs, K, C.byref(nn), C.byref(best))
            held = time.perf_counter() - t0
        else:
            while recs[0].status == pending:
                time.sleep(poll_s)
                p0 = time.perf_counter()
                rc = lib.s2m_loop_verify_poll(h, recs, K, C.byref(nn), C.byref(best))
                held += time.perf_counter() - p0
                assert rc == 0
        assert rc == 0 and nn.value == K and best.value == -1 and all(recs[i].status == rejected for i in range(K))
        return time.perf_counter() - t0, held

    def sequence(keys):
        t0 = time.perf_counter()
        for k in keys:
            rc = lib.s2m_loop_align_launch(h, kc, k, -1, C.byref(rej), C.byref(one))
            assert rc == 0 and one.status == pending, (rc, one.status)
            rc = lib.s2m_loop_collect(h, C.byref(one))
            assert rc == 0 and one.status == rejected
        return time.perf_counter() - t0

    for K in (1, 2, 4, 8):
        if K > len(near):
            break
        cand = near[:K]
        keys = (C.c_int32 * K)(*cand)
        for _ in range(a.warmup):
            lockstep(keys, None); sequence(cand)
        ta, tc = [], []
        for _ in range(max(a.reps, 10)):                     # (a) and (c) take turns
            ta.append(lockstep(keys, None)[0]); tc.append(sequence(cand))
        paced = [lockstep(keys, a.poll_us * 1e-6) for _ in range(max(a.reps, 10))]
        ms = lambda v: round(1e3 * float(v), 4)
        r = {"candidates": cand, "iterations": [recs[i].icp.iterations for i in range(K)], "n_prev": [recs[i].n_prev for i in range(K)],
             "n_cur": recs[0].n_cur,
             "verify_collect_ms": ms(np.median(ta)), "verify_collect_min_ms": ms(min(ta)), "verify_collect_max_ms": ms(max(ta)),
             "held_ms": ms(np.median([p[1] for p in paced])), "paced_latency_ms": ms(np.median([p[0] for p in paced])),
             "sequential_ms": ms(np.median(tc)), "sequential_min_ms": ms(min(tc)), "sequential_max_ms": ms(max(tc))}
        r["sequential_spread_ms"] = round(r["sequential_max_ms"] - r["sequential_min_ms"], 4)
        r["saved_ms"] = round(r["sequential_ms"] - r["verify_collect_ms"], 4)
        # K >= 2: lockstep below the sequence by more than the sequence's own spread; K = 1: not slower by more than that spread
        r["meets_bar"] = bool(r["saved_ms"] > r["sequential_spread_ms"]) if K > 1 else bool(-r["saved_ms"] <= r["sequential_spread_ms"])
        row["K"][str(K)] = r
    return row


def _verify_main(a, s2m, sizes):
    out = {"workload": "tools/bench_loop.py --verify: the revisit of the synchronous line; the K nearest of the RS detector's radius "
                       "candidates (R 15 m, 30 s) of the last key verified in lockstep (s2m_loop_verify_launch + _collect) against the same "
                       "K through sequential s2m_loop_align_launch + s2m_loop_collect pairs; search_num 25, leaf 0.5, fitness -1",
           "reps": max(a.reps, 10), "warmup": a.warmup, "sizes": {}}
    big = None
    for n in sizes:
        true = _true_poses(n)
        if big is None:
            big = _clouds([true[k] for k in range(N_BIG)] + [true[-1]])
            small = big[1][:SMALL_PTS].copy()
        stored = true.copy()
        stored[-1] += DRIFT
        stored = stored.astype(np.float32)
        times = np.arange(n, dtype=np.float64)
        eng = s2m.MapOptimizationS2M()
        for k in range(n):
            eng.saveKeyFrame(stored[k], times[k], big[k] if k < N_BIG else (big[-1] if k == n - 1 else small))
        print(f"{n} keys stored", file=sys.stderr, flush=True)
        rej = s2m.default_loop_params(search_radius=15.0, search_num=25, icp_leaf=0.5, fitness_score=-1.0)
        out["sizes"][str(n)] = _verify_row(eng, s2m, a, stored, times, rej)
        eng.close()
    out["note"] = ("wall clock on the host, medians of (a) lockstep and (c) sequence taken in turns in one process after warm-up; "
                   "held_ms: launch plus polls every poll_us; meets_bar: saved_ms > the sequence's own min-max spread (K = 1: not slower "
                   "than the single launch + collect by more than that spread)")
    print(json.dumps(out))
    with open(a.verify_out, "w") as f:
        f.write(json.dumps(out) + "\n")


def _verify_many_main(a, s2m, n):
    """s2m_loop_verify_many against the loop of s2m_loop_verify it stands for, on the revisit store of --verify."""
    true = _true_poses(n)
    big = _clouds([true[k] for k in range(N_BIG)] + [true[-1]])
    small = big[1][:SMALL_PTS].copy()
    stored = true.copy()
    stored[-1] += DRIFT
    stored = stored.astype(np.float32)
    times = np.arange(n, dtype=np.float64)
    eng = s2m.MapOptimizationS2M()
    for k in range(n):
        eng.saveKeyFrame(stored[k], times[k], big[k] if k < N_BIG else (big[-1] if k == n - 1 else small))
    print(f"{n} keys stored", file=sys.stderr, flush=True)
    rej = s2m.default_loop_params(search_radius=15.0, search_num=25, icp_leaf=0.5, fitness_score=-1.0)
    lib, h = eng.lib, eng.h
    K = 4
    reps = max(a.reps, 5)
    xyz = stored[:, :3].astype(np.float64)
    out = {"workload": "tools/bench_loop.py --verify-many: the revisit of --verify; rows are the last m keys, each against the K = 4 nearest of "
                       "its RS radius candidates (R 15 m, 30 s; fewer where it has fewer), s2m_loop_verify_many against a loop of "
                       "s2m_loop_verify over the same rows; search_num 25, leaf 0.5, fitness -1",
           "keys": n, "reps": reps, "warmup": 2, "m": {}}
    for case in a.verify_many_cases.split(","):
        # the last m keys; or "first28": keys 0 .. 27, the ones that hold real frames, so that every row passes the size gates
        cur_keys = list(range(N_BIG)) if case == "first28" else list(range(n - int(case), n))
        m = len(cur_keys)
        rows = []
        for kc in cur_keys:
            d = np.linalg.norm(xyz - xyz[kc], axis=1)
            near = [int(k) for k in np.argsort(d, kind="stable") if k != kc and d[k] <= 15.0 and abs(times[k] - times[kc]) > 30.0]
            rows.append((kc, near[:K]))
        key_cur, key_pre, n_cand, stride = s2m._verify_many_rows(rows)
        size = C.sizeof(s2m.LoopResult)
        recs_a, recs_b = (s2m.LoopResult * (m * stride))(), (s2m.LoopResult * (m * stride))()
        best_a, best_b = (C.c_int32 * m)(), (C.c_int32 * m)()

        def many():
            t0 = time.perf_counter()
            rc = lib.s2m_loop_verify_many(h, key_cur, key_pre, n_cand, m, stride, -1, C.byref(rej), recs_a, best_a)
            assert rc == 0, rc
            return time.perf_counter() - t0

        def loop():
            t0 = time.perf_counter()
            for r in range(m):
                best_b[r] = -1
                if n_cand[r]:
                    rc = lib.s2m_loop_verify(h, key_cur[r], C.cast(C.byref(key_pre, 4 * r * stride), C.POINTER(C.c_int32)), n_cand[r], -1,
                                             C.byref(rej), C.cast(C.byref(recs_b, size * r * stride), C.POINTER(s2m.LoopResult)),
                                             C.cast(C.byref(best_b, 4 * r), C.POINTER(C.c_int32)))
                    assert rc == 0, rc
            return time.perf_counter() - t0

        many(); loop()                                           # the rows as bytes, before anything is timed
        for r in range(m):
            for i in range(n_cand[r]):
                ga, gb = recs_a[r * stride + i], recs_b[r * stride + i]
                assert C.string_at(C.addressof(ga), size) == C.string_at(C.addressof(gb), size), (m, r, i, ga.status, gb.status)
        assert list(best_a) == list(best_b)
        passes, pairs, nbytes = eng.debugLoopVerifyManyLast()
        status = [recs_a[r * stride + i].status for r in range(m) for i in range(n_cand[r])]
        many(); loop()                                           # two warm-up rounds with the one above
        ta, tb = [], []
        for _ in range(reps):                                    # the two sides take turns
            ta.append(many()); tb.append(loop())
        ms = lambda v: round(1e3 * float(v), 4)
        r = {"rows_with_candidates": int(sum(1 for v in n_cand if v)), "candidates": int(sum(n_cand)), "pairs_aligned": pairs, "passes": passes,
             "submap_bytes": nbytes, "status_counts": {str(k): status.count(k) for k in sorted(set(status))},
             "iterations": [recs_a[r * stride + i].icp.iterations for r in range(m) for i in range(n_cand[r])],
             "many_ms": ms(np.median(ta)), "many_min_ms": ms(min(ta)), "many_max_ms": ms(max(ta)),
             "loop_ms": ms(np.median(tb)), "loop_min_ms": ms(min(tb)), "loop_max_ms": ms(max(tb))}
        r["loop_spread_ms"] = round(r["loop_max_ms"] - r["loop_min_ms"], 4)
        r["saved_ms"] = round(r["loop_ms"] - r["many_ms"], 4)
        if pairs:
            r["many_ms_per_pair"] = round(r["many_ms"] / pairs, 4)
            r["loop_ms_per_pair"] = round(r["loop_ms"] / pairs, 4)
        r["meets_bar"] = bool(r["saved_ms"] > r["loop_spread_ms"]) if m >= 64 or case == "first28" else bool(r["saved_ms"] >= 0.0)
        out["m"][case] = r
    eng.close()
    out["note"] = ("wall clock on the host; the call and the loop take turns in one process after two warm-up rounds, medians with min .. max; "
                   "meets_bar: m >= 64 saved_ms > the loop's own min .. max spread, m = 16 the call is not slower than the loop")
    print(json.dumps(out))
    with open(a.verify_many_out, "w") as f:
        f.write(json.dumps(out) + "\n")


def _relocalize_main(a, s2m, n):
    from liorf_amd import synth
    true = _true_poses(n)
    big = _clouds([true[k] for k in range(N_BIG)] + [true[-1]])
    small = big[1][:SMALL_PTS].copy()
    stored = true.astype(np.float32)
    eng = s2m.MapOptimizationS2M()
    for k in range(n):
        c = big[k] if k < N_BIG else (big[-1] if k == n - 1 else small)
        eng.saveKeyFrame(stored[k], float(k), c)
        eng.makeAndSaveScancontextAndKeys(c)
    print(f"{n} keys stored", file=sys.stderr, flush=True)
    q = true[10].copy()
    q[:2] += (0.6, -0.4)
    q[5] += 0.5
    scene = synth.make_scene(seed=11, half=70.0, n_boxes=92)
    scan = synth.to_xyzi(synth.make_scan(scene, np.array([q[3], q[4], q[5], q[0], q[1], 0.1 + q[2]]), "velodyne64", FRAME_PTS, seed=999))
    out = {"workload": "tools/bench_loop.py --relocalize: s2m_relocalize_scan of a 30 000-point frame cast 0.7 m beside key 10 of the "
                       f"{n}-key revisit and turned by 0.5 rad; all 60 shifts, the K nearest of keys 0..27 (max_dist 1e7), R 15, search_num 25, leaf 0.5, "
                       "fitness 0.3",
           "reps": a.reps, "warmup": a.warmup, "keys": n, "top_k": {}}
    for K in (1, 4, 8):
        # the query searches all keys with the default threshold first (query_ms_all_keys); the alignment is timed on the K nearest
        # of the revisited stretch, keys 0 .. 27, which hold real frames: the other keys all hold the same 1 000-point cloud, whose
        # descriptor is the same for every one of them, and admitting every hit would rank by key among them
        prm = s2m.default_reloc_params(query_top_k=K, query_count=N_BIG, query_max_dist=10000000.0, loop_search_radius=15.0, loop_search_num=25,
                                       loop_icp_leaf=0.5)
        recs, best = eng.relocalizeScan(scan, prm)
        row = {"hits": [r.hit.key for r in recs], "status": [r.status for r in recs], "iterations": [r.icp.iterations for r in recs],
               "n_src": recs[0].n_src if recs else 0, "n_tgt": [r.n_tgt for r in recs], "best": best}
        if best >= 0:
            p = np.array(recs[best].pose_xyzrpy, np.float64)
            row["best_key"] = recs[best].hit.key
            row["best_position_error_m"] = round(float(np.linalg.norm(p[:3] - q[:3])), 5)
            row["best_yaw_error_rad"] = round(float(abs((p[5] - q[5] + np.pi) % (2 * np.pi) - np.pi)), 6)
        row["relocalize_ms"] = _median_ms(lambda: eng.relocalizeScan(scan, prm), a.warmup, a.reps)
        row["query_ms"] = _median_ms(lambda: eng.scQueryScan(scan, prm.query), a.warmup, a.reps)
        row["query_ms_all_keys"] = _median_ms(lambda: eng.scQueryScan(scan, top_k=K, align=s2m.S2M_SC_ALIGN_FULL), a.warmup, a.reps)
        out["top_k"][str(K)] = row
    eng.close()
    out["note"] = "wall clock on the host, median after warm-up; the call waits for its result"
    print(json.dumps(out))
    with open(a.relocalize_out, "w") as f:
        f.write(json.dumps(out) + "\n")


def _two_lap_poses(n):
    """n keys 1 s apart at 0.5 m spacing on two laps of one circle, the second lap 0.3 m outside the first: every key of the
    second lap has the keys of the first within the radius around it."""
    half = n // 2
    th = 2 * np.pi * (np.arange(n) % half) / half
    r = 0.5 * half / (2 * np.pi) + 0.3 * (np.arange(n) >= half)
    p = np.zeros((n, 6), np.float32)
    p[:, 0], p[:, 1], p[:, 5] = r * np.sin(th), r * (1 - np.cos(th)), th
    return p


def _host_radius_rows(xyz, times, keys, r2, w, top_k, chunk=256):
    """What a node does today from its host copy of the poses: a brute-force radius search in numpy, in chunks of queries."""
    rows = []
    for i0 in range(0, len(keys), chunk):
        k = keys[i0:i0 + chunk]
        d = xyz[None, :, :] - xyz[k][:, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        ok = (d2 < r2) & (np.abs(times[None, :] - times[k][:, None]) > w)
        for j in range(len(k)):
            c = np.flatnonzero(ok[j])
            rows.append(c[np.lexsort((c, d2[j, c]))][:top_k])
    return rows


def _detect_many_main(a, s2m, sizes):
    """s2m_loop_detect_keys on stores of one-point key frames (only poses and times matter) against a host radius search."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    R, W = 15.0, 30.0
    r2 = np.float32(R) * np.float32(R)
    one = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    out = {"workload": "tools/bench_loop.py --detect-many: two laps of a circle at 0.5 m key spacing, 1 s apart, the second lap 0.3 m outside the "
                       "first; s2m_loop_detect_keys (R 15 m, 30 s) for all keys against all keys at top_k 1 and 8, and for the last 64 keys, "
                       "against a numpy brute-force radius search over the host copy of the poses in chunks of 256 queries"
                       + (" and scipy's cKDTree (build + query_ball_point + time gate + sort)" if cKDTree else "; scipy is not installed"),
           "reps": a.reps, "warmup": a.warmup, "tile_block_max_splits": list(s2m.loop_detect_shape()), "sizes": {}}
    for n in sizes:
        poses = _two_lap_poses(n)
        times = np.arange(n, dtype=np.float64)
        eng = s2m.MapOptimizationS2M()
        for k in range(n):
            eng.saveKeyFrame(poses[k], times[k], one)
        print(f"{n} keys stored", file=sys.stderr, flush=True)
        xyz = poses[:, :3].copy()
        allk = np.arange(n, dtype=np.int32)
        row = {}
        for name, keys in (("all", allk), ("last64", allk[-64:])):
            for K in (1, 8):
                got = eng.loopDetectKeys(keys, search_radius=R, time_diff_s=W, top_k=K)[0]
                probe = keys[:: max(len(keys) // 64, 1)]                       # the rows of some queries against the host search, before timing
                want = _host_radius_rows(xyz, times, probe, r2, W, K)
                index = {int(k): i for i, k in enumerate(keys)}
                assert all(got[index[int(k)]][1] == [int(v) for v in w] for k, w in zip(probe, want)), (n, name, K)
                r = {"queries": int(len(keys)), "candidates": int(sum(len(c) for _, c in got)),
                     "detect_keys_ms": _median_ms(lambda: eng.loopDetectKeys(keys, search_radius=R, time_diff_s=W, top_k=K), a.warmup, a.reps)}
                prm = s2m.default_loop_detect_params(search_radius=R, time_diff_s=W, top_k=K)
                kp, d2, nc = np.zeros((len(keys), K), np.int32), np.zeros((len(keys), K), np.float32), np.zeros(len(keys), np.int32)
                raw = lambda: eng.lib.s2m_loop_detect_keys(eng.h, keys.ctypes.data_as(C.POINTER(C.c_int32)), None, len(keys), C.byref(prm),
                                                           kp.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_float)),
                                                           nc.ctypes.data_as(C.POINTER(C.c_int32)))
                r["c_call_ms"] = _median_ms(raw, a.warmup, a.reps)             # without the mirror's Python lists
                r["passes"], r["scratch_bytes"] = eng.debugLoopDetectLast()
                r["pair_tests"] = int(len(keys)) * n
                if name == "last64":                                           # what the store splits buy: the same call in one split
                    eng.debugLoopDetectSplits(1)
                    r["c_call_one_split_ms"] = _median_ms(raw, a.warmup, a.reps)
                    eng.debugLoopDetectSplits(0)
                if name == "last64" or n <= 5000:
                    r["host_numpy_ms"] = _median_ms(lambda: _host_radius_rows(xyz, times, keys, r2, W, K), 1, 3)
                else:                                                          # 2.5e9 pairs in numpy: a sample of 1 024 queries, scaled
                    r["host_numpy_ms_scaled_from_1024_queries"] = round(_median_ms(lambda: _host_radius_rows(xyz, times, keys[:1024], r2, W, K), 0, 1) * len(keys) / 1024, 2)
                if cKDTree is not None:
                    def tree():
                        t = cKDTree(xyz)
                        for q, c in zip(keys, t.query_ball_point(xyz[keys], R)):
                            c = np.asarray(c, np.int64)
                            c = c[np.abs(times[c] - times[q]) > W]
                            c[np.argsort(((xyz[c] - xyz[q]) ** 2).sum(1), kind="stable")][:K]
                    r["host_ckdtree_ms"] = _median_ms(tree, 1, 3)
                row[f"{name}_top{K}"] = r
        eng.close()
        out["sizes"][str(n)] = row
    out["note"] = ("wall clock on the host, median after warm-up; every call ends with the library's own synchronisation; detect_keys_ms is the "
                   "Python mirror (it builds lists of rows), c_call_ms the C call on numpy arrays; the store holds no pose graph, so the host "
                   "side starts from the node's own copy of the poses - the copy-out a node pays on top is not in host_*_ms")
    print(json.dumps(out))
    with open(a.detect_many_out, "w") as f:
        f.write(json.dumps(out) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--detect-many", action="store_true", help="measure s2m_loop_detect_keys against a host radius search, and nothing else")
    ap.add_argument("--detect-many-out", default=os.path.join(ROOT, "profiles", "loop_detect_many_bench_line.json"))
    ap.add_argument("--relocalize", action="store_true", help="measure s2m_relocalize_scan at 1, 4 and 8 hits, and nothing else")
    ap.add_argument("--relocalize-out", default=os.path.join(ROOT, "profiles", "relocalize_bench_line.json"))
    ap.add_argument("--verify", action="store_true", help="measure the lockstep verification against sequential closures, and nothing else")
    ap.add_argument("--verify-out", default=os.path.join(ROOT, "profiles", "loop_verify_bench_line.json"))
    ap.add_argument("--verify-many", action="store_true", help="measure s2m_loop_verify_many against a loop of s2m_loop_verify, and nothing else")
    ap.add_argument("--verify-many-out", default=os.path.join(ROOT, "profiles", "loop_verify_many_bench_line.json"))
    ap.add_argument("--verify-many-cases", default="16,64,256,first28", help="m = the last m keys as rows; first28 = keys 0 .. 27 as rows")
    ap.add_argument("--sizes", default="5000,50000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", default="", help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--async", dest="run_async", action="store_true", help="also measure the launched closure (see above)")
    ap.add_argument("--async-out", default=os.path.join(ROOT, "profiles", "loop_async_bench_line.json"))
    ap.add_argument("--poll-us", type=float, default=200.0, help="sleep between two polls of the paced run")
    a = ap.parse_args(argv)
    from liorf_amd import s2m
    async_out = {"workload": "tools/bench_loop.py --async: the revisit of the synchronous line, the closure launched and polled",
                 "icp_range": s2m.S2M_ICP_RANGE, "sizes": {}}
    scans = None
    if a.run_async:
        from liorf_amd import synth
        cfgs = [synth.make_config("kitti64", scan_index=k) for k in range(4)]
        scans = (synth.to_xyzi(cfgs[0]["map"]), [(synth.to_xyzi(c["scan"]), c["pose_init"]) for c in cfgs])

    sizes = [int(s) for s in a.sizes.split(",")]
    if a.detect_many:
        return _detect_many_main(a, s2m, sizes)
    if a.verify:
        return _verify_main(a, s2m, sizes)
    if a.verify_many:
        return _verify_many_main(a, s2m, sizes[0])
    if a.relocalize:
        return _relocalize_main(a, s2m, sizes[0])
    out = {"workload": "revisit: 30 000-point frames at keys 0..27 and the last key, 1 000 points elsewhere; R 15, search_num 25, "
                       "leaf 0.5, fitness 0.3", "sizes": {}}
    big = None
    small = None
    for n in sizes:
        true = _true_poses(n)
        if big is None:
            near = [true[k] for k in range(N_BIG)] + [true[-1]]
            big = _clouds(near)
            small = big[1][:SMALL_PTS].copy()
        stored = true.copy()
        stored[-1] += DRIFT
        stored = stored.astype(np.float32)
        times = np.arange(n, dtype=np.float64)
        clouds = [big[k] if k < N_BIG else small for k in range(n - 1)] + [big[-1]]
        eng = s2m.MapOptimizationS2M()
        for k in range(n):
            eng.saveKeyFrame(stored[k], times[k], clouds[k])
        prm = s2m.default_loop_params(search_radius=15.0, search_num=25, icp_leaf=0.5)
        rej = s2m.default_loop_params(search_radius=15.0, search_num=25, icp_leaf=0.5, fitness_score=-1.0)
        r = s2m.LoopResult()
        ms = _median_ms(lambda: eng.lib.s2m_loop_closure_rs(eng.h, float(times[-1]), C.byref(rej), C.byref(r)), a.warmup, a.reps)
        rej_status = r.status
        if a.run_async:
            async_out["sizes"][str(n)] = _async_row(eng, s2m, a, float(times[-1]), rej, ms, r.key_cur, r.key_pre, scans)
        t0 = time.perf_counter()                       # then the accepted call, once: it records the closure
        acc = eng.performRSLoopClosure(times[-1], prm)
        accepted_ms = 1e3 * (time.perf_counter() - t0)
        row = {"status": acc.status, "key_cur": acc.key_cur, "key_pre": acc.key_pre, "n_cur": acc.n_cur, "n_prev": acc.n_prev,
               "iterations": acc.icp.iterations, "converged": acc.icp.converged, "fitness": acc.icp.fitness_score,
               "accepted_ms": round(accepted_ms, 4), "pose_from": [round(float(v), 5) for v in acc.pose_from],
               "loop_closure_rs_ms": ms}
        assert rej_status == s2m.S2M_LOOP_REJECTED and r.icp.iterations == acc.icp.iterations, (rej_status, row)
        # today's binding: host clouds, per-frame transform, concatenation, two filters, ICP from host memory
        kc, kp = acc.key_cur, acc.key_pre
        ref = s2m.MapOptimizationS2M()

        def host_path():
            cur = ref.voxelGrid(ref.transformPointCloud(clouds[kc], stored[kc]), 0.5)
            parts = [ref.transformPointCloud(clouds[k], stored[k]) for k in range(max(0, kp - 25), min(n - 1, kp + 25) + 1)]
            prev = ref.voxelGrid(np.concatenate(parts), 0.5)
            return cur, prev, ref.icpAlign(cur, prev, max_correspondence_distance=30.0)
        cur, prev, icp = host_path()
        assert (cur.shape[0], prev.shape[0], icp[3]) == (acc.n_cur, acc.n_prev, acc.icp.iterations)
        assert np.array_equal(icp[0].reshape(-1), np.array(acc.icp.T, np.float32))
        row["host_path_ms"] = _median_ms(host_path, a.warmup, a.reps)
        row["icp_ms"] = _median_ms(lambda: ref.icpAlign(cur, prev, max_correspondence_distance=30.0), a.warmup, a.reps)
        row["icp_share"] = round(row["icp_ms"] / row["loop_closure_rs_ms"], 3)
        ref.close()
        # detection alone: one more key far from everything, so that no key passes
        eng.saveKeyFrame(np.array([1e4, 1e4, 0, 0, 0, 0], np.float32), float(n), small)
        row["detect_ms"] = _median_ms(lambda: eng.lib.s2m_loop_closure_rs(eng.h, float(n), C.byref(prm), C.byref(r)), a.warmup, a.reps)
        assert r.status == s2m.S2M_LOOP_NONE
        eng.close()
        out["sizes"][str(n)] = row
    if a.kernel_stats:
        out["kernels_device_us"] = _stats(a.kernel_stats)
    out["note"] = "wall clock, median after warm-up; every call ends with the library's own synchronisation"
    print(json.dumps(out))
    if a.run_async:
        async_out["note"] = ("wall clock on the host, medians after warm-up; search_us are HIP-event times on the loop stream; the closure is "
                             "timed with fitness_score = -1 (rejected after the whole ICP)")
        with open(a.async_out, "w") as f:
            f.write(json.dumps(async_out) + "\n")


if __name__ == "__main__":
    main()
