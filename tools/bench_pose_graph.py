"""Wall time of one pose-graph optimise after one added loop, and of s2m_pg_apply_to_store, against the CPU reference.

The synthetic figure-of-eight of tests/ref/pose_graph_ref.py (seed 20250204, driven twice, keys 1 m apart, 40 loops) at
2 000, 10 000 and 50 000 keys.  The graph is optimised once with its 40 loops; then one more loop is added and the next
optimise is timed - the state a node is in when a closure arrives.  Beside each device figure:
  cpu_optimize_ms   the reference's whole optimise of the same problem (numpy linearisation, scipy sparse normal equations)
  cpu_solve_ms      of that, the sparse solves alone - what a compiled CPU library would also pay
apply_to_store_ms is s2m_pg_apply_to_store over the whole store (10-point frames), set_poses_ms the path it replaces:
s2m_pg_get_poses to the caller and s2m_kf_set_poses back.

  python tools/bench_pose_graph.py [--sizes 2000,10000,50000] [--out profiles/pose_graph_bench_line.json]

--marginals times the covariance read-out instead, on the same graphs after their optimise (median of --reps runs after a
warm-up of each call, the calls alternating inside every repetition):
  marginal_single_ms    s2m_pg_marginal(last key): six CG solves one after the other, the path before the block solve
  marginals_{1,2,8}_ms  s2m_pg_marginals for the last 1, 2 and 8 distinct keys (6, 12 and 48 right-hand sides in lockstep)
  joint_marginal_ms     s2m_pg_joint_marginal(n // 2, last)
with marginals_1_over_single (the ratio of the first two) and eight_times_marginals_1_ms beside marginals_8_ms.

  python tools/bench_pose_graph.py --marginals --sizes 2000,10000 --reps 7 --out profiles/pose_graph_marginals_bench_line.json

--async measures the launched optimise (s2m_pg_optimize_launch / _poll / _collect) against the synchronous call of the same
session, for the same one optimise after one added loop (medians of --reps runs after one warm-up run):
  optimize_ms            (a) s2m_pg_optimize
  launch_ms, held_ms     (b) the launch, and the time the handle is held: the launch plus all polls, one every --poll-us
  latency_ms             (c) from the launch to the poll that delivers the result (polls, ranges: how many of each)
  held_over_sync         held_ms / optimize_ms
  bitwise_equal          result bytes and estimates of the launched solve against the synchronous one, every run
  registration_ms        (d) a 12 000 x 30 000 registration (set_scan + optimize) alone and with the optimise pending

  python tools/bench_pose_graph.py --async --sizes 2000,10000 --out profiles/pose_graph_async_bench_line.json

--consistency times s2m_pg_consistent_loops, the whole C call from the host arrays to the selection, at
64, 512 and 4096 candidates on the dead-reckoned estimates of the figure-of-eight at 10 000 keys (median and minimum of --reps
calls after a warm-up call), beside the NumPy model of the same call in the same process (model_ms, one run) and whether the two
agree (equals_model):

  python tools/bench_pose_graph.py --consistency --reps 7 --out profiles/pg_consistency_bench_line.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402
from liorf_amd import s2m, synth  # noqa: E402


def one_size(n, reps):
    g = P.figure_eight(n, 40)
    half = n // 2
    truth = P.figure_eight(n, 0, truth_only=True)
    i, j = n - 3, n - 3 - half
    rel = P.xyzrpy_from_pose(truth[i][0].T @ truth[j][0], truth[i][0].T @ (truth[j][1] - truth[i][1])).astype(np.float32)
    m = s2m.MapOptimizationS2M()
    out = {}
    try:
        cloud = synth.to_xyzi(np.random.default_rng(0).uniform(-5, 5, (10, 3)).astype(np.float32))
        init = g.poses().astype(np.float32)
        for k in range(n):
            m.saveKeyFrame(init[k], float(k), cloud)
        t = []
        for _ in range(reps):
            CS.load_into(m, g)
            first = m.pgOptimize()
            m.pgAddBetween(i, j, rel, np.full(6, 0.3))
            t0 = time.perf_counter()
            res = m.pgOptimize()
            t.append(time.perf_counter() - t0)
        out.update(first_iterations=first.iterations, first_inner_iterations=first.inner_iterations, iterations=res.iterations,
                   inner_iterations=res.inner_iterations, converged=res.converged, error_after=res.error_after,
                   optimize_ms=round(1e3 * float(np.median(t)), 3))
        ta, ts = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); m.pgApplyToStore(0, n); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); m.correctPoses(m.pgPoses(), 0); ts.append(time.perf_counter() - t0)
        out.update(apply_to_store_ms=round(1e3 * float(np.median(ta)), 3), set_poses_ms=round(1e3 * float(np.median(ts)), 3))
    finally:
        m.close()
    # the CPU reference on the same problem
    P.optimize(g, "normal")
    g.add_between(i, j, rel, np.full(6, 0.3))
    solve_s = [0.0]
    inner = P.solve_step

    def timed(*a):
        t0 = time.perf_counter()
        r = inner(*a)
        solve_s[0] += time.perf_counter() - t0
        return r
    P.solve_step = timed
    try:
        t0 = time.perf_counter()
        ref = P.optimize(g, "normal")
        cpu = time.perf_counter() - t0
    finally:
        P.solve_step = inner
    out.update(cpu_iterations=ref.iterations, cpu_error_after=ref.error_after, cpu_optimize_ms=round(1e3 * cpu, 3),
               cpu_solve_ms=round(1e3 * solve_s[0], 3))
    return out


def marginals_one_size(n, reps):
    g = P.figure_eight(n, 40)
    m = s2m.MapOptimizationS2M()
    try:
        CS.load_into(m, g)
        res = m.pgOptimize()
        last = n - 1
        spread = [last - k * (n // 9) for k in range(8)]            # eight distinct keys over the trajectory, the last one first
        calls = [("marginal_single_ms", lambda: m.pgMarginal(last)), ("marginals_1_ms", lambda: m.pgMarginals(spread[:1])),
                 ("marginals_2_ms", lambda: m.pgMarginals(spread[:2])), ("marginals_8_ms", lambda: m.pgMarginals(spread)),
                 ("joint_marginal_ms", lambda: m.pgJointMarginal(n // 2, last))]
        same = bool(np.array_equal(m.pgMarginal(last), m.pgMarginals([last])[0]))
        t = {name: [] for name, _ in calls}
        for rep in range(reps + 1):                                # the first round is the warm-up
            for name, fn in calls:
                t0 = time.perf_counter()
                fn()                                               # (every call ends in a stream synchronise)
                if rep > 0:
                    t[name].append(time.perf_counter() - t0)
        out = {name: round(1e3 * float(np.median(v)), 3) for name, v in t.items()}
        out.update({name.replace("_ms", "_min_ms"): round(1e3 * float(np.min(v)), 3) for name, v in t.items()})
        out.update(keys=n, n_factors=res.n_factors, optimize_inner_iterations=res.inner_iterations, reps=reps, block_columns=s2m.S2M_PG_BLOCK_COLUMNS,
                   single_block_bitwise_equal=same,
                   marginals_1_over_single=round(out["marginals_1_ms"] / out["marginal_single_ms"], 4),
                   eight_times_marginals_1_ms=round(8 * out["marginals_1_ms"], 3))
        return out
    finally:
        m.close()


def async_one_size(n, reps, poll_us, scans):
    g = P.figure_eight(n, 40)
    half = n // 2
    truth = P.figure_eight(n, 0, truth_only=True)
    i, j = n - 3, n - 3 - half
    rel = P.xyzrpy_from_pose(truth[i][0].T @ truth[j][0], truth[i][0].T @ (truth[j][1] - truth[i][1])).astype(np.float32)
    m = s2m.MapOptimizationS2M()
    lib, h = m.lib, m.h
    pending = s2m.S2M_PG_PENDING
    raw = lambda r: C.string_at(C.addressof(r), C.sizeof(r))

    def ready():                                                   # the state a node is in when a closure arrives
        CS.load_into(m, g)
        m.pgOptimize()
        m.pgAddBetween(i, j, rel, np.full(6, 0.3))

    def launched(poll_s, beside=None):
        r = s2m.PgResult()
        t0 = time.perf_counter()
        rc = lib.s2m_pg_optimize_launch(h, None, C.byref(r))
        t1 = time.perf_counter()
        assert rc == pending, rc
        if beside:
            beside()
        held, polls = t1 - t0, 0
        while rc == pending:
            if poll_s > 0:
                time.sleep(poll_s)
            p0 = time.perf_counter()
            rc = lib.s2m_pg_optimize_poll(h, C.byref(r))
            held += time.perf_counter() - p0
            polls += 1
        assert rc == 0, rc
        return t1 - t0, held, polls, time.perf_counter() - t0, r

    try:
        sync, runs, same = [], [], True
        for k in range(reps + 1):                                  # the first round is the warm-up
            ready()
            t0 = time.perf_counter()
            want = m.pgOptimize()
            t = time.perf_counter() - t0
            want_poses = m.pgPoses()
            ready()
            run = launched(poll_us * 1e-6)
            same = same and raw(run[4]) == raw(want) and bool(np.array_equal(m.pgPoses(), want_poses))
            if k > 0:
                sync.append(t)
                runs.append(run)
        med = lambda k: round(1e3 * float(np.median([x[k] for x in runs])), 4)
        out = dict(keys=n, n_factors=want.n_factors, iterations=want.iterations, inner_iterations=want.inner_iterations, reps=reps, poll_us=poll_us,
                   optimize_ms=round(1e3 * float(np.median(sync)), 4), launch_ms=med(0), held_ms=med(1), latency_ms=med(3),
                   polls=int(np.median([x[2] for x in runs])), bitwise_equal=same)
        out["polls_ms"] = round(out["held_ms"] - out["launch_ms"], 4)
        out["held_over_sync"] = round(out["held_ms"] / out["optimize_ms"], 4)
        out["latency_over_sync"] = round(out["latency_ms"] / out["optimize_ms"], 4)
        ready()
        tight = launched(0.0)
        out.update(latency_tight_ms=round(1e3 * tight[3], 4), polls_tight=tight[2])
        # (d) a registration alone, and between the launch and the first poll of a pending optimise
        cloud, cfgs = scans
        m.setInputCloud(cloud)
        reg = {}
        for name in ("alone", "optimise_pending"):
            ts, still = [], 0
            for q in range(2 + 2 * len(cfgs)):
                scan, pose = cfgs[q % len(cfgs)]

                def register():
                    t0 = time.perf_counter()
                    m.setScan(scan)
                    m.transformTobeMapped = pose.copy()
                    m.scan2MapOptimization()
                    ts.append(time.perf_counter() - t0)
                if name == "alone":
                    register()
                else:
                    ready()
                    run = launched(poll_us * 1e-6, register)
                    still += int(run[2] > 1)                       # (the first poll behind the registration still said pending)
            reg[name + "_ms"] = round(1e3 * float(np.median(ts[2:])), 4)
            if name != "alone":
                reg["still_pending_after_registration"] = still
        reg["registrations"] = 2 * len(cfgs)
        out["registration_ms"] = reg
        return out
    finally:
        m.close()


def consistency_sizes(n, ms, reps):
    """s2m_pg_consistent_loops, the whole C call, on the dead-reckoned estimates of the figure-of-eight at n keys: m candidates,
    three in four true loops from second-lap keys to their first-lap keys (ground truth plus the loops' noise), one in four a
    false loop between two unrelated keys; beside it the NumPy model (tests/ref/pg_consistency_ref.py) in the same process."""
    import pg_consistency_ref as R
    g = P.figure_eight(n, 0)
    truth = P.figure_eight(n, 0, truth_only=True)
    half = n // 2
    X = R.states_of(g.X)
    gpu = s2m.MapOptimizationS2M()
    out = {}
    try:
        gpu.pgReset()
        for k, x in enumerate(X):
            gpu.pgSetEstimate(k, x[:9], x[9:])
        for m in ms:
            rng = np.random.default_rng(P.SEED + m)
            kf = np.sort(rng.choice(np.arange(half, n), m, replace=False)).astype(np.int32)
            kt = (kf - half).astype(np.int32)
            false = rng.random(m) < 0.25
            kt[false] = ((kt[false] + rng.integers(half // 8, half - half // 8, int(false.sum()))) % half).astype(np.int32)
            rel = np.empty((m, 6), np.float32)
            for c in range(m):
                a, b = truth[kf[c]], truth[kf[c] - half]                     # a false loop claims the true relation for another key
                Rz = a[0].T @ b[0] @ P.so3_exp(rng.normal(0.0, 5e-3, 3))
                rel[c] = P.xyzrpy_from_pose(Rz, a[0].T @ (b[1] - a[1]) + rng.normal(0.0, 0.03, 3)).astype(np.float32)
            t = []
            for rep in range(reps + 1):                                    # the first call is the warm-up (it sizes the buffers)
                t0 = time.perf_counter()
                sel, deg, rec = gpu.pgConsistentLoops(kf, kt, rel)
                if rep > 0:
                    t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = R.run(X, kf, kt, rel)
            model_s = time.perf_counter() - t0
            same = bool(np.array_equal(sel, want["selected"]) and np.array_equal(deg, want["degree"]) and rec.start == want["start"] and
                        rec.n_consistent_pairs == want["n_consistent_pairs"])
            out[str(m)] = dict(call_ms=round(1e3 * float(np.median(t)), 4), call_min_ms=round(1e3 * float(np.min(t)), 4),
                               model_ms=round(1e3 * model_s, 1), n_selected=int(rec.n_selected), n_true=int((~false).sum()),
                               true_selected=int((sel & ~false).sum()), false_selected=int((sel & false).sum()),
                               n_consistent_pairs=int(rec.n_consistent_pairs), equals_model=same, reps=reps)
            print(m, json.dumps(out[str(m)]), file=sys.stderr, flush=True)
    finally:
        gpu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,50000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--marginals", action="store_true", help="time the covariance read-out instead of the optimise")
    ap.add_argument("--async", dest="run_async", action="store_true", help="time the launched optimise against the synchronous call")
    ap.add_argument("--poll-us", type=float, default=200.0, help="--async: sleep between two polls")
    ap.add_argument("--consistency", action="store_true", help="time s2m_pg_consistent_loops beside its NumPy model")
    ap.add_argument("--candidates", default="64,512,4096", help="--consistency: the candidate counts")
    ap.add_argument("--keys", type=int, default=10000, help="--consistency: keys of the figure-of-eight")
    a = ap.parse_args()
    if a.consistency:
        line = {"workload": "figure-of-eight driven twice, dead-reckoned estimates, %d keys; loop candidates, three in four true, default "
                            "tolerances; the whole s2m_pg_consistent_loops call and the NumPy model (seed %d)" % (a.keys, P.SEED),
                "keys": a.keys, "candidates": consistency_sizes(a.keys, [int(x) for x in a.candidates.split(",")], a.reps)}
        txt = json.dumps(line)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    if a.run_async:
        cfgs = [synth.make_config("small", scan_index=k) for k in range(4)]
        scans = (synth.to_xyzi(cfgs[0]["map"]), [(synth.to_xyzi(c["scan"]), c["pose_init"]) for c in cfgs])
        line = {"workload": "figure-of-eight driven twice, 40 loops, one optimise after one added loop, synchronous and launched (seed %d); "
                            "registration: %d x %d points" % (P.SEED, scans[1][0][0].shape[0], scans[0].shape[0]), "sizes": {}}
        for n in [int(x) for x in a.sizes.split(",")]:
            line["sizes"][str(n)] = async_one_size(n, a.reps, a.poll_us, scans)
            print(n, json.dumps(line["sizes"][str(n)]), file=sys.stderr, flush=True)
        txt = json.dumps(line)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    if a.marginals:
        line = {"workload": "figure-of-eight driven twice, 40 loops, optimised; marginal covariances at the estimates (seed %d)" % P.SEED, "sizes": {}}
        for n in [int(x) for x in a.sizes.split(",")]:
            line["sizes"][str(n)] = marginals_one_size(n, a.reps)
            print(n, json.dumps(line["sizes"][str(n)]), file=sys.stderr, flush=True)
        txt = json.dumps(line)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    line = {"workload": "figure-of-eight driven twice, 40 loops, one optimise after one added loop (seed %d)" % P.SEED, "sizes": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        line["sizes"][str(n)] = one_size(n, a.reps)
        print(n, json.dumps(line["sizes"][str(n)]), file=sys.stderr, flush=True)
    txt = json.dumps(line)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
