"""Wall time of saving a session into memory and of loading it into a fresh handle, against rebuilding the same handle key by key.

The store is the 5 000-key revisit of tools/bench_loop.py (30 000-point frames at keys 0 .. 27 and the last key, 1 000 points
elsewhere) with every key's descriptor in the ScanContext store and the graph of that run: the odometry chain and the accepted
closure of the last key as a between factor. Medians after warm-up of:
  save_ms            s2m_session_save into a preallocated host buffer (the write callback is one memmove per chunk)
  load_ms            s2m_session_load from that buffer into a handle whose stores were reset (its device arrays are kept, as a
                     node's are that loads a second time), and load_fresh_ms: the one load into a handle just created
  rebuild_ms         the baseline, and the only way before the session calls: per key s2m_kf_add from host records,
                     s2m_sc_add_descriptor, s2m_pg_add_odometry, then the between factor - each of them waits for the stream
  memcpy_h2d_ms /    one hipMemcpy of the blob's byte count between pinned host memory and the device, each way, in the same
  memcpy_d2h_ms      run: how far save and load are from a plain copy (save_over_memcpy, load_over_memcpy)
The line goes to stdout and to profiles/session_bench_line.json (--out).

  python tools/bench_session.py [--keys 5000] [--reps 5] [--warmup 1]

With --append the same blob is appended behind itself instead (s2m_session_append into a handle that holds the session already),
as stored and with an anchor, beside s2m_session_load of the blob into a reset handle in the same process, and
s2m_session_place alone; the line goes to profiles/session_append_bench_line.json. The expectation to report against is
"an append costs about one load": append_over_load is that ratio.
  append_ms          s2m_session_append with a NULL anchor: the handle is reset and loaded again before every repetition (not timed)
  append_anchor_ms   the same with an anchor (k_session_place over the appended keys, the factors moved on the host)
  place_ms           s2m_session_place of the appended session
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_loop as BL


def _median_ms(fn, warmup, reps, before=None):
    ts = []
    for k in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = ts[warmup:]
    return round(1e3 * float(np.median(ts)), 3), round(1e3 * float(min(ts)), 3), round(1e3 * float(max(ts)), 3)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="time s2m_session_append / s2m_session_place instead")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "session_append_bench_line.json" if a.append else "session_bench_line.json")
    from liorf_amd import s2m

    n = a.keys
    true = BL._true_poses(n)
    big = BL._clouds([true[k] for k in range(BL.N_BIG)] + [true[-1]])
    small = big[1][:BL.SMALL_PTS].copy()
    stored = true.copy()
    stored[-1] += BL.DRIFT
    stored = stored.astype(np.float32)
    times = np.arange(n, dtype=np.float64)
    clouds = [big[k] if k < BL.N_BIG else small for k in range(n - 1)] + [big[-1]]

    eng = s2m.MapOptimizationS2M()
    for k in range(n):
        eng.saveKeyFrame(stored[k], times[k], clouds[k])
        eng.makeAndSaveScancontextAndKeys(clouds[k])
        eng.addOdomFactor(stored[k])
    acc = eng.performRSLoopClosure(times[-1], s2m.default_loop_params(search_radius=15.0, search_num=25, icp_leaf=0.5))
    assert acc.status == s2m.S2M_LOOP_ACCEPTED, acc.status
    rel = s2m.between_xyzrpy(acc.pose_from, acc.pose_to)
    var = [acc.icp.fitness_score] * 6
    eng.pgAddBetween(acc.key_cur, acc.key_pre, rel, var)
    eng.pgOptimize()
    print(f"{n} keys stored", file=sys.stderr, flush=True)

    info = eng.session_info()
    size = int(info.bytes)
    buf = (C.c_char * size)()
    base = C.addressof(buf)
    at = [0]

    def wr(_u, data, nbytes):
        C.memmove(base + at[0], data, nbytes)
        at[0] += nbytes
        return 0

    def rd(_u, data, nbytes):
        if at[0] + nbytes > size:
            return s2m.S2M_ERR_FORMAT
        C.memmove(data, base + at[0], nbytes)
        at[0] += nbytes
        return 0
    wr_c, rd_c = s2m.SESSION_WRITE_FN(wr), s2m.SESSION_READ_FN(rd)

    def rewind():
        at[0] = 0

    def save():
        rc = eng.lib.s2m_session_save(eng.h, wr_c, None)
        assert rc == 0 and at[0] == size, (rc, at[0])
    save_ms = _median_ms(save, a.warmup, a.reps, rewind)
    blob = bytes(buf)
    s2m.session_check(blob)

    t0 = time.perf_counter()
    new = s2m.MapOptimizationS2M()
    rewind()
    assert new.lib.s2m_session_load(new.h, rd_c, None, None) == 0
    load_fresh_ms = round(1e3 * (time.perf_counter() - t0), 3)
    assert new.session_save() == blob                   # what was loaded is what was saved

    def reset():
        new.kfReset(); new.scReset(); new.pgReset()
        rewind()

    def load():
        rc = new.lib.s2m_session_load(new.h, rd_c, None, None)
        assert rc == 0, rc
    load_ms = _median_ms(load, a.warmup, a.reps, reset)

    if a.append:
        anchor = (C.c_float * 6)(12.0, -7.0, 0.4, 0.02, -0.03, 0.4)

        def reload():
            reset()
            load()
            rewind()

        def append(anc):
            rc = new.lib.s2m_session_append(new.h, rd_c, None, anc, None, None)
            assert rc == 0, rc
        append_ms = _median_ms(lambda: append(None), a.warmup, a.reps, reload)
        append_anchor_ms = _median_ms(lambda: append(anchor), a.warmup, a.reps, reload)
        assert new.sessionAppended() == (n, n)
        move = (C.c_float * 6)(0.01, -0.02, 0.0, 0.0, 0.0, 0.001)

        def place():
            rc = new.lib.s2m_session_place(new.h, move)
            assert rc == 0, rc
        place_ms = _median_ms(place, a.warmup, a.reps)
        s2m.session_check(new.session_save())
        new.close()
        eng.close()
        names = ("median", "min", "max")
        out = {"workload": f"tools/bench_session.py --append: the {n}-key revisit of tools/bench_loop.py appended behind itself",
               "keys": n, "points": int(info.n_points), "blob_bytes": size, "reps": a.reps, "warmup": a.warmup,
               "load_ms": dict(zip(names, load_ms)), "append_ms": dict(zip(names, append_ms)),
               "append_anchor_ms": dict(zip(names, append_anchor_ms)), "place_ms": dict(zip(names, place_ms)),
               "append_over_load": round(append_ms[0] / load_ms[0], 2), "append_anchor_over_load": round(append_anchor_ms[0] / load_ms[0], 2),
               "place_over_load": round(place_ms[0] / load_ms[0], 3),
               "note": "wall clock on the host, same process; the load is s2m_session_load of the same blob into a reset handle; an "
                       "append includes the callback's memmove of every chunk as the load does"}
        line = json.dumps(out)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return

    # the baseline: the same handle by the per-key adds, from the same host data (descriptors out of the blob)
    hdr = struct.unpack("<II7iIQ6QQ", blob[8:112])
    sizes = hdr[11:17]
    desc_at = 112 + sizes[0] + sizes[1]
    descs = np.frombuffer(blob, "<f8", count=n * 1200, offset=desc_at).reshape(n, 20, 60)

    def rebuild():
        for k in range(n):
            new.saveKeyFrame(stored[k], times[k], clouds[k])
            new.scAddDescriptor(descs[k])
            new.addOdomFactor(stored[k])
        new.pgAddBetween(acc.key_cur, acc.key_pre, rel, var)
    rebuild_ms = _median_ms(rebuild, 0, max(1, min(a.reps, 2)), reset)
    new.close()

    # the yardstick: one pinned copy of the same byte count each way
    import torch
    host = torch.empty(size, dtype=torch.uint8).pin_memory()
    dev = torch.empty(size, dtype=torch.uint8, device="cuda")

    def h2d():
        dev.copy_(host, non_blocking=True)
        torch.cuda.synchronize()

    def d2h():
        host.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
    h2d_ms = _median_ms(h2d, 2, max(a.reps, 5))
    d2h_ms = _median_ms(d2h, 2, max(a.reps, 5))

    names = ("median", "min", "max")
    out = {"workload": f"tools/bench_session.py: the {n}-key revisit of tools/bench_loop.py, every key's descriptor stored, odometry chain "
                       "and the accepted closure in the graph, after one optimise",
           "keys": n, "points": int(info.n_points), "descriptors": int(info.n_descriptors), "factors": int(info.n_factors),
           "blob_bytes": size, "reps": a.reps, "warmup": a.warmup,
           "save_ms": dict(zip(names, save_ms)), "load_ms": dict(zip(names, load_ms)), "load_fresh_ms": load_fresh_ms,
           "rebuild_ms": dict(zip(names, rebuild_ms)),
           "memcpy_d2h_ms": dict(zip(names, d2h_ms)), "memcpy_h2d_ms": dict(zip(names, h2d_ms)),
           "save_gb_per_s": round(size / save_ms[0] / 1e6, 2), "load_gb_per_s": round(size / load_ms[0] / 1e6, 2),
           "save_over_memcpy": round(save_ms[0] / d2h_ms[0], 2), "load_over_memcpy": round(load_ms[0] / h2d_ms[0], 2),
           "rebuild_over_load": round(rebuild_ms[0] / load_ms[0], 1),
           "note": "wall clock on the host; save and load end with the library's own synchronisation and include the callback's "
                   "memmove of every chunk between the pinned staging chunk and the blob in pageable memory; the memcpy yardstick "
                   "moves pinned memory only"}
    eng.close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
