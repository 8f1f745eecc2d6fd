"""Wall time of extractSurroundingKeyFrames() on the resident key-frame store against today's binding.

The chain workload of bench.py:chain_figures (30 000-point ray-cast key frames, map leaf 0.5) with stores of 100, 5 000 and
50 000 keys on a straight trajectory (0.5 m between keys, 1 s apart, density 2.0, radius 50 m). The newest key is at the end
of the line, so the radius search sees one side of it: about thirty centroid frames. A recent-key window of 25 s (instead of
the reference's 10 s; the keys here are 1 s apart) adds twenty recent frames, so that about fifty frames reach the map, as in
bench.py's chain figure.
Keys farther than 60 m from the newest one can never be selected; they hold a 1 000-point cloud so that the largest store
fits in memory and the set-up stays short. Medians after warm-up of:
  extract_surrounding_ms     s2m_extract_surrounding (selection + transform + filter + map index), no readback
  extract_cloud_device_ms    s2m_extract_cloud on the same frame list with the clouds already in HBM (bench.py's chain figure)
  extract_cloud_host_ms      the same list from host memory (the binding INTEGRATION.md showed before the store)
  kf_add_last_downsample_ms  s2m_kf_add(S2M_KF_FROM_LAST_DOWNSAMPLE) of a filtered 120 000-point scan
The frame list comes from the new call's `keys` output.

  python tools/bench_keyframes.py                           one JSON line
  python tools/bench_keyframes.py --selection-only 5000     only the new call, for rocprofv3 --kernel-trace --stats
  python tools/bench_keyframes.py --kernel-stats stats.csv  folds the k_kf_select* rows of such a run into the JSON line
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

FRAME_PTS, RAW_PTS, MAP_LEAF, SCAN_LEAF, DENSITY, RECENT_S = 30000, 120000, 0.5, 0.4, 2.0, 25.0


def _clouds():
    from liorf_amd import synth
    scene = synth.make_scene(seed=11, half=70.0, n_boxes=92)
    rng = np.random.default_rng(1)
    big = []
    for k in range(4):
        pose = np.array([0.01 * np.sin(k), -0.008 * np.cos(k), 0.05 * np.sin(0.2 * k), 3.0 * k - 6.0, 0.3 * np.sin(0.3 * k), 0.0])
        c = synth.to_xyzi(synth.make_scan(scene, pose, "velodyne64", FRAME_PTS, seed=100 + k))
        c[:, 4] = rng.uniform(0, 100, FRAME_PTS).astype(np.float32)
        big.append(c)
    raw = synth.to_xyzi(synth.make_scan(scene, np.array([0.0, 0.0, 0.1, 0.5, 0.2, 0.0]), "velodyne64", RAW_PTS, seed=7))
    return big, big[0][:1000].copy(), raw


def _store(eng, n, big, small):
    x = (np.arange(n, dtype=np.float32) - np.float32(n - 1)) * np.float32(0.5)     # the newest key at the origin
    poses = np.zeros((n, 6), np.float32)
    poses[:, 0] = x
    poses[:, 1] = 0.2 * np.sin(0.1 * np.arange(n))
    poses[:, 5] = 0.01 * np.arange(n)
    times = np.arange(n, dtype=np.float64)
    for k in range(n):
        eng.saveKeyFrame(poses[k], times[k], big[k % len(big)] if x[k] > -60.0 else small)
    return poses, times


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
            m = re.search(r"k_kf_select\w*", r.get("Name", ""))
            if m:
                rows[m.group(0)] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3)}
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,5000,50000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--selection-only", type=int, default=0, help="store size: run only s2m_extract_surrounding")
    ap.add_argument("--kernel-stats", default="", help="rocprofv3 kernel_stats.csv of a --selection-only run")
    a = ap.parse_args(argv)
    import torch
    from liorf_amd import s2m

    big, small, raw = _clouds()
    tc_offset = 5.0                                                 # twenty recent keys (t > t_last + 5 - 25)
    prm = s2m.default_kf_params(density=DENSITY, map_leaf=MAP_LEAF, recent_window_s=RECENT_S)
    sizes = [a.selection_only] if a.selection_only else [int(s) for s in a.sizes.split(",")]
    out = {"workload": "chain: 30 000-point key frames, map leaf 0.5, density 2.0, radius 50 m, recent window 25 s (20 recent keys)",
           "sizes": {}}
    for n in sizes:
        eng = s2m.MapOptimizationS2M()
        poses, times = _store(eng, n, big, small)
        tc = float(times[-1] + tc_offset)
        n_out = C.c_size_t(0)
        surround = lambda: eng.lib.s2m_extract_surrounding(eng.h, tc, C.byref(prm), None, 32, 0, C.byref(n_out), None, 0, None)
        row = {"extract_surrounding_ms": _median_ms(surround, a.warmup, a.reps)}
        if not a.selection_only:
            keys = eng.extractSurroundingKeyFrames(tc, prm)
            clouds = [big[k % len(big)] if poses[k, 0] > -60.0 else small for k in keys]
            row.update(frames=int(len(keys)), points_in=int(sum(c.shape[0] for c in clouds)),
                       laserCloudSurfFromMapDSNum=int(eng.laserCloudSurfFromMapDSNum))
            dev = {id(c): torch.from_numpy(c).cuda() for c in clouds}
            torch.cuda.synchronize()
            ptrs = [(dev[id(c)].data_ptr(), c.shape[0]) for c in clouds]
            kp = poses[keys]
            ref = s2m.MapOptimizationS2M()
            row["extract_cloud_device_ms"] = _median_ms(lambda: ref.extractCloud(32, kp, MAP_LEAF, readback=False, device_frames=ptrs),
                                                        a.warmup, a.reps)
            row["extract_cloud_host_ms"] = _median_ms(lambda: ref.extractCloud(clouds, kp, MAP_LEAF, readback=False), a.warmup, a.reps)
            assert ref.laserCloudSurfFromMapDSNum == eng.laserCloudSurfFromMapDSNum
            ref.close()
            del dev
        out["sizes"][str(n)] = row
        eng.close()
    if not a.selection_only:
        # a revisited area: 20 000 keys on a 20 m circle driven round and round, every one a radius candidate (past the
        # selection's LDS tile of 4 096), 1 000-point clouds; the selection's global-memory sort dominates here
        eng = s2m.MapOptimizationS2M()
        n = 20000
        ang = np.arange(n) * 0.05
        lp = np.zeros((n, 6), np.float32)
        lp[:, 0], lp[:, 1] = 20 * np.cos(ang), 20 * np.sin(ang)
        for k in range(n):
            eng.saveKeyFrame(lp[k], float(k), small)
        tc = float(n - 1 + tc_offset)
        n_out = C.c_size_t(0)
        loop = lambda: eng.lib.s2m_extract_surrounding(eng.h, tc, C.byref(prm), None, 32, 0, C.byref(n_out), None, 0, None)
        out["loop_20000_candidates"] = {"extract_surrounding_ms": _median_ms(loop, a.warmup, a.reps),
                                        "frames": int(len(eng.extractSurroundingKeyFrames(tc, prm)))}
        eng.close()
        eng = s2m.MapOptimizationS2M()
        eng.downsampleCurrentScan(raw, SCAN_LEAF, readback=False)
        pose = np.zeros(6, np.float32)
        k = [0]

        def add():
            k[0] += 1
            eng.saveKeyFrame(pose, float(k[0]))
        out["kf_add_last_downsample_ms"] = _median_ms(add, a.warmup, a.reps)
        out["kf_add_points"] = int(eng.laserCloudSurfLastDSNum)
        eng.close()
    if a.kernel_stats:
        out["selection_kernels_device_us"] = _stats(a.kernel_stats)
    out["note"] = "wall clock, median after warm-up; extract_* include the map index build and end with the library's own synchronisation"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
