"""Wall time of the global map (s2m_global_map) and the saved map (s2m_kf_map_cloud) on the resident key-frame store.

global_map_ms      publishGlobalMap() on stores of 5 000 and 50 000 keys on a 100 m circle driven round and round (0.5 m between
                   keys): every key is a radius candidate of R = 1 000 m. kitti.yaml settings (pose density 10 m, leaf 1.0 m) and
                   M2DGR.yaml settings (pose density 3 m, leaf 1.0 m); 5 000-point key frames. selection_ms is the same store
                   with a pose density and radius that select one frame (the key selection alone, plus a 5 000-point filter).
map_cloud_ms       saveMapService()'s cloud for all keys of 1 000- and 5 000-key stores of 30 000-point frames, leaf 0 (the chunked
                   copy-out of GlobalMap.pcd) and leaf 0.4 (SurfMap.pcd at that resolution), to host memory. host_ms beside it is
                   the composition through host memory: s2m_transform_cloud per key, numpy concatenation, and for leaf 0.4
                   s2m_voxel_downsample of the host cloud.
Medians after warm-up; every call ends with the library's own synchronisation.

  python tools/bench_global_map.py                          one JSON line
  python tools/bench_global_map.py --selection-only 50000   only s2m_global_map on that store, for rocprofv3 --kernel-trace --stats
  python tools/bench_global_map.py --kernel-stats stats.csv folds the k_kf_* / k_rs_* rows of such a run into the JSON line
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

F = np.float32
SETTINGS = {"kitti": (10.0, 1.0), "M2DGR": (3.0, 1.0)}


def _median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t)), 4)


def _clouds(n_pts, k=4):
    from liorf_amd import synth
    scene = synth.make_scene(seed=11, half=70.0, n_boxes=92)
    rng = np.random.default_rng(1)
    out = []
    for i in range(k):
        pose = np.array([0.01 * np.sin(i), -0.008 * np.cos(i), 0.05 * np.sin(0.2 * i), 3.0 * i - 6.0, 0.3 * np.sin(0.3 * i), 0.0])
        c = synth.to_xyzi(synth.make_scan(scene, pose, "velodyne64", n_pts, seed=100 + i))
        c[:, 4] = rng.uniform(0, 100, n_pts).astype(F)
        out.append(c)
    return out


def _circle_store(eng, n, clouds, radius=100.0, step=0.5):
    a = np.arange(n) * (step / radius)
    poses = np.zeros((n, 6), F)
    poses[:, 0], poses[:, 1] = radius * np.cos(a), radius * np.sin(a)
    poses[:, 2] = 0.5 * np.sin(3 * a)
    poses[:, 5] = a + np.pi / 2
    for k in range(n):
        eng.saveKeyFrame(poses[k], float(k), clouds[k % len(clouds)])
    return poses


def _gmap_call(eng, prm):
    n_out, n_keys = C.c_size_t(0), C.c_size_t(0)
    buf = np.zeros((1, 8), F)

    def call():
        rc = eng.lib.s2m_global_map(eng.h, C.byref(prm), buf.ctypes.data, 32, 0, C.byref(n_out), None, 0, C.byref(n_keys))
        assert rc >= 0, eng.lib.s2m_last_error(eng.h)
    return call, n_out, n_keys


def _stats(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"k_(kf|rs|heads|vox|transform|copy)\w*", r.get("Name", ""))
            if m:
                rows[m.group(0)] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3)}
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gmap-sizes", default="5000,50000")
    ap.add_argument("--cloud-sizes", default="1000,5000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cloud-reps", type=int, default=3)
    ap.add_argument("--selection-only", type=int, default=0, help="store size: run only s2m_global_map (kitti settings)")
    ap.add_argument("--kernel-stats", default="", help="rocprofv3 kernel_stats.csv of a --selection-only run")
    a = ap.parse_args(argv)
    from liorf_amd import s2m

    out = {"workload": "keys on a 100 m circle, 0.5 m apart, all within R = 1 000 m; global map: 5 000-point key frames; "
                       "map cloud: 30 000-point key frames", "global_map": {}, "map_cloud": {}}
    small = _clouds(5000)
    gmap_sizes = [a.selection_only] if a.selection_only else [int(s) for s in a.gmap_sizes.split(",") if s]
    for n in gmap_sizes:
        eng = s2m.MapOptimizationS2M()
        _circle_store(eng, n, small)
        row = {}
        for name, (dens, leaf) in SETTINGS.items():
            prm = s2m.default_gmap_params(pose_density=dens, leaf=leaf)
            call, n_out, n_keys = _gmap_call(eng, prm)
            row[name] = {"global_map_ms": _median_ms(call, a.warmup, a.reps), "frames": int(n_keys.value),
                         "points_in": int(n_keys.value) * 5000, "globalMapKeyFramesDS": int(n_out.value)}
            if a.selection_only:
                break
        if not a.selection_only:
            # the selection alone: every key a candidate, one centroid that survives (pose density far above the extent)
            prm = s2m.default_gmap_params(search_radius=1e3, pose_density=1e3, leaf=1.0)
            call, n_out, n_keys = _gmap_call(eng, prm)
            row["selection_ms"] = _median_ms(call, a.warmup, a.reps)
            row["selection_frames"] = int(n_keys.value)
        out["global_map"][str(n)] = row
        eng.close()
    if not a.selection_only:
        big = _clouds(30000)
        for n in [int(s) for s in a.cloud_sizes.split(",") if s]:
            eng = s2m.MapOptimizationS2M()
            poses = _circle_store(eng, n, big)
            total = n * 30000
            host = np.zeros((total, 8), F)
            n_out = C.c_size_t(0)
            row = {"points": total}
            for leaf in (0.0, 0.4):
                def dev():
                    rc = eng.lib.s2m_kf_map_cloud(eng.h, 0, n, leaf, host.ctypes.data, 32, total, C.byref(n_out))
                    assert rc >= 0, eng.lib.s2m_last_error(eng.h)
                ms = _median_ms(dev, 1, a.cloud_reps)
                n_dev = int(n_out.value)

                def composed():
                    cat = np.concatenate([eng.transformPointCloud(big[k % len(big)], poses[k]) for k in range(n)])
                    return eng.voxelGrid(cat, leaf) if leaf > 0 else cat
                t0 = time.perf_counter()
                ref = composed()
                host_ms = round(1e3 * (time.perf_counter() - t0), 1)
                assert ref.shape[0] == n_dev and np.array_equal(ref.view(np.uint32), host[:n_dev].view(np.uint32))
                row["leaf_%g" % leaf] = {"map_cloud_ms": ms, "points_out": n_dev, "host_ms": host_ms}
                del ref
            out["map_cloud"][str(n)] = row
            del host
            eng.close()
    if a.kernel_stats:
        out["kernels_device_us"] = _stats(a.kernel_stats)
    out["note"] = "wall clock, median after warm-up (map_cloud: after one warm-up call; host_ms one run, checked bit for bit)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
