"""Front-end measurement: imageProjection's point filter and IMU deskew on the device against the host loop it replaces.

    python tools/bench_front_end.py [--reps 30] [--warmup 5] [--out profiles/front_end_bench_line.json]
    # device time per kernel: one traced run per row, then merged into the same file
    rocprofv3 --kernel-trace --stats --output-format csv -d out/<config>_pfn<k> -- \\
        python tools/bench_front_end.py --profile-run --config <config> --pfn <k>
    python tools/bench_front_end.py --merge-kernel-stats out [--out profiles/front_end_bench_line.json]

For Velodyne-64 x 2048 (131 072 records of 32 bytes), Ouster-128 x 1024 (131 072 x 48 bytes) and Ouster-128 x 2048
(262 144 x 48 bytes), at point_filter_num 1 and 3, medians over --reps runs after --warmup:
  project_scan_host_ms / project_scan_device_ms   s2m_project_scan from host bytes / from device bytes (cap = 0)
  cpu_project_ms    the C restatement of projectPointCloud() (tests/ref/project_ref.c), one thread, gcc -O3, same machine: the
                    figure the stage replaces - the C loop alone, its output and arguments made before the clock starts. It
                    leaves out pcl::moveFromROSMsg and the per-sensor conversion loop, so it flatters the host.
  chain_new_ms      raw bytes -> installed scan_ds: s2m_project_scan + s2m_downsample_projected
  chain_old_ms      the parent route: C restatement on the host + s2m_downsample_scan of the host cloud
  kernel_us         (after --merge-kernel-stats) mean device time of k_proj_flag / k_proj_prefix / k_proj_scatter over the
                    traced calls (half from host bytes, half from device bytes: the kernels are the same), and the calls
The two chains are run interleaved (A B A B ...), so drift of the machine hits both alike.

With --motion every row is measured with positional deskew on (s2m_project_scan_motion, the MOTION instantiations of
k_proj_prefix / k_proj_scatter, odometry increments of a 30 m/s vehicle) and carries "motion": true; the host figure is then
the C restatement with findPosition()'s commented lines live (tests/ref/front_end_odom_ref.c) and the default output file is
profiles/front_end_odom_bench_line.json. Traced runs of such rows go to <stats_dir>/<config>_pfn<k>_motion. The rows'
`project_scan_plain_device_ms` is s2m_project_scan on the same input in the same process, interleaved with the motion call."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
from liorf_amd import s2m, synth  # noqa: E402
import project_ref as PR  # noqa: E402
import front_end_odom_ref as FR  # noqa: E402

CONFIGS = [("velodyne64x2048", "velodyne", 64, 2048), ("ouster128x1024", "ouster", 128, 1024), ("ouster128x2048", "ouster", 128, 2048)]
SENSOR = {"velodyne": s2m.S2M_SENSOR_VELODYNE, "ouster": s2m.S2M_SENSOR_OUSTER}
KERNELS = ("k_proj_flag", "k_proj_prefix", "k_proj_scatter")
DEFAULT_OUT = os.path.join(ROOT, "profiles", "front_end_bench_line.json")
DEFAULT_OUT_MOTION = os.path.join(ROOT, "profiles", "front_end_odom_bench_line.json")
ODOM_INCRE = (2.9, -0.35, 0.06)          # a 0.1 s sweep at about 30 m/s


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return float(np.median(t))


def merge_kernel_stats(stats_dir, out):
    """rocprofv3's kernel_stats.csv of every <stats_dir>/<config>_pfn<k> run into the rows of `out`."""
    rec = json.load(open(out))
    for row in rec["rows"]:
        d = os.path.join(stats_dir, "%s_pfn%d%s" % (row["config"], row["point_filter_num"], "_motion" if row.get("motion") else ""))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit("expected one kernel_stats.csv under %s, found %d" % (d, len(files)))
        ks = {}
        for line in csv.DictReader(open(files[0])):
            name = line["Name"]
            for k in KERNELS:
                if k in name:
                    ks[k] = dict(mean_us=float(line["AverageNs"]) / 1e3, min_us=float(line["MinNs"]) / 1e3,
                                 max_us=float(line["MaxNs"]) / 1e3, calls=int(line["Calls"]))
        if sorted(ks) != sorted(KERNELS):
            raise SystemExit("kernels missing from %s: %s" % (files[0], sorted(ks)))
        row["kernel_us"] = ks
    json.dump(rec, open(out, "w"), indent=1)
    print("merged kernel stats into", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--motion", action="store_true", help="positional deskew on: s2m_project_scan_motion and the MOTION kernels")
    ap.add_argument("--profile-run", action="store_true", help="only run the projections (under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--config", default=None, help="one of the configs (default: all)")
    ap.add_argument("--pfn", type=int, default=None, help="one point_filter_num (default: 1 and 3)")
    ap.add_argument("--merge-kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.out is None:
        args.out = DEFAULT_OUT_MOTION if args.motion else DEFAULT_OUT
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    import torch
    scene = synth.make_scene(half=70.0, n_boxes=92)
    g = s2m.MapOptimizationS2M()
    rows = []
    for name, sensor, rings, n_az in CONFIGS:
        if args.config not in (None, name):
            continue
        scan = synth.make_raw_scan(scene, synth.POSE_GT, sensor, n_rings=rings, n_az=n_az,
                                   angular_velocity=lambda t: np.array([0.05, -0.03, 0.6]), imu_rate=500.0, stamp=100.0, keep_misses=True)
        rc, T, RX, RY, RZ, cur, avail = s2m.imu_deskew_info(scan["imu"], scan["time_scan_cur"], scan["time_scan_end"])
        assert rc == 0 and avail
        d_raw = torch.from_numpy(scan["raw"]).cuda()
        for pfn in (1, 3):
            if args.pfn not in (None, pfn):
                continue
            proj = s2m.ImageProjectionS2M(g, SENSOR[sensor], n_scan=rings, point_filter_num=pfn)
            proj.cachePointCloud(scan["raw"], scan["time_scan_cur"])
            proj.imuDeskewInfo(scan["imu"])
            case = dict(raw=scan["raw"], layout=PR.LAYOUTS[sensor], params=PR.default_params(n_scan=rings, point_filter_num=pfn),
                        deskew=dict(deskew=True, time_scan_cur=scan["time_scan_cur"], imu_pointer_cur=cur, tables=[T, RX, RY, RZ]))
            if args.motion:                      # what odomDeskewInfo() would have left: available, flag on, the increments
                proj.positionalDeskew, proj.odomAvailable, proj.odomDeskewFlag = True, True, True
                proj.odomIncre = np.array(ODOM_INCRE, np.float32)
                case["motion"] = dict(enabled=1, time_scan_end=proj.timeScanEnd, odom_incre=ODOM_INCRE)
                c_out = FR.c_project_motion(case, "-O3")
                m = c_out.shape[0]

                def c_call(_case=case):
                    return FR.c_project_motion(_case, "-O3").shape[0]
            else:
                c_call, c_out = PR.c_project_prepared(case, "-O3")
                m = c_call()
            got = proj.projectPointCloud()
            assert PR.same_cloud(got, c_out[:m]), "the device result is not the C restatement's"
            if args.profile_run:
                for _ in range(args.reps):
                    proj.projectPointCloud(readback=False)
                    proj.projectPointCloud(readback=False, device_ptr=(d_raw.data_ptr(), scan["n"]))
                continue
            row = dict(config=name, records=int(scan["n"]), stride=int(scan["layout"][0]), point_filter_num=pfn, survivors=int(m))
            if args.motion:
                row["motion"] = True
                dev = (d_raw.data_ptr(), scan["n"])
                tp, tm = [], []
                for k in range(args.warmup + args.reps):
                    a = time.perf_counter(); proj.projectPointCloud(readback=False, device_ptr=dev, positional=False)
                    b = time.perf_counter(); proj.projectPointCloud(readback=False, device_ptr=dev, positional=True)
                    c = time.perf_counter()
                    if k >= args.warmup:
                        tp.append((b - a) * 1e3); tm.append((c - b) * 1e3)
                row["project_scan_plain_device_ms"] = float(np.median(tp))
                row["project_scan_motion_device_ms_interleaved"] = float(np.median(tm))
            row["project_scan_host_ms"] = median_ms(lambda: proj.projectPointCloud(readback=False), args.reps, args.warmup)
            row["project_scan_device_ms"] = median_ms(lambda: proj.projectPointCloud(readback=False, device_ptr=(d_raw.data_ptr(), scan["n"])),
                                                      args.reps, args.warmup)
            row["cpu_project_ms"] = median_ms(c_call, args.reps, args.warmup)

            def new():
                proj.projectPointCloud(readback=False)
                g.downsampleCurrentScanProjected(0.4, readback=False)

            def old():
                g.downsampleCurrentScan(c_out[:c_call()], 0.4, readback=False)
            for _ in range(args.warmup):
                new(); old()
            tn, to = [], []
            for _ in range(args.reps):
                a = time.perf_counter(); new(); b = time.perf_counter(); old(); c = time.perf_counter()
                tn.append((b - a) * 1e3); to.append((c - b) * 1e3)
            row["chain_new_ms"], row["chain_old_ms"] = float(np.median(tn)), float(np.median(to))
            row["chain_new_p10_p90_ms"] = [float(np.percentile(tn, 10)), float(np.percentile(tn, 90))]
            row["chain_old_p10_p90_ms"] = [float(np.percentile(to, 10)), float(np.percentile(to, 90))]
            rows.append(row)
            print(json.dumps(row), flush=True)
    g.close()
    if not args.profile_run:
        rec = dict(tool="tools/bench_front_end.py" + (" --motion" if args.motion else ""), reps=args.reps, warmup=args.warmup, rows=rows,
                   note="cpu_project_ms leaves out pcl::moveFromROSMsg and the conversion loop (it flatters the host)" +
                        ("; with --motion it includes the Python call and the output allocation of the checker" if args.motion else ""))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
