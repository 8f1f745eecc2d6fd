"""s2m_last_timing of a single scan (liorf_amd/csrc/s2m_abi.hip; the scan preparation it times is s2m_prep.hip's): set_scan_ms and optimize_ms are differences of wall-clock
stamps that the kernels bracketing the two intervals store in pinned memory - no event record costs GPU time in a step.
The intervals are device time inside the step, so each is positive and below the host's wall time of the step; the second
range of an early-exit loop, timed by an event pair of its own, is still part of optimize_ms."""
import math
import time

import numpy as np
import pytest
import torch

from liorf_amd import s2m, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_clouds(cfg_small):
    dev = torch.device("cuda", 0)
    d_map = torch.from_numpy(synth.to_xyzi(cfg_small["map"])).to(dev)
    d_scan = torch.from_numpy(synth.to_xyzi(cfg_small["scan"])).to(dev)
    return d_map, d_scan


def _step(g, d_scan, pose):
    t0 = time.perf_counter()
    g.setScanDevice(d_scan.data_ptr(), d_scan.shape[0], 32)
    g.launch(pose)
    r = g.collect()
    wall_ms = (time.perf_counter() - t0) * 1e3
    return r, wall_ms, g.timing()


def test_timing_before_any_scan_is_zero():
    g = s2m.MapOptimizationS2M()
    assert g.timing() == dict(optimize_ms=0.0, set_map_ms=0.0, set_scan_ms=0.0)
    g.close()


@pytest.mark.parametrize("early_exit", [0, 1])
def test_device_intervals_lie_inside_the_step(early_exit, device_clouds, cfg_small):
    d_map, d_scan = device_clouds
    g = s2m.MapOptimizationS2M(early_exit=early_exit)
    g.setInputCloudDevice(d_map.data_ptr(), d_map.shape[0], 32)
    for rep in range(3):                                   # the first step captures the graph; every step has to hold
        r, wall_ms, t = _step(g, d_scan, cfg_small["pose_init"])
        print("early_exit", early_exit, "rep", rep, "wall_ms %.4f" % wall_ms, t)
        assert r.skipped == 0 and r.iters_run > 0
        for k in ("set_scan_ms", "optimize_ms"):
            assert math.isfinite(t[k]) and 0.0 < t[k] < wall_ms, (rep, k, t[k], wall_ms)
        assert t["set_scan_ms"] + t["optimize_ms"] < wall_ms          # the two intervals do not overlap
    g.close()


def test_second_range_is_part_of_optimize_ms(device_clouds, cfg_small, monkeypatch):
    d_map, d_scan = device_clouds

    def best_of(segment, reps=3):
        monkeypatch.setenv("S2M_SEGMENT", segment)
        g = s2m.MapOptimizationS2M(early_exit=1)
        g.setInputCloudDevice(d_map.data_ptr(), d_map.shape[0], 32)
        ms, iters = [], None
        for _ in range(reps + 1):
            r, _, t = _step(g, d_scan, cfg_small["pose_init"])
            ms.append(t["optimize_ms"])
            iters = r.iters_run
        g.close()
        return min(ms[1:]), iters

    two, iters_two = best_of("2")               # the scan converges behind launch 2: launches 2 .. 29 are issued as a second range
    one, iters_one = best_of("8")               # the range boundary lies beyond its convergence
    print("optimize_ms: two ranges %.4f, one range %.4f, iterations %d" % (two, one, iters_one))
    assert iters_two == iters_one and 2 < iters_one <= 8
    assert two > one
