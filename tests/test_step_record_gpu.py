"""The record of a single-scan loop (liorf_amd/csrc/s2m_abi.hip, s2m_kernels.hpp).

  * In a captured loop the k_finalize that ends a range of launches writes DevState and the trace into the pinned mirror the host
    reads; with plain launches (S2M_NO_GRAPH=1) a copy behind the loop brings them back.  Both forms must return the same bits:
    pose, affine, counters and every trace record - for a loop in one range, in two, of one to three launches, for a scan that
    stalls at iteration 0 and for the scan behind it on the same handle.
  * A skipped call (no map, too few features) launches nothing and returns its input pose: nothing of the record an earlier
    scan left in the mirror may show up in it.
"""
import numpy as np
import pytest

from liorf_amd import s2m, synth

pytestmark = pytest.mark.gpu


def _record(g, r):
    """Everything a caller can read of one optimisation, as comparable bits."""
    return dict(pose=np.array(r.pose, np.float32).tobytes(), affine=np.array(r.affine, np.float32).tobytes(),
                iters_run=r.iters_run, converged=r.converged, is_degenerate=r.is_degenerate, n_sel_last=r.n_sel_last,
                skipped=r.skipped, trace=[bytes(t) for t in g.trace()])


def _same(a, b, what):
    for k in a:
        assert a[k] == b[k], (what, k)


@pytest.fixture(scope="module")
def clouds(cfg_small):
    m, s = synth.to_xyzi(cfg_small["map"]), synth.to_xyzi(cfg_small["scan"])
    # beyond the gate of every map point: no correspondence at all, the loop stalls at iteration 0
    far = np.zeros((300, 4), np.float32)
    far[:, :3] = cfg_small["map"].max(0) + 50.0 + np.random.default_rng(3).uniform(0, 5, (300, 3))
    return m, s, far


def _run(monkeypatch, env, m, scans, pose, **prm):
    """One handle, the scans one after the other: the record of each."""
    for k in ("S2M_NO_GRAPH", "S2M_SEGMENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = s2m.MapOptimizationS2M(**prm)
    g.setInputCloud(m)
    out = []
    for s in scans:
        out.append(_record(g, g.optimize(s, pose)))
    g.close()
    return out


CASES = {
    "early_exit_off": (dict(), dict(early_exit=0)),
    "early_exit_first_range": (dict(), dict(early_exit=1)),
    "early_exit_second_range": (dict(S2M_SEGMENT="2"), dict(early_exit=1)),
    "max_iter_1": (dict(), dict(early_exit=0, max_iter=1)),
    "max_iter_2": (dict(), dict(early_exit=0, max_iter=2)),
    "max_iter_3": (dict(), dict(early_exit=0, max_iter=3)),
    "max_iter_1_early_exit": (dict(), dict(early_exit=1, max_iter=1)),
    "max_iter_3_early_exit": (dict(S2M_SEGMENT="2"), dict(early_exit=1, max_iter=3)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_graph_form_equals_plain_launch_form(case, clouds, cfg_small, monkeypatch):
    env, prm = CASES[case]
    m, s, _ = clouds
    plain = _run(monkeypatch, dict(env, S2M_NO_GRAPH="1"), m, [s], cfg_small["pose_init"], **prm)[0]
    graph = _run(monkeypatch, env, m, [s], cfg_small["pose_init"], **prm)[0]
    _same(graph, plain, case)
    assert graph["skipped"] == 0 and len(graph["trace"]) == graph["iters_run"] > 0
    if case == "early_exit_first_range":
        assert graph["converged"] and graph["iters_run"] <= 8          # inside the first range of 8 launches
    if case == "early_exit_second_range":
        assert graph["converged"] and graph["iters_run"] > 2           # the second range was needed
    if case.startswith("max_iter") and not prm["early_exit"]:
        assert graph["iters_run"] == prm["max_iter"]


@pytest.mark.parametrize("prm", [dict(early_exit=0), dict(early_exit=1), dict(early_exit=0, max_iter=1)], ids=str)
def test_stalled_scan_and_the_scan_behind_it(prm, clouds, cfg_small, monkeypatch):
    m, s, far = clouds
    plain = _run(monkeypatch, dict(S2M_NO_GRAPH="1"), m, [far, s, far], cfg_small["pose_init"], **prm)
    graph = _run(monkeypatch, dict(), m, [far, s, far], cfg_small["pose_init"], **prm)
    for k in range(3):
        _same(graph[k], plain[k], k)
    max_iter = prm.get("max_iter", 30)
    for k in (0, 2):
        # the stall: pose unchanged, the no-op record repeated for every iteration the reference would still run
        assert graph[k]["pose"] == np.asarray(cfg_small["pose_init"], np.float32).tobytes()
        assert graph[k]["iters_run"] == max_iter and graph[k]["n_sel_last"] == 0 and not graph[k]["converged"]
        assert len(set(graph[k]["trace"])) == 1 and len(graph[k]["trace"]) == max_iter
    # no stale record: the scan behind the stalled one gives what a fresh handle gives
    fresh = _run(monkeypatch, dict(), m, [s], cfg_small["pose_init"], **prm)[0]
    _same(graph[1], fresh, "behind a stalled scan")
    assert graph[1]["n_sel_last"] > 0 and graph[1]["pose"] != graph[0]["pose"]


def test_skipped_calls_return_the_input_pose_and_nothing_of_an_earlier_record(clouds, cfg_small):
    m, s, _ = clouds
    g = s2m.MapOptimizationS2M(early_exit=0)
    g.setInputCloud(m)
    first = g.optimize(s, cfg_small["pose_init"])
    assert first.skipped == 0 and first.iters_run == 30 and len(g.trace()) == 30
    timing = g.timing()
    pose_in = np.array([0.01, -0.02, 0.03, 1.0, 2.0, 3.0], np.float32)

    def skipped(r, code):
        assert r.skipped == code
        assert np.array(r.pose, np.float32).tobytes() == pose_in.tobytes()
        assert g.transformTobeMapped.tobytes() == pose_in.tobytes()
        assert (r.iters_run, r.converged, r.n_sel_last) == (0, 0, 0) and g.trace() == []
        assert g.timing()["optimize_ms"] == timing["optimize_ms"]          # no loop was launched and timed

    skipped(g.optimize(s[:30], pose_in), 2)                 # n_q <= min_feats
    g.setInputCloud(np.zeros((0, 4), np.float32))
    skipped(g.optimize(s, pose_in), 1)                      # no map
    g.close()
