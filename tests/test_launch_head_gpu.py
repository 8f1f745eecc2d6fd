"""The head of a registration launch (liorf_amd/csrc/s2m_register.hpp, s2m_kernels.hpp: load_heads, lm_request_rows): both
hot blocks are read before the `done` branch, and the partial rows of the previous launch and the wave's first table entry
are asked for before anything else is waited for.  The smallest shapes at which that can go wrong, against a box room of
about 2 000 points:

  * scans of 1, 63, 64, 65, 511 and 513 points: waves without a table entry, a partial wave, workgroups beyond the active ones;
  * a scan so far from the map that iteration 0 finds fewer than min_corr correspondences (`done` / `stalled`: every later
    launch returns at its head);
  * a floor-only map (degenerate: the projector matP is read in every close);
  * early exit with a first range of two launches, so that a second range starts from the transform k_finalize left (T_valid);
  * one handle for scans of growing, then shrinking size (the cached graph, regrown buffers).

Per case the result record and the whole iteration trace are bitwise the same for the default loop (captured graph, iterations
closed in the next launch's prologue), for S2M_NO_FUSE=1 (one k_finalize per iteration) and for S2M_NO_GRAPH=1 (plain
launches) - up to 16 active workgroups the rows are summed in the same order by either closing kernel, and no scan here
has more (a 2 000-point scan has, and its trace differs in the last bits between the forms, before this layout as after) - and agree
with the oracle within the bars tests/test_register_edges_gpu.py::_loop_bars sets for the same quantities."""
import numpy as np
import pytest

from liorf_amd import s2m
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = {"fused_graph": {}, "no_fuse": {"S2M_NO_FUSE": "1"}, "no_graph": {"S2M_NO_GRAPH": "1"}}
POSE_GT = np.array([0.004, -0.003, 0.012, 13.0, 13.0, 3.5])
POSE_INIT = (POSE_GT + np.array([0.006, 0.004, -0.009, 0.04, -0.03, 0.02])).astype(F)
ROOM_PRM = dict(eig_thresh=2.0)        # the default of 100 is for scans of thousands of points: 63 points on three walls would count as degenerate


def _walls(rng, n, floor_only=False):
    """n points on the floor z = 2 and the walls x = 10, y = 10 of a room 8 m wide (no lattice: no ties)."""
    a, b = rng.uniform(0.0, 8.0, n), rng.uniform(0.0, 8.0, n)
    which = np.zeros(n, int) if floor_only else rng.integers(0, 3, n)
    z = np.zeros(n)
    p = np.where((which == 0)[:, None], np.stack([a, b, z], 1), np.where((which == 1)[:, None], np.stack([z, a, b], 1), np.stack([a, z, b], 1)))
    return p + np.array([10.0, 10.0, 2.0])


def _rot(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


@pytest.fixture(scope="module")
def room():
    rng = np.random.default_rng(17)
    R = _rot(*POSE_GT[:3])
    scan = ((_walls(rng, 2000) - POSE_GT[3:]) @ R).astype(F)          # the lidar frame: R^T (p - t)
    floor_scan = ((_walls(rng, 600, floor_only=True) - POSE_GT[3:]) @ R).astype(F)
    return dict(map=_walls(rng, 2000).astype(F), floor=_walls(rng, 2000, floor_only=True).astype(F), scan=scan, floor_scan=floor_scan)


def _record(g, r):
    return dict(pose=np.array(r.pose, F).tobytes(), affine=np.array(r.affine, F).tobytes(), iters_run=r.iters_run,
                converged=r.converged, is_degenerate=r.is_degenerate, n_sel_last=r.n_sel_last, skipped=r.skipped,
                trace=[bytes(t) for t in g.trace()], trace_rec=g.trace())


def _gpu(monkeypatch, env, m, scans, pose, **prm):
    for k in ("S2M_NO_GRAPH", "S2M_NO_FUSE", "S2M_SEGMENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = s2m.MapOptimizationS2M(min_feats=0, **prm)
    g.setInputCloud(m)
    out = [_record(g, g.optimize(s, pose)) for s in scans]
    g.close()
    return out


def _oracle(m, scans, pose, **prm):
    orc = O.Oracle(knn_backend=1, num_threads=8, min_feats=0, **prm)
    orc.set_map(m)
    out = []
    for s in scans:
        orc.set_scan(s)
        r = orc.scan2MapOptimization(pose)
        out.append((r.iters_run, r.converged, r.is_degenerate, r.n_sel_last, np.array(r.pose, F), orc.trace()))
    orc.close()
    return out


def _case(monkeypatch, m, scans, pose, env=None, **prm):
    """The scans on one handle per form: the forms bitwise against each other, the default form against the oracle."""
    runs = {f: _gpu(monkeypatch, dict(FORMS[f], **(env or {})), m, scans, pose, **prm) for f in FORMS}
    ref = _oracle(m, scans, pose, **prm)
    for k in range(len(scans)):
        a = runs["fused_graph"][k]
        print("scan", k, "points", len(scans[k]), "iters", a["iters_run"], "converged", a["converged"], "degenerate", a["is_degenerate"],
              "n_sel", [t.n_sel for t in a["trace_rec"]][:3], "oracle iters", ref[k][0], "n_sel", [t.n_sel for t in ref[k][5]][:3])
        for f in ("no_fuse", "no_graph"):
            for key in a:
                if key != "trace_rec":
                    assert a[key] == runs[f][k][key], (f, k, key)
        it, conv, degen, n_last, pose_o, tr_o = ref[k]
        assert a["skipped"] == 0
        assert (a["iters_run"], a["converged"], a["is_degenerate"]) == (it, conv, degen), k
        assert len(a["trace_rec"]) == len(tr_o) == it
        for x, y in zip(a["trace_rec"], tr_o):
            assert abs(x.n_sel - y.n_sel) <= max(3, int(2e-4 * y.n_sel))
            dx, dy = np.array(x.delta), np.array(y.delta)
            assert np.abs(dx[:3] - dy[:3]).max() <= 1e-4
            assert np.abs(dx[3:] - dy[3:]).max() <= 1e-4
        assert np.abs(np.frombuffer(a["pose"], F) - pose_o).max() <= 1e-4
    return runs["fused_graph"]


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 511, 513])
def test_scan_sizes_around_a_wave_and_a_workgroup(monkeypatch, room, n_q):
    # (min_corr = 20: points next to an edge of the room fit no plane, and 63 points shall still run the loop)
    a = _case(monkeypatch, room["map"], [room["scan"][:n_q]], POSE_INIT, early_exit=0, min_corr=20, **ROOM_PRM)[0]
    assert a["iters_run"] == 30
    if n_q >= 63:
        assert a["n_sel_last"] >= 20                        # the loop ran: these are not the stall below


def test_stall_at_iteration_zero(monkeypatch, room):
    far = POSE_INIT + np.array([0, 0, 0, 60.0, 60.0, 0], F)
    a = _case(monkeypatch, room["map"], [room["scan"][:513], room["scan"][:513]], far, early_exit=0, **ROOM_PRM)
    for r in a:
        assert r["n_sel_last"] == 0 and r["iters_run"] == 30 and not r["converged"]
        assert r["pose"] == far.astype(F).tobytes() and len(set(r["trace"])) == 1


def test_floor_only_map_is_degenerate(monkeypatch, room):
    a = _case(monkeypatch, room["floor"], [room["floor_scan"]], POSE_INIT, early_exit=0, **ROOM_PRM)[0]
    assert a["is_degenerate"] == 1 and a["iters_run"] == 30


def test_second_range_starts_from_the_stored_transform(monkeypatch, room):
    a = _case(monkeypatch, room["map"], [room["scan"][:513]], POSE_INIT, env={"S2M_SEGMENT": "2"}, early_exit=1, **ROOM_PRM)[0]
    assert a["converged"] and 2 < a["iters_run"] < 30


def test_one_handle_growing_then_shrinking_scans(monkeypatch, room):
    sizes = [65, 257, 513, 511, 63]                     # (up to 16 active workgroups: beyond that k_finalize, 32 row groups, and the
                                                        # fused close, 16, add the rows up in different orders)
    a = _case(monkeypatch, room["map"], [room["scan"][:n] for n in sizes], POSE_INIT, early_exit=0, min_corr=20, **ROOM_PRM)
    fresh = _gpu(monkeypatch, {}, room["map"], [room["scan"][:63]], POSE_INIT, early_exit=0, min_corr=20, **ROOM_PRM)[0]
    for key in fresh:
        if key != "trace_rec":
            assert a[-1][key] == fresh[key], key           # nothing of the larger scans is left in the buffers or the graph
