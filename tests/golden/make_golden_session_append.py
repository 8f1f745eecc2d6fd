"""Writes tests/golden/session_append_bounds.json: the floor and the bound (10 x the floor, as make_golden_pose_graph.py takes
its own) for the merged graph of the end-to-end test of tests/test_session_append_gpu.py.

    python tests/golden/make_golden_session_append.py

The graph is that test's, built on the CPU alone: the scripted revisit's odometry chain (session A), the six keys of
session_append_ref.session_b() placed by the anchor the oracle's relocalisation gives, the junction, and one Cauchy between per
key of B to the key of A the place query names for it (relocalize_ref.TRUE_KEY), measured from B's true pose a few millimetres
off - what an accepted alignment returns. The floor is the disagreement of two CPU solves of it, square-root form against normal
equations, poses rounded to float on both sides as the C ABI returns them.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402
import relocalize_ref as R  # noqa: E402
import session_append_ref as AM  # noqa: E402
import session_ref as M  # noqa: E402

from liorf_amd import s2m  # noqa: E402

CROSS_VAR, CROSS_K = [0.05] * 6, 1.0


def merged_graph():
    _, poses_a, _, _, _ = R.revisit()
    _, stored_b, _, true_b, _ = AM.session_b()
    in_map = [np.asarray(R.model(n)["records"][R.model(n)["best"]]["pose"], np.float32) for n in ("Q1", "Q2")]
    anchor, _, _ = AM.anchor_from_pairs([stored_b[k] for k in AM.B_PROBES], in_map, 0.05, 0.005)
    A = M.state_of(anchor)
    g = P.Graph()
    for p in poses_a:
        g.add_odometry(p)
    n0 = g.n
    placed = [AM.readout(AM.compose(A, M.state_of(p))) for p in stored_b]
    rng = np.random.default_rng(1)
    for k, p in enumerate(placed):
        if k == 0:
            Rl, tl = g.X[-1]
            Rn, tn = P.pose_from_xyzrpy(p)
            g.add_between_pose(n0 - 1, n0, Rl.T @ Rn, Rl.T @ (tn - tl), var=[1.0] * 6)      # the junction
            g.X[n0] = (Rn, tn)
        else:
            g.add_odometry(p)
        measured = true_b[k] + np.r_[rng.normal(0, 0.003, 3), rng.normal(0, 2e-4, 3)]
        g.add_between(n0 + k, R.TRUE_KEY, s2m.between_xyzrpy(measured, poses_a[R.TRUE_KEY]), CROSS_VAR, CROSS_K)
    return g


def main():
    ga, gb = merged_graph(), merged_graph()
    ra, rb = P.optimize(ga, "dense_sqrt"), P.optimize(gb, "normal")
    pa, pb = CS.to_f32(ga.poses()), CS.to_f32(gb.poses())
    rel_r, rel_t = P.pose_gap(pa, pb, relative=True)
    abs_r, abs_t = P.pose_gap(pa, pb)
    fabs = abs(ra.error_after - rb.error_after)
    floor = dict(rel_rot=rel_r, rel_trans=rel_t, abs_rot=abs_r, abs_trans=abs_t, error_rel=fabs / ra.error_after, error_abs=fabs)
    out = {"merged_38": dict(iterations=[ra.iterations, rb.iterations], error_after=ra.error_after, floor=floor,
                             bound={k: 10 * v for k, v in floor.items()})}
    print(json.dumps(out["merged_38"]))
    with open(os.path.join(HERE, "session_append_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
