"""Writes tests/golden/pose_graph_marginals_bounds.json: per case of tests/ref/pose_graph_marginals_ref.CASES the floor of
the joint marginal's off-diagonal blocks and the bound the device is held to, 10 x the floor.

    python tests/golden/make_golden_pose_graph_marginals.py

As make_golden_pose_graph.py: the graph is optimised by the dense square-root reference; the reference joint covariance is the
12x12 block of V diag(s^-2) V^T from the SVD of J; the floor is the larger gap to it of the QR of J and of the chain route (the
CPU model of the device's solve; tests/ref/pose_graph_cov_ref.py), per 3x3 block type (rr, rt, tr, tt) of the two off-diagonal
6x6 blocks, each 3x3 block relative to its own norm; the factor 10 is the project's margin for differing summation orders.
Where the chain route lies more than 10 times farther from the SVD than the QR does, its gap is its own error and does not count
(pose_graph_cov_ref.floors; recorded under "chain_route_left_out"): gps_120's tt, 2.2e-7 of Woodbury's cancellation at the key
the GPS factor pins, against 2e-11 for the QR and 6e-12 for the device.  None
of the three routes forms J^T J, whose fp64 inverse - the reference before - left rt and tr floors of 0.2 to 1.0, bounds above 1
that a zero block passed, and a tt bound of 6 %.  The diagonal 6x6 blocks need no bound here: the device returns
s2m_pg_marginal's bits there, which tests/test_pose_graph_gpu.py and tests/test_pose_graph_cov_gpu.py hold.

Blocks that are zero to rounding are held relative to their scale, sqrt(|rr| |tt|) of the two keys' own blocks, under
"held_floor" / "held_bound": in loops_200 (0, 199) key 199's rotation against key 0's translation (the prior leaves it free and
no rotation moves it), in gps_120 (60, 119) key 119's rotation against key 60's translation (the GPS factor pins it).
The bounds are not tightened by hand.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_cov_ref as V  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as P  # noqa: E402


def main():
    out, graphs = {}, {}
    for name, a, b in M.CASES:
        if name not in graphs:
            graphs[name] = CS.build(name)
            P.optimize(graphs[name], "dense_sqrt")
        g = graphs[name]
        want = M.joint_svd(g, a, b)
        both, left_out = V.floors({r: M.cross_gaps(f(g, [a, b]), want) for r, f in (("qr", V.cov_qr), ("chain", V.cov_chain))})
        floor = {k: v for k, v in both.items() if not k.endswith("_held")}
        held = {k: v for k, v in both.items() if k.endswith("_held")}
        out[M.case_id(name, a, b)] = dict(keys=[a, b], floor=floor, bound={k: V.MARGIN * v for k, v in floor.items()},
                                          held_floor=held, held_bound={k: V.MARGIN * v for k, v in held.items()},
                                          chain_route_left_out=left_out)
        print(M.case_id(name, a, b), json.dumps(both), "chain route left out:", json.dumps(left_out))
    with open(os.path.join(HERE, "pose_graph_marginals_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
