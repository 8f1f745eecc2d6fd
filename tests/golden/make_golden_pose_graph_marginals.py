"""Writes tests/golden/pose_graph_marginals_bounds.json: per case of tests/ref/pose_graph_marginals_ref.CASES the floor of
the joint marginal's off-diagonal blocks and the bound the device is held to, 10 x the floor.

    python tests/golden/make_golden_pose_graph_marginals.py

As make_golden_pose_graph.py: the graph is optimised by the dense square-root reference; the reference joint covariance is
the 12x12 sub-block of the dense inverse of J^T J; the floor is its gap to the same block from the SVD of J, per 3x3 block
type (rr, rt, tr, tt) of the two off-diagonal 6x6 blocks, each relative to that block's norm; the factor 10 is the project's
margin for differing summation orders.  The diagonal 6x6 blocks need no bound: the device returns s2m_pg_marginal's bits there.

Which blocks are informative.  J^T J has an eigenvalue of 1e-8 (the prior's translation weight), and its dense inverse
carries the noise of that in the small rotation-translation covariances, as marginal_rt does in pose_graph_bounds.json.
The floors written by this script:
  loops_200 (10, 150): rr 6e-8 and tt 0.6 % - informative; rt 0.23, tr 0.29 - bounds above 1, which say little.
  loops_200 (0, 199):  rr 6e-8 and tt 0.6 % - informative; rt and tr 1.0 - the two references share no digit there
      (key 0 is held by the prior, its rotation hardly correlates with key 199's translation), the bound of 10 says nothing.
  gps_120 (60, 119):   rr 3e-8 and tt 2e-9 - informative; rt 0.18, tr 0.33 - bounds above 1 again.
So every case checks the rotation-rotation and translation-translation cross blocks sharply and the mixed ones loosely.
The bounds are not tightened by hand.
"""
import json
import os
import sys

import numpy as np  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as P  # noqa: E402


def main():
    out, graphs = {}, {}
    for name, a, b in M.CASES:
        if name not in graphs:
            graphs[name] = CS.build(name)
            P.optimize(graphs[name], "dense_sqrt")
        g = graphs[name]
        floor = M.cross_gaps(M.joint_svd(g, a, b), M.joint_dense(g, a, b))
        out[M.case_id(name, a, b)] = dict(keys=[a, b], floor=floor, bound={k: 10 * v for k, v in floor.items()})
        print(M.case_id(name, a, b), json.dumps(floor))
    with open(os.path.join(HERE, "pose_graph_marginals_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
