"""Writes tests/golden/pose_graph_cov_golden.npz (reference covariance blocks) and tests/golden/pose_graph_cov_bounds.json
(floors and the bounds the device is held to) for tests/test_pose_graph_cov_{cpu,gpu}.py.

    python tests/golden/make_golden_pose_graph_cov.py          (about five minutes: two mpmath factorisations)

Per graph of tests/ref/pose_graph_cov_ref.GRAPHS, optimised by the dense square-root reference:

  <name>/X      the optimised estimates, (n, 12): rotation row-major, translation - every CPU check linearises here
  <name>/keys   the keys the matrix spans (the listed keys and those of the joint pairs)
  <name>/cov    the covariance over those keys, (6 k, 6 k): cov_mp at 60 digits on the small graphs, cov_svd on the suite's
  <name>/col_at, col_hi, col_lo   small graphs: two whole columns of (J^T J)^-1, hi + lo carrying 106 bits, for the fixture check

Floor, per graph and 3x3 block type (rr, rt, tr, tt; scale-held blocks apart, as rt_held / tr_held): the larger of the gaps of
cov_qr and cov_chain to the reference (pose_graph_cov_ref.floors) over every block the device is held on (each listed key's 6x6, each listed pair's
12x12); on the small graphs cov_svd's gap to cov_mp counts as well.  Bound = 10 x floor, the project's margin for differing
summation orders; no bound is edited by hand.  The script refuses to write a relative bound of 1e-2 or more, and a scale-held
block other than key 0's mixed rows and columns: a graph that needs either is replaced, not exempted.  (Which side of key 0:
its translation.  The prior leaves it free by 1e4 m and a rotation of the map about key 0 does not move it, so the covariance
of any key's rotation with key 0's translation is 3e-11 against a scale of 1e3 to 4e4.  Key 0's rotation against another
key's translation is an ordinary block, of norm 0.4 to 25.)

What the floors say.  On the graphs without a GPS factor cov_chain, the product's own route, agrees with mpmath to 2e-15 in rr and
tt and 5e-11 to 4e-10 in rt: the weak prior enters it once, in a substitution.  The SVD and the QR of J lose 1e-8 in tt and 1e-4
to 1e-3 in rt to the singular value of 1.6e-5 beside 2e3, so there the floor is the reference's or its neighbours' own error,
and on the suite's graphs, whose reference is the SVD, it is the SVD's.  Under a GPS factor it is the other way round: J is
well conditioned, SVD and QR agree to 5e-11, and cov_chain's Woodbury step cancels (pose_graph_cov_ref.floors): 3.4e-10 in tt
on gps_120_at_45, which sets that floor, and 2e-7 at the pinned key of gps_120 itself, where floors() leaves it out
(tests/golden/make_golden_pose_graph.py and make_golden_pose_graph_marginals.py; "chain_route_left_out" is empty here).  The
old reference, the fp64 inverse of J^T J, is off by 3e-3 to 6e-3 in tt and 0.2 to 0.55 in rt (recorded under "dense_inverse").
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
import pose_graph_cov_ref as V  # noqa: E402
import pose_graph_ref as P  # noqa: E402

RELATIVE_CAP = 1e-2


def main():
    arrays, out = {}, {}
    for name in V.GRAPHS:
        g = V.build(name)
        P.optimize(g, "dense_sqrt")
        n = g.n
        keys, pairs, allk = V.keys_of(name, n), V.pairs_of(name, n), V.all_keys_of(name, n)
        routes = {"qr": V.cov_qr(g, allk), "chain": V.cov_chain(g, allk)}
        if name in V.SMALL:
            col_at = [allk.index(31) * 6 + 2, allk.index(n - 1) * 6 + 4]       # a rotation column and a translation column
            ref, hi, lo = V.cov_mp(g, allk, full_columns=col_at)
            arrays.update({name + "/col_at": V.rows_of(allk)[col_at], name + "/col_hi": hi, name + "/col_lo": lo})
            routes["svd"] = V.cov_svd(g, allk)
        else:
            ref = V.cov_svd(g, allk)
        arrays.update({name + "/X": V.state_array(g.X), name + "/keys": np.array(allk, np.int32), name + "/cov": ref})
        per_route, held = {}, set()
        for r, S in routes.items():
            per_route[r], h = V.tested_gaps(S, ref, allk, keys, pairs)
            held |= h
        floor, left_out = V.floors(per_route)
        bound = {k: V.MARGIN * v for k, v in floor.items()}
        for k, v in bound.items():
            assert k.endswith("_held") or v < RELATIVE_CAP, (name, k, v)
        for a, b, ty in held:                                # only a rotation against key 0's translation
            assert (ty == "rt" and b == 0) or (ty == "tr" and a == 0), (name, a, b, ty)
        out[name] = dict(n=n, keys=keys, pairs=[list(p) for p in pairs], floor=floor, bound=bound, routes=per_route,
                         held=sorted([a, b, ty] for a, b, ty in held), chain_route_left_out=left_out,
                         dense_inverse=V.tested_gaps(V.cov_dense(g, allk), ref, allk, keys, pairs)[0])
        print(name, json.dumps(out[name], sort_keys=True), flush=True)
    np.savez_compressed(os.path.join(HERE, "pose_graph_cov_golden.npz"), **arrays)
    with open(os.path.join(HERE, "pose_graph_cov_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
