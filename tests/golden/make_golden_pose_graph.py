"""Writes tests/golden/pose_graph_bounds.json: per case the floor (the disagreement of two CPU solves of the same
problem, square-root form against normal equations) and the bound the device is held to, 10 x the floor.

    python tests/golden/make_golden_pose_graph.py

The device's arithmetic is the reference's (fp64, same formulas); its summation orders differ, hence the factor 10.
Poses are compared as the C ABI returns them, rounded to float, on both sides of every comparison, so the floors of the
pose quantities already hold that rounding.  An error passes inside its relative or its absolute bound (a graph that
its measurements fit exactly has an error of rounding size, where only the absolute one means anything).  A marginal
is compared per 3x3 block type (rr, rt, tr, tt), each block relative to its own norm in the reference
(tests/ref/pose_graph_cov_ref.block_gaps), at the last key, the middle key and key 32.  Reference: the SVD of J; floor: the gaps
of the QR of J and of the chain route (the CPU model of the device's own solve) to it, the larger of the two - except where
the chain route lies more than 10 times farther off than the QR, which is then its own error and is left out
(pose_graph_cov_ref.floors; recorded under "chain_route_left_out").  That is gps_120's tt: Woodbury's difference loses 2e-7 at
the key the GPS factor pins, where the SVD and the QR agree to 2e-11 and the device lies within 9e-12.  None of the three forms J^T J, whose
condition number is 1e16 here (the prior's translation weight of 1e-8 beside 1e6); its fp64 inverse, the reference before, is
off by 0.5 % in tt and 10-15 % in rt, and the bounds were that loose.  Now tt is held to 1e-7 and rt to 2e-3.  In gps_120 the
GPS factor pins the middle key's translation, and every rotation's covariance with it is zero to rounding: those blocks are
held relative to their scale (marginal_rt_held, marginal_tr_held).  The key-0 bound comes from the square-root reference alone: 10 x the distance it leaves key 0
from its prior.  The incremental case drives both solvers key by key with the same front-end poses.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_cov_ref as V  # noqa: E402
import pose_graph_ref as P  # noqa: E402


def marginal_floors(g):
    """(floor, excluded) per 3x3 block type (scale-held blocks apart) over the 6x6 blocks of CS.marginal_keys: the gaps of the
    QR and the chain route to the SVD of J - three fp64 routes, none of which forms J^T J - through pose_graph_cov_ref.floors,
    which leaves the chain route out where its gap is its own error."""
    keys = CS.marginal_keys(g.n)
    want = V.cov_svd(g, keys)
    routes = {r: V.tested_gaps(f(g, keys), want, keys, keys, ())[0] for r, f in (("qr", V.cov_qr), ("chain", V.cov_chain))}
    floor, excluded = V.floors(routes)
    return {"marginal_" + k: v for k, v in floor.items()}, {"marginal_" + k: v for k, v in excluded.items()}


def main():
    out = {}
    for name in CS.SMALL + CS.LARGE:
        small = name in CS.SMALL
        ga, gb = CS.build(name), CS.build(name)
        prior = ga.poses()[0].copy()
        ra = P.optimize(ga, "dense_sqrt" if small else "chain_sqrt")
        rb = P.optimize(gb, "normal")
        pa, pb = CS.to_f32(ga.poses()), CS.to_f32(gb.poses())
        rel_r, rel_t = P.pose_gap(pa, pb, relative=True)
        abs_r, abs_t = P.pose_gap(pa, pb)
        k0_r, k0_t = P.pose_gap(ga.poses()[:1], prior[None])
        ferr = abs(ra.error_after - rb.error_after) / ra.error_after
        fabs = abs(ra.error_after - rb.error_after)
        c = dict(iterations=[ra.iterations, rb.iterations], error_after=ra.error_after,
                 floor=dict(rel_rot=rel_r, rel_trans=rel_t, abs_rot=abs_r, abs_trans=abs_t, error_rel=ferr, error_abs=fabs, key0_rot=k0_r, key0_trans=k0_t))
        if small:
            fl, c["chain_route_left_out"] = marginal_floors(ga)
            c["floor"].update(fl)
        c["bound"] = {k: 10 * v for k, v in c["floor"].items()}
        out[name] = c
        print(name, json.dumps(c["floor"]))
    odo, loop = CS.incremental_inputs()
    ga, la, ra = CS.incremental_replay(odo, loop, "dense_sqrt")
    gb, lb, rb = CS.incremental_replay(odo, loop, "normal")
    pa, pb = CS.to_f32(ga.poses()), CS.to_f32(gb.poses())
    rel_r, rel_t = P.pose_gap(pa, pb, relative=True)
    fabs = abs(ra.error_after - rb.error_after)
    fl = dict(rel_rot=rel_r, rel_trans=rel_t, error_rel=fabs / ra.error_after, error_abs=fabs)
    out[CS.INCREMENTAL] = dict(error_after=ra.error_after, floor=fl, bound={k: 10 * v for k, v in fl.items()})
    print(CS.INCREMENTAL, json.dumps(fl))
    with open(os.path.join(HERE, "pose_graph_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
