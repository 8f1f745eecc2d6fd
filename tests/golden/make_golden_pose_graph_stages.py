"""Writes tests/golden/pose_graph_stages_bounds.json: per stage and case the floor and the bound the device is held to,
10 x the floor (the margin of pose_graph_bounds.json), for tests/test_pose_graph_stages_gpu.py.

    python tests/golden/make_golden_pose_graph_stages.py

Every floor is a CPU measurement of an fp64 computation against a high-precision one (tests/ref/pose_graph_stages_ref.py),
relative to the largest magnitude in the compared block, and never below one fp64 ulp of it (2^-52): a zero floor would
demand bit equality of differently ordered sums.  Nothing here runs on the device.

  linearize   pose_graph_ref.py against the 50-digit mpmath reference on the 40-key graph, per array; the chain's keys are
              grouped into cases by the size of their residual rotation (the largest gap over a case's keys), every extra
              factor is a case of its own.  Binv is the reference's closed form blkdiag(Jr(phi), R_E^T) W^-1.  Where a floor is
              far above 1e-16 the arithmetic says why: a residual of 1e-8 left by the subtraction of metre-sized numbers
              (chain_placed, cauchy_satisfied) keeps eight digits; 1 - cos(th) in Jr keeps 2.2e-16 / th of the K term (Binv of
              chain_rot_1.1e-05, _0.0001, _0.003); (1 + cos) / sin in Jr^-1 loses six digits at pi - 1e-6; atan2(s, c) / s
              with s = 4.5e-3 loses two to three just below the near-pi threshold.
  scan        the numpy blocked scan (groups of 32, the device's levels) against the longdouble sequential substitution,
              forward and transposed, on the chains and vectors of the scan tests.
  products    K v and K^T u through the fp64 blocked scans against the dense longdouble K.
  cg          a numpy fp64 run of the device's CG recurrences (the operator through the blocked scans): the drift between the
              recurrence's relative residual sqrt(rr / bb) and the true one || (I + K^T K) y - b || / || b || in longdouble.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ref"))
import pose_graph_stages_ref as S  # noqa: E402


def entry(floor):
    floor = {k: S.clamp(v) for k, v in floor.items()}
    return dict(floor=floor, bound={k: 10 * v for k, v in floor.items()})


def main():
    out = {"linearize": {}, "scan": {}, "products": {}, "cg": {}}
    g, names, _calls = S.graph40()
    want = S.stage_arrays(g, S.mp_factors(g, g.X), S.mp_inverse)
    got = S.stage_arrays(g, S.fp64_factors(g, g.X), None, S.fp64_binv(g))
    for case, gaps in S.linearize_gaps(got, want, names, g.chain_names).items():
        out["linearize"][case] = entry(gaps)
        print("linearize", case, json.dumps(out["linearize"][case]["floor"]))
    for n in S.SCAN_N:
        calls, X = S.chain_case(n)
        Binv, Aof = S.chain_blocks_fp64(S.graph_of(calls, X))
        V = np.concatenate(S.scan_vectors(n)).T
        fl = dict(fwd=S.col_gap(S.blocked_scan_f64(Binv, Aof, V, 0), S.fwd_ld(Binv, Aof, V)),
                  bwd=S.col_gap(S.blocked_scan_f64(Binv, Aof, V, 1), S.bwd_ld(Binv, Aof, V)))
        out["scan"][str(n)] = entry(fl)
        print("scan", n, json.dumps(fl))
    for name in sorted(set(S.PRODUCT_CASES + S.CG_CASES)):
        g, _ = S.case_graph(name)
        Binv, Aof = S.chain_blocks_fp64(g)
        Ji, Jj = S.extra_blocks_fp64(g)
        ex = S.extras_of(g)
        K = S.dense_k_ld(Binv, Aof, Ji, Jj, ex)
        ops = S.Fp64Operators(Binv, Aof, Ji, Jj, ex)
        if name in S.PRODUCT_CASES:
            V, U = S.product_vectors(name, g.n, len(ex))
            fl = dict(K=max(S.col_gap(ops.k(v), (K @ v.astype(S.LD))[:, None]) for v in V),
                      KT=max(S.col_gap(ops.kt(u), (K.T @ u.astype(S.LD))[:, None]) for u in U))
            out["products"][name] = entry(fl)
            print("products", name, json.dumps(fl))
        if name in S.CG_CASES:
            fl = {}
            for label, max_it in (("max_iters_1", 1), ("default", S.default_max_cg(len(ex)))):
                drift = 0.0
                for b in S.cg_rhs(name, g.n):
                    y, rr, bb, iters = S.cg_f64(ops.a, b, S.CG_TOL, max_it)
                    true = S.true_residual(K, y, b)
                    drift = max(drift, abs(true - float(np.sqrt(rr / bb))))
                    print("cg", name, label, "iters", iters, "recurrence", float(np.sqrt(rr / bb)), "true", true)
                fl[label] = drift
            out["cg"][name] = entry(fl)
    with open(os.path.join(HERE, "pose_graph_stages_bounds.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
