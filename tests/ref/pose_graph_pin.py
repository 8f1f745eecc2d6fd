"""Digests of what the pose graph computes, to hold a change of its kernels to the bits of the commit before it.

digests(mapper) runs, per graph, the optimise, the estimates in fp64, the marginals, every operator of the linearisation and
the CG in the single and the block form, and the launched optimise on a twin handle, and returns the sha256 of each result's
bytes.  tests/test_pose_graph_pinned_gpu.py compares them with tests/golden/pose_graph_pinned.json, which was written by

  python tests/ref/pose_graph_pin.py --write tests/golden/pose_graph_pinned.json

on an MI355X with the build of the commit named in the file (the commit and the compiler version are there for the record;
only the digests are compared).  Write it again only with a build whose results are meant to become the new anchor.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_cases as CS  # noqa: E402
import pose_graph_ref as P  # noqa: E402

GRAPHS = {
    "prior_only_50": lambda: CS.build("prior_only_50"),          # no off-chain factor
    "eight_33_1": lambda: P.figure_eight(33, 1),                 # crosses a scan group edge
    "loops_200": lambda: CS.build("loops_200"),
    "gps_120": lambda: CS.build("gps_120"),
    "cauchy_outlier_300": lambda: CS.build("cauchy_outlier_300"),
    "eight_1025_3": lambda: P.figure_eight(1025, 3),             # three scan levels
}
APPLY_COLS, CG_COLS = 13, 7


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def _raw(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _cg(y, outs):
    return _sha(y, np.array([(o.rr, o.bb) for o in outs], np.float64), np.array([(o.iters, o.stop) for o in outs], np.int32))


def graph_digests(m, twin, name):
    """{what: sha256} of graph `name` on mapper `m`, the launched optimise on the second handle `twin`."""
    from liorf_amd import s2m
    g, seed = GRAPHS[name](), P.SEED + 100 + list(GRAPHS).index(name)
    out = {}
    CS.load_into(m, g)
    n, nf = m.pgSize()
    extra = nf - n
    zeros = np.zeros((n, 6))
    out["optimize_result"] = _sha(_raw(m.pgOptimize()))
    out["estimates"] = _sha(m.pgRetract(zeros))
    out["marginal_last"] = _sha(m.pgMarginal(n - 1))
    out["marginals"] = _sha(m.pgMarginals([0, 31, 32, 33 % n, n - 1]))
    out["joint_marginal"] = _sha(m.pgJointMarginal(0, n - 1))
    rng = np.random.default_rng(seed)
    ops = [s2m.S2M_DEBUG_PG_FWD, s2m.S2M_DEBUG_PG_BWD] + ([s2m.S2M_DEBUG_PG_K, s2m.S2M_DEBUG_PG_KT] if extra > 0 else [])
    for op in ops:
        v = rng.standard_normal((APPLY_COLS, 6 * (extra if op == s2m.S2M_DEBUG_PG_KT else n)))
        out["apply_%d_single" % op] = _sha(m.pgApply(op, v[0]))
        out["apply_%d_block" % op] = _sha(m.pgApply(op, v, block=True))
    b = rng.standard_normal((CG_COLS, 6 * n))
    out["cg_single"] = _cg(*m.pgCg(b[0]))
    out["cg_block"] = _cg(*m.pgCg(b, block=True))
    CS.load_into(twin, g)
    code, _ = twin.pgOptimizeLaunch()
    assert code == s2m.S2M_PG_PENDING, code
    code, res = twin.pgOptimizeCollect()
    assert code == s2m.S2M_OK, code
    out["launched_result"] = _sha(_raw(res))
    out["launched_estimates"] = _sha(twin.pgRetract(zeros))
    return out


def digests(m, twin=None):
    """{graph: {what: sha256}} on mapper `m` (and a twin handle for the launched optimise; one is made if none is given)."""
    from liorf_amd import s2m
    own = twin is None
    if own:
        twin = s2m.MapOptimizationS2M()
    try:
        return {name: graph_digests(m, twin, name) for name in GRAPHS}
    finally:
        if own:
            twin.close()


def _record(cmd):
    try:
        return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        return ""


def main():
    from liorf_amd import s2m
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit(__doc__)
    m = s2m.MapOptimizationS2M()
    try:
        d = digests(m)
    finally:
        m.close()
    hipcc = [s for s in _record(["hipcc", "--version"]).split("\n") if "HIP version" in s]
    doc = {"written_by": "tests/ref/pose_graph_pin.py --write", "commit": os.environ.get("PG_PIN_COMMIT") or _record(["git", "rev-parse", "HEAD"]),
           "hipcc": hipcc[0] if hipcc else "", "digests": d}
    with open(sys.argv[2], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["digests"], sort_keys=True))


if __name__ == "__main__":
    main()
