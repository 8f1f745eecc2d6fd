"""CPU reference of the joint marginal of two pose-graph keys (s2m_pg_joint_marginal), on tests/ref/pose_graph_ref.py.
Shared by tests/golden/make_golden_pose_graph_marginals.py and tests/test_pose_graph_marginals_gpu.py."""
import numpy as np

import pose_graph_ref as P

# (graph of pose_graph_cases.build, key_a, key_b)
CASES = (("loops_200", 10, 150), ("loops_200", 0, 199), ("gps_120", 60, 119))
TYPES = ("rr", "rt", "tr", "tt")
_R, _T = slice(0, 3), slice(3, 6)
_SL = {"rr": (_R, _R), "rt": (_R, _T), "tr": (_T, _R), "tt": (_T, _T)}


def case_id(name, a, b):
    return "%s:%d:%d" % (name, a, b)


def _rows(a, b):
    return np.r_[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def jacobian(g, X=None):
    return P.assemble(P.linearize(g, g.X if X is None else X)[0], g.n)[0].toarray()


def joint_dense(g, a, b, X=None):
    """Row-major 12x12 over [a's tangent, b's tangent]: the sub-block of the dense inverse of J^T J."""
    J = jacobian(g, X)
    idx = _rows(a, b)
    return np.linalg.inv(J.T @ J)[np.ix_(idx, idx)]


def joint_svd(g, a, b, X=None):
    """The same block from the SVD of J, which never squares J."""
    _u, s, vt = np.linalg.svd(jacobian(g, X), full_matrices=False)
    V = vt.T[_rows(a, b)]
    return (V / (s * s)) @ V.T


def cross_gaps(got, want):
    """Per 3x3 block type the gap of the two off-diagonal 6x6 blocks, each 3x3 block relative to its own norm in `want`
    (the larger of the two)."""
    out = {}
    for ty in TYPES:
        ra, rb = _SL[ty]
        gaps = []
        for r0, c0 in ((0, 6), (6, 0)):
            gb = got[r0:r0 + 6, c0:c0 + 6][ra, rb]
            wb = want[r0:r0 + 6, c0:c0 + 6][ra, rb]
            gaps.append(float(np.linalg.norm(gb - wb) / np.linalg.norm(wb)))
        out["joint_" + ty] = max(gaps)
    return out


def symmetry_gaps(cov):
    """cov[:6, 6:] against the transpose of cov[6:, :6], per 3x3 block type, relative to the block's norm."""
    up, lo = cov[:6, 6:], cov[6:, :6].T
    return {"joint_" + ty: float(np.linalg.norm(up[_SL[ty]] - lo[_SL[ty]]) / np.linalg.norm(up[_SL[ty]])) for ty in TYPES}
