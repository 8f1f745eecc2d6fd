"""CPU reference of the joint marginal of two pose-graph keys (s2m_pg_joint_marginal), on tests/ref/pose_graph_ref.py.
Shared by tests/golden/make_golden_pose_graph_marginals.py and tests/test_pose_graph_marginals_gpu.py."""
import numpy as np

import pose_graph_cov_ref as V
import pose_graph_ref as P

# (graph of pose_graph_cases.build, key_a, key_b)
CASES = (("loops_200", 10, 150), ("loops_200", 0, 199), ("gps_120", 60, 119))
TYPES = ("rr", "rt", "tr", "tt")


def case_id(name, a, b):
    return "%s:%d:%d" % (name, a, b)


def _rows(a, b):
    return np.r_[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def jacobian(g, X=None):
    return P.assemble(P.linearize(g, g.X if X is None else X)[0], g.n)[0].toarray()


def joint_dense(g, a, b, X=None):
    """Row-major 12x12 over [a's tangent, b's tangent]: the sub-block of the dense inverse of J^T J.  J^T J has a condition
    number of 1e16 (the prior's translation weight), so this is good for the rotation-rotation blocks (6e-8) and for a look at
    magnitudes; its translation blocks are off by 0.5 % and its mixed ones by up to 0.5 of their norm.  No test holds the device
    to it: see pose_graph_cov_ref.cov_svd, cov_qr, cov_chain and cov_mp."""
    J = jacobian(g, X)
    idx = _rows(a, b)
    return np.linalg.inv(J.T @ J)[np.ix_(idx, idx)]


def joint_svd(g, a, b, X=None):
    """The same block from the SVD of J, which never squares J (pose_graph_cov_ref.cov_svd): the joint marginal's reference."""
    return V.cov_svd(g, [a, b], X)


def _cross(gaps):
    """Of a pose_graph_cov_ref.block_gaps result over two keys the off-diagonal 6x6 blocks only, worst per 3x3 block type,
    scale-held blocks apart: {"joint_rr": .., "joint_rt_held": ..}."""
    return {"joint_" + k: v for k, v in V.worst({key: g for key, g in gaps.items() if key[0] != key[1]}).items()}


def cross_gaps(got, want):
    """Per 3x3 block type the gap of the two off-diagonal 6x6 blocks, each 3x3 block relative to its own norm in `want` (the
    larger of the two); a block that is zero to rounding relative to its scale, under the name joint_<type>_held."""
    return _cross(V.block_gaps(got, want))


def symmetry_gaps(cov, want):
    """cov[:6, 6:] against the transpose of cov[6:, :6], per 3x3 block type, on cross_gaps' yardstick: the norms of `want`."""
    return _cross(V.symmetry_gaps(cov, want))
