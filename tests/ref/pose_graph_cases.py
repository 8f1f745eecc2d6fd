"""The pose-graph test cases, shared by tests/golden/make_golden_pose_graph.py and tests/test_pose_graph_gpu.py."""
import numpy as np

import pose_graph_ref as P

SMALL = ("prior_only_50", "loops_200", "gps_120", "cauchy_outlier_300")
LARGE = ("eight_2000", "eight_10000")
INCREMENTAL = "incremental_80"
Q32 = 2.0 ** -23                    # one unit in the last place of a float in [1, 2)


def build(name):
    if name == "prior_only_50":
        return P.figure_eight(50, 0)
    if name == "loops_200":
        return P.figure_eight(200, 6)
    if name == "gps_120":
        g = P.figure_eight(120, 3)
        tr = P.figure_eight(120, 0, truth_only=True)
        g.add_gps(60, tr[60][1] + np.array([0.05, -0.04, 0.02]), np.array([0.25, 0.25, 1.0]))
        return g
    if name == "cauchy_outlier_300":
        g = P.figure_eight(300, 5, loop_var=0.5, loop_k=1.0)
        i, j, rel, var, k = g.loops[2]
        bad = rel.copy()
        bad[:3] += np.array([6.0, -4.0, 1.0], np.float32)          # an outlier measurement, Cauchy
        g.add_between(i - 3, j + 2, bad, np.full(6, 0.5), 1.0)
        return g
    if name == "eight_2000":
        return P.figure_eight(2000, 40)
    if name == "eight_10000":
        return P.figure_eight(10000, 40)
    raise KeyError(name)


def marginal_keys(n):
    """The keys whose marginals the small graphs are held on: the last (the one a node reads), the middle, and key 32."""
    return [n - 1, n // 2, 32]


def quanta(poses):
    """Rounding of a float pose vector: (rotation, translation) sizes of one ulp at the largest magnitude."""
    return Q32 * np.pi, Q32 * float(np.abs(np.asarray(poses)[:, :3]).max())


def to_f32(poses):
    return np.asarray(poses, np.float64).astype(np.float32).astype(np.float64)


def load_into(m, g):
    """The reference graph `g` into the device graph of mapper `m` through the C ABI."""
    m.pgReset()
    for c in P.export(g):
        if c[0] == "prior":
            m.pgAddPrior(c[1], c[2], c[3])
        elif c[0] == "between":
            m.pgAddBetween(c[1], c[2], c[3], c[4], c[5])
        else:
            m.pgAddGps(c[1], c[2], c[3])
    for k, p in enumerate(g.poses().astype(np.float32)):
        m.pgSetInitial(k, p)


def incremental_inputs(n=80):
    """The incremental case: the front end's poses (the last corrected pose of the dense square-root reference composed with
    a noisy step), and the loop from the last key back to the matching key of the first lap."""
    rng = np.random.default_rng(P.SEED + 1)
    truth = P.figure_eight(n, 0, truth_only=True)
    odo = [P.xyzrpy_from_pose(*truth[0]).astype(np.float32)]
    ref = P.Graph()
    for k in range(n):
        if k > 0:
            Ra, ta = truth[k - 1]
            Rb, tb = truth[k]
            Rz, tz = Ra.T @ Rb @ P.so3_exp(rng.normal(0, 2e-3, 3)), Ra.T @ (tb - ta) + rng.normal(0, 0.01, 3)
            Rl, tl = ref.X[-1]
            odo.append(P.xyzrpy_from_pose(Rl @ Rz, tl + Rl @ tz).astype(np.float32))
        ref.add_odometry(odo[k])
        P.optimize(ref, "dense_sqrt")
    i, j = n - 1, n - 1 - n // 2
    rel = P.xyzrpy_from_pose(truth[i][0].T @ truth[j][0], truth[i][0].T @ (truth[j][1] - truth[i][1])).astype(np.float32)
    return odo, (i, j, rel, np.full(6, 0.3))


def incremental_replay(odo, loop, solver):
    """Keys one by one with an optimise after each, then the loop and two optimises (the reference repeats its update after a
    closure).  Returns the graph, the latest pose after every key and the last result."""
    g = P.Graph()
    latest = []
    for p in odo:
        g.add_odometry(p)
        P.optimize(g, solver)
        latest.append(g.poses()[-1])
    g.add_between(loop[0], loop[1], loop[2], loop[3])
    P.optimize(g, solver)
    res = P.optimize(g, solver)
    return g, np.array(latest), res
