"""An independent float64 reference of the close of an ICP iteration (liorf_amd/csrc/s2m_icp_close.hpp), and the cases the
close is held to - for tests/test_icp_close_cpu.py, tests/test_icp_close_gpu.py and tests/golden/make_golden_icp_umeyama.py.

* `umeyama_ref`: Eigen::umeyama without scaling from numpy.linalg.svd. Nothing of the header's Jacobi is restated here.
* `umeyama_classes`: cross-covariances by class - random over 12 decades, rank 2, noisy rank 1, equal singular values, near
  reflections, a ratio of 1e7, tiny, huge, and the exact degenerate ones (zero rows, not rounding noise).
* `close_ref`: icp_close_step's decisions restated from the header's contract (PCL 1.10 icp.hpp computeTransformation,
  default_convergence_criteria.hpp hasConverged with max_iterations_similar_transforms_ = 0) on `umeyama_ref`.
* `state_cases`: sums of synthetic correspondences tgt = R(theta) src + t placed on both sides of every threshold.
* the stand-alone host program (tests/ref/icp_close_main.cpp): built by the host compiler, driven through text.
"""
import os
import subprocess
import sys

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DBL_MAX = sys.float_info.max
STATE_WORDS = 38                       # IcpLoopState: T 16 floats, T_step 16 floats, prev_mse (2 words), it, conv, similar, done
EYE16 = np.eye(4, dtype=F).reshape(-1)


# ---- Umeyama ----------------------------------------------------------------------------------------------------------------

def umeyama_ref(mean_src, mean_tgt, sigma):
    """R = U diag(1, 1, sign(det U det V^T)) V^T of sigma = (1/n) sum (tgt - mean_tgt)(src - mean_src)^T, t = mean_tgt - R mean_src,
    in float64. Returns (R, t, s, d): s the singular values (descending), d the sign on the last."""
    A = np.asarray(sigma, np.float64).reshape(3, 3)
    U, s, Vt = np.linalg.svd(A)
    d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    t = np.asarray(mean_tgt, np.float64) - R @ np.asarray(mean_src, np.float64)
    return R, t, s, d


def determined(s, d):
    """The rotation is determined where every pair of (signed) singular values is apart from cancelling: the optimum
    tr(R^T sigma) falls by (s_i + d_j s_j)(1 - cos a) under a rotation by a in the plane (i, j)."""
    sd = (s[0], s[1], d * s[2])
    return min(sd[0] + sd[1], sd[0] + sd[2], sd[1] + sd[2]) >= 1e-3 * s[0]


def _orth(rng, proper=None):
    Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    if proper is not None and (np.linalg.det(Q) > 0) != proper:
        Q[:, 2] = -Q[:, 2]
    return Q


def _usv(rng, s, sign=1.0):
    """U diag(s) V^T with det(U V^T) = sign."""
    U = _orth(rng, True)
    V = _orth(rng, sign > 0)
    return U @ np.diag(s) @ V.T


def umeyama_classes():
    """[(name, mean_src, mean_tgt, sigma 3x3)] in fp32, the same list at every call. A name that starts with `exact_rank0` or
    `exact_rank1` is a cross-covariance with zero rows: what the parent of the completion of U got wrong."""
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, A):
        out.append((name, rng.normal(0, 5, 3).astype(F), rng.normal(0, 5, 3).astype(F), np.asarray(A, np.float64).astype(F)))

    for k in range(200):
        add("random", rng.normal(0, 1, (3, 3)) * 10.0 ** rng.uniform(-6, 6))
    for k in range(100):
        add("rank2", _usv(rng, [rng.uniform(0.5, 2), rng.uniform(0.1, 0.5), 0.0], rng.choice([-1.0, 1.0])))
    for k in range(100):
        add("noisy_rank1", np.outer(rng.normal(0, 1, 3), rng.normal(0, 1, 3)) + rng.normal(0, 1e-9, (3, 3)))
    for k in range(100):
        add("equal_s", _usv(rng, [1.0, 1.0, 1.0]) * 10.0 ** rng.uniform(-2, 2))
    for k in range(100):
        a, b = rng.uniform(0.5, 2), rng.uniform(0.05, 0.4)
        add("two_equal_s", _usv(rng, [a, a, b] if k % 2 else [a, b, b], rng.choice([-1.0, 1.0])))
    for k in range(100):
        s3 = (1e-3, -1e-3, 1e-6, -1e-6)[k % 4]
        add("near_reflection", _usv(rng, [1.0, rng.uniform(0.1, 1.0), abs(s3)], np.sign(s3)))
    for k in range(100):
        add("ratio_1e7", _usv(rng, [1.0, rng.uniform(0.1, 1.0), 1e-7], rng.choice([-1.0, 1.0])))
    for k in range(20):
        add("tiny", rng.normal(0, 1, (3, 3)) * 1e-25)
    for k in range(20):
        add("huge", rng.normal(0, 1, (3, 3)) * 1e18)
    v = rng.normal(0, 1, 3)
    e1, e2 = np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    add("exact_rank0_zero", np.zeros((3, 3)))
    add("exact_rank1_diag200", np.diag([2.0, 0.0, 0.0]))
    add("exact_rank1_e1e2T", np.outer(e1, e2))
    add("exact_rank1_e1vT", np.outer(e1, v))
    add("exact_rank1_ve1T", np.outer(v, e1))
    add("exact_rank1_e3vT_small", np.outer([0, 0, 1e-30], v))
    add("exact_diag110", np.diag([1.0, 1.0, 0.0]))
    add("exact_minus_identity", -np.eye(3))
    add("exact_diag_3_2_-1e-20", np.diag([3.0, 2.0, -1e-20]))
    sub = rng.normal(0, 1, (3, 3)) * 1e-41                      # every entry a subnormal float
    add("exact_subnormal", sub)
    add("exact_rank1_subnormal_one", np.outer([0, 1e-45, 0], [0, 0, 1.0]))   # a single entry, the least subnormal: rank 1
    return out


def is_degenerate(name):
    """exact rank 0 or 1: zero rows in sigma"""
    return name.startswith("exact_rank0") or name.startswith("exact_rank1")


# ---- the stand-alone host program ---------------------------------------------------------------------------------------------

def build_close_exe(directory):
    exe = os.path.join(str(directory), "icp_close_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "liorf_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ref", "icp_close_main.cpp")])
    return exe


def run_umeyama(exe, cases):
    """cases: [(mean_src, mean_tgt, sigma)] fp32 -> T words, uint32 (n, 16)"""
    text = "\n".join(" ".join(float(x).hex() for x in np.concatenate([ms, mt, np.asarray(sg).reshape(-1)])) for ms, mt, sg in cases)
    got = subprocess.run([exe, "umeyama"], input=text + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [line for line in got if line]
    assert len(got) == len(cases)
    return np.array([[int(w, 16) for w in line.split()] for line in got], np.uint32).reshape(len(cases), 16)


def state_words(T=None, T_step=None, prev_mse=DBL_MAX, it=0, conv=0, similar=0, done=0):
    """An IcpLoopState as its 38 32-bit words (little endian, the struct's layout)."""
    w = np.zeros(STATE_WORDS, np.uint32)
    w[0:16] = np.ascontiguousarray(EYE16 if T is None else T, F).reshape(-1).view(np.uint32)
    w[16:32] = np.ascontiguousarray(EYE16 if T_step is None else T_step, F).reshape(-1).view(np.uint32)
    w[32:34] = np.array([prev_mse], np.float64).view(np.uint32)
    w[34:38] = np.array([it, conv, similar, done], np.int32).view(np.uint32)
    return w


def state_fields(w):
    w = np.ascontiguousarray(w, np.uint32)
    it, conv, similar, done = (int(x) for x in w[34:38].view(np.int32))
    return dict(T=w[0:16].view(F).reshape(4, 4), T_step=w[16:32].view(F).reshape(4, 4), prev_mse=float(w[32:34].view(np.float64)[0]),
                it=it, conv=conv, similar=similar, done=done)


def run_close(exe, cases):
    """cases: [(sums 17 float64, state 38 words, max_iter, trans_eps, fit_eps)] -> outgoing states, uint32 (n, 38)"""
    lines = []
    for S, st, max_iter, trans_eps, fit_eps in cases:
        f = state_fields(st)
        lines.append(" ".join([float(x).hex() for x in S] + [float(x).hex() for x in f["T"].reshape(-1)] +
                              [float(x).hex() for x in f["T_step"].reshape(-1)] + [float(f["prev_mse"]).hex()] +
                              [str(f[k]) for k in ("it", "conv", "similar", "done")] + [str(int(max_iter)), float(trans_eps).hex(), float(fit_eps).hex()]))
    got = subprocess.run([exe, "close"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [line for line in got if line]
    assert len(got) == len(cases), (len(got), len(cases))
    return np.array([[int(w, 16) for w in line.split()] for line in got], np.uint32).reshape(len(cases), STATE_WORDS)


# ---- the state machine ----------------------------------------------------------------------------------------------------------

def close_ref(S, st, max_iter, trans_eps, fit_eps):
    """One close in float64 from the header's contract. st: state_fields(). Returns the outgoing fields plus `margin`: how far,
    relative to its threshold, the quantity that decided (or the nearest that could have) lies from it (inf: no threshold was
    consulted), and `ran`: an iteration was closed (T_step and T were written)."""
    S = np.asarray(S, np.float64)
    out = dict(st)
    out["margin"], out["ran"] = np.inf, False
    cnt = S[0]
    if cnt < 3.0:                                              # min_number_correspondences_
        out.update(conv=0, done=1)
        return out
    mse = S[1] / cnt
    # Matrix3f / Vector3f in PCL: the means and the covariance are floats before the SVD sees them
    ms = (S[2:5] / cnt).astype(F).astype(np.float64)
    mt = (S[5:8] / cnt).astype(F).astype(np.float64)
    sg = (S[8:17].reshape(3, 3) / cnt - np.outer(S[5:8] / cnt, S[2:5] / cnt)).astype(F).astype(np.float64)
    R, t, _, _ = umeyama_ref(ms, mt, sg)
    Ts = np.eye(4)
    Ts[:3, :3], Ts[:3, 3] = R, t
    out["T_step"], out["T"] = Ts, Ts @ np.asarray(st["T"], np.float64)
    out["it"], out["ran"] = st["it"] + 1, True
    if out["it"] >= max_iter:                                   # CONVERGENCE_CRITERIA_ITERATIONS
        out.update(conv=1, done=1)
        return out
    rot_thr, trl_thr, mse_abs, mse_rel = 1.0 - trans_eps, trans_eps, 1e-12, fit_eps
    cos_angle = 0.5 * (np.trace(R) - 1.0)
    tsq = float(t @ t)
    margins = [abs(cos_angle - rot_thr) / rot_thr, abs(tsq - trl_thr) / trl_thr]
    if cos_angle >= rot_thr and tsq <= trl_thr:                 # CONVERGENCE_CRITERIA_TRANSFORM
        out.update(conv=1, done=1, margin=min(margins))
        return out
    # not both: the one that failed decides; where both failed either could have turned it only with the other
    failed = [m for m, ok in zip(margins, (cos_angle >= rot_thr, tsq <= trl_thr)) if not ok]
    margin = max(failed)
    prev = st["prev_mse"]
    a = abs(mse - prev)
    m_abs = abs(a / mse_abs - 1.0) if a < 1e200 else np.inf       # (a = DBL_MAX on a first iteration)
    if a < mse_abs:                                             # CONVERGENCE_CRITERIA_ABS_MSE
        out.update(conv=1, done=1, margin=min(margin, m_abs))
        return out
    r = a / prev
    m_rel = abs(r - mse_rel) / mse_rel if mse_rel > 0 else np.inf
    if r < mse_rel:                                             # CONVERGENCE_CRITERIA_REL_MSE
        out.update(conv=1, done=1, margin=min(margin, m_abs, m_rel))
        return out
    out.update(similar=0, prev_mse=mse, margin=min(margin, m_abs, m_rel))
    return out


def rot(axis, theta):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def sums_of(src, tgt, sum_d2):
    """The 17 sums of correspondences src[i] -> tgt[i] (float64), sum d2 given"""
    S = np.zeros(17)
    S[0], S[1] = src.shape[0], sum_d2
    S[2:5], S[5:8] = src.sum(0), tgt.sum(0)
    S[8:17] = (tgt[:, :, None] * src[:, None, :]).sum(0).reshape(-1)
    return S


TRANS_EPS, FIT_EPS = 1e-6, 1e-6        # setTransformationEpsilon / setEuclideanFitnessEpsilon of the call site


def state_cases():
    """[(name, sums, state words, max_iter, trans_eps, fit_eps)]: the same list at every call. The source is centred, so that
    mean_src is rounding noise and t = mean_tgt: a float's rounding of t then moves |t|^2 by 1.2e-7 of itself, below the band."""
    rng = np.random.default_rng(77)
    out = []
    T_in = np.eye(4)
    T_in[:3, :3], T_in[:3, 3] = rot([0.3, -0.5, 0.8], 0.3), [3.0, -2.0, 1.0]
    T_in = T_in.astype(F)

    def pts(n):
        p = rng.normal(0, 2, (n, 3))
        return p - p.mean(0)

    def add(name, theta, t, mse, prev, it=3, max_iter=100, n=24, T=T_in, similar=0, done=0, conv=0):
        src = pts(n)
        tgt = src @ rot(rng.normal(0, 1, 3), theta).T + np.asarray(t, np.float64)
        st = state_words(T=T, T_step=T_in.T, prev_mse=prev, it=it, similar=similar, done=done, conv=conv)   # (T_step: anything, it is overwritten)
        out.append((name, sums_of(src, tgt, mse * n), st, max_iter, TRANS_EPS, FIT_EPS))

    far_t, big = [0.2, -0.1, 0.05], 0.3
    # the rotation threshold: cos(theta) against 1 - 1e-6 with the translation well inside
    for theta in (0.0, 1e-4, 1e-3, np.sqrt(2e-6), 1.6e-3, 2.2e-3, 3e-3, 1e-2, 0.1, 1.0, 3.0):
        add(f"rot_{theta:.3g}", theta, [1e-5, 0, 0], 0.5, 1.0)
    # the translation threshold: |t|^2 against 1e-6 with no rotation
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    for rel in (-0.5, -1e-3, -1e-5, -1e-7, 1e-7, 1e-5, 1e-3, 0.5, 100.0):
        add(f"trl_{rel:+.0e}", 0.0, u * np.sqrt(1e-6 * (1.0 + rel)), 0.5, 1.0)
    # the absolute MSE threshold: |mse - prev| against 1e-12, prev so small that the relative change is far above fit_eps
    for rel in (-0.5, -1e-3, -1e-5, 1e-5, 1e-3, 0.5):
        add(f"abs_{rel:+.0e}", big, far_t, 1e-7 + 1e-12 * (1.0 + rel), 1e-7)
        add(f"abs_down_{rel:+.0e}", big, far_t, 1e-7 - 1e-12 * (1.0 + rel), 1e-7)
    # the relative MSE threshold: |mse - prev| / prev against fit_eps
    for rel in (-0.5, -1e-3, -1e-5, -1e-8, 1e-8, 1e-5, 1e-3, 0.5):
        add(f"rel_{rel:+.0e}", big, far_t, 1.0 - FIT_EPS * (1.0 + rel), 1.0)
        add(f"rel_up_{rel:+.0e}", big, far_t, 3e-4 * (1.0 + FIT_EPS * (1.0 + rel)), 3e-4)
    # nothing fires: the loop goes on, with prev_mse = DBL_MAX of the first iteration and with a real one
    add("first_iteration", big, far_t, 0.4, DBL_MAX, it=0, T=np.eye(4, dtype=F))
    add("first_iteration_guess", big, far_t, 0.4, DBL_MAX, it=0)
    add("first_iteration_still", 0.0, [0, 0, 0], 0.0, DBL_MAX, it=0, T=np.eye(4, dtype=F))    # the transform ends it at once
    add("goes_on", big, far_t, 0.4, 0.7)
    add("goes_on_similar_was_2", big, far_t, 0.4, 0.7, similar=2)
    add("ends_similar_was_2", 0.0, [0, 0, 0], 0.4, 0.7, similar=2)
    # the fewest correspondences: 2 ends the alignment unconverged and leaves T alone, 3 closes an iteration
    add("cnt_2", big, far_t, 0.4, 0.7, n=2)
    add("cnt_3", big, far_t, 0.4, 0.7, n=3)
    add("cnt_3_first", big, far_t, 0.4, DBL_MAX, n=3, it=0)
    out.append(("cnt_0", np.zeros(17), state_words(T=T_in, prev_mse=0.7, it=5), 100, TRANS_EPS, FIT_EPS))
    # the iteration cap: it = max_iter - 1 closes its iteration and ends converged, whatever the thresholds say
    add("cap_last", big, far_t, 0.4, 0.7, it=99)
    add("cap_last_of_1", big, far_t, 0.4, DBL_MAX, it=0, max_iter=1)
    add("cap_before_last", big, far_t, 0.4, 0.7, it=97)
    add("cap_last_still", 0.0, [0, 0, 0], 0.4, 0.4, it=7, max_iter=8)
    return out


def umeyama_close_inputs():
    """[(name, mean_src, mean_tgt, sigma)]: the classes with one of the two means zero (in turn), so that sums exist from which
    the close forms exactly this sigma: sigma = S8 / n - mean_tgt mean_src^T loses nothing where the product is zero."""
    out = []
    for k, (name, ms, mt, sg) in enumerate(umeyama_classes()):
        out.append((name, np.zeros(3, F), mt, sg) if k % 2 == 0 else (name, ms, np.zeros(3, F), sg))
    return out


def umeyama_close_cases():
    """The Umeyama classes as closes: [(name, sums, state words, max_iter, trans_eps, fit_eps)] with four correspondences
    (divisions by 4 are exact), a first iteration from the identity."""
    out = []
    for name, ms, mt, sg in umeyama_close_inputs():
        S = np.zeros(17)
        S[0], S[1] = 4.0, 1.0
        S[2:5], S[5:8] = 4.0 * ms.astype(np.float64), 4.0 * mt.astype(np.float64)
        S[8:17] = 4.0 * sg.astype(np.float64).reshape(-1)
        out.append((name, S, state_words(), 100, TRANS_EPS, FIT_EPS))
    return out


def done_cases():
    """States given as done: the close must hand them back untouched, whatever the sums say."""
    good = state_cases()
    out = []
    for k, (name, S, st, mi, te, fe) in enumerate(good[:6]):
        w = st.copy()
        w[37] = 1
        w[35] = k % 2
        out.append(("done_" + name, S, w, mi, te, fe))
    return out
