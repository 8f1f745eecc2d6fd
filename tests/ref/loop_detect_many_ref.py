"""The model of s2m_loop_detect_keys (include/liorf_s2m.h): detectLoopClosureDistance() (reference
src/mapOptmization.cpp:732-765) for m stored keys against a searched set of the store, top_k candidates per key, restated in
numpy - fp32 d2 in the stated order, ranking by (bits of d2, key), windows in Python integers - and the stores and the fixed
case list that the CPU and the GPU tests share.  `variant` names a plausible wrong reading of the contract."""
import numpy as np

F = np.float32
INT32_MAX = 2**31 - 1
VARIANTS = ("radius_le", "time_ge", "by_key_order", "key_time_when_time_cur_given", "self_excluded_by_name", "rel_window_32bit")
DEFAULTS = dict(search_radius=10.0, time_diff_s=30.0, first=0, count=-1, exclude_lo=0, exclude_hi=0, rel_lo=0, rel_hi=0, top_k=1)


def d2_to(P, q):
    """kf_d2 of every stored position against q: ((dx*dx + dy*dy) + dz*dz) in fp32, one rounding per operation."""
    d = (P - q).astype(F)
    return ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)


def _wrap32(v):
    return (int(v) + 2**31) % 2**32 - 2**31


def detect_keys(P, t, keys, time_cur=None, variant=None, **kw):
    """(key_pre rows, d2 rows, n_cand): row i the first top_k candidates of keys[i] in ascending (bits of d2, key) order."""
    assert variant is None or variant in VARIANTS, variant
    p = {**DEFAULTS, **kw}
    assert not set(kw) - set(DEFAULTS), kw
    P = np.asarray(P, F).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1)
    N = P.shape[0]
    r2 = F(p["search_radius"]) * F(p["search_radius"])                 # (float)(R*R), formed in float
    W = float(F(p["time_diff_s"]))
    first, end = int(p["first"]), N if p["count"] < 0 else int(p["first"]) + int(p["count"])
    rows, d2rows, n = [], [], []
    idx = np.arange(N)
    for i, key in enumerate(int(k) for k in keys):
        if N == 0 or first >= end:
            rows.append([]); d2rows.append(np.zeros(0, F)); n.append(0)
            continue
        in_set = (idx >= first) & (idx < end) & ~((idx >= p["exclude_lo"]) & (idx < p["exclude_hi"]))
        if p["rel_lo"] < p["rel_hi"]:
            lo, hi = key + int(p["rel_lo"]), key + int(p["rel_hi"])            # Python integers: no wrap
            if variant == "rel_window_32bit":
                lo, hi = _wrap32(lo), _wrap32(hi)
            in_set &= ~((idx >= lo) & (idx < hi))
        if variant == "self_excluded_by_name":
            in_set &= idx != key
        d2 = d2_to(P, P[key])
        T = t[key] if time_cur is None or variant == "key_time_when_time_cur_given" else float(time_cur[i])
        dt = np.abs(t - T)
        with np.errstate(invalid="ignore"):
            ok = in_set & ((d2 <= r2) if variant == "radius_le" else (d2 < r2)) & ((dt >= W) if variant == "time_ge" else (dt > W))
        c = np.flatnonzero(ok)
        if variant != "by_key_order":
            c = c[np.lexsort((c, d2[c].view(np.uint32)))]
        c = c[:int(p["top_k"])]
        rows.append([int(v) for v in c]); d2rows.append(d2[c].copy()); n.append(len(c))
    return rows, d2rows, np.array(n, np.int32)


# ---- stores: positions on a 0.25 m lattice, times on a 0.5 s grid -----------------------------------------------------

def make_store(N, seed=0):
    """(P (N, 3) fp32, t (N,) fp64).  A random walk on the 0.25 m lattice (steps of up to 2.5 m) that crosses itself, key i at
    0.5 * i s, with planted keys: revisits a few lattice cells off an older key (exact ties in d2), revisits (6, 8, 0) m off
    an older key (d2 == r2 exactly at R = 10), keys right beside the key 60 before them (|dt| == W exactly at W = 30), and a
    cluster of twelve early keys that later keys return to (more than 8 candidates in the radius)."""
    rng = np.random.default_rng([seed, N])
    step = rng.integers(-10, 11, (N, 3)).astype(np.int64)
    step[:, 2] = rng.integers(-1, 2, N)
    L = np.cumsum(step, axis=0)
    L -= L[0]
    for i in range(4, min(16, N)):                                     # the cluster, around the walk's key 4
        L[i] = L[4] + rng.integers(-6, 7, 3) * [1, 1, 0]
    for i in range(62, N):
        kind = rng.integers(0, 10)
        j = int(rng.integers(0, i - 61))                              # an older key, more than W before key i
        if kind == 0:
            L[i] = L[j] + rng.integers(-2, 3, 3)                      # a near revisit: ties
        elif kind == 1:
            L[i] = L[j] + np.array([24, 32, 0]) * rng.choice([-1, 1])  # (6, 8, 0) m: d2 == 100
        elif kind == 2:
            L[i] = L[i - 60] + rng.integers(-3, 4, 3)                 # |dt| == 30 s exactly
        elif kind == 3:
            L[i] = L[4] + rng.integers(-8, 9, 3) * [1, 1, 0]          # back at the cluster
        elif kind == 4:
            L[i] = L[i - 1] + np.array([400, 0, 0])                   # far from everything before: an empty row
    return (L * 0.25).astype(F), 0.5 * np.arange(N, dtype=np.float64)


def time_cur_for(t, keys, seed=0):
    """One external time per query, on the 0.5 s grid around the key's own: the offsets put |t[key] - T| below, at and above W =
    30 (the last admits the key into its own row) and far off."""
    rng = np.random.default_rng([seed, len(keys), 7])
    off = np.array([0.0, 0.5, -12.0, 30.0, 30.5, -31.0, 100.0])
    return np.asarray(t, np.float64)[np.asarray(keys, np.int64)] + off[rng.integers(0, len(off), len(keys))]


def draw_keys(N, m, seed=0):
    """m query keys of a store of N: all of them in order for m == N, else drawn with repeats, in any order."""
    if m == N:
        return np.arange(N, dtype=np.int32)
    return np.random.default_rng([seed, N, m]).integers(0, N, m).astype(np.int32)


def store_sizes(T):
    return [1, T - 1, T, T + 1, 2 * T + 1]


def query_counts(N, B):
    return sorted({1, B - 1, B, B + 1, N})


def window_cases(N):
    """The searched sets of the window tests over a store of N keys: parameter dictionaries."""
    return [dict(first=N // 5, count=N // 2), dict(exclude_lo=N // 4, exclude_hi=N // 2), dict(rel_lo=-29, rel_hi=INT32_MAX),
            dict(rel_lo=-INT32_MAX, rel_hi=30), dict(first=3, count=N - 5, exclude_lo=10, exclude_hi=40, rel_lo=-29, rel_hi=INT32_MAX),
            dict(rel_lo=5, rel_hi=INT32_MAX)]


def fixed_cases(T, B, seed=0):
    """The fixed case list: (name, N, keys, time_cur or None, parameter dictionary) - every store size at the tile's edges, every
    query count at the block's, top_k 1, 3 and 8, without and with time_cur; then the windows on the largest store."""
    out = []
    for N in store_sizes(T):
        _, t = make_store(N, seed)
        for m in query_counts(N, B):
            keys = draw_keys(N, m, seed)
            for top_k in (1, 3, 8):
                out.append((f"N{N}-m{m}-k{top_k}", N, keys, None, dict(top_k=top_k)))
                out.append((f"N{N}-m{m}-k{top_k}-tc", N, keys, time_cur_for(t, keys, seed), dict(top_k=top_k)))
    N = 2 * T + 1
    _, t = make_store(N, seed)
    keys = draw_keys(N, N, seed)
    for w, kw in enumerate(window_cases(N)):
        out.append((f"N{N}-window{w}", N, keys, None, dict(top_k=3, **kw)))
        out.append((f"N{N}-window{w}-tc", N, keys, time_cur_for(t, keys, seed), dict(top_k=3, **kw)))
    return out
