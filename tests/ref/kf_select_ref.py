"""The key-frame selection (include/liorf_s2m.h (b)-(f), kf_select in liorf_amd/csrc/s2m_voxel.hip) restated stage by stage in
numpy, for the tests that read the stages back through s2m_debug_kf_select_last: the radius candidates in ascending (d2, key), the
centroids of the key-pose VoxelGrid summed in that order (oracle.voxel_grid on the records in that order), the nearest key of
every centroid over all keys (equal distances: the lower key), the entries with the distance test (f), the surviving keys and
the frame table's offsets. Its key list is the one of test_keyframes_cpu.select_surrounding / relocalize_ref.select_at
(test_kf_select_cpu.py holds it to both).

Two plausible but wrong selections, used to show that a store tells them apart:
  "ties_descending"   equal d2 go to the higher key first - in the candidate order (so in the centroid sums) and in the
                      nearest-key search;
  "sum_in_key_order"  the centroid sums are taken in ascending key order instead of rank order.

store(): the 8 193 keys the GPU tests fill in, with planted tie clusters (below); radius_for(): a radius with an exact number
of candidates.
"""
import functools

import numpy as np

from oracle import oracle as O

F = np.float32
PATH_NARROW, PATH_PRE, PATH_WIDE = 0, 1, 2
TILE = 4096                 # kKfTile: keys the single-workgroup kernel takes, candidates it sorts
COUNTS = (0, 1, 2, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 8191, 8192, 8193)    # candidate counts the tests hit exactly
SIZES = (1, 2, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 8191, 8192, 8193)        # store sizes the fill stops at


def d2_of(a, b):
    """kf_d2 / test_keyframes_cpu._d2: ((dx*dx + dy*dy) + dz*dz) in fp32, a: (n, 3), b: (3,)."""
    d = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def expected_path(n_keys, n_cand):
    return PATH_NARROW if n_keys <= TILE else (PATH_PRE if n_cand <= TILE else PATH_WIDE)


def _nearest(P, cents, higher_on_ties=False, chunk=256):
    """argmin over all keys of d2(centroid, key), equal distances to the lower key (or the higher)."""
    P = np.asarray(P, F)
    n = P.shape[0]
    src = P[::-1] if higher_on_ties else P
    out = np.zeros(cents.shape[0], np.int32)
    for s in range(0, cents.shape[0], chunk):
        c = cents[s:s + chunk]
        dx = (c[:, None, 0] - src[None, :, 0]).astype(F)
        dy = (c[:, None, 1] - src[None, :, 1]).astype(F)
        dz = (c[:, None, 2] - src[None, :, 2]).astype(F)
        k = np.argmin(((dx * dx + dy * dy) + dz * dz).astype(F), axis=1)          # the first minimum
        out[s:s + chunk] = (n - 1 - k) if higher_on_ties else k
    return out


def stages(P, centre, R, D, n_recent=0, sizes=None, variant=None):
    """Every stage of one selection on the store P (n x 3 fp32) around `centre`: a dict with
      order        radius candidates (d2 < fl(R*R)) in rank order, ascending (d2, key)         (b)
      cent         centroids of the VoxelGrid with leaf D over the candidates, xyz fp32          (c)
      leaf_too_small  the filter passed its input through: cent = the candidate positions in rank order
      nn           nearest key of every centroid                                                  (d)
      entry_keys, entry_keep   centroid keys then the n_recent newest keys (n-1, n-2, ...), and which pass (f)
      keys, offsets, n_points  the frame table: surviving keys in order, the running sum of their frame sizes
      n_cand, n_cent, n_frames
    sizes: points per key frame (None: offsets and n_points are not made)."""
    assert variant in (None, "ties_descending", "sum_in_key_order")
    P = np.asarray(P, F).reshape(-1, 3)
    n = P.shape[0]
    q = np.asarray(centre, F).reshape(3)
    R = F(R)
    d2 = d2_of(P, q)
    cand = np.flatnonzero(d2 < R * R)
    tie = -cand if variant == "ties_descending" else cand
    order = cand[np.lexsort((tie, d2[cand]))]
    cent = np.zeros((0, 3), F)
    too_small = False
    if order.size:
        summed = np.sort(order) if variant == "sum_in_key_order" else order
        rec = np.zeros((order.size, 8), F)
        rec[:, :3] = P[summed]
        rec[:, 3] = 1.0
        c, too_small = O.voxel_grid(rec, float(D))
        cent = np.ascontiguousarray(c[:, :3])
    nn = _nearest(P, cent, higher_on_ties=variant == "ties_descending")
    recent = np.arange(n - 1, n - 1 - int(n_recent), -1, dtype=np.int32)
    assert recent.size == 0 or recent[-1] >= 0
    entry_keys = np.concatenate([nn, recent]).astype(np.int32)
    pts = np.concatenate([cent, P[recent]]).astype(F)
    d = (pts - q).astype(F)
    dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)).astype(F)
    keep = ~(dist > R)                                                             # (f): farther than R is dropped
    keys = entry_keys[keep]
    out = {"order": order.astype(np.int32), "n_cand": int(order.size), "cent": cent, "n_cent": int(cent.shape[0]),
           "leaf_too_small": bool(too_small), "nn": nn, "entry_keys": entry_keys, "entry_keep": keep, "keys": keys,
           "n_frames": int(keys.size), "path": expected_path(n, int(order.size))}
    if sizes is not None:
        sz = np.asarray(sizes, np.int64)[keys]
        out["offsets"] = np.concatenate([[0], np.cumsum(sz)]).astype(np.int32)
        out["n_points"] = int(sz.sum())
    return out


def radius_for(P, centre, m, span=16):
    """A float32 R > 0 with exactly m keys of P at d2 < fl(R*R): a few floats around the square root of the midpoint between
    the m-th and the (m+1)-th smallest d2 are tried. Raises when none of them hits (equal d2 at the cut)."""
    P = np.asarray(P, F).reshape(-1, 3)
    n = P.shape[0]
    d2 = d2_of(P, centre)
    s = np.sort(d2).astype(np.float64)
    if not 0 <= m <= n:
        raise ValueError("no radius takes %d of %d keys" % (m, n))
    lo = s[m - 1] if m > 0 else 0.0
    hi = s[m] if m < n else s[n - 1] * 1.01 + 1.0
    r = F(np.sqrt(0.5 * (lo + hi)))
    tries = [r]
    up = dn = r
    for _ in range(span):
        up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(0))
        tries += [up, dn]
    for x in tries:
        x = F(x)
        if x > 0 and np.isfinite(x) and int((d2 < x * x).sum()) == m:
            return x
    raise RuntimeError("no float32 radius gives exactly %d candidates (d2 %r .. %r at the cut)" % (m, lo, hi))


# ---- the store -------------------------------------------------------------------------------------------------------------
SEED = 20261
N_KEYS = 8193
N_DECK = 400                                              # keys lifted from the 18 m slab to z = 20 .. 32 m
CENTRE = np.array([3.3712, -2.8149, 0.6431], F)           # generic: on no key, on no voxel edge
CLUSTER_A = (700, 1900, 2300, 3100, 3900)                 # four tied keys below 4 096 and the earlier-ranked key of their voxel
CLUSTER_B = (4094, 4095, 4096, 4097, 4300)                # the tied keys straddle index 4 095 / 4 096
NEAREST_PAIR = (5000, 5500)                               # lanes 136 and 124 of k_kf_select_nearest: waves 2 and 1, 500 keys apart
FAR_SHIFT = np.array([-100000.0, 60000.0, 30.0], F)


def _cell(p, leaf):
    inv = F(1.0) / F(leaf)
    return np.floor((np.asarray(p, F) * inv).astype(F)).astype(np.int64)


def _sum_bits(pts):
    """Centroid bits of the points summed one after the other in fp32 (write_centroid: sum / count)."""
    s = np.zeros(3, F)
    for p in pts:
        s = (s + p).astype(F)
    return (s / F(len(pts))).astype(F).tobytes()


def _alone(P, idx, pts, leaf=2.0):
    """No key of P outside idx shares the leaf-2 voxel of pts (all in one voxel)."""
    c = _cell(pts[0], leaf)
    mask = np.ones(P.shape[0], bool)
    mask[list(idx)] = False
    return not np.any(np.all(_cell(P[mask], leaf) == c, axis=1))


def _tie_cluster(rng, P, idx, h_sign):
    """Four keys at C + (0, +-a, +-b) or C + (0, +-b, +-a), C = CENTRE + (h, 0, 0), with bitwise equal d2 from CENTRE (h*h
    dominates and absorbs what the roundings of the small terms differ by), and a fifth key of the same
    voxel (leaf 0.5, so leaf 2.0 too) that ranks before them but has the highest index: rank order is (k4, k0, k1, k2, k3), key
    order (k0, k1, k2, k3, k4), and ties the other way round (k4, k3, k2, k1, k0). Searched until the three give different
    centroid bits and the four's six distinct pairings of (+-a, +-b) to summation places give at least two."""
    import itertools
    q = CENTRE
    for trial in range(20000):
        h = F(h_sign * rng.uniform(8.0, 20.0))
        a, b = rng.uniform(0.03, 0.2, 2).astype(F)
        C = (q + np.array([h, 0, 0], F)).astype(F)
        offs = [(0, sa * u, sb * v) for u, v in ((a, b), (b, a)) for sa in (1, -1) for sb in (1, -1)]
        four = [(C + np.array(offs[j], F)).astype(F) for j in rng.permutation(8)[:4]]
        early = (C + np.array([-h_sign * rng.uniform(0.05, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)], F)).astype(F)
        pts = four + [early]
        d2 = d2_of(np.stack(pts), q)
        if len(set(d2[:4].tobytes()[4 * i:4 * i + 4] for i in range(4))) != 1 or not d2[4] < d2[0]:
            continue
        if not np.all(_cell(np.stack(pts), 0.5) == _cell(pts[0], 0.5)):
            continue
        if not _alone(P, idx, pts):
            continue
        right = _sum_bits([early] + four)
        if right == _sum_bits([early] + four[::-1]) or right == _sum_bits(four + [early]):
            continue
        if len({_sum_bits(list(p)) for p in itertools.permutations(four)}) < 2:
            continue
        return np.stack(pts), trial
    raise RuntimeError("no order-sensitive tie cluster found")


def _nearest_pair(rng, P, idx):
    """Two keys alone in their voxel whose centroid - the exact midpoint: p2 = p1 + an even number of ulps per coordinate - is
    bitwise equidistant from both, and nearer to them than to any other key."""
    q = CENTRE
    for trial in range(4000):
        p1 = (q + rng.uniform(-12, 12, 3) * [1, 1, 0.3]).astype(F)
        step = np.array([2 * int(rng.integers(2000, 20000)) * np.spacing(np.abs(x)) for x in p1], F)
        p2 = (p1 + step).astype(F)
        c = ((p1 + p2).astype(F) / F(2)).astype(F)
        if (c.astype(np.float64) * 2 != p1.astype(np.float64) + p2.astype(np.float64)).any():
            continue
        e = d2_of(np.stack([p1, p2]), c)
        if e[0].tobytes() != e[1].tobytes():
            continue
        if not np.all(_cell(p1, 0.5) == _cell(p2, 0.5)) or not _alone(P, idx, [p1, p2]):
            continue
        mask = np.ones(P.shape[0], bool)
        mask[list(idx)] = False
        if d2_of(P[mask], c).min() <= e[0]:
            continue
        return np.stack([p1, p2]), trial
    raise RuntimeError("no equidistant pair found")


@functools.lru_cache(maxsize=None)
def store(seed=SEED):
    """(P, sizes, info): N_KEYS key positions over about 120 m x 120 m x 18 m (N_DECK of them on a deck above it, so that the
    voxel indices of leaf 0.5 over the whole store reach the third 11-bit digit) with the planted clusters, the points of every key
    frame (1 .. 7 by key, key 77 has none), and the trials each planted piece took. Read-only arrays."""
    rng = np.random.default_rng(seed)
    P = rng.uniform([-60, -60, -9], [60, 60, 9], (N_KEYS, 3)).astype(F)
    deck = rng.choice(N_KEYS, N_DECK, replace=False)      # an upper deck: the box of all keys holds more than 2^22 voxels of leaf 0.5
    P[deck, 2] = rng.uniform(20, 32, N_DECK).astype(F)
    a, ta = _tie_cluster(rng, P, CLUSTER_A, +1.0)
    P[list(CLUSTER_A)] = a
    b, tb = _tie_cluster(rng, P, CLUSTER_B, -1.0)
    P[list(CLUSTER_B)] = b
    pr, tp = _nearest_pair(rng, P, NEAREST_PAIR)
    P[list(NEAREST_PAIR)] = pr
    sizes = (1 + (np.arange(N_KEYS) * 5 + 3) % 7).astype(np.int32)
    sizes[77] = 0
    P.setflags(write=False)
    sizes.setflags(write=False)
    return P, sizes, {"trials": (ta, tb, tp)}


def frame_cloud(key, n_points):
    """Key frame `key`'s records (n_points x 8 fp32: x, y, z, 1, intensity, 0, 0, 0), a function of the key alone."""
    rng = np.random.default_rng(100000 + int(key))
    a = np.zeros((int(n_points), 8), F)
    a[:, :3] = rng.uniform(-4, 4, (int(n_points), 3)).astype(F)
    a[:, 3] = 1.0
    a[:, 4] = rng.uniform(0, 100, int(n_points)).astype(F)
    return a


def key_pose(P, key):
    """Pose {x, y, z, roll, pitch, yaw} of key `key`: its position and a small rotation that varies by key."""
    k = int(key)
    return np.array([P[k, 0], P[k, 1], P[k, 2], 0.01 * ((k * 7) % 11 - 5), 0.01 * ((k * 3) % 13 - 6), 0.1 * ((k * 5) % 63 - 31)], F)


@functools.lru_cache(maxsize=None)
def store_stages(n_keys, R, D, n_recent=0, centre=None, variant=None, far=False):
    """stages() on the first n_keys keys of store() (shifted by FAR_SHIFT when `far`), cached: the tests share every reference.
    centre: None = CENTRE (shifted with the store), or a tuple."""
    P, sizes, _ = store()
    Pn, c = P[:n_keys], (CENTRE if centre is None else np.asarray(centre, F))
    if far:
        Pn = (Pn + FAR_SHIFT).astype(F)
        c = (c + FAR_SHIFT).astype(F) if centre is None else c
    return stages(Pn, c, F(R), D, n_recent=n_recent, sizes=sizes[:n_keys], variant=variant)


def max_voxel_index(P, order, D):
    """The largest voxel index pcl::VoxelGrid gives the candidates P[order] at leaf D (the third 11-bit pass of the radix sort has
    work to do when it exceeds 2^22)."""
    X = np.asarray(P, F)[order]
    inv = F(1.0) / F(D)
    lo = np.floor((X.min(0) * inv).astype(F)).astype(np.int64)
    hi = np.floor((X.max(0) * inv).astype(F)).astype(np.int64)
    div = hi - lo + 1
    ijk = (np.floor((X * inv).astype(F)) - lo.astype(F)).astype(np.int64)
    return int((ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]).max())
