"""Inputs of the L2 matcher tests (tests/test_gpu_match.py), their oracle results, and a CPU model of the fp8 shortlist.

The matcher ships three forms that must all return the brute-force result bit for bit (csrc/match.hip.h: the matrix cores only prune,
the canonical re-rank decides):
  fused    match_gemm_kernel<false, true> + match_merge_kernel           the default up to a capacity of 64 column tiles (8192 rows)
  unfused  match_gemm_kernel<false, false> + match_rerank_kernel<4 | 0>  tuning "match_fused" = 0, or a capacity beyond 8192 rows
  fp8      desc_to_fp8_kernel + match_gemm_kernel<true, false> + match_rerank_kernel<4 | 0> with its second pass (spvo_set_match_fp8)
A case is named by a tuple (builder name, parameters...); case(key) builds its two sides once, expected(key, ...) evaluates
oracle/matching.py once per (case, direction, selector) however many forms ask for it.

The fp8 model (fp8_model) restates desc_to_fp8_kernel, the fp8 distance GEMM and the two windows of match_rerank_kernel in float64.
It is a model for CHOOSING inputs -- does pass 1 lose the true neighbour on this input, does the bound E8 hold on it -- not a second
oracle: the GPU is compared with matching.bf_match only.
"""
import functools

import numpy as np

import oracle  # noqa: F401
from oracle import matching

FORMS = ("fused", "unfused", "fp8")
SELECTORS = (("KNN", False), ("NN", False), ("NN", True))
RATIO = 0.8


def _unit(rng, n, d=256):
    a = rng.randn(n, d).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


# ------------------------------------------------------------------ builders: name -> f(*params) -> (a, b)
def _sizes(na, nb):
    rng = np.random.RandomState(na * 7 + nb)
    a = _unit(rng, na)
    b = _unit(rng, nb)
    if nb > 10 and na > 10:                                              # plant true correspondences
        m = min(na, nb) // 2
        b[:m] = a[:m] + 0.03 * rng.randn(m, 256).astype(np.float32)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


def _ties():
    rng = np.random.RandomState(5)
    a = _unit(rng, 200)
    b = np.concatenate([a[:50], a[:50], a[:50], a[:50], a[:50], _unit(rng, 300)])   # 5 exact copies
    rng.shuffle(b[250:])
    return a, b


def _zeros():
    """all-zero descriptors: every distance ties at 0"""
    z = np.zeros((40, 256), np.float32)
    return z, z.copy()


def _unnormalised():
    rng = np.random.RandomState(9)
    a = (rng.randn(300, 256) * 10).astype(np.float32)
    b = (rng.randn(400, 256) * 10).astype(np.float32)
    b[:100] = a[:100] + 0.5 * rng.randn(100, 256).astype(np.float32)
    return a, b


def _near_duplicate_clusters():
    """Clusters of rows that differ by a few ulps (what an untrained network produces): dozens of train rows sit inside the error of
    the distance GEMM."""
    rng = np.random.RandomState(11)
    base = _unit(rng, 40)
    rows = []
    for i in range(40):
        reps = 5 + (i * 7) % 90                                            # cluster sizes 5 .. 94: more than one re-score batch
        pert = (rng.randint(-2, 3, size=(reps, 256)) * 2.0 ** -26).astype(np.float32)
        rows.append(base[i] + pert)
    b = np.concatenate(rows + [_unit(rng, 300)])
    b = b[rng.permutation(len(b))]
    a = np.concatenate([base, base + (rng.randint(-1, 2, size=base.shape) * 2.0 ** -25).astype(np.float32), _unit(rng, 100)])
    return a, b


def _near_duplicate_self():
    b = _near_duplicate_clusters()[1]
    return b, b.copy()


def _big_cluster_2048():
    """2048 x 2048 with every row within 1e-6 of one point: every pair is inside the error window"""
    rng = np.random.RandomState(13)
    c = _unit(rng, 1)
    a = (c + rng.randn(2048, 256) * 3e-8).astype(np.float32)
    b = (c + rng.randn(2048, 256) * 3e-8).astype(np.float32)
    b[100:200] = a[300:400]
    return a, b


def _scaled(scale):
    rng = np.random.RandomState(17)
    a = _unit(rng, 500) * np.float32(scale)
    b = np.concatenate([a[:250] * (1 + rng.randn(250, 1).astype(np.float32) * 1e-7), _unit(rng, 380) * np.float32(scale)])
    return a, b


def _fp8_synthetic_700():
    """planted matches plus one 200-row cluster at 1e-3: widens every window of the fp8 shortlist (from test_fp8_shortlist_matcher)"""
    rng = np.random.RandomState(3)
    a = rng.randn(700, 256).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.concatenate([a[:300] + 0.02 * rng.randn(300, 256).astype(np.float32), np.repeat(a[300:301], 200, 0) + 1e-3 * rng.randn(200, 256).astype(np.float32),
                        rng.randn(150, 256).astype(np.float32)])
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b.astype(np.float32)


BIAS_GROUPS = 96


@functools.lru_cache(maxsize=None)
def _bias_build():
    rng = np.random.RandomState(0)
    G = BIAS_GROUPS
    s = np.where(rng.rand(G, 256) < 0.5, -1.0, 1.0).astype(np.float32)
    a = s * np.float32(1.06 / 16)
    bstar = a.copy()
    bstar[np.arange(G), rng.randint(0, 256, G)] *= np.float32(1 - 1e-3)
    dis = []
    for _ in range(2):
        sc = s.copy()
        for g in range(G):
            sc[g, rng.choice(256, 4, replace=False)] *= -1
        dis.append(sc * np.float32(1.065 / 16))
    b = np.concatenate([bstar] + dis + [_unit(rng, 200)])
    perm = rng.permutation(len(b))                                        # train row i is row perm[i] of the list above
    truth = np.argsort(perm)[:G]
    return a, b[perm], truth


def _fp8_rounding_bias():
    """Pass 1 of the fp8 shortlist cannot find these neighbours.  Query a = s * 1.06 / 16 (s: random signs): every entry rounds DOWN to
    1 / 16 in e4m3.  Its true neighbour b* is a with one entry scaled by 1 - 1e-3 (d2 ~ 4e-9) and rounds down as well, so
    dt8(a, b*) = |a|^2 + |b*|^2 - 2 a8.b8* = 2 * 1.1236 - 2 = 0.247.  Two distractors c = s * 1.065 / 16 with four signs flipped
    (d2 = 0.071) round UP to 1.125 / 16: dt8(a, c) = 0.078.  The statistical window is 2e-2 * 2.25 = 0.045: the threshold (second
    smallest dt8 + window) is 0.123, b*'s lower bound 0.202.  Only the rigorous second pass brings b* back -- and it does so with
    |dt8 - d2| at 0.998 of E8.  Query row g's neighbour is train row bias_truth()[g]."""
    return _bias_build()[:2]


def bias_truth():
    """train row of query row g's planted neighbour in ("fp8_rounding_bias",)"""
    return _bias_build()[2]


def _chunk_edges(na, nb):
    """Sizes around the re-rank's 1024-column switch (<4> | <0>) and its 256-column chunks: planted matches, the LAST train row the
    nearest of the last query row (1281: a last chunk of one column), and on the larger side a cluster of up to 300 rows a few ulps
    from one row of the other side (more candidates than one re-score batch, across a chunk boundary)."""
    rng = np.random.RandomState(na * 7 + nb)
    a = _unit(rng, na)
    b = _unit(rng, nb)
    m = min(na, nb) // 2
    b[:m] = a[:m] + 0.03 * rng.randn(m, 256).astype(np.float32)
    b[:m] /= np.linalg.norm(b[:m], axis=1, keepdims=True)
    big, small = (b, a) if nb >= na else (a, b)
    k = min(300, len(big) - m - 1)
    if k > 0:
        big[m:m + k] = small[0] + (rng.randint(-2, 3, size=(k, 256)) * 2.0 ** -26).astype(np.float32)
    b[nb - 1] = a[na - 1] * np.float32(1 + 2.0 ** -12)
    return a, b


def _unit_1e4():
    return _scaled(1e4)


def _single_30():
    """entries of +-1/16 and one entry of 30 per row: 16 * 30 = 480 is beyond e4m3's largest finite value 448"""
    rng = np.random.RandomState(23)

    def rows(n):
        x = np.where(rng.rand(n, 256) < 0.5, -1.0, 1.0).astype(np.float32) / 16
        x[np.arange(n), rng.randint(0, 256, n)] = 30.0
        return x
    a, b = rows(300), rows(400)
    b[:100] = a[:100]
    for g in range(100):
        b[g, rng.choice(256, 3, replace=False)] *= np.float32(0.5)
    return a, b


def _sift_like():
    """128-d rows as cv::SIFT stores them: integers 0 .. 255 (|randn| normalised to 512, rounded, clipped), 100 planted near-copies"""
    rng = np.random.RandomState(29)

    def rows(n):
        x = np.abs(rng.randn(n, 128))
        x = x / np.linalg.norm(x, axis=1, keepdims=True) * 512
        return np.clip(np.rint(x), 0, 255).astype(np.float32)
    a, b = rows(300), rows(400)
    b[:100] = np.clip(a[:100] + rng.randint(-2, 3, size=(100, 128)), 0, 255).astype(np.float32)
    return a, b


def _capacity(na, nb):
    """one side of 8200 rows (65 column tiles: beyond the fused form): 20 planted copies of rows of the small side and 50 exact duplicates
    among the large side's own rows"""
    rng = np.random.RandomState(na * 7 + nb)
    small, big = _unit(rng, min(na, nb)), _unit(rng, max(na, nb))
    pos = rng.choice(len(big), 120, replace=False)
    big[pos[:20]] = small[rng.choice(len(small), 20, replace=False)]
    big[pos[20:70]] = big[pos[70:120]]
    return (small, big) if na <= nb else (big, small)


BUILDERS = {
    "sizes": _sizes, "ties": _ties, "zeros": _zeros, "unnormalised": _unnormalised, "near_duplicate_clusters": _near_duplicate_clusters,
    "near_duplicate_self": _near_duplicate_self, "big_cluster_2048": _big_cluster_2048, "scaled": _scaled, "fp8_synthetic_700": _fp8_synthetic_700,
    "fp8_rounding_bias": _fp8_rounding_bias, "chunk_edges": _chunk_edges, "unit_1e4": _unit_1e4, "single_30": _single_30, "sift_like": _sift_like,
    "capacity": _capacity,
}

SIZES = [(1000, 1000), (997, 613), (1, 1000), (130, 1), (33, 129), (64, 128), (5, 0)]
SCALES = [1e-3, 1.0, 37.0, 1e4]
CHUNK_EDGES = [(70, 1023), (70, 1024), (70, 1025), (70, 1281), (1025, 70), (3, 2)]
CAPACITY = [(70, 8200), (8200, 70)]
OUT_OF_RANGE = [("unnormalised",), ("unit_1e4",), ("single_30",), ("sift_like",)]
# every case the GPU tests run under the fp8 form
FP8_CASES = ([("sizes", na, nb) for na, nb in SIZES] + [("ties",), ("zeros",), ("unnormalised",), ("near_duplicate_clusters",), ("near_duplicate_self",),
             ("big_cluster_2048",)] + [("scaled", s) for s in SCALES] + [("fp8_synthetic_700",), ("fp8_rounding_bias",)]
             + [("chunk_edges", na, nb) for na, nb in CHUNK_EDGES] + OUT_OF_RANGE[1:])


@functools.lru_cache(maxsize=None)
def case(key):
    """(a, b) of the case `key` = (builder name, parameters...): float32, C-contiguous, read-only (they are shared)."""
    a, b = BUILDERS[key[0]](*key[1:])
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    a.flags.writeable = b.flags.writeable = False
    return a, b


@functools.lru_cache(maxsize=None)
def sq_distances(key, swap=False):
    """oracle/matching.py's canonical squared distances of the case (of (b, a) with swap): the 256-step loop runs once per case.
    (a - b)^2 = (b - a)^2 term by term and the sum runs over k in the same order: the transpose IS sq_distances(b, a)."""
    if swap:
        d2 = np.ascontiguousarray(sq_distances(key).T)
    else:
        a, b = case(key)
        d2 = matching.sq_distances(a, b) if len(a) and len(b) else np.zeros((len(a), len(b)), np.float32)
    d2.flags.writeable = False
    return d2


@functools.lru_cache(maxsize=None)
def expected(key, selector, cross, swap=False):
    """matching.bf_match(a, b, selector, cross, RATIO) of the case ((b, a) with swap) -> (idx, dist), read-only."""
    a, b = case(key)
    if swap:
        a, b = b, a
    idx, d = matching.bf_match(a, b, selector, cross, RATIO, d2=sq_distances(key, swap))
    idx.flags.writeable = d.flags.writeable = False
    return idx, d


def expected_form(form, na, nb, selector, cross, capacity_tiles=1):
    """what spvo_match_last_form reports for a match of na x nb rows in `form` (capacity_tiles > 64: the host leaves the fused form on
    its own).  NN + cross-check swaps the sides: the re-rank's rows are then as long as the QUERY side."""
    cols = na if (selector == "NN" and cross) else nb
    fused = form == "fused" and capacity_tiles <= 64
    return dict(fp8=form == "fp8", fused=fused, nch=0 if fused or cols > 1024 else 4, jobs=1)


# ------------------------------------------------------------------ the fp8 shortlist, restated from csrc/match.hip.h in float64
FP8_SCALE = 16.0                 # MATCH_FP8_SCALE
FP8_MAX = 448.0                  # largest finite e4m3 value: 16 * x is clamped to it (|x| <= 28 converts without clamping)
ERR_REL_FP8 = 2e-2               # MATCH_ERR_REL_FP8: pass 1, statistical
ERR_REL_FP8_TAIL = 2.0 ** -13    # MATCH_ERR_REL_FP8_TAIL
E8_FACTOR = 2.001953125          # 2 (1 + 2^-10)


def fp8_copy(x):
    """desc_to_fp8_kernel: 16 * x clamped to +-448, rounded to OCP e4m3 (nearest even), read back and divided by 16 -> float64"""
    import torch
    y = np.clip(np.asarray(x, np.float32) * np.float32(FP8_SCALE), -FP8_MAX, FP8_MAX).astype(np.float32)
    y8 = torch.from_numpy(np.ascontiguousarray(y)).to(torch.float8_e4m3fn).to(torch.float32).numpy()
    return y8.astype(np.float64) / FP8_SCALE


def fp8_model(a, b):
    """-> dict(dt8, e8, cand1): the fp8 GEMM's squared distances [na, nb], the rigorous bound E8 on |dt8 - d2| per pair, and pass 1's
    candidate mask (lower bound dt8 - 2e-2 N <= second smallest upper bound dt8 + 2e-2 N of the row, N = |a|^2 + |b|^2)."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a8, b8 = fp8_copy(a), fp8_copy(b)
    n_a, n_b = (a64 * a64).sum(1), (b64 * b64).sum(1)
    qa, qb = np.linalg.norm(a64 - a8, axis=1), np.linalg.norm(b64 - b8, axis=1)
    N = n_a[:, None] + n_b[None, :]
    dt8 = N - 2.0 * (a8 @ b8.T)
    e8 = E8_FACTOR * (qa[:, None] * np.sqrt(n_b)[None, :] + np.linalg.norm(a8, axis=1)[:, None] * qb[None, :]) + ERR_REL_FP8_TAIL * N
    up, lo = dt8 + ERR_REL_FP8 * N, dt8 - ERR_REL_FP8 * N
    thr = np.sort(up, axis=1)[:, 1] if up.shape[1] >= 2 else np.full(len(up), np.inf)
    return dict(dt8=dt8, e8=e8, cand1=lo <= thr[:, None])
