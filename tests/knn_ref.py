"""Inputs and references of the kNN-Shapley cases that are not plain integer data (tests/small_op_cases.py, KNN), shared by
tests/test_cpu_small_ops.py (conditions on the cases, met by the reference alone) and tests/test_gpu_small_ops.py (the kernel).

special="nonfinite": integer-valued features with NaN and +inf planted so that every key is exact, +inf or NaN -- the order is fully determined
by include/ocl_hip.h K10: numbers ascending (ties by index, +inf a number), then the NaN keys in index order.
data="real": real-valued features of three kinds (KINDS), the float64 distances, a float32 restatement of each of the kernel's four distance
paths in its order of operations, and the number of float32 roundings K behind a key of each path (path_k)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
KINDS = ("normal", "clustered", "near_tie")


def keys64(ef, cf):
    """float64 squared distances [n_eval, n_cand]; a NaN operand or inf - inf gives NaN, inf - finite gives +inf, as in float32."""
    e, c = np.asarray(ef, dtype=np.float64), np.asarray(cf, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((e[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def stable_order(d):
    """torch.argsort(stable=True) per row on the CPU: ascending, ties by index, NaN as the largest value."""
    return torch.argsort(torch.from_numpy(np.ascontiguousarray(d)), dim=1, stable=True).numpy()


# ---- special="nonfinite" -------------------------------------------------------------------------------------------------------------------
def nonfinite_inputs(c):
    """(eval_f, eval_y, cand_f, cand_y).  Candidate 0 holds a NaN, candidate 1 +inf in the last dimension (from 9 candidates on also the
    third-last and second-last candidate: NaN keys and +inf keys far apart in index); evaluation row 0 is plain (one NaN key, one +inf key that
    ties with the padding's), row 1 has +inf in the last dimension (inf - inf: the +inf candidates' keys are NaN, every other key +inf), row 2
    holds a NaN (every key NaN: the index order).  Candidates 2 and n_cand - 1 are equal from 5 candidates on (an exact finite tie)."""
    assert c["special"] == "nonfinite" and c["ne"] == 3 and c["nc"] >= 3
    rng = np.random.default_rng(c["seed"])
    ne, nc, dim = c["ne"], c["nc"], c["dim"]
    ef = rng.integers(-4, 5, (ne, dim)).astype(np.float32)
    cf = rng.integers(-4, 5, (nc, dim)).astype(np.float32)
    if nc >= 5:
        cf[nc - 1] = cf[2]
    cf[0, 1] = np.nan
    cf[1, dim - 1] = np.inf
    if nc >= 9:
        cf[nc - 3, 0] = np.nan
        cf[nc - 2, dim - 1] = np.inf
    ef[1, dim - 1] = np.inf
    ef[2, dim // 2] = np.nan
    ey, cy = rng.integers(0, 3, ne).astype(np.int64), rng.integers(0, 3, nc).astype(np.int64)
    return ef, ey, cf, cy


# ---- data="real" ---------------------------------------------------------------------------------------------------------------------------
def real_inputs(c, kind):
    """(eval_f, eval_y, cand_f, cand_y) of one kind of data:
    normal     standard-normal features;
    clustered  100 + 1e-3 * normal: distances of ~1e-6 * dim between rows of norm ~100 * sqrt(dim), the conditioning on which
               |u|^2 + |v|^2 - 2 u.v in float32 has no correct digit;
    near_tie   standard normal, with c["pairs"] pairs of candidates (p, n_cand - 1 - p): the second a copy of the first with one coordinate
               moved by float32 steps until its float64 distance to evaluation row 0 is 1 + p % 3 (at most 4) float32 ulps larger."""
    assert c["data"] == "real" and kind in KINDS
    rng = np.random.default_rng(c["seed"] * 16 + KINDS.index(kind))
    ne, nc, dim = c["ne"], c["nc"], c["dim"]
    ef, cf = rng.standard_normal((ne, dim)), rng.standard_normal((nc, dim))
    if kind == "clustered":
        ef, cf = 100.0 + 1e-3 * ef, 100.0 + 1e-3 * cf
    ef, cf = ef.astype(np.float32), cf.astype(np.float32)
    if kind == "near_tie":
        e0 = ef[0].astype(np.float64)
        for p in range(c["pairs"]):
            a, b, j = p, nc - 1 - p, p % dim
            cf[b] = cf[a]
            da = float(((e0 - cf[a].astype(np.float64)) ** 2).sum())
            ulp = float(np.spacing(np.float32(da)))
            away = np.float32(np.inf) if cf[a, j] >= ef[0, j] else np.float32(-np.inf)      # away from the evaluation row: the distance grows
            for _ in range(1 << 16):
                cf[b, j] = np.nextafter(cf[b, j], away)
                if float(((e0 - cf[b].astype(np.float64)) ** 2).sum()) - da >= (1 + p % 3) * ulp:
                    break
    ey, cy = rng.integers(0, 3, ne).astype(np.int64), rng.integers(0, 3, nc).astype(np.int64)
    return ef, ey, cf, cy


def near_tie_ulps(c, ef, cf):
    """Per planted pair: (float64 distance of the copy - of the original, to evaluation row 0) in float32 ulps of the original's distance."""
    d = keys64(ef[:1], cf)[0]
    nc = c["nc"]
    return [(d[nc - 1 - p] - d[p]) / float(np.spacing(np.float32(d[p]))) for p in range(c["pairs"])]


def path_k(path, dim):
    """float32 roundings on the longest way from the features to a key of knn_sv_kernel (csrc/aser.hip), so that
    |key - d| <= ((1 + 2^-24)^K - 1) d <= 1.01 K 2^-24 d for a distance d (every term is >= 0: sum |terms| = d):
      * t = e - v is rounded once, and t * t carries that factor twice: 2;
      * s = fmaf(t, t, s) rounds once per step, and the first term of a chain passes through every step of it.  KNN_VEC_*: lane q of four
        adds the elements 4 i + q, i = 0 .. dim / 4 - 1 (the unrolled loop and the remainder loop continue one chain): dim / 4 steps.
        KNN_WAVE: lane l of 64 adds the elements l, l + 64, ...: ceil(dim / 64) steps;
      * KNN_VEC_*: (s0 + s1) + (s2 + s3), two adds on every way.  KNN_WAVE: the shuffle tree over 64 lanes, six adds."""
    if path == "KNN_WAVE":
        return 2 + math.ceil(dim / 64.0) + 6
    assert path in ("KNN_VEC_REM", "KNN_VEC_BOTH", "KNN_VEC_UNROLL") and dim % 4 == 0
    return 2 + dim // 4 + 2


def _fma32(t, s):
    """fmaf(t, t, s) on float32 arrays: t * t is exact in float64 (48 bits); the sum is rounded to 53 bits and then to 24 -- a double rounding
    that differs from the fused one by at most the last bit, in rare cases: good enough for a restatement that conditions the cases."""
    return (t.astype(np.float64) * t.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def restate32(path, ef, cf):
    """The keys [n_eval, n_cand] of the path in float32, operation by operation as the kernel orders them (see path_k)."""
    ef, cf = np.asarray(ef, dtype=np.float32), np.asarray(cf, dtype=np.float32)
    t = ef[:, None, :] - cf[None, :, :]                          # float32 subtraction
    ne, nc, dim = t.shape
    lanes = 64 if path == "KNN_WAVE" else 4
    s = np.zeros((ne, nc, lanes), dtype=np.float32)
    for i in range(0, dim, lanes):
        w = min(lanes, dim - i)
        s[:, :, :w] = _fma32(t[:, :, i:i + w], s[:, :, :w])
    if path == "KNN_WAVE":
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):                           # v += shfl_xor(v, o)
            s = s + s[:, :, lane ^ o]
        return s[:, :, 0]
    return (s[:, :, 0] + s[:, :, 1]) + (s[:, :, 2] + s[:, :, 3])


def inverted_pairs(order, d64, K):
    """Adjacent pairs (a, b) of `order` [n_eval, n_cand] that float64 orders the other way (d_a > d_b, or an exact tie with a > b).  Returns
    (their number, the number of adjacent pairs, and of the pair with the largest (d_a - d_b) / bound: d_a - d_b and
    bound = 1.01 K 2^-24 (d_a + d_b); without an inverted pair, 0 and the smallest bound of any adjacent pair)."""
    rows = np.arange(order.shape[0])[:, None]
    da, db = d64[rows, order[:, :-1]], d64[rows, order[:, 1:]]
    inv = (da > db) | ((da == db) & (order[:, :-1] > order[:, 1:]))
    bound = 1.01 * K * U * (da + db)
    if not inv.any():
        return 0, inv.size, 0.0, float(bound.min()) if bound.size else 0.0
    ratio = np.where(inv, (da - db) / np.where(bound > 0, bound, 1.0), -1.0)
    ratio = np.where(inv & (bound == 0), np.where(da > db, np.inf, 0.0), ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return int(inv.sum()), inv.size, float((da - db)[i]), float(bound[i])
