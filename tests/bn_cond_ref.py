"""float64 / exact-rational reference and derived bounds of the BatchNorm statistics chain on ill-conditioned channels, shared by
tests/test_cpu_bn_cond.py (the bounds can be met: a numpy model of the design and torch-CPU fp32 stay inside them; no GPU) and
tests/test_gpu_bn_cond.py (the kernels stay inside them).

The design (csrc/conv_stats_dev.h): fp32 partial sums of y and y^2 -> double -> a cell (fp64 atomics, or 2^-40 fixed point, truncating, in
deterministic mode); mean = s1 / M, var = max(s2 / M - mean^2, 0) in double (bn_batch_moments); sc = fl32(gamma * invstd),
sh = fl32(fma(-mean, sc, beta)) (bn_scale_shift); z = fl32(fma(y, sc, sh)); the ReLU decision is z > 0.

Exact arithmetic: a product of two fp32 values is exact in float64 (48 bits), so fl32(gamma * invstd) is one rounding of an exact double; an fma
of fp32 values is a rational number rounded once, computed here in fractions.Fraction and rounded to fp32 by integer arithmetic (round_f32),
never through a float64 intermediate.  The sign of fma(y, sc, sh) is the sign of the exact y * sc + sh (a correctly rounded result is zero
only when the exact one is), which float64 also gets right: y * sc is exact in float64 and a float64 sum of two float64 values is zero only
when they cancel exactly -- decide64 is that, decide_exact the Fraction statement it is checked against."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-5))        # the engine's eps is a float
MOMENTUM = float(np.float32(0.1))
FX = 2.0 ** -40                      # the deterministic cells' unit
SUM_K = 8                            # check_stats' constant (tests/test_gpu_layers.py): eight roundings of the sum of magnitudes
Z_REL = 2e-5                         # test_input_transform_against_float64_batchnorm's constant, relative to the terms of z


# ---- exact rounding -------------------------------------------------------------------------------------------------------------------
def round_f32(fr):
    """A Fraction rounded to the nearest fp32 value (ties to even, subnormals included), returned as a Python float holding that value.
    Integer arithmetic only: the binade of |fr| from the bit lengths, n = |fr| / quantum, floor and the remainder against one half."""
    fr = Fraction(fr)
    if fr == 0:
        return 0.0
    sign, a = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()     # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                    # 2^e <= a < 2^(e+1)
    q = max(e - 23, -149)                                         # exponent of the quantum (fp32: 24 significant bits, smallest 2^-149)
    n = a / (Fraction(2) ** q)
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (lo & 1)):
        lo += 1
    assert lo < (1 << 24) * 2 and q + 24 <= 128, "round_f32: overflow"
    return sign * math.ldexp(float(lo), q)                        # lo <= 2^24: exact


def fma_f32(a, b, c):
    """fl32(a * b + c) of three fp32 values (Python floats or numpy scalars): one rounding of the exact rational."""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def scale_shift_exact(gamma, beta, mean, invstd):
    """bn_scale_shift on fp32 arrays of one shape, exactly: sc = fl32(gamma * invstd), sh = fl32(fma(-mean, sc, beta)) -> two float32 arrays."""
    gamma, beta, mean, invstd = (np.asarray(v, np.float32) for v in np.broadcast_arrays(gamma, beta, mean, invstd))
    sc, sh = np.empty(gamma.shape, np.float32), np.empty(gamma.shape, np.float32)
    for i in np.ndindex(gamma.shape):
        s = round_f32(Fraction(float(gamma[i])) * Fraction(float(invstd[i])))
        sc[i] = s
        sh[i] = fma_f32(-float(mean[i]), s, beta[i])
    return sc, sh


def decide_exact(y, sc, sh):
    """The ReLU decision of one element, in rationals: fma(y, sc, sh) > 0 exactly when y * sc + sh > 0."""
    return Fraction(float(y)) * Fraction(float(sc)) + Fraction(float(sh)) > 0


def decide64(y, sc, sh):
    """The same for arrays (see the module docstring for why float64 decides it exactly)."""
    return np.asarray(y, np.float64) * np.asarray(sc, np.float64) + np.asarray(sh, np.float64) > 0


def fma32(a, b, c):
    """fl32(a * b + c) of fp32 arrays, exactly, vectorised: the product is exact in float64, TwoSum gives the float64 sum s and its exact
    residual t; rounding s to fp32 differs from rounding s + t only where s lies exactly midway between two fp32 neighbours, and there t
    decides the side (checked against fma_f32 in tests/test_cpu_bn_cond.py).  Returns float32."""
    a, b, c = (np.asarray(v, np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    r32 = s.astype(np.float32)
    r = r32.astype(np.float64)
    up = np.nextafter(r32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r32, np.float32(-np.inf)).astype(np.float64)
    # s is a float64, r its fp32 rounding (ties to even).  s + t rounds elsewhere only if s is a tie (then t's sign decides) ...
    tie_up, tie_dn = s == (r + up) / 2, s == (r + dn) / 2
    out = np.where(tie_up & (t > 0), up, r)
    out = np.where(tie_dn & (t < 0), dn, out)
    # ... or if s was rounded to the even side of a tie it sits on and t points the other way: covered above, since r is then the even
    # neighbour and (r + up) / 2 or (r + dn) / 2 is s itself
    return out.astype(np.float32)


def root_f32(sc, sh):
    """The fp32 value nearest the root -sh / sc of y -> fma(y, sc, sh) (sc != 0)."""
    return round_f32(-Fraction(float(sh)) / Fraction(float(sc)))


def ladder(center, half=64):
    """The 2 * half + 1 adjacent fp32 values centred on `center` (float32 array, ascending)."""
    out = np.empty(2 * half + 1, np.float32)
    out[half] = np.float32(center)
    for i in range(half):
        out[half + 1 + i] = np.nextafter(out[half + i], np.float32(np.inf))
        out[half - 1 - i] = np.nextafter(out[half - i], np.float32(-np.inf))
    return out


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return np.maximum(np.spacing(x).astype(np.float64), 2.0 ** -149)


# ---- moments --------------------------------------------------------------------------------------------------------------------------
def group_view(y, groups):
    """[n, h, w, C] -> [groups, M, C] float64."""
    y = np.asarray(y, np.float64)
    return y.reshape(groups, -1, y.shape[-1])


def two_pass_moments(y, groups):
    """Two-pass mean and biased variance per (group, channel) of y [n, h, w, C], accumulated in long double (numpy reduces along the pixel axis
    one row after the other: in float64 the reference itself would carry M roundings) and returned as float64."""
    yg = group_view(y, groups).astype(np.longdouble)
    mean = yg.mean(axis=1)
    var = ((yg - mean[:, None, :]) ** 2).mean(axis=1)
    return mean.astype(np.float64), var.astype(np.float64)


def exact_totals(y, groups):
    """[groups, 2, C] float64: sum y and sum y^2 per (group, channel), each the correctly rounded value of the exact sum (y^2 of an fp32 value is
    exact in float64; math.fsum rounds once)."""
    yg = group_view(y, groups)
    out = np.empty((yg.shape[0], 2, yg.shape[2]))
    for g in range(yg.shape[0]):
        for c in range(yg.shape[2]):
            col = yg[g, :, c]
            out[g, 0, c] = math.fsum(col.tolist())
            out[g, 1, c] = math.fsum((col * col).tolist())
    return out


def as_cells_hold(tot, det):
    """The totals as a consumer decodes them from cells that were written once with `tot`: unchanged, or truncated to 2^-40 (deterministic)."""
    tot = np.asarray(tot, np.float64)
    return np.floor(tot / FX) * FX if det else tot.copy()


def moments_from_totals(s1, s2, M):
    """The design's formula (bn_batch_moments) in float64: mean = s1 / M, var = max(s2 / M - mean^2, 0)."""
    mean = np.asarray(s1, np.float64) / M
    var = np.asarray(s2, np.float64) / M - mean * mean
    return mean, np.maximum(var, 0.0), var


def invstd_of(var):
    return 1.0 / np.sqrt(np.asarray(var, np.float64) + EPS)


def bn_forward64(y, groups, gamma, beta, mean=None, var=None):
    """float64 train-mode BatchNorm of y [n, h, w, C] per group (no ReLU): z, mean, var, invstd."""
    yg = group_view(y, groups)
    if mean is None:
        mean, var = two_pass_moments(y, groups)
    invstd = invstd_of(var)
    z = (yg - mean[:, None, :]) * invstd[:, None, :] * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return z.reshape(np.shape(y)), mean, var, invstd


def running_recurrence(mean, var, M, rm0, rv0):
    """The momentum recurrence group by group (nn.BatchNorm2d: unbiased variance), each step evaluated in float64 from the fp32 operands
    the kernel has ((float)mean, (float)unbiased var, the fp32 momentum and fl32(1 - momentum)) and rounded to fp32.  Returns (running mean,
    running var, and for each the largest magnitude a term of the recurrence reached).  A step's fp32 roundings are relative to its terms
    momentum * x and (1 - momentum) * r, not to their sum: with groups of opposite sign the sum cancels (r0, tiny and big channels have means
    of either sign around 0), so "within k ulp" of the recurrence is measured in ulps of the largest term."""
    rm, rv = np.asarray(rm0, np.float32).copy(), np.asarray(rv0, np.float32).copy()
    keep = float(np.float32(1.0) - np.float32(0.1))
    mag_m, mag_v = np.abs(rm).astype(np.float64), np.abs(rv).astype(np.float64)
    for g in range(mean.shape[0]):
        unb = var[g] * M / (M - 1.0) if M > 1 else var[g]
        tm, tv = MOMENTUM * mean[g].astype(np.float32).astype(np.float64), MOMENTUM * unb.astype(np.float32).astype(np.float64)
        mag_m = np.maximum(mag_m, np.maximum(np.abs(tm), keep * np.abs(rm)))
        mag_v = np.maximum(mag_v, np.maximum(np.abs(tv), keep * np.abs(rv)))
        rm = (tm + keep * rm.astype(np.float64)).astype(np.float32)
        rv = (tv + keep * rv.astype(np.float64)).astype(np.float32)
    return rm, rv, mag_m, mag_v


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def partials_per_cell(form):
    """Upper bound on the partial sums one launch adds into one cell (group, sum, channel), from the launch geometry the hook reports (a
    TestConvForm: family, nt, grid_x, grid_y), read off the epilogues.  grid_y splits the output channels in every family (n0 = blockIdx.y *
    COPW), so one channel's cell is fed by the workgroups of one grid row only:
      conv_t / conv_q   a workgroup's tiles come in ascending group order and it flushes once per group run (flush_stats) -- grid_x;
      conv_s            one partial per 16-pixel tile: wave j of a workgroup owns pixel tile j of its nt tiles -- grid_x * nt;
      conv_w / conv_wx  one partial per workgroup (the flush through LDS) and, per group boundary and launch, at most one wave that crosses
                        it and adds the finished group's sums directly -- grid_x + 1."""
    fam = form.family
    if fam in (0, 1):
        return form.grid_x
    if fam == 2:
        return form.grid_x * form.nt
    return form.grid_x + 1


def conv_s_tile_totals(y, groups, det, contracted, pair_squares=False):
    """conv_s_kernel's stats epilogue restated bit for bit -> [groups, 2, C] float64 cell totals (up to the order of the float64 additions).
    One partial per 16-pixel tile: 16 consecutive output pixels, lane r = pixel r of the tile; row16_sum is four DPP steps on the 16 lanes:
    lane ^ 1, lane ^ 2, the mirror inside each half (r -> r ^ 7), the mirror of the row (r -> 15 - r); lane e adds the sum of channel
    4q + e, lane 4 + e its sum of squares.  The sums of y are the same in every lane (fp32 addition commutes).  The sums of squares have two
    legal evaluations of the source's row16_sum(z * z):
      contracted = False   the square rounded, then the four adds (what the source says): the same in every lane;
      contracted = True    the compiler contracts the square into the first add (-ffp-contract=fast; what hipcc emits for gfx950 today:
                           v_mul_f32, v_mov_b32_dpp quad_perm:[1,0,3,2], v_fmac_f32): lane r holds fma(z_r, z_r, fl(z_(r^1)^2)), which
                           differs between the two lanes of a pair, so the later steps are restated lane by lane and channel 4q + e reads
                           lane 4 + e.
    pair_squares: NOT what the kernel does -- the arithmetic of the mutation "one more fp32 add of two partial sums of squares before the
    conversion to double" (tiles 2k and 2k + 1, the two waves of an nt = 2 workgroup), for tests/test_cpu_bn_cond.py to show that the
    GPU file's tolerance separates it from both legal evaluations."""
    yg = group_view(y, groups)
    G, M, Cc = yg.shape
    assert M % 16 == 0
    v = yg.astype(np.float32).reshape(G, M // 16, 16, Cc)
    lanes = np.arange(16)

    def butterfly(a, steps):
        for perm in steps:
            a = a + a[:, :, perm]
        return a
    x1, x2, half, row = lanes ^ 1, lanes ^ 2, lanes ^ 7, 15 - lanes
    s1 = butterfly(v, (x1, x2, half, row))[:, :, 0]
    sq = (v.astype(np.float64) * v.astype(np.float64)).astype(np.float32)
    if contracted:
        a = fma32(v, v, sq[:, :, x1])
        d = butterfly(a, (x2, half, row))
        s2 = np.stack([d[:, :, 4 + (c & 3), c] for c in range(Cc)], axis=-1)
    else:
        s2 = butterfly(sq, (x1, x2, half, row))[:, :, 0]
    if pair_squares:
        assert s2.shape[1] % 2 == 0
        s2 = s2[:, 0::2] + s2[:, 1::2]
    p1, p2 = s1.astype(np.float64), s2.astype(np.float64)
    if det:
        p1, p2 = np.floor(p1 / FX) * FX, np.floor(p2 / FX) * FX
    return np.stack([p1.sum(axis=1), p2.sum(axis=1)], axis=1), M // 16


def sums_bound(sum_abs, nparts, det):
    """|cell total - float64 sum| <= 8 U sum|.| (check_stats' constant), + the float64 additions of the partials, + in deterministic mode one
    truncation of 2^-40 per partial.  sum_abs: sum |y| or sum y^2; nparts: partial sums added into the cell (per group and channel)."""
    return SUM_K * U * sum_abs + nparts * 2.0 ** -53 * sum_abs + (nparts * FX if det else 0.0)


def moments_bound(y, groups, nparts, det):
    """Bounds of (mean, var) derived from totals that meet sums_bound, against the two-pass moments: with a = sums_bound(sum|y|) / M and
    b = sums_bound(sum y^2) / M,  |d mean| <= a  and  |d var| <= b + 2 |mean| a + a^2  (var = s2 / M - mean^2), plus the float64 roundings
    of the formula itself: 4 * 2^-53 * (E[y^2] + mean^2)."""
    yg = group_view(y, groups)
    M = yg.shape[1]
    e1, e2, mean = np.abs(yg).mean(axis=1), (yg * yg).mean(axis=1), yg.mean(axis=1)
    a = sums_bound(e1 * M, nparts, det) / M
    b = sums_bound(e2 * M, nparts, det) / M
    return a, b + 2 * np.abs(mean) * a + a * a + 4 * 2.0 ** -53 * (e2 + mean * mean)


def exact_moments_bound(y, groups, det):
    """(mean, var) from the correctly rounded totals of y (exact_totals) against the two-pass moments: what is left is the float64 of the formula
    itself -- one rounding of each total, the division, the square, the subtraction: 4 roundings relative to at most E[y^2] + mean^2, and the
    rounding of the reference to float64: stated as 8 * 2^-53 (E[y^2] + mean^2); 4 * 2^-53 E|y| for the mean.  In deterministic mode the
    cells' truncation of each total to 2^-40 besides (worst case: t = 2^-40 / M on the mean, t (1 + 2 |mean| + t) on var)."""
    yg = group_view(y, groups)
    M = yg.shape[1]
    e1, e2, mean = np.abs(yg).mean(axis=1), (yg * yg).mean(axis=1), yg.mean(axis=1)
    t = FX / M if det else 0.0
    return 4 * 2.0 ** -53 * e1 + t, 8 * 2.0 ** -53 * (e2 + mean * mean) + t * (1 + 2 * np.abs(mean) + t)


def z_bound(y, groups, gamma, beta, mean, invstd):
    """Per element: 2e-5 * ((|y| + |mean|) * invstd * |gamma| + |beta|) with that element's channel terms (c = 2e-5 / U = 336 fp32 roundings)."""
    yg = np.abs(group_view(y, groups))
    t = (yg + np.abs(mean)[:, None, :]) * invstd[:, None, :] * np.abs(np.asarray(gamma, np.float64)) + np.abs(np.asarray(beta, np.float64))
    return (Z_REL * t).reshape(np.shape(y))


# BatchNorm backward: dy = gamma * invstd * (d - k1 - xhat * k2), k1 = mean(d), k2 = mean(d * xhat), xhat = (y - mean) * invstd.
# Roundings of one output element (fp32, saved mean / invstd rounded to fp32 by the forward):
#   xhat: the two roundings of mean and invstd to fp32, the subtraction, the product                      4
#   xhat * k2, d - k1, (...) - (...), scale = gamma * invstd, scale * (...)                               5
#   k1, k2 rounded to fp32                                                                                2
# = 11 roundings, each relative to a term no larger than |d| + |k1| + |xhat| |k2|; the reference's xhat uses the float64 moments, and the
# rounding of mean to fp32 moves xhat by U |mean| invstd (not by U |xhat|): that term is carried separately.  BWD_C = 16 leaves the difference
# to 11 for the fused multiply-adds the compiler may or may not form.
BWD_C = 16
# the batch sums sum(d), sum(d * xhat) are fp32 partials like the forward's: the same 8 U sum|.| (SUM_K); the products d * xhat inside
# the sum carry xhat's own error
SUMS_C = SUM_K + 4


def bwd_bounds(d, y, groups, gamma, mean, invstd):
    """Per-channel bounds of (dy [groups, C] applied to every element of the channel, dgamma [C], dbeta [C]) for the masked gradient d and
    raw output y [n, h, w, C], float64 statistics mean / invstd [groups, C]:
      xhat error      ex  = U * (4 |xhat| + |mean| invstd)            (max over the channel: a per-channel bound)
      k1 error        e1  = SUM_K U E|d|
      k2 error        e2  = SUMS_C U E|d xhat| + E|d| ex
      |d dy|         <= |gamma| invstd (BWD_C U (max|d| + |k1| + max|xhat| |k2|) + e1 + max|xhat| e2 + ex |k2|)
      |d dgamma|     <= sum over groups of M (e2 + U |k2|),   |d dbeta| <= sum over groups of M (e1 + U |k1|)"""
    dg, yg = group_view(d, groups), group_view(y, groups)
    M = dg.shape[1]
    gamma = np.abs(np.asarray(gamma, np.float64))
    xhat = (yg - mean[:, None, :]) * invstd[:, None, :]
    ax = np.abs(xhat).max(axis=1)
    ex = U * (4 * ax + np.abs(mean) * invstd)
    k1, k2 = dg.mean(axis=1), (dg * xhat).mean(axis=1)
    ad = np.abs(dg)
    e1 = SUM_K * U * ad.mean(axis=1)
    e2 = SUMS_C * U * (ad * np.abs(xhat)).mean(axis=1) + ad.mean(axis=1) * ex
    dy = gamma * invstd * (BWD_C * U * (ad.max(axis=1) + np.abs(k1) + ax * np.abs(k2)) + e1 + ax * e2 + ex * np.abs(k2))
    dgamma = (M * (e2 + U * np.abs(k2))).sum(axis=0)
    dbeta = (M * (e1 + U * np.abs(k1))).sum(axis=0)
    return dy, dgamma, dbeta


def bn_backward64(d, y, groups, gamma, mean, invstd):
    """float64 BatchNorm backward of the (already masked) gradient d: dy, dgamma, dbeta."""
    dg, yg = group_view(d, groups), group_view(y, groups)
    xhat = (yg - mean[:, None, :]) * invstd[:, None, :]
    k1, k2 = dg.mean(axis=1, keepdims=True), (dg * xhat).mean(axis=1, keepdims=True)
    dy = np.asarray(gamma, np.float64) * invstd[:, None, :] * (dg - k1 - xhat * k2)
    return dy.reshape(np.shape(d)), (dg * xhat).sum(axis=(0, 1)), dg.sum(axis=(0, 1))


# ---- a numpy model of the design ------------------------------------------------------------------------------------------------------
def model_totals(y, groups, L, det):
    """The design's cell totals of y [n, h, w, C] (fp32 values).  A partial sum covers L consecutive pixels the way the epilogues form it: 16
    lanes each add L / 16 values in turn (squares by fma: fl32(y * y + s)), then the four-step fp32 butterfly over the 16 lanes (row16_sum);
    each partial is added as a double (deterministic mode: truncated to 2^-40 first).  -> ([groups, 2, C] float64, partials per cell)."""
    assert L % 16 == 0
    yg = group_view(y, groups)
    G, M, Cc = yg.shape
    nparts = (M + L - 1) // L
    pad = nparts * L - M
    y32 = np.concatenate([yg, np.zeros((G, pad, Cc))], axis=1).astype(np.float32).reshape(G, nparts, L // 16, 16, Cc)
    s1, s2 = np.zeros((G, nparts, 16, Cc), np.float32), np.zeros((G, nparts, 16, Cc), np.float32)
    for i in range(L // 16):
        v = y32[:, :, i]
        s1 = s1 + v
        s2 = fma32(v, v, s2)
    for step in (1, 2, 4, 8):       # lane l adds lane l ^ step: after four steps every lane holds the sum
        idx = np.arange(16) ^ step
        s1, s2 = s1 + s1[:, :, idx], s2 + s2[:, :, idx]
    p1, p2 = s1[:, :, 0].astype(np.float64), s2[:, :, 0].astype(np.float64)
    if det:
        p1, p2 = np.floor(p1 / FX) * FX, np.floor(p2 / FX) * FX
    return np.stack([p1.sum(axis=1), p2.sum(axis=1)], axis=1), nparts


def model_forward(y, groups, gamma, beta, totals):
    """The design's forward from given totals: (z float32 before the ReLU, save_mean float32, save_invstd float32, var float64)."""
    yg = group_view(y, groups)
    mean, var, _ = moments_from_totals(totals[:, 0], totals[:, 1], yg.shape[1])
    m32, i32 = mean.astype(np.float32), invstd_of(var).astype(np.float32)
    g32, b32 = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    sc = (g32.astype(np.float64) * i32.astype(np.float64)).astype(np.float32)
    sh = fma32(-m32, sc, np.broadcast_to(b32, sc.shape))
    z = fma32(yg.astype(np.float32), sc[:, None, :], sh[:, None, :])
    return z.reshape(np.shape(y)), m32, i32, var
