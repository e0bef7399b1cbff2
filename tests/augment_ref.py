"""The SCR augmentation (include/ocl_hip.h, K13) stated in plain numpy, from the header's text: no GPU, no library, no torch.

ref_augment(x, params, dtype): the image contract -- 12 floats per image in, pixels out.  dtype=float64 is the reference the kernel
is judged against; dtype=float32 is the same statement with every operation rounded to float32 on its own (numpy rounds each
array operation), an independent float32 restatement whose distance from the float64 one is the yardstick of the GPU test's
tolerance.  Neither looks at the kernel.
ref_aug_params(u, cfg12, h, w): the parameter arithmetic of ocl_scr_augment_uniform in float64, and for every row how far each
rounding decision (rint of a crop side, a fit comparison, floor of a position or of the order, a probability threshold) was from
its boundary, relative to the value rounded: a float32 evaluation can only decide differently where that distance is a few ulp.
MUTANTS: ref_augment with one deliberate error each, of the kind a kernel could carry (tests/test_cpu_small_ops.py shows the
cases of tests/small_op_cases.py tell every observable one from the reference by a wide margin).
augment_case_inputs / aug_params_case_inputs: the inputs of the cases of tests/small_op_cases.py (numpy only, seeded)."""
import itertools
import math

import numpy as np

NPARAM, NUNIFORM, TRIES = 12, 30, 10
PERMS = list(itertools.permutations(range(4)))      # lexicographic: 0 (0,1,2,3), 1 (0,1,3,2), ... 23 (3,2,1,0); 0 b, 1 c, 2 s, 3 hue
MARGIN = 2.0 ** -18                                  # rows whose every decision is further than this from its boundary are compared exactly
U = 2.0 ** -24

# name -> what is wrong
MUTANTS = {
    "order_decode_13": "order index 13 decodes to the permutation of index 14 (every other index is right)",
    "hsv2rgb_sector3_qt": "q and t swapped in sector 3 of hsv2rgb",
    "rgb2hsv_no_wrap": "the h < 0 wrap of rgb2hsv (red is the maximum, g < b) omitted",
    "clamp_to_crop": "source coordinates clamped to the crop box instead of the image",
    "flip_after_coordinate": "the flip mirrors the source coordinate instead of the output column",
    "gray_before_jitter": "grayscale taken before the colour jitter",
}


def rgb2hsv(r, g, b, T=np.float64, wrap=True):
    """Hexcone HSV of arrays r, g, b: (h in [0, 1), s, v).  The maximum channel is r first, then g, on ties; a gray has h = 0."""
    r, g, b = (np.asarray(a, dtype=T) for a in (r, g, b))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    df = mx - mn
    s = np.where(mx > 0, df / np.where(mx > 0, mx, T(1)), T(0)).astype(T)
    d = np.where(df > 0, df, T(1))
    hr = (g - b) / d
    if wrap:
        hr = np.where(hr < 0, hr + T(6), hr)
    hg = (b - r) / d + T(2)
    hb = (r - g) / d + T(4)
    h = np.where(df <= 0, T(0), np.where(mx == r, hr, np.where(mx == g, hg, hb))).astype(T)
    return h / T(6), s, mx


def hsv2rgb(h, s, v, T=np.float64, swap_qt_in=None):
    """Back from HSV; h is any real number, its fractional part is the hue."""
    h, s, v = (np.asarray(a, dtype=T) for a in (h, s, v))
    h6 = (h - np.floor(h)) * T(6)
    i = np.floor(h6).astype(np.int64) % 6
    f = h6 - np.floor(h6)
    one = T(1)
    p, q, t = v * (one - s), v * (one - f * s), v * (one - (one - f) * s)
    sect = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    if swap_qt_in is not None:
        sect[swap_qt_in] = tuple(t if a is q else q if a is t else a for a in sect[swap_qt_in])
    out = []
    for ch in range(3):
        o = sect[5][ch]
        for k in range(4, -1, -1):
            o = np.where(i == k, sect[k][ch], o)
        out.append(o.astype(T))
    return out


def _clamp01(a, T):
    return np.minimum(np.maximum(a, T(0)), T(1))


def _one_image(img, p, T, mutant):
    _, h, w = img.shape
    y0, x0, ch, cw = p[0], p[1], p[2], p[3]
    flip, jit, gray = p[4] > 0.5, p[5] > 0.5, p[11] > 0.5
    half = T(0.5)
    oy, ox = np.arange(h).astype(T), np.arange(w).astype(T)
    if flip and mutant != "flip_after_coordinate":
        ox = T(w - 1) - ox
    sy = y0 + (oy + half) * (ch / T(h)) - half
    sx = x0 + (ox + half) * (cw / T(w)) - half
    if flip and mutant == "flip_after_coordinate":
        sx = T(w - 1) - sx
    if mutant == "clamp_to_crop":
        sy = np.minimum(np.maximum(sy, y0), y0 + ch - T(1))
        sx = np.minimum(np.maximum(sx, x0), x0 + cw - T(1))
    sy = np.minimum(np.maximum(sy, T(0)), T(h - 1))
    sx = np.minimum(np.maximum(sx, T(0)), T(w - 1))
    iy0, ix0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    iy1, ix1 = np.minimum(iy0 + 1, h - 1), np.minimum(ix0 + 1, w - 1)
    fy, fx = (sy - iy0.astype(T))[:, None], (sx - ix0.astype(T))[None, :]
    c = []
    for k in range(3):
        pl = img[k]
        a, b = pl[iy0][:, ix0], pl[iy0][:, ix1]
        cc, dd = pl[iy1][:, ix0], pl[iy1][:, ix1]
        top, bot = a + (b - a) * fx, cc + (dd - cc) * fx
        c.append(top + (bot - top) * fy)

    def to_gray(c):
        g = T(0.299) * c[0] + T(0.587) * c[1] + T(0.114) * c[2]
        return [g, g.copy(), g.copy()]

    if gray and mutant == "gray_before_jitter":
        c = to_gray(c)
    if jit:
        order = int(p[10])
        if mutant == "order_decode_13" and order == 13:
            order = 14
        for op in PERMS[order]:
            if op == 0:
                d = p[6] - T(1)
                c = [_clamp01(v + d, T) for v in c]
            elif op == 1:
                c = [_clamp01(v * p[7], T) for v in c]
            else:
                hh, ss, vv = rgb2hsv(c[0], c[1], c[2], T, wrap=mutant != "rgb2hsv_no_wrap")
                if op == 2:
                    ss = _clamp01(ss * p[8], T)
                else:
                    hh = hh + p[9]
                c = hsv2rgb(hh, ss, vv, T, swap_qt_in=3 if mutant == "hsv2rgb_sector3_qt" else None)
    if gray and mutant != "gray_before_jitter":
        c = to_gray(c)
    return np.stack(c).astype(T)


def ref_augment(x, params, dtype=np.float64, mutant=None):
    """x [n, 3, h, w] and params [n, 12] (float32 values) -> [n, 3, h, w] of `dtype`, every operation carried out in `dtype`."""
    assert mutant is None or mutant in MUTANTS, mutant
    T = np.dtype(dtype).type
    x, params = np.asarray(x).astype(T), np.asarray(params).astype(T)
    assert x.ndim == 4 and x.shape[1] == 3 and params.shape == (x.shape[0], NPARAM), (x.shape, params.shape)
    out = np.empty(x.shape, dtype=T)
    for i in range(x.shape[0]):
        out[i] = _one_image(x[i], params[i], T, mutant)
    return out


# ==========================================================================================================================================
# the parameter arithmetic
# ==========================================================================================================================================
N_DIST = TRIES * 6 + 3 + 3


def _rel(v, boundary):
    return abs(v - boundary) / abs(v) if v != 0 else float("inf")


def _floor_dist(v):
    """floor(v) of a product with a draw: the nearest integer is the boundary; v == 0 (a draw of exactly 0) is exact in any precision."""
    return _rel(v, float(np.rint(v)))


def ref_aug_params(u, cfg12, h, w):
    """u [n, 30] float32 draws, cfg12 as ScrAugment.config() -> (params [n, 12] float64, dist [n, N_DIST]).
    dist: the relative distance |v - boundary| / |v| of every decision taken for the row, inf where a slot is unused: per crop attempt up
    to the accepted one (all ten if none fits) the rint of the width and of the height (boundary: the nearest half-integer) and the four fit
    comparisons on the rounded sides (boundaries 0.5 and size + 0.5); the floor of the two positions and of the order (nearest integer);
    the three probability thresholds (flip, jitter, gray)."""
    u = np.asarray(u, dtype=np.float64)
    s_lo, s_hi, r_lo, r_hi, jb, jc, js, jh, p_jit, p_gray, fb_w, fb_h = [float(v) for v in cfg12]
    H, W = float(h), float(w)
    n = u.shape[0]
    P = np.zeros((n, NPARAM))
    D = np.full((n, N_DIST), np.inf)
    for i in range(n):
        found = False
        cw = ch = 0.0
        for t in range(TRIES):
            area = (s_lo + (s_hi - s_lo) * u[i, t]) * H * W
            r = math.exp(math.log(r_lo) + (math.log(r_hi) - math.log(r_lo)) * u[i, TRIES + t])
            vw, vh = math.sqrt(area * r), math.sqrt(area / r)
            cwt, cht = float(np.rint(vw)), float(np.rint(vh))
            D[i, 6 * t: 6 * t + 6] = [_rel(vw, math.floor(vw) + 0.5), _rel(vh, math.floor(vh) + 0.5), _rel(vw, 0.5), _rel(vw, W + 0.5),
                                      _rel(vh, 0.5), _rel(vh, H + 0.5)]
            if 0 < cwt <= W and 0 < cht <= H:
                found, cw, ch = True, cwt, cht
                break
        e = u[i, 2 * TRIES:]
        k = 6 * TRIES
        if found:
            vy, vx = e[0] * (H - ch + 1.0), e[1] * (W - cw + 1.0)
            D[i, k], D[i, k + 1] = _floor_dist(vy), _floor_dist(vx)
            y0, x0 = min(math.floor(vy), H - 1.0), min(math.floor(vx), W - 1.0)
        else:
            cw, ch = fb_w, fb_h
            y0, x0 = math.floor((H - ch) / 2.0), math.floor((W - cw) / 2.0)
        vo = e[8] * 24.0
        D[i, k + 2] = _floor_dist(vo)
        D[i, k + 3: k + 6] = [_rel(e[2], 0.5), _rel(e[3], p_jit), _rel(e[9], p_gray)]
        P[i] = [y0, x0, ch, cw, float(e[2] < 0.5), float(e[3] < p_jit), 1.0 - jb + 2.0 * jb * e[4], 1.0 - jc + 2.0 * jc * e[5],
                1.0 - js + 2.0 * js * e[6], -jh + 2.0 * jh * e[7], min(max(math.floor(vo), 0.0), 23.0), float(e[9] < p_gray)]
    return P, D


def comparable(D):
    """The rows a float32 evaluation must reproduce exactly: every decision further than MARGIN (32 float32 ulp) from its boundary."""
    return (D > MARGIN).all(1)


def factor_ulps(cfg12):
    """The float32 spacing the four jitter factors are compared in: that of the largest magnitude in the factor's range, 1 + strength
    (brightness, contrast, saturation) or the hue strength.  (A factor is j0 + j1 * draw with |j0| + |j1| at most three times that.)"""
    return np.array([np.spacing(np.float32(1.0 + float(cfg12[4 + k]))) for k in range(3)] + [np.spacing(np.float32(float(cfg12[7])))], dtype=np.float64)


def box_inside_image(P, h, w):
    """What every row must satisfy, compared exactly or not: integer box inside the image, flags 0 / 1, order 0..23, finite factors."""
    P = np.asarray(P, dtype=np.float64)
    y0, x0, ch, cw = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    ok = (P[:, :4] == np.floor(P[:, :4])).all(1) & (y0 >= 0) & (x0 >= 0) & (ch >= 1) & (cw >= 1) & (y0 + ch <= h) & (x0 + cw <= w)
    ok &= np.isin(P[:, [4, 5, 11]], (0.0, 1.0)).all(1) & (P[:, 10] == np.floor(P[:, 10])) & (P[:, 10] >= 0) & (P[:, 10] <= 23)
    return ok & np.isfinite(P).all(1)


# ==========================================================================================================================================
# the inputs of the cases (tests/small_op_cases.py)
# ==========================================================================================================================================
def _row(y0=0.0, x0=0.0, ch=None, cw=None, flip=0, jit=0, b=1.0, c=1.0, s=1.0, hue=0.0, order=0, gray=0, h=None, w=None):
    return [y0, x0, h if ch is None else ch, w if cw is None else cw, flip, jit, b, c, s, hue, order, gray]


def _agent_factors(rng):
    """Jitter factors in the agent's ranges (ColorJitter(0.4, 0.4, 0.4, 0.1))."""
    return dict(b=rng.uniform(0.6, 1.4), c=rng.uniform(0.6, 1.4), s=rng.uniform(0.6, 1.4), hue=rng.uniform(-0.1, 0.1))


def hsv_sector_pixels():
    """35 RGB triples (a 5 x 7 image) chosen by hand: the three maximum-channel branches, the negative-hue wrap (red the maximum, g < b),
    the ties r == g as maximum and g == b, grays, 0 and 1, and a colour in each of the six sectors of hsv2rgb."""
    px = [
        (0.9, 0.5, 0.1), (0.7, 0.9, 0.2), (0.1, 0.8, 0.4), (0.2, 0.5, 0.9), (0.6, 0.1, 0.8), (0.9, 0.2, 0.6),      # sectors 0..5
        (0.8, 0.1, 0.3), (0.95, 0.0, 0.9), (0.5, 0.25, 0.26),                                                        # red max, g < b: h < 0 before the wrap
        (0.3, 0.8, 0.1), (0.1, 0.8, 0.7), (0.05, 0.1, 0.6), (0.55, 0.1, 0.6),                                        # green max; blue max
        (0.7, 0.7, 0.2), (0.7, 0.7, 0.7), (0.9, 0.4, 0.4), (0.2, 0.6, 0.6), (0.3, 0.3, 0.9), (0.8, 0.3, 0.8),        # ties: r == g max, gray, g == b, ...
        (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0),        # black, white, gray, primaries
        (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.5, 0.0), (0.0, 0.5, 1.0),                         # secondaries, saturated
        (2.0 ** -20, 0.0, 0.0), (1.0, 1.0 - 2.0 ** -20, 1.0), (0.25, 0.75, 0.5), (0.75, 0.25, 0.5), (0.4, 0.41, 0.42),
    ]
    assert len(px) == 35
    return np.array(px, dtype=np.float32)


HUE_SHIFTS = [-0.5, -0.1, 0.0, 1.0 / 6.0, 0.1, 1.0]
SAT_FACTORS = [0.0, 0.6, 1.4, 3.0]


def geometry_boxes(h, w):
    """(y0, x0, ch, cw): the full crop, 1 x 1, the four corners (smaller than the image: the clamp to the image fires on either side), tall,
    wide, two fractional boxes (the second reaches past the centre of the last pixel)."""
    qh, qw = max(1.0, h // 3), max(1.0, w // 3)
    return [(0, 0, h, w), (h // 2, w // 2, 1, 1), (0, 0, qh, qw), (0, w - qw, qh, qw), (h - qh, 0, qh, qw), (h - qh, w - qw, qh, qw),
            (0, w // 3, h, max(1.0, w // 4)), (h // 3, 0, max(1.0, h // 4), w), (0.25 * h + 0.3, 0.2 * w + 0.6, 0.5 * h + 0.45, 0.55 * w + 0.2),
            (0.4, 0.7, h - 0.65, w - 0.9)]


def augment_case_inputs(c):
    """(x [rows, 3, h, w] float32, params [rows, 12] float32) of an `augment` case.  rows = n + c['extra']: the kernel is handed the first n,
    the others are there to be left alone."""
    rng = np.random.default_rng(c["seed"])
    n, h, w, kind = c["n"], c["h"], c["w"], c["kind"]
    rows = n + c.get("extra", 0)
    R = lambda **kw: _row(h=h, w=w, **kw)
    x = rng.random((rows, 3, h, w)).astype(np.float32)
    if kind == "orders_same":
        x[:] = x[0]
        P = [R(jit=1, b=1.3, c=c.get("contrast", 0.75), s=1.35, hue=0.08, order=k) for k in range(24)]
    elif kind == "orders_mixed":
        P = []
        for k in range(24):
            ch, cw = rng.integers(8, h + 1), rng.integers(8, w + 1)
            P.append(R(y0=rng.integers(0, h - ch + 1), x0=rng.integers(0, w - cw + 1), ch=ch, cw=cw, flip=k % 2, jit=1, order=k, **_agent_factors(rng)))
    elif kind == "hsv":
        px = hsv_sector_pixels()
        x[:] = px.T.reshape(3, h, w)
        P = [R(jit=1, hue=v, order=0) for v in HUE_SHIFTS] + [R(jit=1, s=v, order=0) for v in SAT_FACTORS]
    elif kind == "clamps":
        edge = np.array([0.0, 2.0 ** -24, 0.01, 0.39, 0.4, 0.41, 0.59, 0.6, 0.61, 1.0 / 1.4, 0.99, 1.0 - 2.0 ** -24, 1.0], dtype=np.float32)
        x.reshape(rows, 3, -1)[:, :, : len(edge)] = edge          # the first pixels of every channel; the rest stays random
        P = [R(jit=1, b=0.6), R(jit=1, b=1.4), R(jit=1, c=0.6), R(jit=1, c=1.4)]
    elif kind == "geometry":
        P = [R(y0=b[0], x0=b[1], ch=b[2], cw=b[3], flip=f) for b in geometry_boxes(h, w) for f in (0, 1)]
    elif kind == "gray":
        P = [R(gray=1), R(gray=1, jit=1, order=17, **_agent_factors(rng)), R(gray=1, jit=1, order=6, flip=1, y0=2, x0=3, ch=h - 4.5, cw=w - 6.25, **_agent_factors(rng))]
    elif kind == "random":
        P = []
        for k in range(rows):
            ch, cw = rng.uniform(1, h), rng.uniform(1, w)
            P.append(R(y0=rng.uniform(0, h - ch), x0=rng.uniform(0, w - cw), ch=ch, cw=cw, flip=rng.integers(0, 2), jit=rng.integers(0, 4) > 0,
                       order=rng.integers(0, 24), gray=rng.integers(0, 4) == 0, **_agent_factors(rng)))
    elif kind == "refuse":
        return np.zeros((1, 3, 1, 1), dtype=np.float32), np.array([R()], dtype=np.float32)
    else:
        raise KeyError(kind)
    P = P + [R() for _ in range(rows - len(P))]
    P = np.array(P[:rows], dtype=np.float32).reshape(rows, NPARAM)
    assert len(P) == rows == x.shape[0], (c["name"], len(P), rows)
    return x, P


_REFERENCES = {}


def augment_case_reference(c):
    """(x, params, float64 reference of the first n rows, E, tolerance) of an `augment` case, computed once per process.
    E = max |ref_augment(float32) - ref_augment(float64)| on the case's own inputs: what rounding every operation to float32 costs for
    these sizes and factors (the source coordinates are formed in float32, so it grows with max(h, w); contrast and saturation amplify
    it).  The tolerance is 4 E -- the device may contract multiply-adds and has its own division -- and at least 8 * 2^-24."""
    if c["name"] not in _REFERENCES:
        x, P = augment_case_inputs(c)
        n = c["n"]
        r64 = ref_augment(x[:n], P[:n], np.float64)
        r32 = ref_augment(x[:n], P[:n], np.float32)
        E = float(np.abs(r32.astype(np.float64) - r64).max()) if n else 0.0
        r64.setflags(write=False)
        _REFERENCES[c["name"]] = (x, P, r64, E, max(4.0 * E, 8.0 * U))
    return _REFERENCES[c["name"]]


def same_image_orders(i, j, contrast):
    """True if the contract gives orders i and j the same image for every input: one turns into the other by exchanging neighbouring
    operations that commute.  Saturation and hue always do (they act on different HSV coordinates: 6 of the 276 pairs differ by that
    alone).  A contrast factor <= 1 cannot reach the clamp on pixels in [0, 1], and scaling r, g, b by one factor scales v and leaves h and
    s alone, so such a contrast commutes with saturation and with hue as well (then only what precedes the brightness step matters: 8
    distinct images among the 24 orders).  Brightness is additive and clamped: it commutes with nothing."""
    commute = [{2, 3}] + ([{1, 2}, {1, 3}] if contrast <= 1.0 else [])
    seen, todo = {PERMS[i]}, [PERMS[i]]
    while todo:
        a = todo.pop()
        for k in range(3):
            if {a[k], a[k + 1]} in commute:
                b = a[:k] + (a[k + 1], a[k]) + a[k + 2:]
                if b not in seen:
                    seen.add(b)
                    todo.append(b)
    return PERMS[j] in seen


def flags_only(p, h, w):
    """A parameter row that only moves pixels: full crop, no jitter, no gray.  Its output is the input (mirrored if flip), bit for bit."""
    return p[0] == 0 and p[1] == 0 and p[2] == h and p[3] == w and p[5] <= 0.5 and p[11] <= 0.5


def aug_params_config(c):
    """cfg12 of an `aug_params` case, by the arithmetic of ScrAugment.config() / fallback_crop() (the CPU test holds the two equal)."""
    h, w = float(c["h"]), float(c["w"])
    ratio = (3.0 / 4.0, 4.0 / 3.0)
    in_ratio = w / h
    fw, fh = (w, round(w / ratio[0])) if in_ratio < ratio[0] else (round(h * ratio[1]), h) if in_ratio > ratio[1] else (w, h)
    return [c["scale"][0], c["scale"][1], ratio[0], ratio[1], 0.4, 0.4, 0.4, 0.1, 0.8, 0.2, float(fw), float(fh)]


def aug_params_case_inputs(c):
    """u [n, 30] float32 in [0, 1 - 2^-24] (what torch.rand can return).  special='extremes': the first rows are all 0, all 1 - 2^-24, and
    a drawn crop with the ten other draws all 0 / all 1 - 2^-24."""
    rng = np.random.default_rng(c["seed"])
    u = (rng.integers(0, 1 << 24, (c["n"], NUNIFORM)).astype(np.float64) * U).astype(np.float32)
    if c.get("special") == "extremes":
        top = np.float32(1.0 - U)
        u[0], u[1] = 0.0, top
        u[2, 2 * TRIES:], u[3, 2 * TRIES:] = 0.0, top
    return u
