"""GPU: every convolution, weight-gradient and BatchNorm kernel form of the engine, one layer at a time, against a float64 reference
(torch CPU), through the single-layer hooks of csrc/layer_api.hip (ocl_test_*).

Tier 1 (integer-exact).  Every fp32 MFMA of the engine is exact fp32 (v_mfma_f32_16x16x4_f32 and the 4x4x1 form: each product rounds
like an fmaf chain, no reduced-precision path), so with small-integer inputs, weights and gradients -- every partial sum below 2^24 --
every form's result is exact whatever its tiling and summation order.  Outputs and weight gradients are compared for BIT equality with
the float64 reference: a dropped, doubled or misplaced product, tile, tap or channel quad is an O(1) error.  One case per form in
layer_forms.COVERED (the cheapest pass / layer the planner gives it at; tests/test_cpu_forms.py checks that list against the planner);
each case asserts that the hook ran the form it names.  The same case bodies run every form at its edge sizes -- most images, odd
images per group, the other lattices -- in tests/test_gpu_form_grid.py.  Sentinel inputs (non-zero only in the last image, the last pixel, the border,
the last channel quad) make a dropped tile visible even where the rest of the tensor would hide it.

Tier 2 (random fp32): |got - ref| <= 1.01 * K * 2^-24 * sum|x * w| per element (a bound an exact-fp32 kernel cannot exceed), and the
RMS error no worse than 4x that of a plain fp32 CPU computation of the same data: a bf16 / tf32 shortcut in any form fails it.  The
input transform (xf: the producer's BatchNorm + ReLU applied while staging) and the BatchNorm kernels are checked this way against
float64 BatchNorm; a ReLU decision is only allowed to differ where the pre-activation is within fp32 round-off of zero."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_forms as LF
from guarded import FILL, SLACK, assert_slack_untouched, dev   # (shared with test_gpu_small_ops.py)

pytestmark = pytest.mark.gpu

EPI_STATS, EPI_AFFINE, EPI_RES, EPI_RESMASK, EPI_RELU, EPI_ACCUM, EPI_BNB = 1, 2, 4, 8, 16, 32, 64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    yield L
    L.ocl_set_deterministic(0)


def cells(reps_groups_c):
    """Zeroed accumulator cells: [8][groups][2][C] of 16 bytes (as int64 pairs)."""
    g, c = reps_groups_c
    return torch.zeros(8 * g * 2 * c * 2 + SLACK, dtype=torch.int64, device="cuda")


def cell_totals(cells_t, groups, c, det):
    """The totals of [8][groups][2][c] cells, decoded as the kernels do (fx_total): [groups, 2, c] float64."""
    raw = cells_t[: 8 * groups * 2 * c * 2].cpu().numpy().reshape(8, groups, 2, c, 2)
    if not det:
        return raw[..., 0].copy().view(np.float64).sum(axis=0)
    lo = raw[..., 0].view(np.uint64).sum(axis=0, dtype=np.uint64)
    hi = raw[..., 1].sum(axis=0)
    out = hi.astype(np.float64) / 256.0 + lo.astype(np.float64) / 2.0 ** 40
    out[(hi >= 2 ** 55) | (hi <= -2 ** 55)] = np.nan
    return out


def encode_cells(tot, det):
    """[groups, 2, c] float64 totals as cells (replica 0 holds them): what a producer's EPI_STATS launch would have left."""
    g, _, c = tot.shape
    raw = np.zeros((8, g, 2, c, 2), dtype=np.int64)
    if not det:
        raw[0, ..., 0] = tot.astype(np.float64).view(np.int64)
    else:
        q = tot * 2.0 ** 40
        h = np.floor(q / 2.0 ** 32)
        raw[0, ..., 1] = h.astype(np.int64)
        raw[0, ..., 0] = (q - h * 2.0 ** 32).astype(np.uint64).view(np.int64)
    t = torch.zeros(raw.size + SLACK, dtype=torch.int64, device="cuda")
    t[: raw.size].copy_(torch.from_numpy(raw.reshape(-1)))
    return t


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ints(shape, gen, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def shape_of(d):
    pad = 1 if d.k == 3 else 0
    ho = (d.hin + 2 * pad - d.k) // d.stride + 1
    wo = (d.win + 2 * pad - d.k) // d.stride + 1
    return (4 if d.cin == 3 else d.cin), ho, wo, pad


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def ref_fwd(x, w, d):
    """x [n,h,w,cinT] float64 (NHWC), w [cout,cin,k,k] float64 -> y NHWC float64."""
    return nhwc(F.conv2d(nchw(x[..., : d.cin]), w, stride=d.stride, padding=1 if d.k == 3 else 0))


def ref_dgrad(dy, w, d):
    """dy NHWC [n,ho,wo,cout] -> dx NHWC [n,hin,win,cin] (autograd of the float64 convolution)."""
    pad = 1 if d.k == 3 else 0
    return nhwc(torch.nn.grad.conv2d_input((dy.shape[0], d.cin, d.hin, d.win), w, nchw(dy), stride=d.stride, padding=pad))


def ref_wgrad(x, dy, d):
    pad = 1 if d.k == 3 else 0
    return torch.nn.grad.conv2d_weight(nchw(x[..., : d.cin]), (d.cout, d.cin, d.k, d.k), nchw(dy), stride=d.stride, padding=pad)


def run_conv(lib, d, x, w, flags=0, out0=None, **ops):
    """One layer through ocl_test_conv: returns (out float64 NHWC, forms, stats cells or None)."""
    from ocl_amd import ffi
    cinT, ho, wo, _ = shape_of(d)
    oshape = (d.n, ho, wo, d.cout) if d.dir == 0 else (d.n, d.hin, d.win, d.cin)
    if out0 is None and d.dir == 1 and d.k == 1 and d.stride == 2:
        out0 = torch.zeros(oshape)   # (the 1x1 stride-2 data gradient writes the even pixels only; the engine accumulates it onto dx)
    out = dev(out0.float() if out0 is not None else torch.full(oshape, float("nan")))
    o = ffi.TestConvOps()
    keep = [dev(x.float()), dev(w.float()), out]
    o.in_, o.w, o.out, o.flags = p(keep[0]), p(keep[1]), p(out), flags
    stats = None
    if flags & (EPI_STATS | EPI_BNB):
        stats = cells(((d.groups if (d.dir == 0 or d.bnb) else 1), oshape[3]))
        o.stats = p(stats)
    for k, v in ops.items():
        if isinstance(v, torch.Tensor):
            t = v if v.is_cuda else dev(v.float() if v.is_floating_point() else v)
            keep.append(t)
            setattr(o, k, p(t))
        else:
            setattr(o, k, v)
    forms = (ffi.TestConvForm * 4)()
    n = lib.ocl_test_conv(C.byref(d), C.byref(o), forms, 4, None)
    assert n > 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    assert_slack_untouched(out, "conv output")
    return out.double().cpu(), [forms[i] for i in range(n)], stats


def run_wgrad(lib, descs, xs, dys, multi=0, accumulate=0, grad0=None, xf_ops=None):
    from ocl_amd import ffi
    n = len(descs)
    sizes = [d.cout * d.cin * d.k * d.k for d in descs]
    flat = torch.full((sum(sizes) + SLACK,), float(FILL), device="cuda")
    flat[: sum(sizes)].zero_()
    if grad0 is not None:
        flat[: sum(sizes)].copy_(torch.cat([g.reshape(-1) for g in grad0]).float())
    arr_d = (ffi.TestWgradDesc * n)(*descs)
    arr_o = (ffi.TestWgradOps * n)()
    keep, off = [], 0
    for i in range(n):
        xt, dyt = dev(xs[i].float()), dev(dys[i].float())
        keep += [xt, dyt]
        arr_o[i].x, arr_o[i].dy = p(xt), p(dyt)
        arr_o[i].grad = C.c_void_p(flat.data_ptr() + 4 * off)
        if xf_ops is not None:
            arr_o[i].xf = 1
            for k, v in xf_ops[i].items():
                t = dev(v.float())
                keep.append(t)
                setattr(arr_o[i], k, p(t))
        off += sizes[i]
    forms = (ffi.TestWgradForm * n)()
    rc = lib.ocl_test_wgrad(arr_d, arr_o, n, multi, accumulate, forms, None)
    assert rc == 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    assert bool((flat[sum(sizes):] == FILL).all()), "weight gradient written past the end"
    out, off = [], 0
    for i, d in enumerate(descs):
        out.append(flat[off: off + sizes[i]].double().cpu().view(d.cout, d.cin, d.k, d.k))
        off += sizes[i]
    return out, [forms[i] for i in range(n)]


def find_entry(lib, key):
    hw, n, g, layer, dr = LF.COVERED[key]
    train = 0 if key.endswith("/affine") else 1
    for k, e in LF.net_forms(lib, hw, n, g, train):
        if k == key and e.layer == layer and e.dir == dr:
            return e
    raise AssertionError("the planner no longer gives %s at %r: regenerate layer_forms.COVERED" % (key, LF.COVERED[key]))


def assert_exact(got, ref, what):
    bad = (got != ref)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ (first at %s: got %r, want %r)" % (
            what, int(bad.sum()), bad.numel(), idx, float(got[tuple(idx)]), float(ref[tuple(idx)])))


def stats_ref(y, groups):
    """y NHWC float64 -> [groups, 2, C] sums / sums of squares."""
    n = y.shape[0]
    yg = y.reshape(groups, n // groups, -1, y.shape[-1])
    return torch.stack([yg.sum(dim=(1, 2)), (yg * yg).sum(dim=(1, 2))], dim=1).numpy()


def check_stats(got, ref, absref, what):
    # sums of integers are exact in float64 whatever the order, but a kernel keeps a per-lane / per-tile partial in fp32 first (sums of squares
    # of integers up to 5760^2 are not exact in fp32), and tests/test_gpu_bn_cond.py uses the same limit on real-valued outputs: the sums are
    # bounded by fp32 roundings of the sum of magnitudes instead of bit equality.  The 8 is a budget of eight such roundings (8 * 2^-24 * sum|.|),
    # not a worst case: a partial of L terms followed by the 16-lane butterfly can lose (L / 16 + 4) roundings in the worst case, but the
    # roundings of a sum do not line up -- a float64 model of the design with partials of 16 - 256 values stays inside it on every regime of
    # tests/bn_cond_cases.py (tests/test_cpu_bn_cond.py) and the kernels measure below 1 (profiles/bn_cond_parity.txt), while a product or
    # a partial kept in a narrower format, or a dropped pixel, is off by orders of magnitude more
    err = np.abs(got - ref)
    lim = 8 * U * absref + 1e-9
    assert np.all(err <= lim), "%s: batch sums off by %g (limit %g)" % (what, float((err - lim).max()), float(lim.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# tier 1: one exact case per planner form
# ---------------------------------------------------------------------------------------------------------------------------------
CONV_KEYS = sorted(k for k in LF.COVERED if not k.startswith("wg"))
# tier 1 in the default batch-sum mode for every key, and in deterministic mode (fixed-point cells; conv_s_kernel's MODE = 1 build) for
# every key whose epilogue accumulates batch sums
EXACT_CASES = [(k, 0) for k in LF.EXACT_CONV_KEYS] + [(k, 1) for k in LF.EXACT_CONV_KEYS if k.endswith("/stats") or k.endswith("/bnb")]


def _case_data(d, seed):
    g = torch.Generator().manual_seed(seed)
    cinT, ho, wo, _ = shape_of(d)
    w = ints((d.cout, d.cin, d.k, d.k), g)
    if d.dir == 0:
        x = ints((d.n, d.hin, d.win, cinT), g)
        if d.cin == 3:
            x[..., 3] = 0
    else:
        x = ints((d.n, ho, wo, d.cout), g)
    return x, w, g


@pytest.mark.parametrize("key,det", EXACT_CASES)
def test_conv_form_is_exact(lib, key, det):
    lib.ocl_set_deterministic(det)
    try:
        _conv_form_is_exact(lib, key, det)
    finally:
        lib.ocl_set_deterministic(0)


def _conv_form_is_exact(lib, key, det):
    e = find_entry(lib, key)
    d = e.desc
    x, w, g = _case_data(d, zlib.crc32(key.encode()) % 10007)
    epi = key.split("/")[1]
    ops, flags, out0 = {}, 0, None
    if d.dir == 0:
        ref = ref_fwd(x, w, d)
    else:
        ref = ref_dgrad(x, w, d)
    C_out = ref.shape[-1]
    if epi == "stats":
        flags = EPI_STATS
    elif epi == "affine":   # eval-mode BatchNorm folded: power-of-two scale, integer shift, + residual, ReLU
        scale = 2.0 ** torch.randint(-1, 2, (C_out,), generator=g).double()
        shift = ints((C_out,), g, -3, 3)
        res = ints(ref.shape, g)
        flags = EPI_AFFINE | EPI_RES | EPI_RELU
        ops.update(scale=scale, shift=shift, res=res)
        ref = torch.clamp(ref * scale + shift + res, min=0)
    elif epi == "plain":   # the data gradient's epilogues in turn
        variant = sum(map(ord, key)) % 3
        if variant == 1:
            out0 = ints(ref.shape, g)
            flags = EPI_ACCUM
            ref = ref + out0
        elif variant == 2:
            res, mask = ints(ref.shape, g), ints(ref.shape, g)
            flags = EPI_RESMASK
            ops.update(res=res, resmask=mask)
            ref = ref + res * (mask > 0)
    elif epi == "bnb":   # masked gradient d = dx * (z > 0) + sum(d), sum(d * (y - mean)) with mean 0: integers throughout
        y, z = ints(ref.shape, g), ints(ref.shape, g)
        G = d.groups
        zeros = torch.zeros(G, C_out)
        ops.update(bnb_y=y, bnb_z=z, bnb_mean=zeros, bnb_invstd=torch.ones(G, C_out), bnb_gamma=torch.ones(C_out),
                   bnb_beta=torch.zeros(C_out))
        flags = EPI_BNB
        ref = ref * (z > 0)
    full_ref = ref
    if d.dir == 1 and d.k == 1 and d.stride == 2:   # only the even pixels are written (and get the epilogue); the rest keep their value
        init = out0 if out0 is not None else torch.zeros(ref.shape, dtype=torch.float64)
        ref = init.clone()
        ref[:, ::2, ::2] = full_ref[:, ::2, ::2]
    got, forms, stats = run_conv(lib, d, x, w, flags, out0, **ops)
    keys = [LF.conv_key(f, epi) for f in forms]
    print("FORM", key, "ran", keys, "n=%d groups=%d layer=%d det=%d" % (d.n, d.groups, e.layer, det))
    assert key in keys, (key, keys)
    assert_exact(got, ref, key)
    if epi == "stats":
        check_stats(cell_totals(stats, d.groups, C_out, det), stats_ref(ref, d.groups), stats_ref(ref.abs(), d.groups), key)
    if epi == "bnb":
        G = d.groups
        n = ref.shape[0]
        dg = ref.reshape(G, n // G, -1, C_out)
        yg = y.reshape(G, n // G, -1, C_out)
        want = torch.stack([dg.sum(dim=(1, 2)), (dg * yg).sum(dim=(1, 2))], dim=1).numpy()
        mag = torch.stack([dg.abs().sum(dim=(1, 2)), (dg * yg).abs().sum(dim=(1, 2))], dim=1).numpy()
        check_stats(cell_totals(stats, G, C_out, det), want, mag, key)


@pytest.mark.parametrize("key", LF.WGRAD_KEYS)
def test_wgrad_form_is_exact(lib, key):
    _wgrad_form_is_exact(lib, key, ".m" in key)


def _wgrad_form_is_exact(lib, key, merged):
    """merged: through conv_wgrad_multi_kernel (a '.m' key's own launch), or the layer's plan as a launch of its own."""
    e = find_entry(lib, key)
    d = e.wdesc
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) % 10007)
    cinT, ho, wo, _ = shape_of(d)
    x = ints((d.n, d.hin, d.win, cinT), g)
    if d.cin == 3:
        x[..., 3] = 0
    dy = ints((d.n, ho, wo, d.cout), g)
    ref = ref_wgrad(x, dy, d)
    xf_ops = None
    if key.endswith("/xf"):   # transform with gamma 1, beta 0, mean 0, invstd 1: relu(x) staged, still exact
        G = d.xf_groups
        xf_ops = [dict(xf_mean=torch.zeros(G, cinT), xf_invstd=torch.ones(G, cinT), xf_gamma=torch.ones(cinT), xf_beta=torch.zeros(cinT))]
        ref = ref_wgrad(torch.clamp(x, min=0), dy, d)
    acc = sum(map(ord, key)) % 2
    grad0 = [ints(ref.shape, g)] if acc else None
    got, forms = run_wgrad(lib, [d], [x], [dy], multi=1 if merged else 0, accumulate=acc, grad0=grad0, xf_ops=xf_ops)
    k = LF.wgrad_key(forms[0], xf_ops is not None, ".m" in key)
    print("FORM", key, "ran", k, "n=%d layer=%d accumulate=%d merged=%d" % (d.n, e.layer, acc, merged))
    assert k == key
    assert_exact(got[0], ref + (grad0[0] if acc else 0), key)


def test_wgrad_multi_launch_of_a_whole_pass_is_exact(lib):
    """All layers of a 20-image pass whose weight gradients leave in one conv_wgrad_multi_kernel launch per form set, as the engine does."""
    ents = [e for k, e in LF.net_forms(lib, 32, 20, 2, 1) if e.dir == 2 and e.wg_merged and e.wform.multi >= 0]
    g = torch.Generator().manual_seed(3)
    for s in (0, 1):
        grp = [e for e in ents if e.wform.multi // 4 == s]
        if len(grp) < 2:
            continue
        descs, xs, dys, refs = [], [], [], []
        for e in grp:
            d = type(e.wdesc).from_buffer_copy(e.wdesc)   # (xf_groups kept: the plan's LDS as in the pass; the transform is not applied)
            cinT, ho, wo, _ = shape_of(d)
            x = ints((d.n, d.hin, d.win, cinT), g)
            if d.cin == 3:
                x[..., 3] = 0
            dy = ints((d.n, ho, wo, d.cout), g)
            descs.append(d); xs.append(x); dys.append(dy); refs.append(ref_wgrad(x, dy, d))
        got, forms = run_wgrad(lib, descs, xs, dys, multi=1)
        print("FORM multi set", s, [f.multi for f in forms])
        for i in range(len(grp)):
            assert_exact(got[i], refs[i], "multi set %d layer %d" % (s, grp[i].layer))


# ---------------------------------------------------------------------------------------------------------------------------------
# sentinels and batch sizes: a dropped or doubled tile must be an O(1) error
# ---------------------------------------------------------------------------------------------------------------------------------
def _desc(cin, cout, k, stride, hw, n, groups=1, dr=0, **kw):
    from ocl_amd import ffi
    d = ffi.TestConvDesc(cin=cin, cout=cout, k=k, stride=stride, hin=hw, win=hw, n=n, groups=groups, dir=dr, merge=1)
    for a, v in kw.items():
        setattr(d, a, v)
    return d


# every Reduced-ResNet18 layer shape at 32 x 32 / 84 x 84: the stem, 3x3 stride 1 at 20 .. 160 channels, 3x3 stride 2, the 1x1
# stride-2 shortcut
LAYER_SHAPES = [(3, 20, 3, 1), (20, 20, 3, 1), (20, 40, 3, 2), (20, 40, 1, 2), (40, 40, 3, 1), (40, 80, 3, 2), (80, 80, 3, 1),
                (80, 160, 3, 2), (80, 160, 1, 2), (160, 160, 3, 1)]
HW_AT = {20: 1, 40: 2, 80: 4, 160: 8}   # input size divisor of the layer's input


def _sentinel(shape, kind, gen):
    """A tensor [n, h, w, c] of small integers that is zero except where `kind` puts it."""
    n, h, w, c = shape
    t = torch.zeros(shape, dtype=torch.float64)
    v = ints(shape, gen)
    v[v == 0] = 1
    if kind == "last_image":
        t[-1] = v[-1]
    elif kind == "last_pixel":
        t[-1, -1, -1] = v[-1, -1, -1]
    elif kind == "border":
        t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]
    elif kind == "last_quad":
        t[..., c - 4:] = v[..., c - 4:]
    return t


@pytest.mark.parametrize("kind", ["last_image", "last_pixel", "border", "last_quad"])
@pytest.mark.parametrize("n,groups", [(1, 1), (7, 1), (13, 1), (10, 2), (22, 2)])
def test_sentinels_every_layer_shape(lib, kind, n, groups):
    hw0 = 32
    g = torch.Generator().manual_seed(n * 31 + len(kind))
    for cin, cout, k, stride in LAYER_SHAPES:
        hw = hw0 // HW_AT.get(cin, 1)
        for dr in (0, 1, 2):
            if dr == 1 and cin == 3:
                continue
            d = _desc(cin, cout, k, stride, hw, n, groups, min(dr, 1))
            cinT, ho, wo, _ = shape_of(d)
            w = ints((cout, cin, k, k), g)
            if dr == 0:
                x = _sentinel((n, hw, hw, cinT), kind, g)
                if cin == 3:
                    x[..., 3] = 0
                got, forms, _ = run_conv(lib, d, x, w)
                assert_exact(got, ref_fwd(x, w, d), "fwd %s %r" % (kind, (cin, cout, k, stride)))
            elif dr == 1:
                dy = _sentinel((n, ho, wo, cout), kind, g)
                got, forms, _ = run_conv(lib, d, dy, w)
                assert_exact(got, ref_dgrad(dy, w, d), "dgrad %s %r" % (kind, (cin, cout, k, stride)))
            else:
                from ocl_amd import ffi
                wd = ffi.TestWgradDesc(cin=cin, cout=cout, k=k, stride=stride, hin=hw, win=hw, n=n)
                x = _sentinel((n, hw, hw, cinT), kind, g) if kind != "last_quad" else ints((n, hw, hw, cinT), g)
                if cin == 3:
                    x[..., 3] = 0
                dy = _sentinel((n, ho, wo, cout), kind, g)
                got, _ = run_wgrad(lib, [wd], [x], [dy])
                assert_exact(got[0], ref_wgrad(x, dy, wd), "wgrad %s %r" % (kind, (cin, cout, k, stride)))


@pytest.mark.parametrize("hw,n,groups", [(84, 3, 1), (32, 220, 2)])
def test_large_pass_every_layer_shape_exact(lib, hw, n, groups):
    """84 x 84 and the 220-view pass in two groups (odd images per group: 3, and 110 / 2 ... ) on every layer shape, every direction."""
    g = torch.Generator().manual_seed(hw + n)
    for cin, cout, k, stride in LAYER_SHAPES:
        h = hw // HW_AT.get(cin, 1)
        if hw == 84 and cin > 20:
            h = {40: 42, 80: 21, 160: 11}[cin]
        d = _desc(cin, cout, k, stride, h, n, groups, 0)
        cinT, ho, wo, _ = shape_of(d)
        w = ints((cout, cin, k, k), g)
        x = ints((n, h, h, cinT), g)
        if cin == 3:
            x[..., 3] = 0
        got, _, _ = run_conv(lib, d, x, w)
        assert_exact(got, ref_fwd(x, w, d), "fwd %r" % ((cin, cout, k, stride),))
        dy = ints((n, ho, wo, cout), g)
        if cin != 3:
            for merge in (1, 0):
                dd = _desc(cin, cout, k, stride, h, n, groups, 1, merge=merge)
                got, forms, _ = run_conv(lib, dd, dy, w)
                assert_exact(got, ref_dgrad(dy, w, dd), "dgrad merge=%d %r" % (merge, (cin, cout, k, stride)))
        from ocl_amd import ffi
        wd = ffi.TestWgradDesc(cin=cin, cout=cout, k=k, stride=stride, hin=h, win=h, n=n)
        got, _ = run_wgrad(lib, [wd], [x], [dy])
        assert_exact(got[0], ref_wgrad(x, dy, wd), "wgrad %r" % ((cin, cout, k, stride),))


@pytest.mark.parametrize("force", [dict(force_cs=1), dict(force_q4=1), dict(force_cw=1), dict(force_pipe=-1, force_cs=-1, force_q4=-1, force_cw=-1),
                                   dict(force_mt=1, force_nt=2, force_cs=-1, force_q4=-1, force_cw=-1)])
def test_forced_forms_exact(lib, force):
    """Forms the planner reaches only when forced (benchmarks, A/B references), where they fit."""
    g = torch.Generator().manual_seed(11)
    ran = set()
    for cin, cout, k, stride in LAYER_SHAPES:
        hw = 32 // HW_AT.get(cin, 1)
        for dr in (0, 1):
            if dr == 1 and cin == 3:
                continue
            d = _desc(cin, cout, k, stride, hw, 6, 1, dr, **force)
            if lib.ocl_test_conv_plan(C.byref(d), None, 0) <= 0:
                continue
            x, w, _ = _case_data(d, 5)
            got, forms, _ = run_conv(lib, d, x, w)
            ran.update(LF.conv_key(f, "forced") for f in forms)
            assert_exact(got, (ref_fwd if dr == 0 else ref_dgrad)(x, w, d), "%r %r dir %d" % (force, (cin, cout, k, stride), dr))
    print("FORM forced", force, sorted(ran))
    assert ran


# ---------------------------------------------------------------------------------------------------------------------------------
# tier 2: random fp32
# ---------------------------------------------------------------------------------------------------------------------------------
def _bound_check(got, ref64, mag, K, cpu32, what):
    err = (got - ref64).abs()
    lim = 1.01 * K * U * mag
    assert bool((err <= lim).all()), "%s: error %g above the exact-fp32 bound" % (what, float((err - lim).max()))
    rms, rms32 = float(err.pow(2).mean().sqrt()), float((cpu32 - ref64).abs().pow(2).mean().sqrt())
    assert rms <= 4 * rms32 + 1e-30, "%s: RMS error %g vs fp32 CPU %g" % (what, rms, rms32)


# (every third /plain and /stats key of the grid before it became dense, and one key of each family the dense grid added)
TIER2_KEYS = ['q1.pf12/plain', 'q2.pf12/stats', 's1/stats', 't1x1.res.c1.pf4/plain', 't1x1.res.c1.pf8/stats', 't1x1.ring.c1.pf4/stats',
              't1x1.ring.c4.pf4/plain', 't1x1.two.c4.pf8/plain', 't2x1.res.c1.pf8/plain', 't2x1.res.c4.pf8/plain', 't2x1.ring.c1.pf8/stats',
              't2x2.two.c1.pf8/plain', 't3x1.ring.c1.pf4/stats', 't3x1.ring.c4.pf8/plain', 't3x2.two.c1.pf8/stats', 't5x1.ring.c1.pf8/stats',
              't5x2.two.c1.pf8/plain', 'wx1x1/stats', 't2x1.two.c4.pf8/plain', 't4x1.two.c1.pf8/stats', 't5x1.res.c1.pf8/plain',
              "wg3x2.pf8/plain", "wgq3.pf8/plain", "wg1x2.pf8/plain"]


@pytest.mark.parametrize("key", TIER2_KEYS)
def test_random_fp32_within_the_exact_fp32_bound(lib, key):
    e = find_entry(lib, key)
    g = torch.Generator().manual_seed(7)
    if key.startswith("wg"):
        d = e.wdesc
        cinT, ho, wo, _ = shape_of(d)
        x = torch.randn((d.n, d.hin, d.win, cinT), generator=g, dtype=torch.float64).float().double()
        if d.cin == 3:
            x[..., 3] = 0
        dy = torch.randn((d.n, ho, wo, d.cout), generator=g, dtype=torch.float64).float().double()
        got, _ = run_wgrad(lib, [d], [x], [dy])
        ref = ref_wgrad(x, dy, d)
        mag = ref_wgrad(x.abs(), dy.abs(), d)
        cpu32 = ref_wgrad(x.float(), dy.float(), d).double()
        _bound_check(got[0], ref, mag, d.n * ho * wo, cpu32, key)
        return
    d = e.desc
    cinT, ho, wo, _ = shape_of(d)
    w = (torch.randn((d.cout, d.cin, d.k, d.k), generator=g, dtype=torch.float64) * 0.1).float().double()
    if d.dir == 0:
        x = torch.randn((d.n, d.hin, d.win, cinT), generator=g, dtype=torch.float64).float().double()
        if d.cin == 3:
            x[..., 3] = 0
        f, K = ref_fwd, d.k * d.k * d.cin
    else:
        x = torch.randn((d.n, ho, wo, d.cout), generator=g, dtype=torch.float64).float().double()
        f, K = ref_dgrad, d.k * d.k * d.cout
    got, forms, _ = run_conv(lib, d, x, w)
    _bound_check(got, f(x, w, d), f(x.abs(), w.abs(), d), K, f(x.float(), w.float(), d).double(), key)


def _bn_ref(y, groups, gamma, beta, eps=1e-5):
    """float64 train-mode BatchNorm per group: z, mean, invstd, unbiased var."""
    n = y.shape[0]
    yg = y.reshape(groups, -1, y.shape[-1])
    mean = yg.mean(dim=1)
    var = yg.var(dim=1, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    z = ((yg - mean[:, None]) * invstd[:, None] * gamma + beta).reshape(y.shape)
    return z, mean, invstd, yg.var(dim=1, unbiased=True)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("key", LF.XF_KEYS)
def test_input_transform_against_float64_batchnorm(lib, key, det):
    """conv2 of a block applies bn1 + ReLU of conv1's raw output while staging, from conv1's batch sums (EPI_STATS cells), and writes
    bn1's saved statistics and running statistics on the way."""
    _input_transform_against_float64_batchnorm(lib, key, det)


def _input_transform_against_float64_batchnorm(lib, key, det):
    """Returns the worst error / bound over the outputs that are held to the bound (for the parity reports)."""
    e = find_entry(lib, key)
    d = e.desc
    lib.ocl_set_deterministic(det)
    try:
        g = torch.Generator().manual_seed(13 + det)
        cinT, ho, wo, _ = shape_of(d)
        G = d.groups
        y = (torch.randn((d.n, d.hin, d.win, cinT), generator=g, dtype=torch.float64) * 2 + 0.3).float().double()
        w = (torch.randn((d.cout, d.cin, 3, 3), generator=g, dtype=torch.float64) * 0.1).float().double()
        gamma = (1 + 0.1 * torch.randn(cinT, generator=g, dtype=torch.float64)).float().double()
        beta = (0.1 * torch.randn(cinT, generator=g, dtype=torch.float64)).float().double()
        xf_stats = encode_cells(stats_ref(y, G), det)
        z, mean, invstd, uvar = _bn_ref(y, G, gamma, beta)
        a = torch.clamp(z, min=0)
        sm, si = dev(torch.zeros(G, cinT)), dev(torch.zeros(G, cinT))
        rm, rv, nbt = dev(torch.zeros(cinT)), dev(torch.ones(cinT)), dev(torch.zeros(1, dtype=torch.int64))
        got, forms, stats = run_conv(lib, d, y, w, EPI_STATS, xf=1, xf_stats=xf_stats, xf_gamma=gamma, xf_beta=beta, xf_save_mean=sm,
                                     xf_save_invstd=si, xf_running_mean=rm, xf_running_var=rv, xf_nbt=nbt)
        assert key in [LF.conv_key(f, "stats_xf") for f in forms]
        np.testing.assert_allclose(sm.double().cpu().numpy(), mean.numpy(), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(si.double().cpu().numpy(), invstd.numpy(), rtol=1e-5)
        # running statistics: momentum 0.1, applied once per group in group order, the unbiased variance
        erm, erv = torch.zeros(cinT, dtype=torch.float64), torch.ones(cinT, dtype=torch.float64)
        for gi in range(G):
            erm, erv = 0.9 * erm + 0.1 * mean[gi], 0.9 * erv + 0.1 * uvar[gi]
        np.testing.assert_allclose(rm.double().cpu().numpy(), erm.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rv.double().cpu().numpy(), erv.numpy(), rtol=1e-5, atol=1e-6)
        assert int(nbt[0]) == G
        ref = ref_fwd(a, w, d)
        mag = ref_fwd(a, w.abs(), d)
        # a ReLU decision may only differ where the pre-activation is within fp32 round-off of zero: those outputs are excluded; elsewhere
        # the transformed input carries the saved statistics' float32 rounding (relative ~1e-6 of its terms) besides the fp32 products
        mb = mean.repeat_interleave(d.n // G, 0)[:, None, None, :]
        ib = invstd.repeat_interleave(d.n // G, 0)[:, None, None, :]
        terms = (y.abs() + mb.abs()) * ib * gamma.abs() + beta.abs()
        amb = (z.abs() <= 1e-5 * terms).double()
        hit = ref_fwd(amb, torch.ones_like(w), d) > 0
        err = (got - ref).abs()
        lim = 2e-5 * ref_fwd(terms, w.abs(), d) + 1.01 * d.k * d.k * d.cin * U * mag
        bad = (err > lim) & ~hit
        assert not bool(bad.any()), "%s: %d outputs off (worst %g)" % (key, int(bad.sum()), float((err - lim)[bad].max()))
        check_stats(cell_totals(stats, G, d.cout, det), stats_ref(got, G), stats_ref(got.abs(), G), key)
        return float((err / lim.clamp(min=1e-300))[~hit].max())
    finally:
        lib.ocl_set_deterministic(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _err_ratio(got, ref, rtol, atol):
    """Worst |got - ref| / (atol + rtol * |ref|): what assert_allclose holds below 1 (printed for the parity records)."""
    got, ref = got.double().cpu().numpy(), ref.numpy()
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def _bn_case(g, n, hw, c, groups):
    y = (torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64) * 1.5 + 0.2).float().double()
    gamma = (1 + 0.2 * torch.randn(c, generator=g, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(c, generator=g, dtype=torch.float64)).float().double()
    return y, gamma, beta


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups,two,frozen", [(10, 32, 20, 2, False, False), (7, 16, 40, 1, True, False), (22, 8, 80, 2, True, False),
                                                     (5, 4, 160, 1, False, True), (3, 11, 160, 1, True, True),
                                                     # three and eight groups: one running-statistics update per group, in group order
                                                     (6, 4, 160, 3, True, False), (8, 8, 20, 8, False, False), (8, 4, 20, 8, True, False)])
def test_bn_forward_against_float64(lib, det, n, hw, c, groups, two, frozen):
    from ocl_amd import ffi
    lib.ocl_set_deterministic(det)
    try:
        g = torch.Generator().manual_seed(n + c)
        y, gamma, beta = _bn_case(g, n, hw, c, groups)
        yb, gb, bb = _bn_case(g, n, hw, c, groups)
        if groups > 2:
            # group means of alternating sign and growing size (-1, 2, -3, ...): the running recurrence weighs group i by 0.1 * 0.9^(G - 1 - i),
            # so an update in another order, or one that stops early, is off by far more than the bound
            off = torch.tensor([(-1.0) ** (i + 1) * (i + 1) for i in range(groups)], dtype=torch.float64).repeat_interleave(n // groups)
            y, yb = (y + off[:, None, None, None]).float().double(), (yb - 0.5 * off[:, None, None, None]).float().double()
        a = ffi.TestBnFwdArgs(m_per_group=n // groups * hw * hw, groups=groups, c=c, relu=1, momentum=0.1, eps=1e-5)
        keep = {}

        def put(name, t):
            keep[name] = t if (isinstance(t, torch.Tensor) and t.is_cuda) else dev(t.float() if t.is_floating_point() else t)
            setattr(a, name, p(keep[name]))
        z = dev(torch.full(y.shape, float("nan")))
        put("y", y); put("z", z); put("gamma", gamma); put("beta", beta)
        st = encode_cells(stats_ref(y, groups), det)
        keep["st"] = st
        a.stats = p(st)
        for s in ("", "_b") if two else ("",):
            put("running_mean" + s, torch.zeros(c)); put("running_var" + s, torch.ones(c)); put("nbt" + s, torch.zeros(1, dtype=torch.int64))
            put("save_mean" + s, torch.zeros(groups, c)); put("save_invstd" + s, torch.zeros(groups, c))
        fm = fv = fmb = fvb = None
        if frozen:
            fm, fv = 0.1 * torch.randn(c, generator=g, dtype=torch.float64), 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
            fm, fv = fm.float().double(), fv.float().double()
            put("frozen_mean", fm); put("frozen_var", fv)
            a.running_mean = a.running_var = a.nbt = None
        if two:
            put("yb", yb); put("gamma_b", gb); put("beta_b", bb)
            stb = encode_cells(stats_ref(yb, groups), det)
            keep["stb"] = stb
            a.stats_b = p(stb)
            if frozen:
                fmb, fvb = (0.1 * torch.randn(c, generator=g, dtype=torch.float64)).float().double(), (0.5 + torch.rand(c, generator=g, dtype=torch.float64)).float().double()
                put("frozen_mean_b", fmb); put("frozen_var_b", fvb)
                a.running_mean_b = a.running_var_b = a.nbt_b = None
        assert lib.ocl_test_bn_fwd(C.byref(a), None) == 0, lib.ocl_last_error()
        torch.cuda.synchronize()

        def norm(yy, gm, bt, fmean, fvar):
            if fmean is not None:
                return (yy - fmean) / torch.sqrt(fvar + 1e-5) * gm + bt, None, None, None
            zz, mean, invstd, uvar = _bn_ref(yy, groups, gm, bt)
            return zz, mean, invstd, uvar
        za, mean, invstd, uvar = norm(y, gamma, beta, fm, fv)
        want = za
        if two:
            zb, meanb, invstdb, uvarb = norm(yb, gb, bb, fmb, fvb)
            want = za + zb
        want = torch.clamp(want, min=0)
        got = z.double().cpu()
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
        if not frozen:
            np.testing.assert_allclose(keep["save_mean"].double().cpu().numpy(), mean.numpy(), rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(keep["save_invstd"].double().cpu().numpy(), invstd.numpy(), rtol=1e-5)
            erm, erv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
            for gi in range(groups):
                erm, erv = 0.9 * erm + 0.1 * mean[gi], 0.9 * erv + 0.1 * uvar[gi]
            print("BN fwd err / bound: z %.3f save_mean %.3f save_invstd %.3f running_mean %.3f running_var %.3f" % (
                _err_ratio(z, want, 2e-5, 2e-5), _err_ratio(keep["save_mean"], mean, 1e-6, 1e-6), _err_ratio(keep["save_invstd"], invstd, 1e-5, 0.0),
                _err_ratio(keep["running_mean"], erm, 1e-5, 1e-6), _err_ratio(keep["running_var"], erv, 1e-5, 1e-6)))
            np.testing.assert_allclose(keep["running_mean"].double().cpu().numpy(), erm.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(keep["running_var"].double().cpu().numpy(), erv.numpy(), rtol=1e-5, atol=1e-6)
            assert int(keep["nbt"][0]) == groups
    finally:
        lib.ocl_set_deterministic(0)


def _bn_bwd_ref(dz, zmask, y, groups, gamma, frozen_invstd=None):
    """float64 autograd of relu-masked train-mode BatchNorm per group: dy, dgamma, dbeta."""
    d = dz * (zmask > 0) if zmask is not None else dz
    c = y.shape[-1]
    yg, dg = y.reshape(groups, -1, c), d.reshape(groups, -1, c)
    if frozen_invstd is not None:
        return (d * gamma * frozen_invstd), None, None
    mean = yg.mean(dim=1, keepdim=True)
    invstd = 1.0 / torch.sqrt(yg.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
    xhat = (yg - mean) * invstd
    k1, k2 = dg.mean(dim=1, keepdim=True), (dg * xhat).mean(dim=1, keepdim=True)
    dy = (gamma * invstd * (dg - k1 - xhat * k2)).reshape(y.shape)
    return dy, (dg * xhat).sum(dim=(0, 1)), dg.sum(dim=(0, 1))


@pytest.mark.parametrize("det", [0, 1])
# want: the exact path (ocl_test_bn_bwd's code), from launch_bn_bwd's sizing on the MI355X's 256 CUs
@pytest.mark.parametrize("n,hw,c,groups,nsets,one_pass,want", [
    (4, 4, 160, 2, 1, 1, 1011), (8, 4, 160, 1, 2, 1, 1012),            # bn_bwd_chan_kernel<1, 1|2> (<= 512 pixels, >= 16 channel quads)
    (4, 16, 40, 1, 1, 1, 2031), (4, 16, 40, 1, 2, 1, 2032),            # bn_bwd_fused_kernel<3, 1|2>
    (2, 16, 20, 2, 2, 1, 2032),
    (6, 16, 40, 2, 1, 1, 2061), (10, 32, 20, 2, 2, 1, 2062),           # bn_bwd_fused_kernel<6, 1|2>
    (12, 16, 80, 1, 2, 1, 2062),
    (40, 32, 20, 2, 1, 1, 2121),                                       # bn_bwd_fused_kernel<12, 1>
    (10, 32, 20, 2, 1, 0, 3001), (10, 16, 40, 2, 2, 0, 3002),          # reduce + apply
    # three to eight groups: reduce + apply whatever one_pass says (the one-pass and per-channel kernels hold two groups), the sums of two
    # sets addressed [set][G][2][C]; the smallest maps, one or two images per group
    (3, 4, 160, 3, 1, 1, 3001), (8, 8, 20, 4, 1, 1, 3001), (8, 4, 160, 8, 1, 0, 3001), (16, 4, 20, 8, 1, 1, 3001),
    (6, 8, 20, 3, 2, 1, 3002), (4, 4, 160, 4, 2, 1, 3002), (8, 8, 160, 4, 2, 0, 3002),
    (10, 8, 160, 5, 2, 1, 3002), (5, 4, 20, 5, 2, 0, 3002), (8, 4, 20, 8, 2, 1, 3002)])
def test_bn_backward_paths_against_float64(lib, det, n, hw, c, groups, nsets, one_pass, want):
    from ocl_amd import ffi
    lib.ocl_set_deterministic(det)
    try:
        g = torch.Generator().manual_seed(n * 7 + c + nsets)
        dz = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
        zm = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
        a = ffi.TestBnBwdArgs(m_per_group=n // groups * hw * hw, groups=groups, c=c, nsets=nsets, one_pass=one_pass)
        keep = [dev(dz.float()), dev(zm.float())]
        a.dz, a.z = p(keep[0]), p(keep[1])
        refs = []
        for s in range(nsets):
            y, gamma, beta = _bn_case(g, n, hw, c, groups)
            _, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
            ts = [dev(t.float()) for t in (y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
            keep += ts
            for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts):
                getattr(a, f)[s] = t.data_ptr()
            refs.append((_bn_bwd_ref(dz, zm, y, groups, gamma), ts))
        path = lib.ocl_test_bn_bwd(C.byref(a), None)
        assert path >= 0, lib.ocl_last_error()
        print("BN path", path, "n=%d hw=%d c=%d groups=%d nsets=%d" % (n, hw, c, groups, nsets))
        assert path == want, (path, want)
        for (dy, dgm, dbt), ts in refs:
            print("BN bwd err / bound: dy %.3f dgamma %.3f dbeta %.3f" % (
                _err_ratio(ts[5], dy, 1e-4, 2e-5 * float(dy.abs().max())), _err_ratio(ts[6], dgm, 1e-4, 1e-4 * float(dgm.abs().max())),
                _err_ratio(ts[7], dbt, 1e-4, 1e-4 * float(dbt.abs().max()))))
            np.testing.assert_allclose(ts[5].double().cpu().numpy(), dy.numpy(), rtol=1e-4, atol=2e-5 * float(dy.abs().max()))
            np.testing.assert_allclose(ts[6].double().cpu().numpy(), dgm.numpy(), rtol=1e-4, atol=1e-4 * float(dgm.abs().max()))
            np.testing.assert_allclose(ts[7].double().cpu().numpy(), dbt.numpy(), rtol=1e-4, atol=1e-4 * float(dbt.abs().max()))
    finally:
        lib.ocl_set_deterministic(0)


def test_bn_backward_frozen_and_mask_from_y(lib):
    from ocl_amd import ffi
    g = torch.Generator().manual_seed(5)
    n, hw, c, groups = 6, 16, 40, 1
    dz = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
    y, gamma, beta = _bn_case(g, n, hw, c, groups)
    _, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
    # mask_from_y: the ReLU mask recomputed as fma(y, scale, shift) > 0
    a = ffi.TestBnBwdArgs(m_per_group=n * hw * hw, groups=1, c=c, nsets=1, mask_from_y=1, one_pass=1)
    ts = [dev(t.float()) for t in (dz, y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
    a.dz = p(ts[0])
    for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts[1:]):
        getattr(a, f)[0] = t.data_ptr()
    path = lib.ocl_test_bn_bwd(C.byref(a), None)
    assert path == 2061, (path, lib.ocl_last_error())   # the one-pass kernel (the engine's path for this case) recomputes the mask
    zpre = (y - mean) * invstd * gamma + beta
    dy, dgm, dbt = _bn_bwd_ref(dz, zpre, y, 1, gamma)
    amb = zpre.abs() < 1e-5
    ok = ~amb.any(dim=(1, 2, 3))   # images without a near-zero pre-activation compare element-wise
    assert bool(ok.any())
    got = ts[6].double().cpu()
    np.testing.assert_allclose(got[ok].numpy(), dy[ok].numpy(), rtol=1e-4, atol=2e-5 * float(dy.abs().max()))
    # dgamma / dbeta: a mask decision that may differ (near-zero pre-activation) moves them by at most that pixel's contribution
    xhat = (y - mean) * invstd
    slack_g = (dz.abs() * xhat.abs() * amb).sum(dim=(0, 1, 2)).numpy()
    slack_b = (dz.abs() * amb).sum(dim=(0, 1, 2)).numpy()
    got_g, got_b = ts[7].double().cpu().numpy(), ts[8].double().cpu().numpy()
    assert np.all(np.abs(got_g - dgm.numpy()) <= slack_g + 1e-4 * np.abs(dgm.numpy()) + 1e-4 * float(dgm.abs().max())), "dgamma"
    assert np.all(np.abs(got_b - dbt.numpy()) <= slack_b + 1e-4 * np.abs(dbt.numpy()) + 1e-4 * float(dbt.abs().max())), "dbeta"
    # frozen: dy = gamma * invstd * dpre (constant statistics), no mean terms
    a2 = ffi.TestBnBwdArgs(m_per_group=n * hw * hw, groups=1, c=c, nsets=1, frozen=1)
    zm = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
    ts2 = [dev(t.float()) for t in (dz, zm, y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
    a2.dz, a2.z = p(ts2[0]), p(ts2[1])
    for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts2[2:]):
        getattr(a2, f)[0] = t.data_ptr()
    path = lib.ocl_test_bn_bwd(C.byref(a2), None)
    assert path == 3001, path
    inv32 = invstd.float().double()
    want = dz * (zm > 0) * gamma * inv32[0]
    np.testing.assert_allclose(ts2[7].double().cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    # three and eight groups (every bn1 backward of such a pass): reduce + apply with mask_from_y, and accumulating onto a preset gradient
    for n, hw, c, groups, accumulate in [(6, 8, 20, 3, 0), (3, 4, 160, 3, 1), (8, 4, 160, 8, 1)]:
        dz = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
        y, gamma, beta = _bn_case(g, n, hw, c, groups)
        _, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
        dg0 = torch.randn(c, generator=g, dtype=torch.float64).float().double() * accumulate
        db0 = torch.randn(c, generator=g, dtype=torch.float64).float().double() * accumulate
        a = ffi.TestBnBwdArgs(m_per_group=n // groups * hw * hw, groups=groups, c=c, nsets=1, mask_from_y=1, one_pass=1, accumulate=accumulate)
        ts = [dev(t.float()) for t in (dz, y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(dg0.float()), dev(db0.float())]
        a.dz = p(ts[0])
        for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts[1:]):
            getattr(a, f)[0] = t.data_ptr()
        path = lib.ocl_test_bn_bwd(C.byref(a), None)
        assert path == 3001, (path, lib.ocl_last_error())
        mb, ib = mean.repeat_interleave(n // groups, 0)[:, None, None, :], invstd.repeat_interleave(n // groups, 0)[:, None, None, :]
        zpre = (y - mb) * ib * gamma + beta
        dy, dgm, dbt = _bn_bwd_ref(dz, zpre, y, groups, gamma)
        amb = zpre.abs() < 1e-5
        # a group without a near-zero pre-activation compares element-wise (a mask decision moves the whole group's means)
        ok = ~amb.reshape(groups, -1).any(dim=1).repeat_interleave(n // groups, 0)
        assert bool(ok.any())
        np.testing.assert_allclose(ts[6].double().cpu()[ok].numpy(), dy[ok].numpy(), rtol=1e-4, atol=2e-5 * float(dy.abs().max()))
        xhat = (y - mb) * ib
        slack_g = (dz.abs() * xhat.abs() * amb).sum(dim=(0, 1, 2)).numpy()
        slack_b = (dz.abs() * amb).sum(dim=(0, 1, 2)).numpy()
        got_g, got_b = ts[7].double().cpu().numpy() - dg0.numpy(), ts[8].double().cpu().numpy() - db0.numpy()
        lim_g = slack_g + 1e-4 * np.abs(dgm.numpy()) + 1e-4 * float(dgm.abs().max()) + 2 * U * accumulate * (np.abs(dg0.numpy()) + np.abs(dgm.numpy()))
        lim_b = slack_b + 1e-4 * np.abs(dbt.numpy()) + 1e-4 * float(dbt.abs().max()) + 2 * U * accumulate * (np.abs(db0.numpy()) + np.abs(dbt.numpy()))
        assert np.all(np.abs(got_g - dgm.numpy()) <= lim_g), ("dgamma", n, hw, c, groups)
        assert np.all(np.abs(got_b - dbt.numpy()) <= lim_b), ("dbeta", n, hw, c, groups)


@pytest.mark.parametrize("det", [0, 1])
def test_bnb_epilogue_then_apply_e_against_float64(lib, det):
    """Data gradient of conv2 with EPI_BNB (bn1's two sums in its epilogue) followed by bn_bwd_apply_e == float64 BatchNorm backward."""
    lib.ocl_set_deterministic(det)
    try:
        g = torch.Generator().manual_seed(17)
        n, groups, hw, c = 10, 2, 16, 40
        d = _desc(c, c, 3, 1, hw, n, groups, 1, bnb=1)
        dy2 = torch.randn((n, hw, hw, c), generator=g, dtype=torch.float64).float().double()
        w = (0.1 * torch.randn((c, c, 3, 3), generator=g, dtype=torch.float64)).float().double()
        y, gamma, beta = _bn_case(g, n, hw, c, groups)
        zz, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
        z = torch.clamp(zz, min=0).float().double()
        got_d, forms, stats = run_conv(lib, d, dy2, w, EPI_BNB, bnb_y=y, bnb_z=z, bnb_mean=mean, bnb_invstd=invstd, bnb_gamma=gamma, bnb_beta=beta)
        dx = ref_dgrad(dy2, w, d)
        dmask = dx * (z > 0)
        np.testing.assert_allclose(got_d.numpy(), dmask.numpy(), rtol=1e-5, atol=1e-5 * float(dmask.abs().max()))
        outs = [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
        ins = [dev(t.float()) for t in (got_d, y, mean, invstd, gamma)]
        rc = lib.ocl_test_bn_apply_e(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), p(stats), n // groups * hw * hw, groups, c,
                                     p(outs[0]), p(outs[1]), p(outs[2]), 0, None)
        assert rc == 0, lib.ocl_last_error()
        torch.cuda.synchronize()
        want, dgm, dbt = _bn_bwd_ref(dx, z, y, groups, gamma)
        np.testing.assert_allclose(outs[0].double().cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-5 * float(want.abs().max()))
        np.testing.assert_allclose(outs[1].double().cpu().numpy(), dgm.numpy(), rtol=1e-4, atol=1e-4 * float(dgm.abs().max()))
        np.testing.assert_allclose(outs[2].double().cpu().numpy(), dbt.numpy(), rtol=1e-4, atol=1e-4 * float(dbt.abs().max()))
    finally:
        lib.ocl_set_deterministic(0)


def test_deterministic_cells_at_their_limits(lib):
    """Deterministic-mode cells: a total just under 2^47 built from many partial sums (each |v| < 7e13) comes back exact; a total beyond the
    range and a non-finite partial sum read back as NaN.  The producer is an EPI_STATS forward of 2 x 41 x 41 pixels whose outputs, their
    squares and every partial sum of them are exact in fp32."""
    lib.ocl_set_deterministic(1)
    try:
        n, hw = 2, 41
        px = n * hw * hw
        d = _desc(4, 4, 1, 1, hw, n, 1, 0)
        w = torch.zeros((4, 4, 1, 1), dtype=torch.float64)
        for i in range(4):
            w[i, i] = 1
        x = torch.zeros((n, hw, hw, 4), dtype=torch.float64)
        x[..., 0] = 2.0 ** 22            # sum of squares 3362 * 2^44 ~ 5.9e16: outside the range, reads back as NaN
        x[..., 1] = 1.5 * 2.0 ** 17      # sum of squares 3362 * 2.25 * 2^34 = 1.30e14 = 0.92 * 2^47: inside, near the limit -- exact
        x[..., 2] = -3.0
        x[0, 0, 0, 3] = 3e38             # times 2: overflows to inf in the output -- a non-finite partial sum poisons its cells
        w[3, 3] = 2
        got, _, stats = run_conv(lib, d, x, w, EPI_STATS)
        tot = cell_totals(stats, 1, 4, True)
        v = 1.5 * 2.0 ** 17
        assert px * v * v > 0.9 * 2.0 ** 47
        assert tot[0, 0, 1] == px * v and tot[0, 1, 1] == px * v * v, (tot[0, :, 1], px * v, px * v * v)
        assert tot[0, 0, 2] == -3.0 * px and tot[0, 1, 2] == 9.0 * px
        assert tot[0, 0, 0] == px * 2.0 ** 22 and np.isnan(tot[0, 1, 0])
        assert np.isnan(tot[0, 0, 3]) and np.isnan(tot[0, 1, 3])
    finally:
        lib.ocl_set_deterministic(0)


@pytest.mark.parametrize("one_pass,want", [(1, 2031), (0, 3001)])   # bn_bwd_fused_kernel<3, 1>; bn_bwd_reduce_kernel + bn_bwd_apply_kernel
def test_deterministic_flag_reaches_the_bn_backward_kernels(lib, one_pass, want):
    """The BatchNorm backward writes and reads its batch sums inside its own translation unit, so no host-side decoding of the cells can
    tell which mode its kernels ran in: a mode flag that never reaches that unit gives right answers in the wrong mode.  The range limit does
    tell: channel 0's gradient is 2^47 at every pixel (exact in fp32; a single element is above the 7e13 limit of a fixed-point partial sum),
    so the default mode sums it exactly (1024 * 2^47 = 2^57) and the deterministic mode must poison that channel's cells (NaN)."""
    from ocl_amd import ffi
    n, hw, c, groups = 4, 16, 40, 1
    g = torch.Generator().manual_seed(29)
    dz = ints((n, hw, hw, c), g)
    dz[..., 0] = 2.0 ** 47
    zm = torch.ones((n, hw, hw, c), dtype=torch.float64)
    y, gamma, beta = _bn_case(g, n, hw, c, groups)
    _, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
    dy, dgm, dbt = (t[..., 1:].numpy() for t in _bn_bwd_ref(dz, zm, y, groups, gamma))
    try:
        for det in (0, 1):
            lib.ocl_set_deterministic(det)
            a = ffi.TestBnBwdArgs(m_per_group=n * hw * hw, groups=groups, c=c, nsets=1, one_pass=one_pass)
            keep = [dev(dz.float()), dev(zm.float())]
            a.dz, a.z = p(keep[0]), p(keep[1])
            ts = [dev(t.float()) for t in (y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
            for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts):
                getattr(a, f)[0] = t.data_ptr()
            path = lib.ocl_test_bn_bwd(C.byref(a), None)
            assert path == want, (path, want, lib.ocl_last_error())
            got_dy, got_dgm, got_dbt = (t.double().cpu().numpy() for t in ts[5:])
            if det:
                assert np.isnan(got_dbt[0]) and np.isnan(got_dgm[0]), (got_dbt[0], got_dgm[0])
            else:
                assert got_dbt[0] == n * hw * hw * 2.0 ** 47, got_dbt[0]
                assert np.isfinite(got_dy).all() and np.isfinite(got_dgm).all() and np.isfinite(got_dbt).all()
            # channels 1 - 39 are ordinary in both modes
            np.testing.assert_allclose(got_dy[..., 1:], dy, rtol=1e-4, atol=2e-5 * float(np.abs(dy).max()))
            np.testing.assert_allclose(got_dgm[1:], dgm, rtol=1e-4, atol=1e-4 * float(np.abs(dgm).max()))
            np.testing.assert_allclose(got_dbt[1:], dbt, rtol=1e-4, atol=1e-4 * float(np.abs(dbt).max()))
    finally:
        lib.ocl_set_deterministic(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# forms reachable only through a switch read once per process: each set in a fresh child interpreter (never os.exec*)
# ---------------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import ocl_amd
from ocl_amd import ffi
ffi.init()
import test_gpu_layers as T
print("RESULT " + json.dumps(T.switch_cases(ffi.lib(), %(which)r)))
"""


def _layer_desc(lib, key):
    """The layer / pass of COVERED[key], whatever form the planner of this process gives it."""
    hw, n, g, layer, dr = LF.COVERED[key]
    for _, e in LF.net_forms(lib, hw, n, g, 0 if key.endswith("/affine") else 1):
        if e.layer == layer and e.dir == dr:
            return e
    raise AssertionError(key)


def switch_cases(lib, which):
    """Runs the integer-exact cases of one switch set (in the child); returns the forms that ran."""
    torch.set_num_threads(16)
    ran = {}
    g = torch.Generator().manual_seed(23)
    conv = {"A": [("wx3x1/plain", dict(force_cw=1)), ("s1/plain", {})], "B": [("s2/plain", {})]}[which]
    for key, force in conv:
        d = type(_layer_desc(lib, key).desc).from_buffer_copy(_layer_desc(lib, key).desc)
        for a, v in force.items():
            setattr(d, a, v)
        x, w, _ = _case_data(d, 3)
        got, forms, _ = run_conv(lib, d, x, w)
        assert_exact(got, ref_dgrad(x, w, d), key)
        ran[key] = [LF.conv_key(f, "plain") for f in forms]
    wkey = {"A": "wgq3.pf8/plain", "B": "wg2x2.pf8/plain"}[which]
    wd = _layer_desc(lib, wkey).wdesc
    cinT, ho, wo, _ = shape_of(wd)
    x, dy = ints((wd.n, wd.hin, wd.win, cinT), g), ints((wd.n, ho, wo, wd.cout), g)
    gw, wf = run_wgrad(lib, [wd], [x], [dy])
    assert_exact(gw[0], ref_wgrad(x, dy, wd), wkey)
    ran[wkey] = [LF.wgrad_key(wf[0], wd.xf_groups > 0, False)]
    from ocl_amd import ffi
    for n, hw, c, groups in [(4, 4, 160, 2), (6, 16, 40, 2)]:
        dz = ints((n, hw, hw, c), g)
        zm = ints((n, hw, hw, c), g)
        y, gamma, beta = _bn_case(g, n, hw, c, groups)
        _, mean, invstd, _ = _bn_ref(y, groups, gamma, beta)
        a = ffi.TestBnBwdArgs(m_per_group=n // groups * hw * hw, groups=groups, c=c, nsets=1, one_pass=1)
        ts = [dev(t.float()) for t in (dz, zm, y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
        a.dz, a.z = p(ts[0]), p(ts[1])
        for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts[2:]):
            getattr(a, f)[0] = t.data_ptr()
        path = lib.ocl_test_bn_bwd(C.byref(a), None)
        assert path >= 0, lib.ocl_last_error()
        dyr, dgm, dbt = _bn_bwd_ref(dz, zm, y, groups, gamma)
        np.testing.assert_allclose(ts[7].double().cpu().numpy(), dyr.numpy(), rtol=1e-4, atol=2e-5 * float(dyr.abs().max()))
        np.testing.assert_allclose(ts[8].double().cpu().numpy(), dgm.numpy(), rtol=1e-4, atol=1e-4 * float(dgm.abs().max()))
        ran["bn%dx%d" % (n, c)] = [path]
    return ran


@pytest.mark.parametrize("which,env,want", [
    ("A", dict(OCL_CONV_WX="0", OCL_CONV_S_NT="2", OCL_WGRAD_Q="0", OCL_BN_CHAN="0"),
     {"wx3x1/plain": ["w3x1/plain"], "s1/plain": ["s2/plain"], "wgq3.pf8/plain": ["wg3x2.pf8/plain"], "bn4x160": [2031], "bn6x40": [2061]}),
    ("B", dict(OCL_CONV_S_NT="1", OCL_WGRAD_Q="2", OCL_BN_FUSED="0"),
     {"s2/plain": ["s1/plain"], "wg2x2.pf8/plain": ["wgq3.pf8/plain"], "bn4x160": [3001], "bn6x40": [3001]})])
def test_switch_only_forms_in_a_fresh_process(lib, which, env, want):
    """conv_w_kernel instead of conv_wx (OCL_CONV_WX=0), conv_s_kernel with the other pixel-tile count (OCL_CONV_S_NT), the weight gradient
    without / with the 4x4x1 form (OCL_WGRAD_Q=0 / 2), BatchNorm backward without the small-map kernel (OCL_BN_CHAN=0) or the one-pass
    kernel (OCL_BN_FUSED=0): integer-exact against float64 (BatchNorm: tier 2), and each runs the form the switch selects."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    tests = os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "tests": tests, "which": which}], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", **env), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print("FORM switch", which, got)
    assert got == want
