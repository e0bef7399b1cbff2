"""GPU: the glue kernels of csrc/conv_aux.hip, bn_fold_kernel / bn_apply_saved_kernel of csrc/bn.hip and the head chain of net.hip (head_forward,
head_backward), case by case (tests/aux_cases.py), stage by stage: the reference of every stage is float64 numpy / torch-CPU computed from the
ENGINE's own fp32 input to that stage, so rounding does not compound and every stage keeps a tight bound.

Tier 1 (bit-equal): layout and the combined weight-pack launch on any data (pack elements equal the OIHW gather of the documented layouts
[t][ci>>2][co][ci&3] / [t][co>>2][ci][co&3]; padding, packs outside the mask and regions not passed keep their pre-fill; cleared regions are zero),
fill, relu_bwd, the average pool's backward (1/16 is a power of two), pool forward and colsum on small integers, bn_fold and bn_apply_saved
on power-of-two scales.
Tier 2 (random fp32), the project's two yardsticks (tests/parity_bounds.py), no new number:
  * sums of products (colsum, avgpool, the three GEMMs of every linear stage): |got - ref| <= 1.01 * (K + 2) * 2^-24 * sum|terms| with K the
    fp32-accumulated products and the bias among the terms (test_gemm_small_random_within_fp32_bound's bound); colsum and the pool have no
    such extra terms: K = rows (+ 1 when accumulating) and 16;
  * l2norm forward / backward and bn_fold: max(4 x the error of the same formula in torch-CPU fp32, 4 ulp of the largest reference element); the
    formulas are F.normalize(v, dim=1, eps=1e-12) with its autograd gradient, and gamma / sqrt(rv + eps), beta - rm * scale.  Rows of very
    different magnitude (the clamped rows, the 1e15 row) and the classes of running variance are judged separately: a whole-tensor maximum
    would let the large rows hide the small ones;
  * the head's gradients when accumulating: the hook runs twice on the same data, and pre-fill + the overwrite-mode result must be met within
    one fp32 addition's rounding, 2^-24 |pre + g_ow|;
  * bn_apply_saved on random data: relu(fma(y, sc, sh)) with sc = fl(gamma * invstd), sh = fl(fma(-mean, sc, beta)) (bn_scale_shift), restated
    exactly (float64 product, TwoSum, fp32 midpoints resolved by the residual) -- bit-equal.
Every tensor sits between sentinels (guarded.Guarded): inputs unchanged, guards intact after each call.  With OCL_PARITY_REPORT=<file> the tier-2
figures go to aux_parity.txt next to it (profiles/aux_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_cases as AC
import parity_bounds as PB
from guarded import Guarded

pytestmark = pytest.mark.gpu

U = PB.U
REPORT = []
OP = dict(layout=0, pool_fwd=1, pool_bwd=2, l2_fwd=3, l2_bwd=4, relu_bwd=5, colsum=6, fill=7, bn_fold=8, bn_apply=9)


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    yield L
    path = os.environ.get("OCL_PARITY_REPORT")
    if path and REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "aux_parity.txt"), "w") as f:
            f.write("# tier-2 parity of the glue kernels and the head chain against float64 (tests/test_gpu_aux.py), stage by stage from the engine's own\n"
                    "# fp32 stage input: kernel error, the error of plain torch-CPU fp32 on the same inputs (e_ref; '-' where the bound is derived), the\n"
                    "# bound, and error / bound (must be <= 1).  Head cases: the worst tensor of each stage group\n")
            f.write("%-40s %-14s %12s %12s %12s %8s\n" % ("case", "tensor", "kernel_err", "e_ref", "bound", "ratio"))
            for row in REPORT:
                f.write("%-40s %-14s %12.4g %12s %12.4g %8.3f\n" % row)
            worst = max(REPORT, key=lambda r: r[5])
            f.write("# closest to its bound: %s %s (ratio %.3f)\n" % (worst[0], worst[1], worst[5]))


def case_of(op):
    return pytest.mark.parametrize("name", AC.ids(op))


def stream():
    from ocl_amd import ffi
    return ffi.stream()


def ok(lib, rc, what):
    assert rc == 0, "%s failed (%d): %s" % (what, rc, lib.ocl_last_error())


def aux(lib, op, what, p=(), i=(), f=()):
    from ocl_amd import ffi
    a = ffi.TestAuxArgs()
    for k, t in enumerate(p):
        a.p[k] = t if isinstance(t, int) or t is None else t.data_ptr()
    for k, v in enumerate(i):
        a.i[k] = int(v)
    for k, v in enumerate(f):
        a.f[k] = float(v)
    ok(lib, lib.ocl_test_aux(OP[op], C.byref(a), stream()), what)


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(np.asarray(ref), dtype=np.float32)
    return got.shape == ref.shape and got.tobytes() == ref.tobytes()


def host(t):
    return t.cpu().numpy()


# ==========================================================================================================================================
# layout
# ==========================================================================================================================================
@case_of("layout")
def test_layout(lib, name):
    """NCHW segments -> one NHWC4 batch, bit for bit; the fourth lane of every pixel is +0.0."""
    c = AC.find("layout", name)
    rng = np.random.default_rng(c["seed"])
    hw, ns = c["hw"], c["ns"]
    g = Guarded()
    xs = [rng.standard_normal((n, 3, hw, hw)).astype(np.float32) for n in ns]
    d_xs = [g.inp(x, 0, "x%d" % k) for k, x in enumerate(xs)]
    N = sum(ns)
    d_o = g.out((N, hw, hw, 4), torch.float32, 0, "out")
    ptrs = (C.c_void_p * len(ns))(*[t.data_ptr() for t in d_xs])
    cnts = (C.c_int32 * len(ns))(*ns)
    aux(lib, "layout", name, p=[C.addressof(ptrs), C.addressof(cnts), d_o], i=[len(ns), hw, hw])
    g.check(name)
    ref = np.zeros((N, hw, hw, 4), np.float32)
    ref[..., :3] = np.concatenate(xs, 0).transpose(0, 2, 3, 1)
    assert same_bits(host(d_o), ref), name


# ==========================================================================================================================================
# avg_pool2d(4) + flatten
# ==========================================================================================================================================
def _pool_ref(z64, n, h, w, c):
    ph, pw = h // 4, w // 4
    win = z64[:, :ph * 4, :pw * 4, :].reshape(n, ph, 4, pw, 4, c)
    return win.sum((2, 4)).transpose(0, 3, 1, 2).reshape(n, c * ph * pw) / 16.0, np.abs(win).sum((2, 4)).transpose(0, 3, 1, 2).reshape(n, c * ph * pw) / 16.0


@case_of("avgpool")
def test_avgpool(lib, name):
    """Forward: small integers exact, random data within 16 fp32 additions; what lies outside the 4-aligned window (11 x 11 -> 8 x 8) is huge
    in the forward's input, so a read of it shows.  Backward: dfeat / 16 is exact for any data, and rows / columns outside the window are
    written +0.0 (the output starts as a sentinel)."""
    c = AC.find("avgpool", name)
    rng = np.random.default_rng(c["seed"])
    n, h, w, ch = c["n"], c["h"], c["w"], c["c"]
    ph, pw = h // 4, w // 4
    D = ch * ph * pw
    for kind in ("int", "rand"):
        z = rng.integers(-8, 9, (n, h, w, ch)).astype(np.float32) if kind == "int" else rng.standard_normal((n, h, w, ch)).astype(np.float32)
        z[:, ph * 4:, :, :] = 3e30
        z[:, :, pw * 4:, :] = 3e30
        g = Guarded()
        d_z, d_f = g.inp(z, 0, "z"), g.out((n, D), torch.float32, 0, "feat")
        aux(lib, "pool_fwd", name, p=[d_z, d_f], i=[n, h, w, ch])
        g.check(name)
        ref, terms = _pool_ref(z.astype(np.float64), n, h, w, ch)
        if kind == "int":
            assert same_bits(host(d_f), ref), name
        else:
            PB.check_derived(REPORT, "avgpool/" + name, "feat", host(d_f), ref, 1.01 * 16 * U * terms)
    df = rng.standard_normal((n, D)).astype(np.float32)
    g = Guarded()
    d_df, d_dz = g.inp(df, 0, "dfeat"), g.out((n, h, w, ch), torch.float32, 0, "dz")
    aux(lib, "pool_bwd", name, p=[d_df, d_dz], i=[n, h, w, ch])
    g.check(name)
    ref = np.zeros((n, h, w, ch), np.float32)
    up = (df.reshape(n, ch, ph, pw) / np.float32(16)).transpose(0, 2, 3, 1)
    ref[:, :ph * 4, :pw * 4, :] = np.repeat(np.repeat(up, 4, 1), 4, 2)
    assert same_bits(host(d_dz), ref), "%s: backward (the cropped rows / columns must be +0.0)" % name


# ==========================================================================================================================================
# l2norm
# ==========================================================================================================================================
def l2_rows(rng, n, d):
    """Rows of varied magnitude; for n = 7 the last three are all zero, of magnitude 1e-20 (both clamped by eps) and of magnitude 1e15."""
    v = rng.standard_normal((n, d)).astype(np.float32)
    mags = [1.0, 1e-3, 37.0, 1e4]
    for r in range(n):
        v[r] *= np.float32(mags[r % 4])
    if n >= 7:
        v[n - 3] = 0.0
        v[n - 2] = (rng.standard_normal(d) * 1e-20).astype(np.float32)
        v[n - 1] = (rng.standard_normal(d) * 1e15).astype(np.float32)
    return v


def l2_refs(v, g=None):
    """F.normalize(v, dim=1, eps=1e-12) (and its gradient for dL/dout = g) in float64 and in fp32, and the clamped norms."""
    res = []
    for dt in (torch.float64, torch.float32):
        t = torch.from_numpy(v).to(dt).requires_grad_(g is not None)
        o = F.normalize(t, dim=1, eps=1e-12)
        nrm = t.detach().norm(dim=1).clamp_min(1e-12)
        if g is not None:
            o.backward(torch.from_numpy(g).to(dt))
        res.append((o.detach().numpy(), nrm.numpy(), t.grad.numpy() if g is not None else None))
    return res


def check_l2_fwd(case, v, out, norms):
    (o64, n64, _), (o32, n32, _) = l2_refs(v)
    for r in range(v.shape[0]):
        PB.check_vs_torch32(REPORT, case, "out[%d]" % r, out[r], o64[r], o32[r])
        PB.check_vs_torch32(REPORT, case, "norm[%d]" % r, norms[r:r + 1], n64[r:r + 1], n32[r:r + 1])


def check_l2_bwd(case, v, g, dv):
    (_, n64, g64), (_, _, g32) = l2_refs(v, g)
    for r in range(v.shape[0]):
        PB.check_vs_torch32(REPORT, case, "dv[%d]" % r, dv[r], g64[r], g32[r])
    return n64


@case_of("l2norm")
def test_l2norm(lib, name):
    """Forward with and without the second output; the backward runs on the forward's own out / norms.  Clamped rows (norm < 1e-12): torch's
    gradient is g / 1e-12 with no projection term, and the kernel must agree within the bound."""
    c = AC.find("l2norm", name)
    rng = np.random.default_rng(c["seed"])
    n, d = c["n"], c["d"]
    v = l2_rows(rng, n, d)
    outs = []
    for with_out2 in (0, 1):
        g = Guarded()
        d_v, d_o, d_n = g.inp(v, 0, "v"), g.out((n, d), torch.float32, 0, "out"), g.out((n,), torch.float32, 0, "norms")
        d_o2 = g.out((n, d), torch.float32, 0, "out2") if with_out2 else None
        aux(lib, "l2_fwd", name, p=[d_v, d_o, d_n, d_o2], i=[n, d])
        g.check(name)
        outs.append((host(d_o), host(d_n)))
        if with_out2:
            assert same_bits(host(d_o2), outs[-1][0]), "%s: out2 differs from out" % name
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "%s: out2 changes the result" % name
    out, norms = outs[0]
    check_l2_fwd("l2norm/" + name, v, out, norms)
    dout = rng.standard_normal((n, d)).astype(np.float32)
    g = Guarded()
    d_o, d_n, d_g, d_dv = g.inp(out, 0, "out"), g.inp(norms, 0, "norms"), g.inp(dout, 0, "dout"), g.out((n, d), torch.float32, 0, "dv")
    aux(lib, "l2_bwd", name, p=[d_o, d_n, d_g, d_dv], i=[n, d])
    g.check(name)
    dv = host(d_dv)
    n64 = check_l2_bwd("l2norm/" + name, v, dout, dv)
    if n >= 7:
        assert n64[n - 3] == 1e-12 and n64[n - 2] == 1e-12 and n64[n - 1] > 1e15, "the rows are not the ones the case is there for"
        assert norms[n - 3] == np.float32(1e-12) and norms[n - 2] == np.float32(1e-12)


# ==========================================================================================================================================
# relu_bwd, fill
# ==========================================================================================================================================
@case_of("relu_bwd")
def test_relu_bwd(lib, name):
    """dx = a > 0 ? dy : +0.0, out of place and in place; +0.0, -0.0 and negatives block, positive denormals pass."""
    c = AC.find("relu_bwd", name)
    rng = np.random.default_rng(c["seed"])
    n = c["n"]
    a = rng.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.17549435e-38, -3.0, 2.0 ** -126], np.float32)
    a[:: max(1, n // 64)] = special[np.arange(len(a[:: max(1, n // 64)])) % len(special)]
    if n == 1:
        a[0] = np.float32(1e-40)
    dy = rng.standard_normal(n).astype(np.float32)
    dy[dy == 0] = 1.0
    ref = np.where(a > 0, dy, np.float32(0.0)).astype(np.float32)
    for in_place in (0, 1):
        g = Guarded()
        d_a = g.inp(a, 0, "a")
        if in_place:
            d_dy = g.out((n,), torch.float32, 0, "dy/dx", init=dy)
            d_dx = d_dy
        else:
            d_dy, d_dx = g.inp(dy, 0, "dy"), g.out((n,), torch.float32, 0, "dx")
        aux(lib, "relu_bwd", name, p=[d_dy, d_a, d_dx], i=[n])
        g.check(name)
        assert same_bits(host(d_dx), ref), "%s in_place=%d" % (name, in_place)


@case_of("fill")
def test_fill(lib, name):
    """Every element takes the value's bits; n = 0 returns before launching."""
    c = AC.find("fill", name)
    n = c["n"]
    for v in (0.0, -0.0, 1.25, -3.0e-39):
        g = Guarded()
        d_p = g.out((max(n, 1),), torch.float32, 0, "p")
        aux(lib, "fill", name, p=[d_p], i=[n], f=[v])
        g.check(name)
        got = host(d_p)
        if n == 0:
            assert Guarded.is_poison(got[:1]).all()
        else:
            assert same_bits(got, np.full(n, v, np.float32)), "%s value %r" % (name, v)


# ==========================================================================================================================================
# colsum
# ==========================================================================================================================================
@case_of("colsum")
def test_colsum(lib, name):
    """out[c] (+)= sum_r m[r][c].  Overwrite mode starts from NaN; small integers are exact; random data within rows (+ 1) fp32 additions."""
    c = AC.find("colsum", name)
    rng = np.random.default_rng(c["seed"])
    rows, cols = c["rows"], c["cols"]
    for kind in ("int", "rand"):
        for acc in (0, 1):
            if kind == "int":
                m, o0 = rng.integers(-8, 9, (rows, cols)).astype(np.float32), rng.integers(-100, 101, cols).astype(np.float32)
            else:
                m, o0 = rng.standard_normal((rows, cols)).astype(np.float32), rng.standard_normal(cols).astype(np.float32)
            g = Guarded()
            d_m = g.inp(m, 0, "m")
            d_o = g.out((cols,), torch.float32, 0, "out", init=o0 if acc else np.full(cols, np.nan, np.float32))
            aux(lib, "colsum", name, p=[d_m, d_o], i=[rows, cols, acc])
            g.check(name)
            m64 = m.astype(np.float64)
            ref = m64.sum(0) + (o0 if acc else 0.0)
            terms = np.abs(m64).sum(0) + (np.abs(o0) if acc else 0.0)
            if kind == "int":
                assert same_bits(host(d_o), ref), "%s acc=%d" % (name, acc)
            else:
                PB.check_derived(REPORT, "colsum/%s/acc%d" % (name, acc), "out", host(d_o), ref, 1.01 * (rows + acc) * U * terms)


# ==========================================================================================================================================
# BatchNorm: eval-mode fold, apply from saved statistics
# ==========================================================================================================================================
def net_info(lib, hw, nf=20, n_classes=10, head=0, feat_dim=0, n=1):
    """Tensor table {name: (offset, shape)}, BatchNorm table [(name, stat_off, C)], n_params, n_stats of the engine's net."""
    from ocl_amd import ffi
    net = C.c_void_p()
    d = ffi.NetDesc(hw, hw, nf, n_classes, head, feat_dim, n, 1)
    ok(lib, lib.ocl_net_create(C.byref(d), C.byref(net)), "net_create")
    tensors, bns = {}, []
    buf = C.create_string_buffer(64)
    for i in range(lib.ocl_net_num_tensors(net)):
        off, nd, shp = ffi.i64(0), ffi.i32(0), (ffi.i64 * 4)()
        ok(lib, lib.ocl_net_tensor_info(net, i, buf, C.byref(off), C.byref(nd), shp), "tensor_info")
        tensors[buf.value.decode()] = (off.value, tuple(shp[k] for k in range(nd.value)))
    for i in range(lib.ocl_net_num_bn(net)):
        off, ch = ffi.i64(0), ffi.i32(0)
        ok(lib, lib.ocl_net_bn_info(net, i, buf, C.byref(off), C.byref(ch)), "bn_info")
        bns.append((buf.value.decode(), off.value, ch.value))
    info = dict(tensors=tensors, bns=bns, n_params=lib.ocl_net_param_count(net), n_stats=lib.ocl_net_bn_stat_count(net),
                feat=lib.ocl_net_feature_dim(net), out=lib.ocl_net_out_dim(net))
    lib.ocl_net_destroy(net)
    return info


def _fold_run(lib, c, params, running, eps):
    g = Guarded()
    d_p, d_r, d_o = g.inp(params, 0, "params"), g.inp(running, 0, "running"), g.out((len(running),), torch.float32, 0, "fold")
    aux(lib, "bn_fold", c["name"], p=[d_p, d_r, d_o], i=[c["hw"], c["nf"]], f=[eps])
    g.check(c["name"])
    return host(d_o)


@case_of("bn_fold")
def test_bn_fold(lib, name):
    """The whole network's BatchNorm table in one launch: scale = gamma / sqrt(rv + eps), shift = beta - rm * scale at the running
    statistics' own offsets.  Power-of-two data (eps = 0) bit-equal; random data with running variances 0, 1e-12 and 1e6 and gammas 0 and
    negative among them, each class of variance judged on its own."""
    c = AC.find("bn_fold", name)
    rng = np.random.default_rng(c["seed"])
    info = net_info(lib, c["hw"], c["nf"])
    assert len(info["bns"]) == 20 and sum(2 * ch for _, _, ch in info["bns"]) == info["n_stats"]
    for kind in ("pow2", "rand"):
        params = rng.standard_normal(info["n_params"]).astype(np.float32)
        running = np.full(info["n_stats"], np.nan, np.float32)
        cls = np.zeros(info["n_stats"], np.int64)          # per output element: class of running variance
        ref = np.zeros(info["n_stats"], np.float64)
        ref32 = np.zeros(info["n_stats"], np.float32)
        eps = 0.0 if kind == "pow2" else 1e-5
        for bname, so, ch in info["bns"]:
            go, bo = info["tensors"][bname + ".weight"][0], info["tensors"][bname + ".bias"][0]
            if kind == "pow2":
                gamma = (2.0 ** rng.integers(-3, 4, ch) * rng.choice([-1.0, 1.0], ch)).astype(np.float32)
                rv = (4.0 ** rng.integers(-3, 4, ch)).astype(np.float32)
                rm, beta = rng.integers(-8, 9, ch).astype(np.float32), rng.integers(-8, 9, ch).astype(np.float32)
                k = np.zeros(ch, np.int64)
            else:
                gamma, beta = params[go:go + ch].copy(), params[bo:bo + ch].copy()
                gamma[1], gamma[2] = 0.0, -abs(gamma[2]) - 0.5
                rv = rng.uniform(0.05, 4.0, ch).astype(np.float32)
                rv[0], rv[1], rv[3], rv[4] = 0.0, 1e-12, 1e6, 1e-12
                rm = rng.standard_normal(ch).astype(np.float32)
                k = np.zeros(ch, np.int64)
                k[0], k[1], k[3], k[4] = 1, 2, 3, 2
            params[go:go + ch], params[bo:bo + ch] = gamma, beta
            running[so:so + ch], running[so + ch:so + 2 * ch] = rm, rv
            e64 = float(np.float32(eps))
            sc = gamma.astype(np.float64) / np.sqrt(rv.astype(np.float64) + e64)
            ref[so:so + ch], ref[so + ch:so + 2 * ch] = sc, beta.astype(np.float64) - rm.astype(np.float64) * sc
            tg, tb, tm, tv = (torch.from_numpy(a) for a in (gamma, beta, rm, rv))
            s32 = tg / torch.sqrt(tv + eps)
            ref32[so:so + ch], ref32[so + ch:so + 2 * ch] = s32.numpy(), (tb - tm * s32).numpy()
            cls[so:so + ch], cls[so + ch:so + 2 * ch] = 2 * k, 2 * k + 1
        assert not np.isnan(running).any()
        got = _fold_run(lib, c, params, running, eps)
        if kind == "pow2":
            assert same_bits(got, ref), name
        else:
            for k, what in enumerate(["scale", "shift", "scale/rv=0", "shift/rv=0", "scale/rv=1e-12", "shift/rv=1e-12", "scale/rv=1e6", "shift/rv=1e6"]):
                sel = cls == k
                assert sel.any()
                PB.check_vs_torch32(REPORT, "bn_fold/" + name, what, got[sel], ref[sel], ref32[sel])


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _fma32(a, b, c):
    """fl32(a * b + c) of fp32 values, exactly: the product is exact in float64, TwoSum gives the float64 sum s and its exact residual t, and
    where s lies exactly midway between two fp32 neighbours (the only place rounding s instead of s + t can differ) t decides the side."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    r32 = s.astype(np.float32)
    r = r32.astype(np.float64)
    up, dn = np.nextafter(r32, np.float32(np.inf)).astype(np.float64), np.nextafter(r32, np.float32(-np.inf)).astype(np.float64)
    r = np.where((s == (r + up) / 2) & (t > 0), up, r)
    return np.where((s == (r + dn) / 2) & (t < 0) & (r == r32), dn, r)


@case_of("bn_apply_saved")
def test_bn_apply_saved(lib, name):
    """z = relu(fma(y, sc, sh)), sc = gamma * invstd, sh = fma(-mean, sc, beta) per group and channel (bn_scale_shift): power-of-two scales on
    small integers exact in any order; random data bit-equal to the exact restatement of the three fp32 roundings (_fma32), above the grid
    cap as well."""
    c = AC.find("bn_apply_saved", name)
    rng = np.random.default_rng(c["seed"])
    m, G, ch = c["m"], c["g"], c["c"]
    for kind in ("pow2", "rand"):
        if kind == "pow2":
            y = rng.integers(-8, 9, (G, m, ch)).astype(np.float32)
            gamma = (2.0 ** rng.integers(-2, 3, ch) * rng.choice([-1.0, 1.0], ch)).astype(np.float32)
            invstd = (2.0 ** rng.integers(-2, 3, (G, ch))).astype(np.float32)
            mean, beta = rng.integers(-4, 5, (G, ch)).astype(np.float32), rng.integers(-4, 5, ch).astype(np.float32)
        else:
            y = rng.standard_normal((G, m, ch)).astype(np.float32)
            gamma, beta = rng.standard_normal(ch).astype(np.float32), rng.standard_normal(ch).astype(np.float32)
            invstd, mean = rng.uniform(0.2, 5.0, (G, ch)).astype(np.float32), rng.standard_normal((G, ch)).astype(np.float32)
        g = Guarded()
        d_y, d_m, d_i = g.inp(y, 0, "y"), g.inp(mean, 0, "mean"), g.inp(invstd, 0, "invstd")
        d_g, d_b, d_z = g.inp(gamma, 0, "gamma"), g.inp(beta, 0, "beta"), g.out((G, m, ch), torch.float32, 0, "z")
        aux(lib, "bn_apply", name, p=[d_y, d_m, d_i, d_g, d_b, d_z], i=[m, G, ch])
        g.check(name)
        sc = _f32(gamma.astype(np.float64)[None, :] * invstd.astype(np.float64))      # (a product of two fp32 values is exact in float64)
        sh = _fma32(-mean, sc, np.broadcast_to(beta[None, :], mean.shape))
        ref = np.maximum(_fma32(y, sc[:, None, :], sh[:, None, :]), 0.0)
        got = host(d_z)
        assert (got >= 0).all(), name
        assert np.array_equal(got.astype(np.float64), ref), "%s %s: %d elements differ" % (name, kind, int((got != ref).sum()))


# ==========================================================================================================================================
# the combined weight-pack launch
# ==========================================================================================================================================
@case_of("pack_all")
def test_pack_all(lib, name):
    """The engine's multi-layer launch with its own table: every element of the arena against the OIHW gather of the documented layouts,
    everything else (padding rows / columns, alignment gaps, packs outside the mask) the pre-fill; the two clear regions all-zero cells
    when passed, untouched when not."""
    from ocl_amd import ffi
    c = AC.find("pack_all", name)
    rng = np.random.default_rng(c["seed"])
    sizes, table = (ffi.i64 * 2)(), (ffi.i64 * (9 * 32))()
    L = lib.ocl_test_pack_all(c["hw"], c["nf"], c["mask"], None, None, None, 0, None, 0, table, 32, sizes, None)
    assert L == 20, lib.ocl_last_error()
    n_params, arena_floats = sizes[0], sizes[1]
    params = rng.standard_normal(n_params).astype(np.float32)
    cells_a, cells_b = 192000, 37          # (16-byte cells; the first is larger than one stride of the launch's clearing row)
    g = Guarded()
    d_p = g.inp(params, 0, "params")
    d_arena = g.out((arena_floats,), torch.float32, 0, "arena")
    d_za, d_zb = g.out((cells_a * 4,), torch.float32, 0, "zero_a"), g.out((cells_b * 4,), torch.float32, 0, "zero_b")
    za, zb = (d_za, d_zb) if c["clear"] else (None, None)
    rc = lib.ocl_test_pack_all(c["hw"], c["nf"], c["mask"], C.c_void_p(d_p.data_ptr()), C.c_void_p(d_arena.data_ptr()),
                               C.c_void_p(za.data_ptr()) if za is not None else None, cells_a if c["clear"] else 0,
                               C.c_void_p(zb.data_ptr()) if zb is not None else None, cells_b if c["clear"] else 0, None, 0, None, stream())
    assert rc == L, lib.ocl_last_error()
    g.check(name)
    ref = Guarded.poison_array(arena_floats, np.float32)       # (the pre-fill of the leg that runs: -7777, or all-ones bits in the NaN leg)
    for l in range(L):
        w_off, tf_off, td_off, Cout, Cin, ntaps, CinP, CoutP, CiP = table[9 * l: 9 * l + 9]
        w = params[w_off: w_off + Cout * Cin * ntaps].reshape(Cout, Cin, ntaps)
        if c["mask"] & 1:
            A = ref[tf_off: tf_off + ntaps * CinP * CoutP].reshape(ntaps, CinP // 4, CoutP, 4)     # [t][ci >> 2][co][ci & 3]
            for ci in range(Cin):
                A[:, ci >> 2, :Cout, ci & 3] = w[:, ci, :].T
        if (c["mask"] & 2) and td_off >= 0:
            B = ref[td_off: td_off + ntaps * Cout * CiP].reshape(ntaps, Cout // 4, CiP, 4)         # [t][co >> 2][ci][co & 3]
            for co in range(Cout):
                B[:, co >> 2, :Cin, co & 3] = w[co].T
    assert Guarded.is_poison(ref).any() and not Guarded.is_poison(ref).all()
    got = host(d_arena)
    assert same_bits(got, ref), "%s: %d arena elements differ" % (name, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    for d_t, what in ((d_za, "zero_a"), (d_zb, "zero_b")):
        raw = host(d_t).view(np.uint32)
        if c["clear"]:
            assert not raw.any(), "%s: %s is not all-zero cells" % (name, what)
        else:
            assert Guarded.is_poison(host(d_t)).all(), "%s: %s was written without being passed" % (name, what)


# ==========================================================================================================================================
# the head chain
# ==========================================================================================================================================
def lin_check(case, tensor, got, a64, b64, extra=None):
    """got = a @ b (+ extra, broadcast) within the small GEMM's bound; a, b, extra float64 views of the engine's fp32 tensors."""
    ref, terms = a64 @ b64, np.abs(a64) @ np.abs(b64)
    if extra is not None:
        ref, terms = ref + extra, terms + np.abs(extra)
    PB.check_derived(REPORT, case, tensor, got, ref, 1.01 * (a64.shape[1] + 2) * U * terms)


def worst_rows(report, start, case):
    """Keep the row closest to its bound of each tensor family the head case recorded since `start` (the report stays readable)."""
    rows, keep = report[start:], {}
    del report[start:]
    for r in rows:
        fam = r[1].split("[")[0]
        if fam not in keep or r[5] > keep[fam][5]:
            keep[fam] = r
    report.extend(keep.values())


@case_of("head")
def test_head(lib, name):
    """head_forward on a given feature batch, then the head half of the backward, every stage tensor against the float64 stage function of
    the previous ENGINE tensor (ReLU mask: the engine's h1 > 0).  The stage checks judge the overwrite-mode run.  An accumulate case runs
    the hook twice on the same feat, dout and params -- overwriting, then accumulating onto a random pre-fill: the stage tensors are
    bit-identical, and every head gradient is pre-fill + the overwrite-mode result within one fp32 addition's rounding,
    |g_acc - (pre + g_ow)| <= 2^-24 |pre + g_ow|.  encoder.linear of a SupConResNet: gradient exactly 0 when overwriting, bit-unchanged when
    accumulating.  Nothing outside the head's tensors changes in either run."""
    from ocl_amd import ffi
    c = AC.find("head", name)
    rng = np.random.default_rng(c["seed"])
    kind, hw, acc = c["kind"], c["hw"], c["acc"]
    side_min = lib.ocl_test_head_side_min_batch(hw)
    n = c["n"]
    if n == "side":
        assert side_min > 0, "this process keeps every pass on one stream"
        n = side_min
    info = net_info(lib, hw, 20, c["n_classes"], kind, c["feat_dim"], n)
    T, FD, OD = info["tensors"], info["feat"], info["out"]
    assert FD == (160 if hw == 32 else 640) and OD == {0: c["n_classes"], 1: c["feat_dim"], 2: c["feat_dim"], 3: FD}[kind]
    params = (rng.standard_normal(info["n_params"]) * 0.1).astype(np.float32)
    grads0 = rng.standard_normal(info["n_params"]).astype(np.float32)
    feat = np.abs(rng.standard_normal((n, FD))).astype(np.float32)
    zero_row = kind in (2, 3) and n >= 2
    assert zero_row == ("head:zero_feat_row" in c["also"]) and (kind == 1) == ("head:dead_h1_columns" in c["also"])
    if zero_row:
        feat[1] = 0.0
    dout = rng.standard_normal((n, OD)).astype(np.float32)

    def P(tname):
        off, shp = T[tname]
        return params[off: off + int(np.prod(shp))].reshape(shp)
    lin = "linear" if kind == 0 else "encoder.linear"
    dead = [3, 64, FD - 1]
    if kind == 1:
        P("head.0.weight")[dead] = 0.0
        P("head.0.bias")[dead] = -1.0
    head_tensors = sorted(k for k in T if k.startswith(("head.", lin)))
    outside = np.ones(info["n_params"], bool)
    for tname in head_tensors:
        off, shp = T[tname]
        outside[off: off + int(np.prod(shp))] = False
    stage_shapes = (("h1", (n, FD)), ("h2", (n, OD)), ("norms", (n,)), ("out", (n, OD)), ("dh2", (n, OD)), ("dh1", (n, FD)), ("dfeat", (n, FD)))

    def run(accumulate):
        g = Guarded()
        d_p, d_g = g.inp(params, 0, "params"), g.out((info["n_params"],), torch.float32, 0, "grads", init=grads0)
        d_feat, d_dout = g.inp(feat, 0, "feat"), g.inp(dout, 0, "dout")
        o = {k: g.out(shape, torch.float32, 0, k) for k, shape in stage_shapes}
        a = ffi.TestHeadArgs()
        a.head, a.hw, a.nf, a.n, a.n_classes, a.feat_dim, a.accumulate, a.side_stream = kind, hw, 20, n, c["n_classes"], c["feat_dim"], accumulate, -1
        a.n_params = info["n_params"]
        a.params, a.grads, a.feat, a.dout = d_p.data_ptr(), d_g.data_ptr(), d_feat.data_ptr(), d_dout.data_ptr()
        for k, t in o.items():
            setattr(a, k, t.data_ptr())
        ok(lib, lib.ocl_test_head(C.byref(a), stream()), name)
        g.check(name)
        assert a.side_stream == (1 if side_min and n >= side_min else 0), "%s: stream decision %d (side stream from n = %d)" % (name, a.side_stream, side_min)
        grads = host(d_g)
        assert grads[outside].tobytes() == grads0[outside].tobytes(), "%s: a gradient outside the head was written" % name
        return {k: host(t) for k, t in o.items()}, grads

    def G(grads, tname):
        off, shp = T[tname]
        return grads[off: off + int(np.prod(shp))].reshape(shp)

    # ---- overwrite mode: every stage against float64 of the engine's own previous tensor --------------------------------------------------
    e, grads = run(0)
    e64 = {k: v.astype(np.float64) for k, v in e.items()}
    used = {0: (), 1: ("h1", "h2", "norms", "dh2", "dh1"), 2: ("h2", "norms", "dh2"), 3: ("norms",)}[kind] + ("out", "dfeat")
    for k in e:
        if k not in used:
            assert Guarded.is_poison(e[k]).all(), "%s: kind %d wrote %s" % (name, kind, k)
    case, start = "head/" + name, len(REPORT)
    f64, d64 = feat.astype(np.float64), dout.astype(np.float64)
    W = {k: P(k).astype(np.float64) for k in head_tensors}

    def wb_check(wname, bname, dy64, x64):
        """dW = dy^T x (K = n products) and db = colsum(dy) (n additions)."""
        lin_check(case, "d" + wname, G(grads, wname), dy64.T, x64)
        PB.check_derived(REPORT, case, "d" + bname, G(grads, bname), dy64.sum(0), 1.01 * dy64.shape[0] * U * np.abs(dy64).sum(0))

    checked = []
    if kind == 0:
        lin_check(case, "out", e["out"], f64, W["linear.weight"].T, extra=W["linear.bias"][None, :])
        wb_check("linear.weight", "linear.bias", d64, f64)
        lin_check(case, "dfeat", e["dfeat"], d64, W["linear.weight"])
        checked = ["linear.weight", "linear.bias"]
    else:
        for tname in (lin + ".weight", lin + ".bias"):
            assert not G(grads, tname).view(np.uint32).any(), "%s: %s is not +0.0 everywhere" % (name, tname)
        checked = [lin + ".weight", lin + ".bias"]
        if kind == 1:
            pre = f64 @ W["head.0.weight"].T + W["head.0.bias"][None, :]
            terms = np.abs(f64) @ np.abs(W["head.0.weight"]).T + np.abs(W["head.0.bias"])[None, :]
            PB.check_derived(REPORT, case, "h1", e["h1"], np.maximum(pre, 0.0), 1.01 * (FD + 2) * U * terms)     # (ReLU is 1-Lipschitz)
            assert (e["h1"][:, dead] == 0).all() and (e["h1"] >= 0).all(), "%s: the dead columns of h1 are alive" % name
            lin_check(case, "h2", e["h2"], e64["h1"], W["head.2.weight"].T, extra=W["head.2.bias"][None, :])
            w2, b2, x2 = "head.2.weight", "head.2.bias", e64["h1"]
        elif kind == 2:
            lin_check(case, "h2", e["h2"], f64, W["head.weight"].T, extra=W["head.bias"][None, :])
            w2, b2, x2 = "head.weight", "head.bias", f64
        v = e["h2"] if kind in (1, 2) else feat
        check_l2_fwd(case, v, e["out"], e["norms"])
        dv = e["dh2"] if kind in (1, 2) else e["dfeat"]
        check_l2_bwd(case, v, dout, dv)
        if zero_row and kind == 3:      # the all-zero feature row is a clamped row of the normalisation: out 0, gradient dout / 1e-12
            assert e["norms"][1] == np.float32(1e-12) and not e["out"][1].view(np.uint32).any(), "%s: the zero row is not clamped" % name
        if zero_row and kind == 2:      # ... and contributes the bias alone to the projection
            assert same_bits(e["h2"][1], P("head.bias")), "%s: h2 of the zero feature row is not the bias" % name
        if kind in (1, 2):
            wb_check(w2, b2, e64["dh2"], x2)
            checked += [w2, b2]
        if kind == 1:
            mask = (e["h1"] > 0).astype(np.float64)
            full, terms = e64["dh2"] @ W[w2], np.abs(e64["dh2"]) @ np.abs(W[w2])
            PB.check_derived(REPORT, case, "dh1", e["dh1"], full * mask, 1.01 * (OD + 2) * U * terms * mask)
            assert not e["dh1"][:, dead].view(np.uint32).any(), "%s: gradient through a dead column" % name
            wb_check("head.0.weight", "head.0.bias", e64["dh1"], f64)
            lin_check(case, "dfeat", e["dfeat"], e64["dh1"], W["head.0.weight"])
            checked += ["head.0.weight", "head.0.bias"]
        elif kind == 2:
            lin_check(case, "dfeat", e["dfeat"], e64["dh2"], W[w2])
    assert sorted(checked) == head_tensors
    # ---- accumulate mode on the same data: pre-fill + the overwrite-mode result, one fp32 addition ---------------------------------------------
    if acc:
        e_acc, grads_acc = run(1)
        for k in e:
            assert same_bits(e_acc[k], e[k]), "%s: stage tensor %s depends on accumulate" % (name, k)
        for tname in head_tensors:
            pre, g_ow, g_acc = G(grads0, tname), G(grads, tname), G(grads_acc, tname)
            if kind != 0 and tname.startswith(lin):
                assert same_bits(g_acc, pre), "%s: %s changed while accumulating" % (name, tname)
                continue
            want = pre.astype(np.float64) + g_ow.astype(np.float64)
            PB.check_derived(REPORT, case, "acc:d" + tname, g_acc, want, U * np.abs(want))
    worst_rows(REPORT, start, case)


# ==========================================================================================================================================
# the NaN leg: one case per stage (per kernel of the glue ops; per head kind, overwrite and accumulate)
# ==========================================================================================================================================
NAN_LEG = [("layout", "one32"), ("layout", "two"), ("avgpool", "11x11_n3"), ("l2norm", "d128_n7"), ("relu_bwd", "n257"), ("colsum", "9x100"),
           ("fill", "n257"), ("fill", "n0"), ("bn_fold", "net32"), ("bn_apply_saved", "m1023_g2"), ("pack_all", "hw32_TF_noclear"),
           ("pack_all", "hw32_ALL_clear"), ("head", "k0_hw32_n7_acc0"), ("head", "k1_hw32_n7_acc0"), ("head", "k1_hw32_n7_acc1"),
           ("head", "k2_hw32_n7_acc0"), ("head", "k3_hw32_n7_acc0"), ("head", "k1_hw32_side_acc0")]
STAGE_TESTS = {"layout": test_layout, "avgpool": test_avgpool, "l2norm": test_l2norm, "relu_bwd": test_relu_bwd, "colsum": test_colsum,
               "fill": test_fill, "bn_fold": test_bn_fold, "bn_apply_saved": test_bn_apply_saved, "pack_all": test_pack_all, "head": test_head}


@pytest.mark.parametrize("op,name", NAN_LEG, ids=lambda v: v)
def test_nan_leg_equals_the_finite_leg(lib, op, name):
    """The stage's test once more with every output, workspace and guard region holding 0xFFFFFFFF instead of -7777 / 4096
    (guarded.run_both_legs): its own assertions hold, and every output -- every stage tensor of the head chain, the whole pack arena with
    its unwritten padding -- is bit-identical in the two legs."""
    from guarded import run_both_legs
    assert set(STAGE_TESTS) == set(AC.CASES) and {op_ for op_, _ in NAN_LEG} == set(AC.CASES)
    AC.find(op, name)
    n0 = len(REPORT)
    try:
        run_both_legs(lambda: STAGE_TESTS[op](lib, name), "%s/%s" % (op, name))
    finally:
        del REPORT[n0:]
