"""GPU: the BatchNorm statistics chain on ill-conditioned and degenerate channels, in both batch-sum modes, against float64 and exact-rational
references (tests/bn_cond_ref.py) on the cases of tests/bn_cond_cases.py.

(a) producers: every stats epilogue on real-valued outputs whose channels realise |mean| / std from 0 to 1000, a dead and a constant channel,
    scales 1e-4 and 1e3 -- cell totals against the float64 sums of the kernel's own output, and the moments derived from them against two-pass
    float64 moments;
(b) consumers of given cells (totals exact for an ill-conditioned y): saved and running statistics to the ulp, z within a per-element bound;
    totals whose one-pass variance comes out slightly negative;
(c) one ReLU decision, six places that take it: on ladders of adjacent fp32 values around the root of fma(y, sc, sh), every place agrees bit
    for bit with the exact decision;
(d) the backward paths on channels of mixed conditioning and gradient scale, bounded per channel;
(e) one whole train pass on bright low-contrast and near-flat images, with test_train_forward_backward_vs_oracle's assertions.

With OCL_PARITY_REPORT=<file> the figures go to bn_cond_parity.txt next to it (profiles/bn_cond_parity.txt)."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest
import torch

import bn_cond_cases as BC
import bn_cond_ref as R
import layer_forms as LF
import parity_bounds as PB
import test_gpu_layers as TL
from test_gpu_layers import EPI_BNB, EPI_STATS, cell_totals, dev, encode_cells, find_entry, p, run_conv, run_wgrad, shape_of

pytestmark = pytest.mark.gpu

U, FX = R.U, R.FX
REPORT, NOTES, T0 = [], [], time.time()
SITE_K, REGIME_ERR, Z_ERR = {}, {}, {}     # key -> worst err / (U sum|.|);  regime -> worst (rel var err, rel invstd err);  regime -> worst |z err|


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    yield L
    L.ocl_set_deterministic(0)
    path = os.environ.get("OCL_PARITY_REPORT")
    if path and REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "bn_cond_parity.txt"), "w") as f:
            f.write("# the BatchNorm statistics chain on ill-conditioned channels (tests/test_gpu_bn_cond.py): error against float64, the derived bound\n"
                    "# (tests/bn_cond_ref.py) and error / bound (must be <= 1); the row of a tensor is its element closest to its bound\n")
            f.write("%-58s %-14s %12s %12s %12s %8s\n" % ("case", "tensor", "kernel_err", "e_ref", "bound", "ratio"))
            for row in REPORT:
                f.write("%-58s %-14s %12.4g %12s %12.4g %8.3f\n" % row)
            f.write("# measured K = |cell total - float64 sum| / (2^-24 sum|.|) per stats epilogue (the bound's constant is 8)\n")
            for k in sorted(SITE_K):
                f.write("K %-40s %.3f\n" % (k, SITE_K[k]))
            f.write("# per regime, worst over the producer cases: relative error of var and of invstd = 1 / sqrt(var + eps) derived from the cells,\n"
                    "# against the two-pass float64 moments of the kernel's own output; beside it torch-CPU fp32 var() of the same output (dead / const: absolute)\n")
            for k in BC.NAMES:
                if k in REGIME_ERR:
                    e = REGIME_ERR[k]
                    f.write("regime %-8s engine var_rel %.3e invstd_rel %.3e   torch-fp32 var_rel %.3e invstd_rel %.3e   ratio (var) %s\n" % (
                        (k,) + tuple(e) + ("%.3g" % (e[0] / e[2]) if e[2] > 0 else "-",)))
            f.write("# per regime, worst |z - float64| of bn_fwd from exact cells (one set), beside torch-CPU fp32 F.batch_norm on the same data\n")
            for k in BC.NAMES:
                if k in Z_ERR:
                    f.write("regime %-8s engine z_err %.3e   torch-fp32 z_err %.3e   ratio %s\n" % (
                        k, Z_ERR[k][0], Z_ERR[k][1], "%.3g" % (Z_ERR[k][0] / Z_ERR[k][1]) if Z_ERR[k][1] > 0 else "-"))
            for line in NOTES:
                f.write(line + "\n")
            f.write("# wall time of this file's tests up to here: %.1f s\n" % (time.time() - T0))


def T64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def host(t):
    return t.double().cpu().numpy()


def with_mode(fn):
    @functools.wraps(fn)
    def run(lib, det, *a, **k):
        lib.ocl_set_deterministic(det)
        try:
            return fn(lib, det, *a, **k)
        finally:
            lib.ocl_set_deterministic(0)
    return run


def bn_fwd(lib, y, groups, gamma, beta, st, relu=1, second=None):
    """ocl_test_bn_fwd on y [n, h, w, c] float64 with the cells st; second = (yb, gamma_b, beta_b, cells_b).  Returns a dict of host float64 arrays."""
    from ocl_amd import ffi
    n, c = y.shape[0], y.shape[-1]
    a = ffi.TestBnFwdArgs(m_per_group=y[0].size // c * (n // groups), groups=groups, c=c, relu=relu, momentum=0.1, eps=1e-5)
    keep = {}

    def put(name, t):
        keep[name] = t if t.is_cuda else dev(t.float() if t.is_floating_point() else t)
        setattr(a, name, p(keep[name]))
    put("y", T64(y)); put("z", torch.full(y.shape, float("nan"))); put("gamma", T64(gamma)); put("beta", T64(beta))
    put("stats", st)
    for s in ("", "_b") if second else ("",):
        put("running_mean" + s, torch.zeros(c)); put("running_var" + s, torch.ones(c)); put("nbt" + s, torch.zeros(1, dtype=torch.int64))
        put("save_mean" + s, torch.zeros(groups, c)); put("save_invstd" + s, torch.zeros(groups, c))
    if second:
        put("yb", T64(second[0])); put("gamma_b", T64(second[1])); put("beta_b", T64(second[2])); put("stats_b", second[3])
    assert lib.ocl_test_bn_fwd(C.byref(a), None) == 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    TL.assert_slack_untouched(keep["z"], "bn_fwd z")
    return {k: (int(v[0]) if k.startswith("nbt") else host(v)) for k, v in keep.items() if k not in ("stats", "stats_b")}


def within_ulps(got, ref64, k, what):
    """|got - ref64| <= k ulp32(ref64), got an fp32 array, ref64 the float64 value it should be the rounding of."""
    err, lim = np.abs(got - ref64), k * R.ulp32(ref64)
    assert np.isfinite(got).all() and (err <= lim).all(), "%s: off by %.3g ulp" % (what, float((err / R.ulp32(ref64)).max()))


# =====================================================================================================================================
# (a) producers
# =====================================================================================================================================
def _dims(d):
    return (d.n, d.hin, d.win, d.cin, d.cout, d.k, d.stride)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("key", [c["key"] for c in BC.PRODUCERS])
@with_mode
def test_producer_sums_and_moments_on_ill_conditioned_outputs(lib, det, key):
    producer_case(lib, det, key)


def producer_case(lib, det, key, want=None, force=None):
    """One producer case at one and (even n) two groups.  want: the form the hook must report (default: key); force: fields set in the layer's
    description (the switch-only family runs the layer of a covered key in a child process, see test_conv_w_kernel_producer_in_a_fresh_process)."""
    want = want or key
    e = TL._layer_desc(lib, key) if force is not None else find_entry(lib, key)
    xf = key.endswith("_xf")
    for groups in (1, 2):
        d = type(e.desc).from_buffer_copy(e.desc)
        if groups == 2 and d.n % 2:
            continue
        d.groups = groups
        for a_, v_ in (force or {}).items():
            setattr(d, a_, v_)
        seed = sum(map(ord, key)) + groups
        ops = {}
        if xf:   # the staged activation: BatchNorm + ReLU of a raw output; the constant channel through gamma = 0, beta = 1
            rng = np.random.default_rng(seed)
            cin_t = shape_of(d)[0]
            yin = (rng.standard_normal((d.n, d.hin, d.win, cin_t)) * 2 + 0.3).astype(np.float32).astype(np.float64)
            gamma, beta = BC.affine(rng, cin_t)
            cc = BC.const_channel(d.cin)
            gamma[cc], beta[cc] = 0.0, 1.0
            tot = R.exact_totals(yin, groups)
            st_in = encode_cells(tot, det)
            z32, _, _, _ = R.model_forward(yin, groups, gamma, beta, cell_totals(st_in, groups, cin_t, det))
            act = np.maximum(z32, 0).astype(np.float64)
            assert (act[..., cc] == 1.0).all()
            _, w = BC.producer_inputs(_dims(d), groups, seed, act=act)
            x = T64(yin)
            sm, si = dev(torch.zeros(groups, cin_t)), dev(torch.zeros(groups, cin_t))
            ops = dict(xf=1, xf_stats=st_in, xf_gamma=T64(gamma), xf_beta=T64(beta), xf_save_mean=sm, xf_save_invstd=si)
        else:
            x, w = BC.producer_inputs(_dims(d), groups, seed)
        got, forms, stats = run_conv(lib, d, x, w, EPI_STATS, **ops)
        epi = key.split("/")[1]
        keys = [LF.conv_key(f, epi) for f in forms]
        assert want in keys, (want, keys)
        case = "producer/%s/g%d/det%d" % (want, groups, det)
        y = got.numpy()
        cout = y.shape[-1]
        M = y[0].size // cout * (d.n // groups)
        # the output itself against the float64 convolution (one group of the input-transform forms: of the exact staged activation)
        xin = T64(act) if xf else x
        ref = BC.conv64(xin, w, d.stride).numpy()
        mag = BC.conv64(xin.abs(), w.abs(), d.stride).numpy()
        PB.check_derived(REPORT, case, "out", y, ref, 1.01 * (d.k * d.k * d.cin) * U * mag)
        # the cells against the float64 sums of the kernel's own output; deterministic mode: one 2^-40 truncation per partial sum, their count
        # per cell from the launch geometry the hook reports
        form = forms[keys.index(want)]
        nparts = R.partials_per_cell(form)
        assert 1 <= nparts <= M * groups, (case, nparts)
        tot = cell_totals(stats, groups, cout, det)
        yg = R.group_view(y, groups)
        s1, s2, a1 = yg.sum(axis=1), (yg * yg).sum(axis=1), np.abs(yg).sum(axis=1)
        PB.check_derived(REPORT, case, "sum", tot[:, 0], s1, R.sums_bound(a1, nparts, det))
        PB.check_derived(REPORT, case, "sumsq", tot[:, 1], s2, R.sums_bound(s2, nparts, det))
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.nanmax(np.concatenate([np.abs(tot[:, 0] - s1) / (U * a1), np.abs(tot[:, 1] - s2) / (U * s2)]))
        if not det:   # (the constant of the fp32 partials; in deterministic mode the 2^-40 truncations of a 1e-4-scale channel would dominate it)
            SITE_K[want] = max(SITE_K.get(want, 0.0), float(k))
        # conv_s_kernel's epilogue is restated bit for bit (bn_cond_ref.conv_s_tile_totals): the cell totals are the restatement's up to the
        # order of the float64 additions.  The sums of squares must be ONE of the two legal evaluations of the source's row16_sum(z * z) --
        # the square rounded and then added, or contracted into the butterfly's first add -- in every cell of the launch: any other fp32
        # rounding in the epilogue (one more fp32 add of two partial sums before the conversion to double) matches neither, where the 8 U
        # bound leaves room for it.
        if form.family == 2:
            assert (y[0].size // cout) % 16 == 0
            fits = {}
            for contracted in (False, True):
                mt, ntile = R.conv_s_tile_totals(y, groups, det, contracted)
                assert ntile <= nparts
                lim = ntile * 2.0 ** -52 * np.stack([a1, s2], axis=1) + (FX if det else 0.0)
                err = np.abs(tot - mt)
                fits[contracted] = (bool((err <= lim).all()), mt, lim)
            mt, lim = fits[False][1], fits[False][2]
            PB.check_derived(REPORT, case, "sum(tiles)", tot[:, 0], mt[:, 0], lim[:, 0])
            which = True if fits[True][0] else False
            NOTES.append("tiles %s: sums of squares match the %s evaluation" % (case, "contracted" if which else "two-rounding"))
            PB.check_derived(REPORT, case, "sumsq(tiles)", tot[:, 1], fits[which][1][:, 1], fits[which][2][:, 1])
        # the moments every consumer derives from them against the two-pass moments
        mean, var, _ = R.moments_from_totals(tot[:, 0], tot[:, 1], M)
        m2, v2 = R.two_pass_moments(y, groups)
        bm, bv = R.moments_bound(y, groups, nparts, det)
        PB.check_derived(REPORT, case, "mean", mean, m2, bm)
        PB.check_derived(REPORT, case, "var", var, v2, bv)
        v32 = torch.from_numpy(yg).float().var(dim=1, unbiased=False).double().numpy()     # torch-CPU fp32 on the same data
        for c in range(cout):
            name = BC.regime_of(c)[0]
            rv = float(np.abs(var[:, c] - v2[:, c]).max() / max(v2[:, c].max(), 1e-300)) if v2[:, c].max() > 0 else float(np.abs(var[:, c]).max())
            ri = float((np.abs(R.invstd_of(var[:, c]) - R.invstd_of(v2[:, c])) / R.invstd_of(v2[:, c])).max())
            tv = v32[:, c]
            rtv = float(np.abs(tv - v2[:, c]).max() / v2[:, c].max()) if v2[:, c].max() > 0 else float(np.abs(tv).max())
            rti = float((np.abs(R.invstd_of(tv) - R.invstd_of(v2[:, c])) / R.invstd_of(v2[:, c])).max())
            old = REGIME_ERR.get(name, (0.0, 0.0, 0.0, 0.0))
            REGIME_ERR[name] = (max(old[0], rv), max(old[1], ri), max(old[2], rtv), max(old[3], rti))
        # dead and constant rows: the output is exactly constant, borders included, so their sums are exact products
        for c in range(cout):
            name, mu, _, kind = BC.regime_of(c)
            if kind == "const":
                sign = np.where((np.arange(d.n) < d.n // groups) | xf, 1.0, -1.0)[:, None, None]
                assert (y[..., c] == mu * sign).all(), (case, name)


_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
import ocl_amd
from ocl_amd import ffi
ffi.init()
torch.set_num_threads(16)
import test_gpu_bn_cond as T
lib = ffi.lib()
for det in (0, 1):
    lib.ocl_set_deterministic(det)
    T.producer_case(lib, det, %(key)r, want=%(want)r, force=%(force)r)
lib.ocl_set_deterministic(0)
print("RESULT " + json.dumps({"K": T.SITE_K, "rows": [list(r) for r in T.REPORT]}))
"""


def test_conv_w_kernel_producer_in_a_fresh_process(lib):
    """conv_w_kernel's stats epilogue runs only with OCL_CONV_WX=0, a switch read once per process: the wx3x1/stats layer in a fresh child
    interpreter (never os.exec*), both batch-sum modes, one and two groups, the same assertions as every other producer."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    c = BC.SWITCH_PRODUCER
    src = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), key=c["key"], want=c["want"], force=c["force"])
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", **c["env"]), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert c["want"] in res["K"], res["K"]
    SITE_K.update(res["K"])
    REPORT.extend(tuple(row) for row in res["rows"])


# =====================================================================================================================================
# (b) consumers of given cells
# =====================================================================================================================================
def _consumer_case(seed, n, hw, c, groups, det):
    rng = np.random.default_rng(seed)
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    st = encode_cells(R.exact_totals(y, groups), det)
    tot = cell_totals(st, groups, c, det)   # what the kernel decodes (deterministic mode: the totals truncated to 2^-40)
    return y, gamma, beta, st, tot


def _check_saved(case, out, sfx, tot, M, groups):
    mean, var, _ = R.moments_from_totals(tot[:, 0], tot[:, 1], M)
    within_ulps(out["save_mean" + sfx], mean, 1, case + " save_mean" + sfx)
    within_ulps(out["save_invstd" + sfx], R.invstd_of(var), 2, case + " save_invstd" + sfx)
    c = mean.shape[1]
    rm, rv, mag_m, mag_v = R.running_recurrence(mean, var, M, np.zeros(c), np.ones(c))
    # 4 ulp of the rounded recurrence; where the groups' terms cancel (the largest term above twice the result: means of either sign around 0 in
    # the r0 / tiny / big channels) no fp32 evaluation can meet that, and the ulp is the largest term's (see running_recurrence)
    for what, ref, mag in (("running_mean", rm, mag_m), ("running_var", rv, mag_v)):
        got, ref = out[what + sfx], ref.astype(np.float64)
        lim = 4 * R.ulp32(np.where(mag <= 2 * np.abs(ref), ref, mag))
        assert np.isfinite(got).all() and (np.abs(got - ref) <= lim).all(), \
            "%s %s%s: off by %.3g times its limit of 4 ulp" % (case, what, sfx, float((np.abs(got - ref) / lim).max()))
    assert out["nbt" + sfx] == groups


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups,two", [(10, 32, 20, 2, False), (6, 16, 40, 1, True), (12, 8, 160, 2, True), (5, 4, 80, 1, False)])
@with_mode
def test_bn_forward_of_exact_cells_on_ill_conditioned_channels(lib, det, n, hw, c, groups, two):
    case = "bn_fwd/n%d_hw%d_c%d_g%d_%s/det%d" % (n, hw, c, groups, "two" if two else "one", det)
    y, gamma, beta, st, tot = _consumer_case(n * 100 + c, n, hw, c, groups, det)
    M = n // groups * hw * hw
    second = None
    if two:
        yb, gb, bb, stb, totb = _consumer_case(n * 100 + c + 1, n, hw, c, groups, det)
        second = (yb, gb, bb, stb)
    out = bn_fwd(lib, y, groups, gamma, beta, st, relu=1, second=second)
    _check_saved(case, out, "", tot, M, groups)
    z64, mean, var, invstd = R.bn_forward64(y, groups, gamma, beta)
    bound = R.z_bound(y, groups, gamma, beta, mean, invstd)
    # the moments from exact totals against the two-pass moments: only the float64 roundings of the formula and the cells' encoding are left
    mk, vk, _ = R.moments_from_totals(tot[:, 0], tot[:, 1], M)
    bm, bv = R.exact_moments_bound(y, groups, det)
    PB.check_derived(REPORT, case, "mean(exact)", mk, mean, bm)
    PB.check_derived(REPORT, case, "var(exact)", vk, var, bv)
    if two:
        _check_saved(case, out, "_b", totb, M, groups)
        zb64, meanb, varb, invstdb = R.bn_forward64(yb, groups, gb, bb)
        bound = bound + R.z_bound(yb, groups, gb, bb, meanb, invstdb) + U * np.abs(z64 + zb64)
        z64 = z64 + zb64
    PB.check_derived(REPORT, case, "z", out["z"], np.maximum(z64, 0), bound)
    if not two:   # a dead channel gives exactly relu(beta)
        for ch in range(c):
            if BC.regime_of(ch)[0] == "dead":
                assert (out["z"][..., ch] == max(beta[ch], 0.0)).all(), (case, ch)
    if not two:
        import torch.nn.functional as F
        per = n // groups
        zt = np.concatenate([F.batch_norm(T64(y[g * per:(g + 1) * per]).float().permute(0, 3, 1, 2), None, None, T64(gamma).float(), T64(beta).float(),
                                          True, 0.1, R.EPS).permute(0, 2, 3, 1).double().numpy() for g in range(groups)])
        err, errt = np.abs(out["z"] - np.maximum(z64, 0)), np.abs(np.maximum(zt, 0) - np.maximum(z64, 0))
        for ch in range(c):
            name = BC.regime_of(ch)[0]
            old = Z_ERR.get(name, (0.0, 0.0))
            Z_ERR[name] = (max(old[0], float(err[..., ch].max())), max(old[1], float(errt[..., ch].max())))


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups,family", BC.XF_CONSUMERS)
@with_mode
def test_input_transform_of_exact_cells_on_ill_conditioned_channels(lib, det, n, hw, c, groups, family):
    """The other consumer of exact cells: a convolution's input transform (identity on the centre tap, so the output is the staged activation),
    with the running update its lead workgroup makes: the same assertions as bn_fwd, at one and two groups, in the family the table names."""
    case = "conv_xf/n%d_hw%d_c%d_g%d/det%d" % (n, hw, c, groups, det)
    y, gamma, beta, st, tot = _consumer_case(n * 100 + c + 7, n, hw, c, groups, det)
    M = n // groups * hw * hw
    d = TL._desc(c, c, 3, 1, hw, n, groups, 0, xf=1)
    w = torch.zeros((c, c, 3, 3), dtype=torch.float64)
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    sm, si = dev(torch.zeros(groups, c)), dev(torch.zeros(groups, c))
    rm, rv, nbt = dev(torch.zeros(c)), dev(torch.ones(c)), dev(torch.zeros(1, dtype=torch.int64))
    got, forms, _ = run_conv(lib, d, T64(y), w, 0, xf=1, xf_stats=st, xf_gamma=T64(gamma), xf_beta=T64(beta), xf_save_mean=sm, xf_save_invstd=si,
                             xf_running_mean=rm, xf_running_var=rv, xf_nbt=nbt)
    assert [LF.FAMILIES[f.family] for f in forms] == [family], (case, [LF.conv_key(f, "stats_xf") for f in forms])
    out = dict(save_mean=host(sm), save_invstd=host(si), running_mean=host(rm), running_var=host(rv), nbt=int(nbt[0]))
    _check_saved(case, out, "", tot, M, groups)
    z64, mean, var, invstd = R.bn_forward64(y, groups, gamma, beta)
    PB.check_derived(REPORT, case, "act", got.numpy(), np.maximum(z64, 0), R.z_bound(y, groups, gamma, beta, mean, invstd))
    for ch in range(c):
        if BC.regime_of(ch)[0] == "dead":
            assert (got.numpy()[..., ch] == max(beta[ch], 0.0)).all(), (case, ch)


@pytest.mark.parametrize("det", [0, 1])
@with_mode
def test_slightly_negative_one_pass_variance_is_clamped(lib, det):
    """Every channel is the constant fl32(1000.1); channel j's sum of squares is j + 1 float64 ulps BELOW M c^2 (deterministic mode: the cells'
    truncation of M partial sums loses less than one such ulp more), so s2 / M - mean^2 < 0 in every channel: only the clamp stands between
    the forward and a NaN.  bn_fwd and the convolution's input transform."""
    n, hw, c, groups = 4, 8, 20, 1
    M = n * hw * hw
    y = np.full((n, hw, hw, c), BC.CONST)
    rng = np.random.default_rng(3)
    gamma, beta = BC.affine(rng, c)
    s2 = np.full(c, M * BC.CONST * BC.CONST)
    for j in range(c):
        for _ in range(j + 1):
            s2[j] = np.nextafter(s2[j], 0.0)
    tot = np.stack([np.full(c, M * BC.CONST), s2])[None]
    st = encode_cells(tot, det)
    tk = cell_totals(st, 1, c, det)
    _, var, raw = R.moments_from_totals(tk[:, 0], tk[:, 1], M)
    assert (raw < 0).all() and (var == 0).all(), raw
    case = "negvar/det%d" % det
    inv0 = 1.0 / np.sqrt(R.EPS)
    zb = R.z_bound(y, 1, gamma, beta, np.full((1, c), BC.CONST), np.full((1, c), inv0))
    out = bn_fwd(lib, y, 1, gamma, beta, st, relu=0)
    for k, v in out.items():
        assert np.isfinite(v).all(), (case, k)
    within_ulps(out["save_invstd"], np.full((1, c), inv0), 1, case + " save_invstd")
    within_ulps(out["save_mean"], np.full((1, c), BC.CONST), 1, case + " save_mean")
    PB.check_derived(REPORT, case, "z", out["z"], np.broadcast_to(beta, y.shape), zb)
    assert (out["running_var"] >= 0).all()
    # the same cells through a convolution's input transform (identity on the centre tap: the output is the staged activation)
    d = TL._desc(c, c, 3, 1, hw, n, 1, 0, xf=1)
    w = torch.zeros((c, c, 3, 3), dtype=torch.float64)
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    sm, si = dev(torch.zeros(1, c)), dev(torch.zeros(1, c))
    rm, rv, nbt = dev(torch.zeros(c)), dev(torch.ones(c)), dev(torch.zeros(1, dtype=torch.int64))
    got, forms, _ = run_conv(lib, d, T64(y), w, 0, xf=1, xf_stats=st, xf_gamma=T64(gamma), xf_beta=T64(beta), xf_save_mean=sm, xf_save_invstd=si,
                             xf_running_mean=rm, xf_running_var=rv, xf_nbt=nbt)
    assert np.isfinite(got.numpy()).all() and np.isfinite(host(rv)).all() and (host(rv) >= 0).all()
    within_ulps(host(si), np.full((1, c), inv0), 1, case + " xf_save_invstd")
    PB.check_derived(REPORT, case, "xf_act", got.numpy(), np.broadcast_to(np.maximum(beta, 0), y.shape), zb)


# =====================================================================================================================================
# (c) one ReLU decision, six places that take it
# =====================================================================================================================================
HALF = 64   # 129 rungs
ON_BOUNDARY = 6   # a dead channel (regime 6) whose beta is 0 in the ladder cases
assert BC.regime_of(ON_BOUNDARY)[0] == "dead"


def ladder_pixels(rng, n, hw, groups):
    """Per group, 2 * HALF + 1 scattered pixels (image, row, column) of that group's images: the first and the last pixel of the group (image
    corners) and border pixels included."""
    per, out = n // groups, []
    for g in range(groups):
        M = per * hw * hw
        assert M >= 2 * HALF + 1
        pick = rng.permutation(M)[: 2 * HALF + 1]
        pick[0], pick[1], pick[2] = 0, M - 1, hw - 1
        pick = np.unique(pick)
        while len(pick) < 2 * HALF + 1:
            pick = np.unique(np.concatenate([pick, rng.integers(0, M, 2 * HALF + 1 - len(pick))]))
        pick = rng.permutation(pick)
        out.append(np.stack([g * per + pick // (hw * hw), pick // hw % hw, pick % hw], axis=1))
    return out


def make_ladder(lib, det, n, hw, c, groups, seed):
    """Regime data y, cells that encode its moments, the statistics bn_fwd saves from them (read back from a first call), the exact scale / shift
    of those fp32 values, and y with rung j of every channel's ladder at pixel j of its group's scattered pixels."""
    rng = np.random.default_rng(seed)
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    beta[beta == 0] = 0.25      # (a root at exactly 0 would make a ladder of subnormals)
    beta[ON_BOUNDARY] = 0.0     # ... except on this dead channel, which gets no ladder: y = 0, sh = beta = 0, so EVERY element is exactly on the
                                # boundary (fma(y, sc, sh) == 0: not positive) -- a place that decides with >= instead of > differs everywhere
    st = encode_cells(R.exact_totals(y, groups), det)
    first = bn_fwd(lib, y, groups, gamma, beta, st, relu=1)
    sm, si = first["save_mean"].astype(np.float32), first["save_invstd"].astype(np.float32)
    sc, sh = R.scale_shift_exact(gamma[None, :], beta[None, :], sm, si)
    pix = ladder_pixels(rng, n, hw, groups)
    for g in range(groups):
        for ch in range(c):
            if ch == ON_BOUNDARY:
                assert sh[g, ch] == 0 and (y[..., ch] == 0).all()
                continue
            lad = R.ladder(R.root_f32(sc[g, ch], sh[g, ch]), HALF)
            y[pix[g][:, 0], pix[g][:, 1], pix[g][:, 2], ch] = lad.astype(np.float64)
    per = n // groups
    scb, shb = np.repeat(sc, per, axis=0)[:, None, None, :], np.repeat(sh, per, axis=0)[:, None, None, :]
    act = np.maximum(R.fma32(y.astype(np.float32), scb, shb), np.float32(0))
    dec = R.decide64(y, scb, shb)
    assert ((act > 0) == dec).all()
    # the ladders are not vacuous: the exact decision changes inside each, at least 8 rungs from either end (tests/test_cpu_bn_cond.py
    # checks the same on the model's statistics)
    for g in range(groups):
        dd = dec[pix[g][:, 0], pix[g][:, 1], pix[g][:, 2], :]
        flips = np.abs(np.diff(dd.astype(np.int8), axis=0)).sum(axis=0)
        where = np.abs(np.diff(dd.astype(np.int8), axis=0)).argmax(axis=0)
        lad_ch = np.arange(c) != ON_BOUNDARY
        assert (flips[lad_ch] == 1).all() and (where[lad_ch] >= 8).all() and (where[lad_ch] <= 2 * HALF - 9).all(), (flips, where)
        assert not dec[..., ON_BOUNDARY].any()
        for ch in (0, c - 1):   # the vectorised decision against the rational one, on whole ladders
            for j in range(2 * HALF + 1):
                i = tuple(pix[g][j])
                assert bool(dd[j, ch]) == R.decide_exact(y[i + (ch,)], sc[g, ch], sh[g, ch])
    return dict(y=y, gamma=gamma, beta=beta, st=st, sm=sm, si=si, sc=sc, sh=sh, act=act, dec=dec, pix=pix, n=n, hw=hw, c=c, groups=groups)


def same_bits(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    bad = got != ref
    assert not bad.any(), "%s: %d of %d elements differ (first %r: got %r, want %r)" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(ref[bad][0]))


def bn_bwd(lib, L, dz, one_pass, frozen, mask_from_y=1, zmask=None, sets=None):
    from ocl_amd import ffi
    n, hw, c, groups = L["n"], L["hw"], L["c"], L["groups"]
    sets = sets or [(L["y"], L["sm"], L["si"], L["gamma"], L["beta"])]
    a = ffi.TestBnBwdArgs(m_per_group=n // groups * hw * hw, groups=groups, c=c, nsets=len(sets), mask_from_y=mask_from_y, one_pass=one_pass, frozen=frozen)
    keep = [dev(T64(dz).float())]
    a.dz = p(keep[0])
    if zmask is not None:
        keep.append(dev(T64(zmask).float()))
        a.z = p(keep[-1])
    outs = []
    for s, (y, mean, invstd, gamma, beta) in enumerate(sets):
        ts = [dev(T64(t).float()) for t in (y, mean, invstd, gamma, beta)] + [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
        keep += ts
        for f, t in zip(("y", "mean", "invstd", "gamma", "beta", "dy", "dgamma", "dbeta"), ts):
            getattr(a, f)[s] = t.data_ptr()
        outs.append(ts[5:])
    path = lib.ocl_test_bn_bwd(C.byref(a), None)
    assert path >= 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    for o in outs:
        TL.assert_slack_untouched(o[0], "bn_bwd dy")
    return path, [[host(t) for t in o] for o in outs]


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups", BC.LADDERS)
@with_mode
def test_six_places_take_one_relu_decision(lib, det, n, hw, c, groups):
    from ocl_amd import ffi
    L = make_ladder(lib, det, n, hw, c, groups, 100 + c + groups)
    y, gamma, beta, act, dec, pix = L["y"], L["gamma"], L["beta"], L["act"], L["dec"], L["pix"]
    case = "ladder/n%d_hw%d_c%d_g%d/det%d" % (n, hw, c, groups, det)
    per = n // groups
    # 1. bn_fwd: derives the statistics itself from the cells
    out = bn_fwd(lib, y, groups, gamma, beta, L["st"], relu=1)
    same_bits(out["save_mean"], L["sm"], case + " save_mean")
    same_bits(out["save_invstd"], L["si"], case + " save_invstd")
    same_bits(out["z"], act, case + " bn_fwd")
    # 2. bn_apply_saved: from the saved statistics
    z = dev(torch.full(y.shape, float("nan")))
    ts = [dev(T64(t).float()) for t in (y, L["sm"], L["si"], gamma, beta)]
    a = ffi.TestAuxArgs()
    for k, t in enumerate(ts + [z]):
        a.p[k] = t.data_ptr()
    a.i[0], a.i[1], a.i[2] = per * hw * hw, groups, c
    assert lib.ocl_test_aux(9, C.byref(a), None) == 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    same_bits(host(z), act, case + " bn_apply_saved")
    # 3. a convolution's input-transform staging: identity on the centre tap, the output is the staged activation (zero padding adds zeros)
    d = TL._desc(c, c, 3, 1, hw, n, groups, 0, xf=1)
    w = torch.zeros((c, c, 3, 3), dtype=torch.float64)
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    sm, si = dev(torch.zeros(groups, c)), dev(torch.zeros(groups, c))
    got, forms, _ = run_conv(lib, d, T64(y), w, 0, xf=1, xf_stats=L["st"], xf_gamma=T64(gamma), xf_beta=T64(beta), xf_save_mean=sm, xf_save_invstd=si)
    assert [LF.FAMILIES[f.family] for f in forms] == ["t"], [LF.conv_key(f, "stats_xf") for f in forms]   # (the site the case claims: conv_t_kernel)
    same_bits(host(sm), L["sm"], case + " xf save_mean")
    same_bits(host(si), L["si"], case + " xf save_invstd")
    same_bits(got.numpy(), act, case + " conv xf staging")
    # 4. the weight gradient's staging: dy one-hot, output channel co probes pixel P[co]: grad[co, ci, centre] = a[P[co], ci]
    wd = ffi.TestWgradDesc(cin=c, cout=c, k=3, stride=1, hin=hw, win=hw, n=n, xf_groups=groups)
    xf_ops = [dict(xf_mean=T64(L["sm"]), xf_invstd=T64(L["si"]), xf_gamma=T64(gamma), xf_beta=T64(beta))]
    rng = np.random.default_rng(7)
    extra = np.stack([rng.integers(0, n, c), rng.integers(0, hw, c), rng.integers(0, hw, c)], axis=1)    # ordinary pixels too
    probes = np.concatenate(pix + [extra])
    for b in range(0, len(probes), c):
        P = probes[b: b + c]
        dy = torch.zeros((n, hw, hw, c), dtype=torch.float64)
        dy[P[:, 0], P[:, 1], P[:, 2], torch.arange(len(P))] = 1.0
        grad, _ = run_wgrad(lib, [wd], [T64(y)], [dy], xf_ops=xf_ops)
        same_bits(grad[0][: len(P), :, 1, 1].numpy(), act[P[:, 0], P[:, 1], P[:, 2], :], case + " wgrad xf staging (probes %d..)" % b)
    # 5. EPI_BNB without a stored z: strictly positive integer gradient and weights, so the zero pattern of the output is the mask
    db = TL._desc(c, c, 3, 1, hw, n, groups, 1, bnb=1)
    g = torch.Generator().manual_seed(5)
    dy2, wb = TL.ints((n, hw, hw, c), g, 1, 2), TL.ints((c, c, 3, 3), g, 1, 2)
    gd, forms, _ = run_conv(lib, db, dy2, wb, EPI_BNB, bnb_y=T64(y), bnb_mean=T64(L["sm"]), bnb_invstd=T64(L["si"]), bnb_gamma=T64(gamma), bnb_beta=T64(beta))
    print(case, "EPI_BNB ran", [LF.conv_key(f, "bnb") for f in forms])
    dx = TL.ref_dgrad(dy2, wb, db).numpy()
    assert (dx > 0).all()
    TL.assert_exact(gd, T64(dx * dec), case + " EPI_BNB mask")
    # 6. the BatchNorm backward kernels, mask_from_y, frozen: dy = gamma * invstd * dpre, its zero pattern is the mask (gamma != 0)
    dz = np.ones_like(y)
    path, outs = bn_bwd(lib, L, dz, one_pass=0, frozen=1)
    assert path == 3001, path
    assert ((outs[0][0] != 0) == dec).all(), case + " bn_bwd frozen mask"
    same_bits(outs[0][2], dec.sum(axis=(0, 1, 2)), case + " bn_bwd frozen dbeta (reduce kernel's mask)")
    NOTES.append("ladder %s: %d elements, %d in ladders, all six places agree with the exact decision" % (case, dec.size, groups * (c - 1) * (2 * HALF + 1)))


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups,one_pass,want", BC.MASK_PATHS)
@with_mode
def test_mask_from_y_of_every_backward_path_is_the_exact_decision(lib, det, n, hw, c, groups, one_pass, want):
    """The non-frozen backward paths show their recomputed mask through dbeta = sum(mask * dz): dz puts distinct powers of two on 12 pixels of
    each group (group 0: 2^0 .. 2^11, group 1: 2^12 .. 2^23; every partial sum is an integer below 2^24, exact in fp32), so dbeta's bits are the
    decisions at those pixels -- ladder rungs, twelve per group and launch."""
    L = make_ladder(lib, det, n, hw, c, groups, 200 + want)
    y, dec, pix = L["y"], L["dec"], L["pix"]
    case = "mask_from_y/%d/det%d" % (want, det)
    rungs = 2 * HALF + 1
    for b in range(0, rungs, 12):
        dz = np.zeros_like(y)
        expect = np.zeros(c)
        for g in range(groups):
            P = pix[g][b: b + 12]
            wgt = 2.0 ** (np.arange(len(P)) + 12 * g)
            dz[P[:, 0], P[:, 1], P[:, 2], :] = wgt[:, None]
            expect += (dec[P[:, 0], P[:, 1], P[:, 2], :] * wgt[:, None]).sum(axis=0)
        path, outs = bn_bwd(lib, L, dz, one_pass=one_pass, frozen=0)
        assert path == want, (path, want)
        same_bits(outs[0][2], expect, case + " dbeta bits (rungs %d..)" % b)
    # every element at once: dz = 1, dbeta = the number of positive decisions per channel (< 2^24)
    path, outs = bn_bwd(lib, L, np.ones_like(y), one_pass=one_pass, frozen=0)
    assert path == want
    same_bits(outs[0][2], dec.sum(axis=(0, 1, 2)), case + " dbeta count")


# =====================================================================================================================================
# (d) backward paths on heterogeneous channels
# =====================================================================================================================================
def _dz(rng, shape):
    dz = np.empty(shape, np.float32)
    for ch in range(shape[-1]):
        s = BC.DZ_SCALES[ch % len(BC.DZ_SCALES)]
        r = rng.standard_normal(shape[:-1])
        dz[..., ch] = 5 + 0.01 * r if s == "cancel" else s * r
    return dz.astype(np.float64)


def _check_bwd(case, got, d, y, groups, gamma, mean, invstd):
    dy, dgm, dbt = R.bn_backward64(d, y, groups, gamma, mean, invstd)
    b_dy, b_dg, b_db = R.bwd_bounds(d, y, groups, gamma, mean, invstd)
    per = y.shape[0] // groups
    PB.check_derived(REPORT, case, "dy", got[0], dy, np.repeat(b_dy, per, axis=0)[:, None, None, :])
    PB.check_derived(REPORT, case, "dgamma", got[1], dgm, b_dg)
    PB.check_derived(REPORT, case, "dbeta", got[2], dbt, b_db)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("n,hw,c,groups,nsets,one_pass,want", BC.BWD_PATHS)
@with_mode
def test_bn_backward_paths_on_heterogeneous_channels(lib, det, n, hw, c, groups, nsets, one_pass, want):
    rng = np.random.default_rng(n * 7 + c + nsets)
    dz = _dz(rng, (n, hw, hw, c))
    zm = rng.standard_normal((n, hw, hw, c)).astype(np.float32).astype(np.float64)
    zm[..., 3::4] = 1.0     # (the "cancel" channels pass the mask whole: d - k1 cancels to 0.01 of d)
    sets = []
    for s in range(nsets):
        y = BC.regime_tensor(rng, n, hw, c)
        gamma, beta = BC.affine(rng, c)
        mean, var = R.two_pass_moments(y, groups)
        invstd = R.invstd_of(var)
        sets.append((y, mean, invstd, gamma, beta))
    L = dict(n=n, hw=hw, c=c, groups=groups)
    path, outs = bn_bwd(lib, L, dz, one_pass=one_pass, frozen=0, mask_from_y=0, zmask=zm, sets=sets)
    assert path == want, (path, want)
    d = dz * (zm > 0)
    for s in range(nsets):
        y, mean, invstd, gamma, _ = sets[s]
        _check_bwd("bn_bwd/%d/set%d/det%d" % (want, s, det), outs[s], d, y, groups, gamma, mean, invstd)


@pytest.mark.parametrize("det", [0, 1])
@with_mode
def test_bnb_epilogue_then_apply_e_on_heterogeneous_channels(lib, det):
    """EPI_BNB (the masked gradient and its two batch sums in the data gradient's epilogue) then bn_bwd_apply_e: the masked gradient against the
    float64 data gradient, the BatchNorm backward stage against float64 from the kernel's own fp32 masked gradient."""
    n, groups, hw, c = 10, 2, 16, 40
    rng = np.random.default_rng(17)
    d = TL._desc(c, c, 3, 1, hw, n, groups, 1, bnb=1)
    dy2 = T64(rng.standard_normal((n, hw, hw, c)).astype(np.float32))
    w = (0.1 * rng.standard_normal((c, c, 3, 3)))
    for ci in range(c):   # the gradient's scale per BatchNorm channel (the data gradient's output channel = the weights' input channel)
        s = BC.DZ_SCALES[ci % 4]
        w[:, ci] *= 1.0 if s == "cancel" else s
    w = T64(w.astype(np.float32))
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    z64, mean, var, invstd = R.bn_forward64(y, groups, gamma, beta)
    z = np.maximum(z64, 0).astype(np.float32).astype(np.float64)
    m32, i32 = mean.astype(np.float32), invstd.astype(np.float32)
    got_d, forms, stats = run_conv(lib, d, dy2, w, EPI_BNB, bnb_y=T64(y), bnb_z=T64(z), bnb_mean=T64(m32), bnb_invstd=T64(i32), bnb_gamma=T64(gamma),
                                   bnb_beta=T64(beta))
    case = "bnb_apply_e/det%d" % det
    dx = TL.ref_dgrad(dy2, w, d).numpy()
    mag = TL.ref_dgrad(dy2.abs(), w.abs(), d).numpy()
    PB.check_derived(REPORT, case, "d", got_d.numpy(), dx * (z > 0), 1.01 * 9 * c * U * mag)
    outs = [dev(torch.full(y.shape, float("nan"))), dev(torch.zeros(c)), dev(torch.zeros(c))]
    ins = [dev(T64(t).float()) for t in (got_d.numpy(), y, m32, i32, gamma)]
    rc = lib.ocl_test_bn_apply_e(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), p(stats), n // groups * hw * hw, groups, c,
                                 p(outs[0]), p(outs[1]), p(outs[2]), 0, None)
    assert rc == 0, lib.ocl_last_error()
    torch.cuda.synchronize()
    _check_bwd(case, [host(t) for t in outs], got_d.numpy(), y, groups, gamma, mean, invstd)


# =====================================================================================================================================
# (e) one whole pass
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["bright_low_contrast", "near_flat"])
def test_whole_pass_on_ill_conditioned_images(cuda, kind):
    """The ER cifar100 pass of test_train_forward_backward_vs_oracle (n = 10) on x = 0.9 + 0.1 rand (|mean| / std = 7 at the stem) and on
    near-flat images, with that test's assertions and tolerances."""
    import test_gpu_net as TN
    rng = np.random.default_rng(10)
    if kind == "bright_low_contrast":
        x = 0.9 + 0.1 * rng.random((10, 3, 32, 32))
    else:
        x = 0.5 + 0.02 * rng.random((10, 3, 32, 32))
    TN.train_forward_backward_vs_oracle(cuda, "ER", "cifar100", None, 10, 1, images=x.astype(np.float32))
