"""CPU: the BatchNorm conditioning suite (tests/test_gpu_bn_cond.py) tests what it says it tests, and its bounds can be met.

* the producer cases realise their regimes: the float64 moments of the float64 convolution of a case's fp32 inputs are the nominal mu and sigma
  within 1 %, dead and constant rows exactly constant, borders included;
* every call site of fx_add / fx_fetch_add (outside conv_stats_dev.h) and of bn_scale_shift, parsed from csrc/*.hip and *.h, is a required
  site, and every required site is claimed by a case or listed as unreachable with its reason: a new call site without a case fails here;
* two models stay inside every bound of tests/bn_cond_ref.py on the cases' data: a numpy model of the design (fp32 partial sums of 16, 64 and
  256 values, double cells, the 2^-40 truncation) and torch-CPU fp32 F.batch_norm with its autograd;
* the ladders are not vacuous: the exact decision changes inside each, at least 8 rungs from either end;
* the Fraction -> fp32 rounding and the vectorised exact fma agree with numpy / with each other."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cond_cases as BC
import bn_cond_ref as R
import layer_forms as LF
import parity_bounds as PB
from conftest import ROOT
import ocl_amd  # noqa: F401
from ocl_amd import ffi

CSRC = os.path.join(ROOT, "online-continual-learning_amd", "csrc")
REPORT = []


# ---- the rounding helpers --------------------------------------------------------------------------------------------------------------
def test_round_f32_agrees_with_numpy_on_exact_products():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(10000) * 10.0 ** rng.integers(-20, 20, 10000)).astype(np.float32)
    b = (rng.standard_normal(10000) * 10.0 ** rng.integers(-15, 15, 10000)).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)        # exact in float64: one rounding to fp32 is the correct rounding
    want = prod.astype(np.float32)
    ok = np.isfinite(want) & (np.abs(prod) > 1e-300)
    assert ok.sum() > 9000
    for i in np.flatnonzero(ok):
        got = R.round_f32(Fraction(float(a[i])) * Fraction(float(b[i])))
        assert np.float32(got) == want[i] and float(np.float32(got)) == got, (a[i], b[i], got, want[i])
    # ties to even, and the subnormal range
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert R.round_f32(one + ulp / 2) == 1.0 and R.round_f32(one + 3 * ulp / 2) == float(one + 2 * ulp)
    assert R.round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == float(one + ulp)
    assert R.round_f32(Fraction(1, 2 ** 150)) == 0.0 and R.round_f32(Fraction(3, 2 ** 150)) == 2.0 ** -148
    assert R.round_f32(-Fraction(5, 3)) == float(np.float32(-5.0 / 3.0))


def test_vectorised_fma_and_decision_agree_with_the_rational_ones():
    rng = np.random.default_rng(2)
    n = 3000
    y = (1000 + rng.standard_normal(n)).astype(np.float32)
    sc = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    sh = (-(y.astype(np.float64) * sc.astype(np.float64)) * (1 + rng.integers(-3, 4, n) * 2.0 ** -24)).astype(np.float32)   # near cancellation
    # exact ties of the float64 sum: y * sc + sh = 1 + 2^-24 (+- a residual below float64's reach)
    y[:200], sc[:200] = 1.0, 1.0
    sh[:200] = np.float32(2.0 ** -24)
    y[100:200] = np.float32(1 + 2.0 ** -23)
    got = R.fma32(y, sc, sh)
    dec = R.decide64(y, sc, sh)
    for i in range(n):
        assert float(got[i]) == R.fma_f32(y[i], sc[i], sh[i]), i
        assert bool(dec[i]) == R.decide_exact(y[i], sc[i], sh[i]) == (float(got[i]) > 0), i
    # a tie of the float64 sum whose residual decides: 2^30 + 2^6 (a tie of fp32 at 2^30: spacing 2^7) + 2^-30
    a, b, c = np.float32(2.0 ** 30 + 2.0 ** 7), np.float32(1.0), np.float32(-2.0 ** 6)
    assert float(R.fma32(a, b, c)) == R.fma_f32(a, b, c)
    a, b, c = np.float32(2.0 ** 15 + 2.0 ** -8), np.float32(2.0 ** 15 + 2.0 ** -8), np.float32(2.0 ** 6)
    assert float(R.fma32(a, b, c)) == R.fma_f32(a, b, c)


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
def enclosing_function(lines, i):
    """The name of the function whose definition (a line starting in column 0 with __global__ / __device__ / static / int / void) precedes line i."""
    for j in range(i, -1, -1):
        ln = lines[j]
        if ln[:1] in " \t#/}" or not re.match(r"(?:__global__|__device__|static|int|void)\b", ln):
            continue
        ln = re.sub(r"__launch_bounds__\([^)]*\)|__attribute__\(\([^)]*\)\)", "", ln)
        m = re.search(r"(\w+)\s*\(", ln)
        if m:
            return m.group(1)
    raise AssertionError("no enclosing function above line %d" % (i + 1))


def parsed_sites():
    sites = set()
    for name in sorted(os.listdir(CSRC)):
        if not (name.endswith(".hip") or name.endswith(".h")):
            continue
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        for i, ln in enumerate(lines):
            code = ln.split("//")[0]
            if re.match(r"(?:template|__device__|__global__)", ln) and re.search(r"\b(?:fx_add|fx_fetch_add|bn_scale_shift)\s*\(", ln.split("{")[0]):
                continue   # the helper's own definition
            if name != "conv_stats_dev.h" and re.search(r"\bfx_(?:add|fetch_add)\s*(?:<[^>]*>)?\s*\(", code):
                sites.add((name, enclosing_function(lines, i), "fx"))
            if re.search(r"\bbn_scale_shift\s*\(", code):
                sites.add((name, enclosing_function(lines, i), "ss"))
    return sites


def test_every_call_site_is_required_and_every_required_site_is_claimed():
    sites = parsed_sites()
    required = set(BC.REQUIRED_SITES)
    assert len(required) == len(BC.REQUIRED_SITES)
    assert sites == required, "call sites without a case: %s; required sites that no longer exist: %s" % (sorted(sites - required), sorted(required - sites))
    claimed = {s for c in BC.PRODUCERS + BC.CONSUMERS + [BC.SWITCH_PRODUCER] for s in c["sites"]}
    assert claimed <= required, sorted(claimed - required)
    assert required - claimed == set(BC.EXEMPT_SITES), (sorted(required - claimed), sorted(BC.EXEMPT_SITES))
    assert all(BC.EXEMPT_SITES.values())
    # the GPU file runs every producer and every consumer the table names
    txt = open(os.path.join(ROOT, "tests", "test_gpu_bn_cond.py")).read()
    assert '[c["key"] for c in BC.PRODUCERS]' in txt
    for c in BC.CONSUMERS + [BC.SWITCH_PRODUCER]:
        assert ("\ndef %s(" % c["test"]) in txt, c["test"]
    for key in (c["key"] for c in BC.PRODUCERS):
        assert key in LF.COVERED, key
    assert len(BC.REGIMES) == 10 and BC.NAMES == ["r0", "r1", "r10", "r100", "r1000", "rneg100", "dead", "const", "tiny", "big"]


# ---- the producer cases realise their regimes -------------------------------------------------------------------------------------------
def _entry(lib, key):
    hw, n, g, layer, dr = LF.COVERED[key]
    for k, e in LF.net_forms(lib, hw, n, g, 1):
        if k == key and e.layer == layer and e.dir == dr:
            return e
    raise AssertionError(key)


@pytest.mark.parametrize("key", [c["key"] for c in BC.PRODUCERS])
def test_producer_cases_realise_their_regimes(key):
    torch.set_num_threads(8)
    lib = ffi.lib()
    d = _entry(lib, key).desc
    dims = (d.n, d.hin, d.win, d.cin, d.cout, d.k, d.stride)
    xf = key.endswith("_xf")
    for groups in (1, 2):
        if groups == 2 and d.n % 2:
            continue
        d2 = type(d).from_buffer_copy(d)
        d2.groups = groups
        forms = (ffi.TestConvForm * 4)()
        cnt = lib.ocl_test_conv_plan(C.byref(d2), forms, 4)
        assert key in [LF.conv_key(forms[i], key.split("/")[1]) for i in range(cnt)], "the planner gives %s another form with %d groups" % (key, groups)
        seed = sum(map(ord, key)) + groups
        if xf:
            rng = np.random.default_rng(seed)
            cin_t = 4 if d.cin == 3 else d.cin
            yin = (rng.standard_normal((d.n, d.hin, d.win, cin_t)) * 2 + 0.3).astype(np.float32).astype(np.float64)
            gamma, beta = BC.affine(rng, cin_t)
            cc = BC.const_channel(d.cin)
            gamma[cc], beta[cc] = 0.0, 1.0
            z32, _, _, _ = R.model_forward(yin, groups, gamma, beta, R.exact_totals(yin, groups))
            x = torch.from_numpy(np.maximum(z32, 0).astype(np.float64))
            assert bool((x[..., cc] == 1.0).all())
            _, w = BC.producer_inputs(dims, groups, seed, act=x.numpy())
        else:
            x, w = BC.producer_inputs(dims, groups, seed)
        y = BC.conv64(x, w, d.stride).numpy()
        mean, var = R.two_pass_moments(y, groups)
        for c in range(d.cout):
            name, mu, sigma, kind = BC.regime_of(c)
            for g in range(groups):
                sign = 1.0 if (g == 0 or xf) else -1.0     # (ReLU'd activations are not mirrored)
                if kind == "const":
                    per = d.n // groups
                    assert (y[g * per:(g + 1) * per, ..., c] == sign * mu).all(), (key, name)
                    continue
                assert abs(mean[g, c] - sign * mu) <= 0.01 * max(abs(mu), sigma), (key, name, mean[g, c])
                assert abs(np.sqrt(var[g, c]) - sigma) <= 0.01 * sigma, (key, name, np.sqrt(var[g, c]))


# ---- the bounds can be met -------------------------------------------------------------------------------------------------------------
SHAPES = [(10, 32, 20, 2), (6, 16, 40, 1), (12, 8, 160, 2), (5, 4, 80, 1)]     # the consumer cases of the GPU file


@pytest.mark.parametrize("n,hw,c,groups", SHAPES)
def test_design_model_and_torch_fp32_stay_inside_the_forward_bounds(n, hw, c, groups):
    rng = np.random.default_rng(n * 100 + c)
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    M = n // groups * hw * hw
    yg = R.group_view(y, groups)
    s1, s2, a1 = yg.sum(axis=1), (yg * yg).sum(axis=1), np.abs(yg).sum(axis=1)
    m2, v2 = R.two_pass_moments(y, groups)
    case = "n%d_hw%d_c%d_g%d" % (n, hw, c, groups)
    for det in (0, 1):
        for L in (16, 64, 256):
            tot, nparts = R.model_totals(y, groups, L, det)
            assert nparts == -(-M // L)
            what = "%s/L%d/det%d" % (case, L, det)
            PB.check_derived(REPORT, what, "sum", tot[:, 0], s1, R.sums_bound(a1, nparts, det))
            PB.check_derived(REPORT, what, "sumsq", tot[:, 1], s2, R.sums_bound(s2, nparts, det))
            if not det:
                with np.errstate(divide="ignore", invalid="ignore"):
                    print("model K %s %.3f" % (what, np.nanmax(np.concatenate([np.abs(tot[:, 0] - s1) / (R.U * a1), np.abs(tot[:, 1] - s2) / (R.U * s2)]))))
            mean, var, _ = R.moments_from_totals(tot[:, 0], tot[:, 1], M)
            bm, bv = R.moments_bound(y, groups, nparts, det)
            PB.check_derived(REPORT, what, "mean", mean, m2, bm)
            PB.check_derived(REPORT, what, "var", var, v2, bv)
        # consumers of exact cells: the model's saved statistics and z
        tk = R.as_cells_hold(R.exact_totals(y, groups), det)
        mk, vk, _ = R.moments_from_totals(tk[:, 0], tk[:, 1], M)
        bm, bv = R.exact_moments_bound(y, groups, det)
        PB.check_derived(REPORT, case, "mean(exact)", mk, m2, bm)
        PB.check_derived(REPORT, case, "var(exact)", vk, v2, bv)
        z32, sm, si, _ = R.model_forward(y, groups, gamma, beta, tk)
        z64, mean, var, invstd = R.bn_forward64(y, groups, gamma, beta)
        PB.check_derived(REPORT, case + "/model/det%d" % det, "z", z32, z64, R.z_bound(y, groups, gamma, beta, mean, invstd))
    # torch fp32 on the same data, group by group
    per = n // groups
    z32 = np.concatenate([F.batch_norm(torch.from_numpy(y[g * per:(g + 1) * per]).float().permute(0, 3, 1, 2), None, None,
                                       torch.from_numpy(gamma).float(), torch.from_numpy(beta).float(), True, 0.1, R.EPS).permute(0, 2, 3, 1).numpy()
                          for g in range(groups)])
    PB.check_derived(REPORT, case + "/torch32", "z", z32, z64, R.z_bound(y, groups, gamma, beta, mean, invstd))


def _dz(rng, shape):
    dz = np.empty(shape, np.float32)
    for ch in range(shape[-1]):
        s = BC.DZ_SCALES[ch % len(BC.DZ_SCALES)]
        r = rng.standard_normal(shape[:-1])
        dz[..., ch] = 5 + 0.01 * r if s == "cancel" else s * r
    return dz.astype(np.float64)


def model_backward(d, y, groups, gamma, mean, invstd, L):
    """The design's backward in numpy fp32: saved statistics rounded to fp32, xhat = (y - mean) * invstd, fp32 partial sums of L values of d and of
    fma(d, xhat, .), double totals, k1 / k2 rounded to fp32, dy = scale * (d - k1 - xhat * k2) one fp32 operation at a time."""
    f = np.float32
    dg, yg = R.group_view(d, groups).astype(f), R.group_view(y, groups).astype(f)
    m32, i32, g32 = mean.astype(f)[:, None, :], invstd.astype(f)[:, None, :], np.asarray(gamma, f)
    xhat = (yg - m32) * i32
    G, M, Cc = dg.shape
    nparts = (M + L - 1) // L
    pad = nparts * L - M
    dp = np.concatenate([dg, np.zeros((G, pad, Cc), f)], axis=1).reshape(G, nparts, L, Cc)
    xp = np.concatenate([xhat, np.zeros((G, pad, Cc), f)], axis=1).reshape(G, nparts, L, Cc)
    sd, sx = np.zeros((G, nparts, Cc), f), np.zeros((G, nparts, Cc), f)
    for i in range(L):
        sd = sd + dp[:, :, i]
        sx = R.fma32(dp[:, :, i], xp[:, :, i], sx)
    td, tx = sd.astype(np.float64).sum(axis=1), sx.astype(np.float64).sum(axis=1)
    k1, k2 = (td / M).astype(f)[:, None, :], (tx / M).astype(f)[:, None, :]
    dy = (g32 * i32) * ((dg - k1) - xhat * k2)
    return dy.astype(np.float64).reshape(d.shape), tx.sum(axis=0).astype(f).astype(np.float64), td.sum(axis=0).astype(f).astype(np.float64)


@pytest.mark.parametrize("n,hw,c,groups", [(4, 4, 160, 2), (4, 16, 40, 1), (10, 32, 20, 2), (12, 16, 80, 1)])
def test_design_model_and_torch_fp32_stay_inside_the_backward_bounds(n, hw, c, groups):
    rng = np.random.default_rng(n * 7 + c)
    dz = _dz(rng, (n, hw, hw, c))
    zm = rng.standard_normal((n, hw, hw, c))
    zm[..., 3::4] = 1.0
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    mean, var = R.two_pass_moments(y, groups)
    invstd = R.invstd_of(var)
    d = dz * (zm > 0)
    dy, dgm, dbt = R.bn_backward64(d, y, groups, gamma, mean, invstd)
    b_dy, b_dg, b_db = R.bwd_bounds(d, y, groups, gamma, mean, invstd)
    per = n // groups
    b_el = np.repeat(b_dy, per, axis=0)[:, None, None, :]
    case = "bwd/n%d_hw%d_c%d_g%d" % (n, hw, c, groups)
    for L in (16, 64, 256):
        got = model_backward(d, y, groups, gamma, mean, invstd, L)
        PB.check_derived(REPORT, case + "/model/L%d" % L, "dy", got[0], dy, b_el)
        PB.check_derived(REPORT, case + "/model/L%d" % L, "dgamma", got[1], dgm, b_dg)
        PB.check_derived(REPORT, case + "/model/L%d" % L, "dbeta", got[2], dbt, b_db)
    # torch fp32 BatchNorm backward, group by group, from the same saved statistics the kernels are given (fl32 of the float64 ones) and the
    # masked gradient as the incoming one
    outs, gg, gb = [], torch.zeros(c), torch.zeros(c)
    for g in range(groups):
        yt = torch.from_numpy(y[g * per:(g + 1) * per]).float().permute(0, 3, 1, 2).contiguous()
        dt = torch.from_numpy(d[g * per:(g + 1) * per]).float().permute(0, 3, 1, 2).contiguous()
        gi, gw, gbias = torch.ops.aten.native_batch_norm_backward(dt, yt, torch.from_numpy(gamma).float(), None, None, torch.from_numpy(mean[g]).float(),
                                                                 torch.from_numpy(invstd[g]).float(), True, R.EPS, [True, True, True])
        outs.append(gi.permute(0, 2, 3, 1).numpy())
        gg, gb = gg + gw, gb + gbias
    PB.check_derived(REPORT, case + "/torch32", "dy", np.concatenate(outs), dy, b_el)
    PB.check_derived(REPORT, case + "/torch32", "dgamma", gg.numpy(), dgm, b_dg)
    PB.check_derived(REPORT, case + "/torch32", "dbeta", gb.numpy(), dbt, b_db)


# ---- the ladders are not vacuous -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c,groups", BC.LADDERS + [m[:4] for m in BC.MASK_PATHS[:1]])
def test_the_exact_decision_changes_inside_every_ladder(n, hw, c, groups):
    rng = np.random.default_rng(100 + c + groups)
    y = BC.regime_tensor(rng, n, hw, c)
    gamma, beta = BC.affine(rng, c)
    beta[beta == 0] = 0.25
    beta[6] = 0.0        # the GPU file's on-boundary channel: dead, beta = 0, no ladder (every element is exactly on the boundary)
    _, sm, si, _ = R.model_forward(y, groups, gamma, beta, R.exact_totals(y, groups))
    sc, sh = R.scale_shift_exact(gamma[None, :], beta[None, :], sm, si)
    for g in range(groups):
        for ch in range(c):
            if ch == 6:
                assert BC.regime_of(ch)[0] == "dead" and sh[g, ch] == 0 and not R.decide64(y[..., ch], sc[g, ch], sh[g, ch]).any()
                continue
            assert sc[g, ch] != 0
            lad = R.ladder(R.root_f32(sc[g, ch], sh[g, ch]), 64)
            assert len(lad) == 129 and (np.diff(lad.astype(np.float64)) > 0).all()
            dec = [R.decide_exact(v, sc[g, ch], sh[g, ch]) for v in lad]
            flips = [j for j in range(128) if dec[j] != dec[j + 1]]
            assert len(flips) == 1 and 8 <= flips[0] <= 119, (g, ch, BC.regime_of(ch)[0], flips)
            assert (R.decide64(lad, sc[g, ch], sh[g, ch]) == np.array(dec)).all()


# ---- the tile restatement of conv_s separates one more fp32 rounding ---------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
def test_one_more_fp32_add_of_two_partial_sums_matches_neither_legal_evaluation(groups):
    """The GPU file holds conv_s_kernel's sums of squares to one of the two legal evaluations of row16_sum(z * z), within the float64 additions'
    round-off.  On the s2/stats case's own data (the float64 convolution rounded to fp32 stands in for the kernel's output) the arithmetic of the
    mutation -- the two waves' fp32 partial sums of squares added in fp32 before the conversion to double -- is outside that tolerance of
    BOTH evaluations in most cells of the channels that are not constant (one cell suffices to fail the GPU assertion), in both batch-sum
    modes; the two legal evaluations themselves differ as well."""
    lib = ffi.lib()
    d = _entry(lib, "s2/stats").desc
    x, w = BC.producer_inputs((d.n, d.hin, d.win, d.cin, d.cout, d.k, d.stride), groups, sum(map(ord, "s2/stats")) + groups)
    y = BC.conv64(x, w, d.stride).numpy().astype(np.float32).astype(np.float64)
    yg = R.group_view(y, groups)
    s2 = (yg * yg).sum(axis=1)
    live = np.array([BC.regime_of(c)[3] != "const" for c in range(d.cout)])
    for det in (0, 1):
        legal = [R.conv_s_tile_totals(y, groups, det, c)[0][:, 1] for c in (False, True)]
        mut = [R.conv_s_tile_totals(y, groups, det, c, pair_squares=True)[0][:, 1] for c in (False, True)]
        ntile = yg.shape[1] // 16
        lim = ntile * 2.0 ** -52 * s2 + (R.FX if det else 0.0)
        for m in mut:
            for l in legal:
                out = np.abs(m - l)[:, live] > lim[:, live]     # (the GPU assertion needs EVERY cell inside: one cell outside fails it)
                assert out.mean() > 0.5, (det, out.mean())
        assert (np.abs(legal[0] - legal[1])[:, live] > lim[:, live]).mean() > 0.5
        # on the dead and constant channels every partial sum is a power-of-two multiple of one fp32 value: exact under any regrouping
        assert (mut[1][:, ~live] == legal[1][:, ~live]).all()
