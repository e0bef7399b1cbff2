"""GPU: every kernel of the small-op files of csrc/ (small_op_cases.SOURCES), the two augmentation kernels included, path by path (tests/small_op_cases.py), against float64 references
written here (the augmentation's: tests/augment_ref.py) from the formulas include/ocl_hip.h cites -- independent of oracle/ (fp32) and of the library.

Tier 1 (bit-equal, data chosen so that fp32 is exact): gather / scatter / pair / u8 (any data), the small GEMM and the column reductions on small
integers, SGD with power-of-two hyper-parameters, argsort order, kNN order and Shapley values on integer-valued features (with NaN and +inf
planted among them: include/ocl_hip.h K10's total order), NCM ties and NaN distances, labels outside the row in ce / ce_seg / mir (K6, K12).
Tier 2 (random fp32, per-element error against float64):
  * sums of products: |got - ref| <= 1.01 * K * 2^-24 * sum|terms|, K the number of fp32-accumulated terms (derived, no measured number);
  * the kNN order on real-valued features: an adjacent pair that float64 orders the other way is within 1.01 * K * 2^-24 * (d_a + d_b), K the
    roundings of the case's distance path (tests/knn_ref.py); the Shapley values are bit-equal to the oracle's for the kernel's order;
  * transcendental kernels (ce, ce_seg, kd, mir, supcon): the same formula evaluated by plain torch-CPU fp32 on the same inputs has error e_ref
    against float64 (max over the tensor); the kernel's must be <= max(4 * e_ref, 4 ulp of the largest |reference| element).  4: the kernel and
    torch differ in summation order and in expf / logf (each ~2 ulp per term), nothing else; a wrong factor, a dropped term or a wrong max is orders
    of magnitude.  On the shapes the golden tests bound by 1e-5 the bound is capped at 1e-5.
Every tensor handed to the library sits between sentinel regions (guarded.Guarded); after each call the regions are intact and inputs unchanged.
Each case asserts that the entry point takes the path the table names (ocl_test_small_op_path on the real pointers).  Refusals are only tested
where the plan says the entry point returns before launching.  With OCL_PARITY_REPORT=<file> the tier-2 figures are written there, and the
augmentation's (per case: E, the tolerance, the device error) to augment_parity.txt next to it (profiles/augment_parity.txt)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as AR
import knn_ref as KR
import parity_bounds as PB
import small_op_cases as SC
from guarded import Guarded

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PFX = "OCL" + "_PATH_"
REPORT = []
AUG_REPORT = []


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    yield L
    path = os.environ.get("OCL_PARITY_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("# tier-2 parity of the small kernels against float64 (tests/test_gpu_small_ops.py): kernel error, the error of plain torch-CPU\n"
                    "# fp32 on the same inputs (e_ref; '-' where the bound is derived), the bound, and error / bound (must be <= 1)\n")
            f.write("%-44s %-8s %12s %12s %12s %8s\n" % ("case", "tensor", "kernel_err", "e_ref", "bound", "ratio"))
            for row in REPORT:
                f.write("%-44s %-8s %12.4g %12s %12.4g %8.3f\n" % row)
            worst = max(REPORT, key=lambda r: r[5])
            f.write("# closest to its bound: %s %s (ratio %.3f)\n" % (worst[0], worst[1], worst[5]))
    if path and AUG_REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "augment_parity.txt"), "w") as f:
            f.write("# the SCR augmentation kernels against the float64 statement of their contract (tests/augment_ref.py, tests/test_gpu_small_ops.py)\n"
                    "# augment/*: E = max |float32 restatement - float64| on the case's inputs, tolerance = max(4 E, 8 * 2^-24), device error = max |kernel - float64|\n"
                    "# aug_params/*: E column = rows compared exactly (all rounding decisions > 2^-18 from a boundary), tolerance and error in float32 spacings\n"
                    "#               of the jitter factors; the integer parameters of those rows are equal\n")
            f.write("%-36s %-8s %5s %12s %12s %12s %8s\n" % ("case", "size", "n", "E", "tolerance", "device_err", "ratio"))
            for case, size, n, E, tol, err in AUG_REPORT:
                f.write("%-36s %-8s %5d %12.4g %12.4g %12.4g %8.3f\n" % (case, size, n, E, tol, err, err / tol))


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    from ocl_amd import ffi
    return ffi.stream()


def ok(lib, rc, what):
    assert rc == 0, "%s failed (%d): %s" % (what, rc, lib.ocl_last_error())


def header_paths():
    import re
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "ocl_hip.h")).read()
    return {name: int(v) for name, v in re.findall(PFX + r"([A-Z0-9_]+)\s*=\s*(\d+)", txt)}


def assert_path(lib, op, case, ptrs=None):
    """The entry point takes the path the case claims, with the tensors' real addresses."""
    from ocl_amd import ffi
    args = SC.plan_args(op, case, [t.data_ptr() if t is not None else 0 for t in ptrs] if ptrs else None)
    if op == "pair" and ptrs:
        args[1] = ptrs[1].data_ptr()
    if op == "sgd" and ptrs:
        args[1], args[2] = ptrs[1].data_ptr(), (ptrs[2].data_ptr() if ptrs[2] is not None else 0)
    plan = ffi.SmallOpPlan()
    code = lib.ocl_test_small_op_path(SC.OPS[op][0], (ffi.i64 * len(args))(*args), len(args), C.byref(plan))
    assert code == header_paths()[case["path"]], "%s/%s takes path %d, not %s" % (op, case["name"], code, case["path"])
    return plan


def case_of(op):
    return pytest.mark.parametrize("name", SC.ids(op))


def find(op, name):
    return [c for c in SC.CASES[op] if c["name"] == name][0]


def check_vs_torch32(case, tensor, got, ref64, ref32, cap=None):
    """Transcendental kernels: error <= max(4 * e_ref, 4 ulp of the largest |reference| element) (tests/parity_bounds.py)."""
    PB.check_vs_torch32(REPORT, case, tensor, got, ref64, ref32, cap)


def check_derived(case, tensor, got, ref64, bound):
    PB.check_derived(REPORT, case, tensor, got, ref64, bound)


# ==========================================================================================================================================
# float64 references
# ==========================================================================================================================================
def ref_ce(x, y):
    """Row losses lse(x) - x[y] and d(row loss)/dx = softmax(x) - onehot(y) (torch.nn.CrossEntropyLoss)."""
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    rows = (np.log(s) + m)[:, 0] - x[np.arange(len(y)), y]
    g = e / s
    g[np.arange(len(y)), y] -= 1.0
    return rows, g


def ref_ce_seg(x, y, seg):
    """Mean over rows of the cross-entropy of a softmax over the columns of the label's segment (agents/base.py:96-108); columns with
    seg == -1 take part in no row.  Returns (mean loss, d/dx)."""
    n = len(y)
    mask = seg[None, :] == seg[y][:, None]
    xm = np.where(mask, x, -np.inf)
    m = xm.max(1, keepdims=True)
    e = np.exp(xm - m)
    s = e.sum(1, keepdims=True)
    rows = (np.log(s) + m)[:, 0] - x[np.arange(n), y]
    g = e / s
    g[np.arange(n), y] -= 1.0
    return rows.mean(), g / n


def ref_kd(s, t, T):
    """utils/kd_manager.py:6-11: mean_r(-sum_j softmax(t/T) log_softmax(s/T)) T^2 and its gradient (softmax(s/T) - softmax(t/T)) T / n."""
    def logsm(z):
        z = z - z.max(1, keepdims=True)
        return z - np.log(np.exp(z).sum(1, keepdims=True))
    ls, lt = logsm(s / T), logsm(t / T)
    loss = (-np.exp(lt) * ls).sum(1).mean() * T * T
    return loss, (np.exp(ls) - np.exp(lt)) * T / s.shape[0]


def ref_supcon(f, y, bsz, n_views, T, block=512):
    """SupConLoss, contrast_mode 'all' (utils/loss.py:19-96) on view-major float64 features [A, dim], and d(loss)/d(features), `block`
    anchors at a time.  An anchor without a positive has loss 0/0 = NaN; autograd sends NaN to every logit of its row."""
    A, _ = f.shape
    lab = np.tile(np.asarray(y), n_views)
    df = np.zeros_like(f)
    total = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for b0 in range(0, A, block):
            I = np.arange(b0, min(A, b0 + block))
            L = f[I] @ f.T / T
            L = L - L.max(1, keepdims=True)
            notself = np.ones_like(L)
            notself[np.arange(len(I)), I] = 0.0
            ex = np.exp(L) * notself
            se = ex.sum(1, keepdims=True)
            logp = L - np.log(se)
            pos = (lab[I][:, None] == lab[None, :]) * notself
            npos = pos.sum(1, keepdims=True)
            total += float((-(pos * logp).sum(1) / npos[:, 0]).sum())
            G = (ex / se - pos / npos) / A            # d(mean loss) / d(logit_ij); row of NaN where npos == 0 (0 / 0 for every j)
            G[np.arange(len(I)), I] = np.where(npos[:, 0] == 0, np.nan, 0.0)
            df[I] += G @ f / T
            df += G.T @ f[I] / T
    return total / A, df


def ref_knn_order(ef, cf):
    """float64 squared distances [n_eval, n_cand] and their stable ascending order (ties: lower candidate index first)."""
    e, c = np.asarray(ef, dtype=np.float64), np.asarray(cf, dtype=np.float64)
    d = ((e[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    return d, np.argsort(d, axis=1, kind="stable")


def shapley_subsets(dist_row, match_row, k):
    """The Shapley value of every candidate for one evaluation point, from the definition over subsets (2^n utilities, n <= 12), float64:
    v(S) = (1/k) * number of label matches among the min(k, |S|) nearest members of S (aser_utils.py:7-27).  The permutation form of the same
    definition is oracle.knn_shapley_bruteforce (n! terms: usable to n = 8; tests/test_cpu_small_ops.py checks the two against each other).
    For k > n the reference's closed form (last factor 1 / N, aser_utils.py:46-49) is not this value (tests/test_cpu_oracle_golden.py): the
    kernel follows the reference there and is compared with the oracle only."""
    n = len(dist_row)
    rank = sorted(range(n), key=lambda j: (dist_row[j], j))
    util = np.zeros(1 << n)
    for mask in range(1, 1 << n):
        near = [j for j in rank if mask >> j & 1][:k]
        util[mask] = sum(bool(match_row[j]) for j in near) / float(k)
    w = [math.factorial(s) * math.factorial(n - s - 1) / math.factorial(n) for s in range(n)]
    phi = np.zeros(n)
    for j in range(n):
        for mask in range(1 << n):
            if not mask >> j & 1:
                phi[j] += w[bin(mask).count("1")] * (util[mask | 1 << j] - util[mask])
    return phi


def logits_for(rng, n, c, scale):
    """Random logits times `scale`; the second-to-last row has one dominant logit, the last row equal logits (where n allows)."""
    x = (rng.standard_normal((n, c)) * scale).astype(np.float32)
    if n >= 3:
        x[n - 2, rng.integers(0, c)] += np.float32(60.0 * scale)
        x[n - 1, :] = np.float32(0.5 * scale)
    return x


def t32(fn, *arrays):
    """fn on torch-CPU fp32 leaf tensors; returns (value, gradient of value.sum() w.r.t. the first array) as numpy."""
    ts = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
    ts[0].requires_grad_(True)
    v = fn(*ts)
    v.sum().backward()
    return v.detach().numpy(), ts[0].grad.numpy()


# ==========================================================================================================================================
# Tier 1: gather / scatter / pair / u8
# ==========================================================================================================================================
def _indices(rng, c, unique=False):
    R, n = c["R"], c["n"]
    if unique:
        return rng.permutation(R)[: min(n, R)].astype(np.int64)
    if c.get("idx") == "repeat":
        return rng.integers(0, 2, n).astype(np.int64) * (R - 1)
    return rng.integers(0, R, n).astype(np.int64)


@case_of("rows")
def test_gather_rows_is_exact(lib, name):
    c = find("rows", name)
    rng = np.random.default_rng(c["seed"])
    src = rng.standard_normal((c["R"], c["row"])).astype(np.float32)
    idx = _indices(rng, c)
    g = Guarded()
    d_src, d_idx = g.inp(src, c["off"][0], "src"), g.inp(idx, 0, "idx")
    d_dst = g.out((len(idx), c["row"]), torch.float32, c["off"][1], "dst")
    assert_path(lib, "rows", c, [d_src, d_dst])
    ok(lib, lib.ocl_gather_rows(vp(d_src), vp(d_idx), len(idx), c["row"] * 4, vp(d_dst), stream()), name)
    g.check(name)
    assert d_dst.cpu().numpy().tobytes() == src[idx].tobytes()


@case_of("rows")
def test_scatter_rows_is_exact_and_leaves_other_rows(lib, name):
    c = find("rows", name)
    rng = np.random.default_rng(c["seed"] + 1000)
    idx = _indices(rng, c, unique=True)      # (duplicate indices in a scatter are the caller's problem: the header)
    src = rng.standard_normal((len(idx), c["row"])).astype(np.float32)
    dst0 = rng.standard_normal((c["R"], c["row"])).astype(np.float32)
    g = Guarded()
    d_src, d_idx = g.inp(src, c["off"][0], "src"), g.inp(idx, 0, "idx")
    d_dst = g.out(None, off=c["off"][1], name="dst", init=dst0)
    assert_path(lib, "rows", dict(c, n=len(idx)), [d_src, d_dst])
    ok(lib, lib.ocl_scatter_rows(vp(d_dst), vp(d_idx), len(idx), c["row"] * 4, vp(d_src), stream()), name)
    g.check(name)
    exp = dst0.copy()
    exp[idx] = src
    assert d_dst.cpu().numpy().tobytes() == exp.tobytes()     # indexed rows replaced, every other row untouched


@case_of("pair")
def test_gather_pair_is_exact(lib, name):
    c = find("pair", name)
    rng = np.random.default_rng(c["seed"])
    a = rng.standard_normal((c["R"], c["row_a"])).astype(np.float32)
    b = rng.integers(-2 ** 31, 2 ** 31 - 1, (c["R"], c["row_b"])).astype(np.int32)
    idx = _indices(rng, c)
    g = Guarded()
    d_a, d_b = g.inp(a, c["off"], "a"), g.inp(b, 0, "b")
    d_da, d_db = g.out((c["n"], c["row_a"]), torch.float32, 0, "dst_a"), g.out((c["n"], c["row_b"]), torch.int32, 0, "dst_b")
    if c["idx"] == "host":
        host = torch.from_numpy(idx)
        d_idx = g.out((max(c["n"], 1),), torch.int64, 0, "idx_dev")
        hp = C.c_void_p(host.data_ptr())
    else:
        d_idx, hp = g.inp(idx if c["n"] else np.zeros(1, dtype=np.int64), 0, "idx_dev"), None
    assert_path(lib, "pair", c, [d_a, d_da])
    ok(lib, lib.ocl_gather_rows_pair(vp(d_a), c["row_a"] * 4, vp(d_da), vp(d_b), c["row_b"] * 4, vp(d_db), hp, vp(d_idx), c["n"], stream()), name)
    g.check(name)
    assert d_da.cpu().numpy().tobytes() == a[idx].tobytes() and d_db.cpu().numpy().tobytes() == b[idx].tobytes()
    if c["idx"] == "host" and c["n"]:
        assert np.array_equal(d_idx.cpu().numpy()[: c["n"]], idx)     # the uploaded index vector


@case_of("u8")
def test_gather_u8_images_is_exact(lib, name):
    c = find("u8", name)
    rng = np.random.default_rng(c["seed"])
    src = rng.integers(0, 256, (c["R"], c["h"], c["w"], c["c"])).astype(np.uint8)
    idx = _indices(rng, c)
    g = Guarded()
    d_src, d_idx = g.inp(src, c["off"], "src"), g.inp(idx if c["n"] else np.zeros(1, dtype=np.int64), 0, "idx")
    d_dst = g.out((c["n"], c["c"], c["h"], c["w"]), torch.float32, 0, "dst")
    assert_path(lib, "u8", c)
    ok(lib, lib.ocl_gather_u8_hwc_to_f32_chw(vp(d_src), vp(d_idx), c["n"], c["h"], c["w"], c["c"], vp(d_dst), stream()), name)
    g.check(name)
    exp = (src[idx].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)).astype(np.float32)     # ToTensor: .float().div(255)
    assert d_dst.cpu().numpy().tobytes() == np.ascontiguousarray(exp).tobytes()


# ==========================================================================================================================================
# Tier 1: SGD
# ==========================================================================================================================================
@case_of("sgd")
def test_sgd_is_exact_on_integers(lib, name):
    """p, g integers in [-1024, 1024], lr = 2^-3, wd = 2^-2, gs = 2^-1: p - lr (wd p + gs g) is a multiple of 2^-5 below 2^11, exact in fp32
    in any evaluation order (fused or not).  Also wd = 0, gs = 1 (the plain step)."""
    c = find("sgd", name)
    rng = np.random.default_rng(c["seed"])
    n = c["n"]
    p0 = rng.integers(-1024, 1025, n).astype(np.float32)
    g0 = rng.integers(-1024, 1025, n).astype(np.float32)
    for lr, wd, gs in [(0.125, 0.25, 0.5), (0.5, 0.0, 1.0)]:
        exp = (p0.astype(np.float64) - lr * (wd * p0.astype(np.float64) + gs * g0.astype(np.float64))).astype(np.float32)
        for with_out in (False, True):
            g = Guarded()
            d_g = g.inp(g0, 0, "grads")
            d_p = g.inp(p0, c["off"], "params") if with_out or c["path"] == "SGD_REFUSED" else g.out(None, off=c["off"], name="params", init=p0)
            d_o = g.out((n,), torch.float32, 0, "out") if with_out else None
            assert_path(lib, "sgd", c, [d_p, d_g, d_o])
            rc = lib.ocl_sgd_step(vp(d_p), vp(d_g), n, lr, wd, gs, vp(d_o), stream())
            g.check(name)
            if c["path"] == "SGD_REFUSED":
                assert rc != 0 and b"16-B aligned" in lib.ocl_last_error()
                continue
            ok(lib, rc, name)
            got = (d_o if with_out else d_p).cpu().numpy()
            assert got.tobytes() == exp.tobytes(), "%s lr=%g wd=%g gs=%g out=%s: %d elements differ" % (name, lr, wd, gs, with_out, int((got != exp).sum()))


# ==========================================================================================================================================
# small GEMM: tier 1 on integers, tier 2 on random fp32
# ==========================================================================================================================================
def _run_gemm(lib, c, a, b, bias, c0, name):
    m, n, k = c["m"], c["n"], c["k"]
    g = Guarded()
    d_a = g.inp(np.ascontiguousarray(a.T) if c["at"] else a, 0, "a")
    d_b = g.inp(np.ascontiguousarray(b.T) if c["bt"] else b, 0, "b")
    d_bias = g.inp(bias, 0, "bias") if c["bias"] else None
    d_c = g.out(None, name="c", init=c0)
    a_rs, a_cs = (1, m) if c["at"] else (k, 1)
    b_rs, b_cs = (1, k) if c["bt"] else (n, 1)
    assert_path(lib, "gemm", c)
    ok(lib, lib.ocl_gemm_small(vp(d_a), a_rs, a_cs, vp(d_b), b_rs, b_cs, vp(d_c), n + c["pad"], m, n, k, vp(d_bias), c["relu"], c["acc"], stream()), name)
    g.check(name)
    got = d_c.cpu().numpy()
    assert got[:, n:].tobytes() == c0[:, n:].tobytes(), "%s: columns beyond n written" % name
    return got[:, :n]


def _gemm_ref(c, a, b, bias, c0):
    r = a.astype(np.float64) @ b.astype(np.float64)
    terms = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    if c["bias"]:
        r, terms = r + bias, terms + np.abs(bias)
    if c["acc"]:
        r, terms = r + c0[:, : c["n"]], terms + np.abs(c0[:, : c["n"]])
    return (np.maximum(r, 0.0) if c["relu"] else r), terms


@case_of("gemm")
def test_gemm_small_is_exact_on_integers(lib, name):
    """|a|, |b| <= 8, k <= 640: every partial sum is an integer below 2^24 whatever the order."""
    c = find("gemm", name)
    rng = np.random.default_rng(c["seed"])
    m, n, k = c["m"], c["n"], c["k"]
    a = rng.integers(-8, 9, (m, k)).astype(np.float32)
    b = rng.integers(-8, 9, (k, n)).astype(np.float32)
    bias = rng.integers(-8, 9, n).astype(np.float32)
    c0 = rng.integers(-50, 51, (m, n + c["pad"])).astype(np.float32)
    got = _run_gemm(lib, c, a, b, bias, c0, name)
    ref, _ = _gemm_ref(c, a, b, bias, c0)
    assert np.array_equal(got.astype(np.float64), ref), "%s: %d elements differ" % (name, int((got != ref).sum()))


@case_of("gemm")
def test_gemm_small_random_within_fp32_bound(lib, name):
    c = find("gemm", name)
    rng = np.random.default_rng(c["seed"] + 5000)
    m, n, k = c["m"], c["n"], c["k"]
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    c0 = rng.standard_normal((m, n + c["pad"])).astype(np.float32)
    got = _run_gemm(lib, c, a, b, bias, c0, name)
    ref, terms = _gemm_ref(c, a, b, bias, c0)
    check_derived("gemm/" + name, "c", got, ref, 1.01 * (k + 2) * U * terms)


# ==========================================================================================================================================
# column reductions and the ASER score
# ==========================================================================================================================================
def _pow2(v):
    return v & (v - 1) == 0


@case_of("col_reduce")
def test_col_reduce(lib, name):
    """Integers: sum / max / min exact, mean exact where rows is a power of two.  Random fp32: the sums are accumulated in float64, one fp32
    rounding at the end (K = 1)."""
    c = find("col_reduce", name)
    rng = np.random.default_rng(c["seed"])
    rows, cols = c["rows"], c["cols"]
    for kind in ("int", "rand"):
        m = rng.integers(-8, 9, (rows, cols)).astype(np.float32) if kind == "int" else rng.standard_normal((rows, cols)).astype(np.float32)
        m64 = m.astype(np.float64)
        for mode, ref in enumerate([m64.sum(0), m64.mean(0), m64.max(0), m64.min(0)]):
            g = Guarded()
            d_m, d_o = g.inp(m, 0, "m"), g.out((cols,), torch.float32, 0, "out")
            assert_path(lib, "col_reduce", c)
            ok(lib, lib.ocl_col_reduce(vp(d_m), rows, cols, mode, vp(d_o), stream()), name)
            g.check(name)
            got = d_o.cpu().numpy().astype(np.float64)
            if mode >= 2 or (kind == "int" and (mode == 0 or _pow2(rows))):
                assert np.array_equal(got, ref), "%s %s mode %d" % (name, kind, mode)
            else:
                check_derived("col_reduce/%s/%s" % (name, kind), ["sum", "mean"][mode], got, ref,
                              1.01 * U * np.abs(m64).sum(0) / (rows if mode == 1 else 1))


@case_of("aser")
def test_aser_score(lib, name):
    """aser_retrieve.py:77-86: asvm = mean(coop) - mean(adv), asv = max(coop) - min(adv), neg_sv = -sum(adv), per candidate column."""
    c = find("aser", name)
    rng = np.random.default_rng(c["seed"])
    na, nc, n = c["n_adv"], c["n_coop"], c["n_cand"]
    for kind in ("int", "rand"):
        draw = (lambda s: rng.integers(-8, 9, s).astype(np.float32)) if kind == "int" else (lambda s: rng.standard_normal(s).astype(np.float32))
        adv, coop = draw((na, n)), draw((nc, n))
        a64, c64 = adv.astype(np.float64), coop.astype(np.float64)
        for typ, ref in enumerate([c64.mean(0) - a64.mean(0), c64.max(0) - a64.min(0), -a64.sum(0)]):
            g = Guarded()
            d_a, d_c, d_o = g.inp(adv, 0, "adv"), g.inp(coop, 0, "coop"), g.out((n,), torch.float32, 0, "out")
            assert_path(lib, "aser", c)
            ok(lib, lib.ocl_aser_score(vp(d_a), na, vp(d_c) if typ != 2 else None, nc if typ != 2 else 0, n, typ, vp(d_o), stream()), name)
            g.check(name)
            got = d_o.cpu().numpy().astype(np.float64)
            if kind == "int" and (typ != 0 or (_pow2(na) and _pow2(nc))):
                assert np.array_equal(got, ref), "%s type %d" % (name, typ)
            else:
                # float64 sums; fp32 roundings: the two means (or extrema: exact) and their difference, or the one sum: K <= 3
                terms = [np.abs(c64).mean(0) + np.abs(a64).mean(0), np.abs(c64).max(0) + np.abs(a64).max(0), np.abs(a64).sum(0)][typ]
                check_derived("aser/%s/%s" % (name, kind), ["asvm", "asv", "neg_sv"][typ], got, ref, 1.01 * 3 * U * terms)


# ==========================================================================================================================================
# argsort
# ==========================================================================================================================================
def _argsort_data(rng, n, kind):
    v = rng.standard_normal(n).astype(np.float32)
    if kind == "ties":
        v = rng.integers(-3, 4, n).astype(np.float32)
    elif kind == "zeros":
        v = np.where(rng.integers(0, 2, n) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        v[0], v[-1] = np.float32(-0.0), np.float32(0.0)
    elif kind == "equal":
        v[:] = 1.5
    elif kind == "inf":
        v[rng.integers(0, n, max(1, n // 8))] = np.inf
        v[rng.integers(0, n, max(1, n // 8))] = -np.inf
        v[0], v[-1] = -np.inf, np.inf
    elif kind in ("nan", "nan_inf"):
        v[rng.integers(0, n, n // 6)] = np.nan
        if kind == "nan_inf":
            v[rng.integers(0, n, n // 6)] = np.inf
            v[rng.integers(0, n, n // 6)] = -np.inf
            v[0], v[1], v[2] = np.inf, np.nan, np.inf      # +inf before a NaN by index: NaN must still come first
    return v


@case_of("argsort")
def test_argsort_desc_order(lib, name):
    """Descending, ties in ascending index order (-0.0 == +0.0 is a tie), +-inf at the ends; NaN first, before +inf, in index order
    (the header): exactly torch.argsort(descending=True, stable=True) on the CPU."""
    c = find("argsort", name)
    rng = np.random.default_rng(c["seed"])
    n = c["n"]
    v = _argsort_data(rng, n, c["data"])
    g = Guarded()
    d_v, d_o = g.inp(v, 0, "v"), g.out((n,), torch.int64, 0, "idx")
    assert_path(lib, "argsort", c)
    rc = lib.ocl_argsort_desc(vp(d_v), n, vp(d_o), stream())
    g.check(name)
    if c["path"] == "ARGSORT_REFUSED":
        assert rc != 0
        assert bool(Guarded.is_poison(d_o).all())
        return
    ok(lib, rc, name)
    got = d_o.cpu().numpy()
    exp_torch = torch.argsort(torch.from_numpy(v), descending=True, stable=True).numpy()
    if not np.isnan(v).any():
        exp = np.argsort(-v.astype(np.float64), kind="stable")      # stable float64 sort of the negated values: the documented tie rule
        assert np.array_equal(exp, exp_torch)
    assert np.array_equal(got, exp_torch), "%s: first difference at rank %d" % (name, int(np.nonzero(got != exp_torch)[0][0]))


# ==========================================================================================================================================
# kNN-Shapley
# ==========================================================================================================================================
def _knn_call(lib, c, ef, ey, cf, cy, what):
    """One ocl_knn_sv call on guarded tensors, on the path the case names: (sorted_idx, sv_out) as numpy.  Guards intact, inputs unchanged, every
    row of sorted_idx a permutation of the candidates, no cell of sv_out left unwritten, every value finite."""
    ne, nc, dim, k = c["ne"], c["nc"], c["dim"], c["k"]
    g = Guarded()
    d_ef, d_ey, d_cf, d_cy = g.inp(ef, 0, "eval_f"), g.inp(ey, 0, "eval_y"), g.inp(cf, c["off"], "cand_f"), g.inp(cy, 0, "cand_y")
    d_sv, d_ord = g.out((ne, nc), torch.float32, 0, "sv"), g.out((ne, nc), torch.int64, 0, "order")
    assert_path(lib, "knn", c, [d_cf])
    ok(lib, lib.ocl_knn_sv(vp(d_ef), vp(d_ey), ne, vp(d_cf), vp(d_cy), nc, dim, k, vp(d_sv), vp(d_ord), stream()), what)
    g.check(what)
    order, sv = d_ord.cpu().numpy(), d_sv.cpu().numpy()
    assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(nc), (ne, 1))), "%s: a row of sorted_idx is no permutation" % what
    assert not Guarded.is_poison(sv).any(), "%s: %d cells of sv_out were not written" % (what, int(Guarded.is_poison(sv).sum()))
    assert np.isfinite(sv).all(), what
    return order, sv


def _knn_nonfinite_case(lib, c):
    """special="nonfinite" (knn_ref.nonfinite_inputs): NaN and +inf among integer-valued features.  Every key is exact, +inf or NaN, so K10's
    total order -- torch.argsort(keys, stable=True) -- is fully determined: sorted_idx must be that order, sv_out the oracle's bits for it."""
    from oracle import ocl_oracle as O
    ef, ey, cf, cy = KR.nonfinite_inputs(c)
    exp_order = KR.stable_order(KR.keys64(ef, cf))
    order, sv = _knn_call(lib, c, ef, ey, cf, cy, c["name"])
    for r in range(c["ne"]):
        assert np.array_equal(order[r], exp_order[r]), "%s row %d: %s, not %s" % (c["name"], r, order[r].tolist(), exp_order[r].tolist())
    exp, _ = O.knn_sv(ef, ey, cf, cy, c["k"], order=exp_order)
    assert sv.tobytes() == exp.tobytes(), "%s: max diff %g" % (c["name"], np.abs(sv - exp).max())


def _knn_real_case(lib, c):
    """data="real" (knn_ref.real_inputs: standard normal, clustered, near ties): the kernel's order must be an ascending order of the float64
    distances up to the path's rounding -- every adjacent pair that float64 orders the other way is within 1.01 K 2^-24 (d_a + d_b), K =
    knn_ref.path_k (derived there from the kernel's code: 2 for the subtraction under the square, the fused steps of the longest lane chain,
    the final adds or the shuffle tree) -- and, given that order, sv_out has the oracle's bits."""
    from oracle import ocl_oracle as O
    K = KR.path_k(c["path"], c["dim"])
    for kind in KR.KINDS:
        what = "knn/%s/%s" % (c["name"], kind)
        ef, ey, cf, cy = KR.real_inputs(c, kind)
        order, sv = _knn_call(lib, c, ef, ey, cf, cy, what)
        n_inv, n_pairs, gap, bound = KR.inverted_pairs(order, KR.keys64(ef, cf), K)
        PB.record(REPORT, what, "order", gap, None, bound)
        print("%s: K = %d, %d of %d adjacent pairs inverted against float64, worst gap %.4g, bound %.4g" % (what, K, n_inv, n_pairs, gap, bound))
        assert gap <= bound, "%s: the order is not ascending in float64 beyond round-off: gap %.4g, bound %.4g" % (what, gap, bound)
        exp, _ = O.knn_sv(ef, ey, cf, cy, c["k"], order=order)
        assert sv.tobytes() == exp.tobytes(), "%s: max diff %g" % (what, np.abs(sv - exp).max())


@case_of("knn")
def test_knn_sv_on_integer_features(lib, name):
    """Integer-valued features: squared distances are exact in fp32, so the order -- index-ordered ties included -- is fully determined; with
    NaN and +inf planted among them (special="nonfinite") it still is.  The cases on real-valued features (data="real") are judged by the
    derived bound of their distance path (_knn_real_case)."""
    from oracle import ocl_oracle as O
    c = find("knn", name)
    if c.get("special") == "nonfinite":
        return _knn_nonfinite_case(lib, c)
    if c.get("data") == "real":
        return _knn_real_case(lib, c)
    rng = np.random.default_rng(c["seed"])
    ne, nc, dim, k = c["ne"], c["nc"], c["dim"], c["k"]
    ef = rng.integers(-4, 5, (ne, dim)).astype(np.float32)
    cf = rng.integers(-4, 5, (nc, dim)).astype(np.float32)
    if nc >= 4:
        cf[nc - 1] = cf[0]          # exact ties between candidates far apart in index
        cf[nc // 2] = cf[1]
    ey, cy = rng.integers(0, 3, ne).astype(np.int64), rng.integers(0, 3, nc).astype(np.int64)
    g = Guarded()
    d_ef, d_ey, d_cf, d_cy = g.inp(ef, 0, "eval_f"), g.inp(ey, 0, "eval_y"), g.inp(cf, c["off"], "cand_f"), g.inp(cy, 0, "cand_y")
    if c["path"] == "KNN_REFUSED":
        d_sv, d_ord = g.out((16,), torch.float32, 0, "sv"), g.out((16,), torch.int64, 0, "order")
        assert assert_path(lib, "knn", c, [d_cf]).grid_x == 0
        assert lib.ocl_knn_sv(vp(d_ef), vp(d_ey), ne, vp(d_cf), vp(d_cy), nc, dim, k, vp(d_sv), vp(d_ord), stream()) != 0
        g.check(name)
        assert bool(Guarded.is_poison(d_sv).all())
        return
    d_sv, d_ord = g.out((ne, nc), torch.float32, 0, "sv"), g.out((ne, nc), torch.int64, 0, "order")
    assert_path(lib, "knn", c, [d_cf])
    ok(lib, lib.ocl_knn_sv(vp(d_ef), vp(d_ey), ne, vp(d_cf), vp(d_cy), nc, dim, k, vp(d_sv), vp(d_ord), stream()), name)
    g.check(name)
    d64, order = ref_knn_order(ef, cf)
    assert d64.max() < 2 ** 24
    assert np.array_equal(d_ord.cpu().numpy(), order), name
    exp, _ = O.knn_sv(ef, ey, cf, cy, k, order=order)        # (pinned to the reference golden by test_cpu_oracle_golden.py)
    got = d_sv.cpu().numpy()
    assert got.tobytes() == exp.tobytes(), "%s: max diff %g" % (name, np.abs(got - exp).max())
    # against the definition, where the reference's closed form is the Shapley value (k <= n_cand: see shapley_subsets)
    if nc <= 12 and k <= nc:
        for r in range(ne):
            bf = shapley_subsets(d64[r], cy == ey[r], k)
            assert np.abs(got[r].astype(np.float64) - bf).max() <= nc * 2.0 ** -23, (name, r)


def test_knn_sv_op_orders_nonfinite_features(cuda):
    """ops.knn_sv(want_order=True), the call the ASER plugins make, on the non-finite cases' data: every row of the order is a permutation of
    the candidates -- the stable order of the keys -- and the values are the oracle's for it (the op allocates sv_out uninitialised)."""
    from ocl_amd import ops
    from oracle import ocl_oracle as O
    for c in [c for c in SC.CASES["knn"] if c.get("special") == "nonfinite"]:
        ef, ey, cf, cy = KR.nonfinite_inputs(c)
        sv, order = ops.knn_sv(*(torch.from_numpy(a).cuda() for a in (ef, ey, cf, cy)), c["k"], want_order=True)
        order, sv = order.cpu().numpy(), sv.cpu().numpy()
        for r in range(c["ne"]):
            assert sorted(order[r].tolist()) == list(range(c["nc"])), (c["name"], r, order[r].tolist())
        exp_order = KR.stable_order(KR.keys64(ef, cf))
        assert np.array_equal(order, exp_order), c["name"]
        assert sv.tobytes() == O.knn_sv(ef, ey, cf, cy, c["k"], order=exp_order)[0].tobytes(), c["name"]


# ==========================================================================================================================================
# NCM
# ==========================================================================================================================================
def _norm_k(d):
    """fp32 roundings behind one normalised element f / sqrt(sum f^2): the sum's chain (ceil(d / 256) fused steps, then an 8-step tree), as a
    relative error of the norm (half of the sum's), the square root and the division."""
    return 0.5 * (math.ceil(d / 256.0) + 8) + 2


@case_of("ncm_means")
def test_ncm_class_means(lib, name):
    """agents/base.py:121-142: per class, the mean of the L2-normalised features, L2-normalised.  Counts exact; a class without a sample keeps its
    row.  Bound: each normalised term carries _norm_k(d) roundings, the float64 mean adds one, the final normalisation _norm_k(d) again; an
    error e_j of mu_j moves mu_j / |mu| by at most e_j / |mu| + |m_j| (sum_i |mu_i| e_i) / |mu|^2."""
    c = find("ncm_means", name)
    rng = np.random.default_rng(c["seed"])
    n, d, ncls = c["n"], c["d"], c["n_cls"]
    class_ids = (rng.permutation(50)[:ncls] + 3).astype(np.int64)
    present = class_ids[: ncls - c["absent"]]
    labels = present[rng.integers(0, len(present), n)].astype(np.int64)
    labels[: len(present)] = present
    feat = rng.standard_normal((n, d)).astype(np.float32)
    g = Guarded()
    d_f, d_l, d_ids = g.inp(feat, 0, "feat"), g.inp(labels, 0, "labels"), g.inp(class_ids, 0, "class_ids")
    d_m, d_cnt = g.out((ncls, d), torch.float32, 0, "means"), g.out((ncls,), torch.int32, 0, "counts")
    assert_path(lib, "ncm_means", c)
    ok(lib, lib.ocl_ncm_class_means(vp(d_f), vp(d_l), n, d, vp(d_ids), ncls, vp(d_m), vp(d_cnt), stream()), name)
    g.check(name)
    got, cnt = d_m.cpu().numpy().astype(np.float64), d_cnt.cpu().numpy()
    f64 = feat.astype(np.float64)
    fn = f64 / np.linalg.norm(f64, axis=1, keepdims=True)
    K = _norm_k(d)
    for ci, cls in enumerate(class_ids):
        sel = labels == cls
        assert cnt[ci] == sel.sum()
        if not sel.any():
            assert Guarded.is_poison(got[ci]).all(), "%s: the row of a class without samples was written" % name
            continue
        mu = fn[sel].mean(0)
        e = 1.01 * (K + 1) * U * np.abs(fn[sel]).mean(0)
        nrm = np.linalg.norm(mu)
        ref = mu / nrm
        bound = e / nrm + np.abs(ref) * (np.abs(mu) * e).sum() / nrm ** 2 + 1.01 * K * U * np.abs(ref)
        check_derived("ncm_means/%s/class%d" % (name, ci), "means", got[ci], ref, bound)


@case_of("ncm_predict")
def test_ncm_predict(lib, name):
    """agents/base.py:159-176: argmin over classes of |f / |f| - mean_c|^2, the first minimum on an exact tie.  ties=1: duplicated mean rows and
    features proportional to one of the pair, so two distances are computed from identical numbers: the lower index must win.  Otherwise the
    prediction must be the float64 argmin unless the two distances are within the fp32 bound of each other: a distance carries
    (ceil(d / 64) + 6) roundings on sum t^2 and the normalisation's error in t = f / |f| - mu."""
    c = find("ncm_predict", name)
    rng = np.random.default_rng(c["seed"])
    n, d, ncls = c["n"], c["d"], c["n_cls"]
    means = rng.standard_normal((ncls, d)).astype(np.float32)
    means /= np.linalg.norm(means, axis=1, keepdims=True)
    feat = rng.standard_normal((max(n, 1), d)).astype(np.float32)[:n]
    if c["ties"]:
        for j in range(0, ncls - 1, 2):
            means[j + 1] = means[j]
        feat = (means[rng.integers(0, ncls, n)] * np.float32(3.0) + rng.standard_normal((n, d)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    if c.get("nan"):
        # NaN distances (K11): torch.min's rule on the CPU, the first NaN wins and otherwise the first minimum.  Rows near one mean each, so
        # that the rows without a NaN are decided far outside round-off
        feat = (means[rng.integers(0, ncls, n)] * np.float32(3.0) + rng.standard_normal((n, d)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        if c["nan"] == "feat":
            feat[n // 2, d - 1] = np.nan
        for cls in {"mean": [3], "two_means": [4, 2], "feat": []}[c["nan"]]:
            means[cls, cls] = np.nan
    g = Guarded()
    d_f = g.inp(feat if n else np.zeros((1, d), dtype=np.float32), 0, "feat")
    d_m, d_p = g.inp(means, 0, "means"), g.out((max(n, 1),), torch.int64, 0, "pred")
    assert_path(lib, "ncm_predict", c)
    ok(lib, lib.ocl_ncm_predict(vp(d_f), n, d, vp(d_m), ncls, vp(d_p), stream()), name)
    g.check(name)
    pred = d_p.cpu().numpy()
    if n == 0:
        assert Guarded.is_poison(pred).all()
        return
    f64 = feat.astype(np.float64)
    fn = f64 / np.linalg.norm(f64, axis=1, keepdims=True)
    t = fn[:, None, :] - means.astype(np.float64)[None, :, :]
    d64 = (t ** 2).sum(-1)
    if c.get("nan"):
        exp = torch.min(torch.from_numpy(d64), 1).indices.numpy()
        nan_rows = np.isnan(d64).any(1)
        assert nan_rows.sum() == (1 if c["nan"] == "feat" else n) and (exp[nan_rows] == {"mean": 3, "two_means": 2, "feat": 0}[c["nan"]]).all()
        assert np.array_equal(exp[~nan_rows], d64[~nan_rows].argmin(1))
        assert np.array_equal(pred, exp), "%s: %s, torch.min gives %s" % (name, pred.tolist(), exp.tolist())
        return
    bound = 1.01 * (math.ceil(d / 64.0) + 6) * U * d64 + 2 * 1.01 * (_norm_k(d) + 1) * U * (np.abs(t) * np.abs(fn)[:, None, :]).sum(-1)
    assert ((pred >= 0) & (pred < ncls)).all()
    best = d64.argmin(1)
    rows = np.arange(n)
    gap = d64[rows, pred] - d64[rows, best]
    assert (gap <= bound[rows, pred] + bound[rows, best]).all(), "%s: a prediction is not the nearest mean beyond fp32 round-off" % name
    if c["ties"]:
        # rows (0, 1), (2, 3), ... of the means are identical: the winner of an exactly tied pair is its lower (even) index
        assert (pred % 2 == 0).all(), "%s: the higher index of a tied pair won in %d rows" % (name, int((pred % 2 == 1).sum()))
        assert np.array_equal(pred // 2, best // 2), name


# ==========================================================================================================================================
# cosine-max
# ==========================================================================================================================================
@case_of("cosine")
def test_cosine_max(lib, name):
    """max_i dot(mem_i, g) / max(|mem_i| |g|, eps) (buffer_utils.py:51-56).  The kernel keeps fp32 partial sums per thread (a chain of
    ceil(per-workgroup units / 256) fused steps, x4 for float4 units), float64 from there; then fp32 square roots, product and division.
    Bound per row: E(dot) / w + |cos| (E(mm) / 2mm + E(gg) / 2gg) + 8 ulp |cos|, with E(s) = 1.01 K 2^-24 sum|terms| + 2^-24 |s|."""
    from ocl_amd import ffi
    c = find("cosine", name)
    rng = np.random.default_rng(c["seed"])
    n, k, eps = c["n"], c["k"], 1e-8
    mem = rng.standard_normal((k, n)).astype(np.float32)
    gv = rng.standard_normal(n).astype(np.float32)
    sp = c.get("special")
    if sp == "zero_row":
        mem[1] = 0.0
    if sp == "zero_g":
        gv[:] = 0.0
    if sp == "max_last":
        mem[k - 1] = gv * np.float32(2.0) + rng.standard_normal(n).astype(np.float32) * np.float32(0.05)
    g = Guarded()
    d_mem, d_g = g.inp(mem, c["off"][0], "mem"), g.inp(gv, c["off"][1], "g")
    ws_bytes = lib.ocl_cosine_max_workspace_bytes(k)
    assert ws_bytes == 512 * (2 * k + 1) * 8
    outs = []
    plan = None
    for rep in range(2):
        d_ws, d_o = g.out((ws_bytes // 8,), torch.float64, 0, "workspace%d" % rep), g.out((1,), torch.float32, 0, "out%d" % rep)
        plan = assert_path(lib, "cosine", c, [d_mem, d_g])
        ok(lib, lib.ocl_cosine_max(vp(d_mem), k, n, vp(d_g), eps, vp(d_o), vp(d_ws), stream()), name)
        outs.append(d_o)
    g.check(name)
    a, b = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert a.tobytes() == b.tobytes(), "%s: two calls differ (%r, %r)" % (name, a, b)     # no atomics: bit-reproducible
    m64, g64 = mem.astype(np.float64), gv.astype(np.float64)
    dot, mm, gg = m64 @ g64, (m64 * m64).sum(1), float(g64 @ g64)
    w = np.maximum(np.sqrt(mm) * math.sqrt(gg), eps)
    cos = dot / w
    vec = c["path"].startswith("COS_VEC")
    units = n // 4 if vec else n
    K = math.ceil(math.ceil(units / plan.aux) / 256.0) * (4 if vec else 1) + 1
    E = lambda s, terms: 1.01 * K * U * terms + U * np.abs(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_w = np.where(mm > 0, E(mm, mm) / (2 * mm), 0.0) + (E(gg, gg) / (2 * gg) if gg > 0 else 0.0)
    bound = E(dot, np.abs(m64) @ np.abs(g64)) / w + np.abs(cos) * rel_w + 8 * 2 * U * np.abs(cos) + 2.0 ** -149
    if sp == "zero_g":
        assert (cos == 0).all()
    if sp == "zero_row":
        assert cos[1] == 0.0
    if sp == "max_last":
        assert int(cos.argmax()) == k - 1
    ref = float(cos.max())
    check_derived("cosine/" + name, "max", a, np.array([ref]), np.array([float(bound.max())]))


# ==========================================================================================================================================
# Tier 2: cross-entropy, segmented cross-entropy, KD, MIR
# ==========================================================================================================================================
def _cap(c):
    """The shapes the golden tests (test_gpu_kernels.py) bound by 1e-5: the new bound must not be looser there."""
    return 1e-5 if c["scale"] == 1 and (c["n"], c["c"]) == (10, 100) else None


def _labels_outside_case(lib, op, c):
    """bad_labels cases of ce, ce_seg and mir (K6, K12): the labels c, c + 5 and -1 in the first, a middle and the last row.  Every tensor is
    guarded, so label-addressed reads with these offsets would stay inside the test's own allocation (and return a sentinel or a neighbour's
    logit: a finite, wrong loss).  The contract: a bad row's loss (and so the mean, and the MIR score) is NaN; every other row's loss and
    dlogits have the bits of the same call with valid labels in the bad rows; a bad row's dlogits stay inside the row -- the softmax alone
    (ce: the valid call's row except at that call's label) or, segmented, zeros."""
    rng = np.random.default_rng(c["seed"])
    n, cc = c["n"], c["c"]
    bad = SC.bad_labels(n, cc)
    bad_rows = [r for r, _ in bad]
    assert len(set(bad_rows)) == 3 and bad_rows[0] == 0 and bad_rows[2] == n - 1 and [v for _, v in bad] == [cc, cc + 5, -1]
    x, x2 = logits_for(rng, n, cc, c["scale"]), logits_for(rng, n, cc, c["scale"])
    seg = rng.integers(0, c.get("seg", 1), cc).astype(np.int32)
    seg[rng.permutation(cc)[: cc // 4]] = -1
    live = np.nonzero(seg >= 0)[0]
    y_ok = live[rng.integers(0, len(live), n)].astype(np.int64)
    y_bad = y_ok.copy()
    for r, v in bad:
        y_bad[r] = v
    good_rows = np.array([r for r in range(n) if r not in bad_rows])

    def run(y, tag):
        g = Guarded()
        d_x, d_y = g.inp(x, 0, "logits"), g.inp(y, 0, "y")
        if op == "mir":
            d_x2, d_o = g.inp(x2, 0, "post"), g.out((n,), torch.float32, 0, "scores")
            assert_path(lib, "mir", c)
            ok(lib, lib.ocl_mir_scores(vp(d_x), vp(d_x2), vp(d_y), n, cc, vp(d_o), stream()), tag)
            g.check(tag)
            return d_o.cpu().numpy(), None
        d_dx = g.out((n, cc), torch.float32, 0, "dlogits")
        assert_path(lib, op, c)
        if op == "ce":
            red = 1 if c["red"] == "mean" else 0
            d_l, d_l2 = g.out((1 if red else n,), torch.float32, 0, "loss"), g.out((1 if red else n,), torch.float32, 0, "loss2")
            ok(lib, lib.ocl_ce_fwd_bwd(vp(d_x), vp(d_y), n, cc, red, vp(d_l), vp(d_dx), stream()), tag)
            ok(lib, lib.ocl_ce_fwd_bwd(vp(d_x), vp(d_y), n, cc, red, vp(d_l2), None, stream()), tag)
        else:
            d_s = g.inp(seg, 0, "seg")
            d_l, d_l2 = g.out((1,), torch.float32, 0, "loss"), g.out((1,), torch.float32, 0, "loss2")
            ok(lib, lib.ocl_ce_segmented_fwd_bwd(vp(d_x), vp(d_y), vp(d_s), n, cc, vp(d_l), vp(d_dx), stream()), tag)
            ok(lib, lib.ocl_ce_segmented_fwd_bwd(vp(d_x), vp(d_y), vp(d_s), n, cc, vp(d_l2), None, stream()), tag)
        g.check(tag)
        assert d_l.cpu().numpy().tobytes() == d_l2.cpu().numpy().tobytes()
        return d_l.cpu().numpy(), d_dx.cpu().numpy()

    l_ok, dx_ok = run(y_ok, c["name"] + " (valid labels)")
    l_bad, dx_bad = run(y_bad, c["name"])
    assert np.isfinite(l_ok).all()
    if len(l_bad) == n:                                             # per-row losses / scores
        assert np.isnan(l_bad[bad_rows]).all(), "%s: rows %s: %s" % (c["name"], bad_rows, l_bad[bad_rows].tolist())
        assert l_bad[good_rows].tobytes() == l_ok[good_rows].tobytes()
    else:
        assert np.isnan(l_bad).all(), "%s: the mean is %r" % (c["name"], l_bad.tolist())
    if dx_bad is None:
        return
    assert not Guarded.is_poison(dx_bad).any()
    assert dx_bad[good_rows].tobytes() == dx_ok[good_rows].tobytes(), "%s: the gradient of a row with a valid label changed" % c["name"]
    for r in bad_rows:
        if op == "ce":
            keep = np.arange(cc) != y_ok[r]
            assert dx_bad[r][keep].tobytes() == dx_ok[r][keep].tobytes() and np.isfinite(dx_bad[r]).all(), (c["name"], r)
            assert dx_bad[r, y_ok[r]] > dx_ok[r, y_ok[r]]          # the softmax, without the valid call's -1 at its label
        else:
            assert (dx_bad[r] == 0).all(), (c["name"], r)


@case_of("ce")
def test_cross_entropy(lib, name):
    """Loss and gradient in one call, loss only (dlogits NULL: bit-equal loss), reduction none and mean; the gradient target is a row block
    in the middle of a larger buffer (guarded on both sides like every tensor here)."""
    c = find("ce", name)
    if c.get("bad_labels"):
        return _labels_outside_case(lib, "ce", c)
    rng = np.random.default_rng(c["seed"])
    n, cc = c["n"], c["c"]
    x = logits_for(rng, n, cc, c["scale"])
    y = rng.integers(0, cc, n).astype(np.int64)
    red = 1 if c["red"] == "mean" else 0
    rows, grad = ref_ce(x.astype(np.float64), y)
    ref_loss, ref_grad = (np.array([rows.mean()]), grad / n) if red else (rows, grad)
    l32, g32 = t32(lambda a, b: F.cross_entropy(a, b, reduction=c["red"]), x, y)
    g = Guarded()
    d_x, d_y = g.inp(x, 0, "logits"), g.inp(y, 0, "y")
    d_l, d_dx = g.out((n if not red else 1,), torch.float32, 0, "loss"), g.out((n, cc), torch.float32, 0, "dlogits")
    d_l2 = g.out((n if not red else 1,), torch.float32, 0, "loss (no gradient)")
    assert_path(lib, "ce", c)
    ok(lib, lib.ocl_ce_fwd_bwd(vp(d_x), vp(d_y), n, cc, red, vp(d_l), vp(d_dx), stream()), name)
    ok(lib, lib.ocl_ce_fwd_bwd(vp(d_x), vp(d_y), n, cc, red, vp(d_l2), None, stream()), name)
    g.check(name)
    assert d_l.cpu().numpy().tobytes() == d_l2.cpu().numpy().tobytes()
    check_vs_torch32("ce/" + name, "loss", d_l.cpu().numpy(), ref_loss, l32.reshape(ref_loss.shape), _cap(c))
    check_vs_torch32("ce/" + name, "grad", d_dx.cpu().numpy(), ref_grad, g32, _cap(c))


@case_of("ce_seg")
def test_cross_entropy_segmented(lib, name):
    c = find("ce_seg", name)
    if c.get("bad_labels"):
        return _labels_outside_case(lib, "ce_seg", c)
    rng = np.random.default_rng(c["seed"])
    n, cc = c["n"], c["c"]
    x = logits_for(rng, n, cc, c["scale"])
    seg = rng.integers(0, c["seg"], cc).astype(np.int32)
    seg[rng.permutation(cc)[: cc // 4]] = -1             # columns that take part in no row, at random positions
    live = np.nonzero(seg >= 0)[0]
    y = live[rng.integers(0, len(live), n)].astype(np.int64)
    ref_loss, ref_grad = ref_ce_seg(x.astype(np.float64), y, seg.astype(np.int64))
    mask = torch.from_numpy(seg[None, :] == seg[y][:, None])
    l32, g32 = t32(lambda a, b: F.cross_entropy(torch.where(mask, a, torch.tensor(-float("inf"))), b), x, y)
    g = Guarded()
    d_x, d_y, d_s = g.inp(x, 0, "logits"), g.inp(y, 0, "y"), g.inp(seg, 0, "seg")
    d_l, d_dx, d_l2 = g.out((1,), torch.float32, 0, "loss"), g.out((n, cc), torch.float32, 0, "dlogits"), g.out((1,), torch.float32, 0, "loss2")
    assert_path(lib, "ce_seg", c)
    ok(lib, lib.ocl_ce_segmented_fwd_bwd(vp(d_x), vp(d_y), vp(d_s), n, cc, vp(d_l), vp(d_dx), stream()), name)
    ok(lib, lib.ocl_ce_segmented_fwd_bwd(vp(d_x), vp(d_y), vp(d_s), n, cc, vp(d_l2), None, stream()), name)
    g.check(name)
    assert d_l.cpu().numpy().tobytes() == d_l2.cpu().numpy().tobytes()
    got = d_dx.cpu().numpy()
    dead = seg[None, :] != seg[y][:, None]
    assert (got[dead] == 0).all(), "%s: gradient in a column outside the row's segment" % name
    check_vs_torch32("ce_seg/" + name, "loss", d_l.cpu().numpy(), np.array([ref_loss]), l32.reshape(1))
    check_vs_torch32("ce_seg/" + name, "grad", got, ref_grad, g32)


@case_of("kd")
def test_kd_loss(lib, name):
    """utils/kd_manager.py:6-11 at temperatures other than the goldens' 2.  With scores * (1 / T) in place of the reference's scores / T the
    gradient of n7_c1000_s30_T3 was off by 9.72e-06 (bound 4.96e-07, torch fp32 1.24e-07): kd_kernel divides now."""
    from oracle import ocl_oracle as O
    c = find("kd", name)
    rng = np.random.default_rng(c["seed"])
    n, cc, T = c["n"], c["c"], c["T"]
    s, t = logits_for(rng, n, cc, c["scale"]), logits_for(rng, n, cc, c["scale"])
    ref_loss, ref_grad = ref_kd(s.astype(np.float64), t.astype(np.float64), T)
    l32, g32 = t32(lambda a, b: O.loss_fn_kd(a, b, T), s, t)
    g = Guarded()
    d_s, d_t = g.inp(s, 0, "scores"), g.inp(t, 0, "target")
    d_l, d_ds, d_l2 = g.out((1,), torch.float32, 0, "loss"), g.out((n, cc), torch.float32, 0, "dscores"), g.out((1,), torch.float32, 0, "loss2")
    assert_path(lib, "kd", c)
    ok(lib, lib.ocl_kd_fwd_bwd(vp(d_s), vp(d_t), n, cc, T, vp(d_l), vp(d_ds), stream()), name)
    ok(lib, lib.ocl_kd_fwd_bwd(vp(d_s), vp(d_t), n, cc, T, vp(d_l2), None, stream()), name)
    g.check(name)
    assert d_l.cpu().numpy().tobytes() == d_l2.cpu().numpy().tobytes()
    cap = 1e-5 if (n, cc, c["scale"], T) == (10, 100, 1, 2.0) else None
    check_vs_torch32("kd/" + name, "loss", d_l.cpu().numpy(), np.array([ref_loss]), l32.reshape(1), cap)
    check_vs_torch32("kd/" + name, "grad", d_ds.cpu().numpy(), ref_grad, g32, cap)


@case_of("mir")
def test_mir_scores(lib, name):
    """post CE - pre CE per sample (mir_retrieve.py:26-28).  The score is small against the two losses; with the difference taken between two
    fp32-rounded losses the kernel missed this bound on n1_c5_s1 (error 2.401e-07, bound 2.384e-07, torch fp32 1.6e-09 on that single
    element); mir_kernel now combines the pieces of both losses in double (1.209e-07 on the same case)."""
    from oracle import ocl_oracle as O
    c = find("mir", name)
    if c.get("bad_labels"):
        return _labels_outside_case(lib, "mir", c)
    rng = np.random.default_rng(c["seed"])
    n, cc = c["n"], c["c"]
    pre, post = logits_for(rng, n, cc, c["scale"]), logits_for(rng, n, cc, c["scale"])
    y = rng.integers(0, cc, n).astype(np.int64)
    ref = ref_ce(post.astype(np.float64), y)[0] - ref_ce(pre.astype(np.float64), y)[0]
    r32 = O.mir_scores(torch.from_numpy(pre), torch.from_numpy(post), torch.from_numpy(y)).numpy()
    g = Guarded()
    d_a, d_b, d_y, d_o = g.inp(pre, 0, "pre"), g.inp(post, 0, "post"), g.inp(y, 0, "y"), g.out((n,), torch.float32, 0, "scores")
    assert_path(lib, "mir", c)
    ok(lib, lib.ocl_mir_scores(vp(d_a), vp(d_b), vp(d_y), n, cc, vp(d_o), stream()), name)
    g.check(name)
    check_vs_torch32("mir/" + name, "scores", d_o.cpu().numpy(), ref, r32)


# ==========================================================================================================================================
# Tier 2: SupCon
# ==========================================================================================================================================
def _supcon_inputs(c):
    rng = np.random.default_rng(c["seed"])
    bsz, nv, dim = c["bsz"], c["n_views"], c["dim"]
    f = rng.standard_normal((nv * bsz, dim)).astype(np.float32)
    f = (f / np.linalg.norm(f.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)       # L2-normalised, as in the product
    if nv == 1:
        y = (np.arange(bsz) % max(1, bsz // 2)).astype(np.int64)        # every label at least twice
        y = y[rng.permutation(bsz)]
    else:
        y = rng.integers(0, max(2, bsz // 4), bsz).astype(np.int64)
    return f, y


def _supcon_call(lib, g, d_f, d_y, c, want_grad, tag):
    A = c["bsz"] * c["n_views"]
    d_ws = g.out((lib.ocl_supcon_workspace_bytes(A) // 4,), torch.float32, 0, "workspace " + tag)
    d_l = g.out((1,), torch.float32, 0, "loss " + tag)
    d_df = g.out((A, c["dim"]), torch.float32, 0, "dfeat " + tag) if want_grad else None
    ok(lib, lib.ocl_supcon_fwd_bwd(vp(d_f), vp(d_y), c["bsz"], c["n_views"], c["dim"], c["T"], vp(d_l), vp(d_df), vp(d_ws), stream()), c["name"])
    return d_l, d_df


@case_of("supcon")
def test_supcon(lib, name):
    from oracle import ocl_oracle as O
    c = find("supcon", name)
    bsz, nv, dim, T = c["bsz"], c["n_views"], c["dim"], c["T"]
    A = bsz * nv
    assert lib.ocl_supcon_workspace_bytes(A) == (A * A + A + 64) * 4
    if c["path"] == "SUPCON_REFUSED":
        g = Guarded()
        d_f, d_y = g.inp(np.zeros((A, dim), dtype=np.float32), c["off"], "feat"), g.inp(np.zeros(bsz, dtype=np.int64), 0, "y")
        d_ws, d_l, d_df = g.out((1024,), torch.float32, 0, "workspace"), g.out((1,), torch.float32, 0, "loss"), g.out((A, dim), torch.float32, 0, "dfeat")
        assert assert_path(lib, "supcon", c, [d_f]).grid_x == 0      # refused on the host: nothing is launched on the small workspace
        assert lib.ocl_supcon_fwd_bwd(vp(d_f), vp(d_y), bsz, nv, dim, T, vp(d_l), vp(d_df), vp(d_ws), stream()) != 0
        assert b"too large" in lib.ocl_last_error()
        g.check(name)
        assert bool(Guarded.is_poison(d_l).all()) and bool(Guarded.is_poison(d_df).all())
        return
    f, y = _supcon_inputs(c)
    g = Guarded()
    d_f, d_y = g.inp(f, c["off"], "feat"), g.inp(y, 0, "y")
    loss_only = c.get("want") == "loss"
    assert_path(lib, "supcon", c, [d_f])
    d_l, d_df = _supcon_call(lib, g, d_f, d_y, c, not loss_only, "a")
    d_l2, d_df2 = _supcon_call(lib, g, d_f, d_y, c, loss_only, "b")      # the other of {full, loss only}
    g.check(name)
    assert d_l.cpu().numpy().tobytes() == d_l2.cpu().numpy().tobytes(), "%s: the loss-only call's loss differs from the full call's" % name
    ref_loss, ref_df = ref_supcon(f.astype(np.float64), y, bsz, nv, T)
    f_bvd = np.ascontiguousarray(f.reshape(nv, bsz, dim).transpose(1, 0, 2))
    l32, g32 = t32(lambda a, b: O.supcon_loss(a, b, T), f_bvd, y)
    g32 = np.ascontiguousarray(g32.transpose(1, 0, 2)).reshape(A, dim)
    cap = 1e-5 if (bsz, nv, dim, c["off"]) == (110, 2, 128, 0) else None
    check_vs_torch32("supcon/" + name, "loss", d_l.cpu().numpy(), np.array([ref_loss]), l32.reshape(1), cap)
    check_vs_torch32("supcon/" + name, "dfeat", (d_df if d_df is not None else d_df2).cpu().numpy(), ref_df, g32, cap)


def test_supcon_anchor_without_positive_is_nan_everywhere(lib):
    """n_views = 1 and a label that occurs once: the reference's loss is 0/0 = NaN and autograd makes EVERY element of the gradient NaN."""
    from oracle import ocl_oracle as O
    for bsz, dim, off, labels in [(5, 8, 0, [0, 0, 1, 1, 2]), (37, 6, 0, None), (220, 128, 1, None)]:
        rng = np.random.default_rng(bsz)
        c = dict(name="nopos%d" % bsz, bsz=bsz, n_views=1, dim=dim, T=0.07, off=off)
        f = rng.standard_normal((bsz, dim)).astype(np.float32)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        y = np.array(labels if labels else list(np.arange(bsz - 1) % 7) + [99], dtype=np.int64)
        ref_loss, ref_df = ref_supcon(f.astype(np.float64), y, bsz, 1, 0.07)
        assert np.isnan(ref_loss) and np.isnan(ref_df).all()
        l32, g32 = t32(lambda a, b: O.supcon_loss(a, b, 0.07), f.reshape(bsz, 1, dim), y)
        assert np.isnan(l32) and np.isnan(g32).all()          # the reference formula under autograd, fp32
        g = Guarded()
        d_f, d_y = g.inp(f, off, "feat"), g.inp(y, 0, "y")
        d_l, d_df = _supcon_call(lib, g, d_f, d_y, c, True, "full")
        d_l2, _ = _supcon_call(lib, g, d_f, d_y, c, False, "loss")
        g.check(c["name"])
        assert bool(torch.isnan(d_l).all()) and bool(torch.isnan(d_l2).all())
        nan = torch.isnan(d_df)
        assert bool(nan.all()), "bsz %d: %d of %d gradient elements are finite" % (bsz, int((~nan).sum()), nan.numel())


# ==========================================================================================================================================
# SCR augmentation: the image kernel and the parameter kernel against the float64 statement of their contract (tests/augment_ref.py)
# ==========================================================================================================================================
def _off3(c):
    return c["off"] if isinstance(c["off"], tuple) else (c["off"],) * 3


def _augment_refused(lib, c):
    """The plan refuses on the host: both entry points return an error before any launch, so the (small) sentinel-filled outputs stay
    as they were; through ops the error is a RuntimeError."""
    from ocl_amd import ffi, ops
    n, h, w = c["n"], c["h"], c["w"]
    real = n * h * w <= 1 << 20                      # the tensors can have the shape the call names (otherwise: one pixel; nothing is read)
    rows, hh, ww = (n, h, w) if real else (1, 1, 1)
    g = Guarded()
    d_x = g.inp(np.zeros((rows, 3, hh, ww), dtype=np.float32), 0, "x")
    d_p = g.inp(np.tile(np.array([0, 0, h, w, 0, 0, 1, 1, 1, 0, 0, 0], dtype=np.float32), (rows, 1)), 0, "params")
    d_u = g.inp(np.zeros((rows, AR.NUNIFORM), dtype=np.float32), 0, "u")
    d_o, d_par = g.out((rows, 3, hh, ww), torch.float32, 0, "out"), g.out((rows, AR.NPARAM), torch.float32, 0, "params out")
    cfg = [0.2, 1.0, 0.75, 4.0 / 3.0, 0.4, 0.4, 0.4, 0.1, 0.8, 0.2, float(w), float(h)]
    assert assert_path(lib, "augment", c).grid_x == 0
    rc = lib.ocl_scr_augment(vp(d_x), vp(d_o), n, h, w, vp(d_p), stream())
    assert rc != 0 and b"too large" in lib.ocl_last_error()
    with pytest.raises(RuntimeError):
        ffi.check(rc, "scr_augment")
    rc = lib.ocl_scr_augment_uniform(vp(d_x), vp(d_o), n, h, w, vp(d_u), (C.c_double * 12)(*cfg), vp(d_par), stream())
    assert rc != 0 and b"too large" in lib.ocl_last_error()
    if real:
        with pytest.raises(RuntimeError):
            ops.scr_augment(d_x, d_p)
        with pytest.raises(RuntimeError):
            ops.scr_augment_uniform(d_x, d_u, cfg, out=d_o)
    g.check(c["name"])
    assert bool(Guarded.is_poison(d_o).all()) and bool(Guarded.is_poison(d_par).all())


@case_of("augment")
def test_scr_augment_against_float64(lib, name):
    """ocl_scr_augment (and ops.scr_augment, bit-equal to it) against ref_augment in float64, every element, the edge ring included.
    Tolerance: 4 E, E the distance of the float32 restatement from float64 on the case's own inputs, at least 8 * 2^-24
    (augment_ref.augment_case_reference; nothing of it looks at the kernel).  Rows that only move pixels (full crop, no jitter, no gray) are
    the input, or its mirror image, bit for bit.  Rows past n -- of x, params and out -- are left alone."""
    from ocl_amd import ops
    c = find("augment", name)
    if c["path"] == "AUGMENT_REFUSED":
        return _augment_refused(lib, c)
    n, h, w = c["n"], c["h"], c["w"]
    off = _off3(c)
    x, P, r64, E, tol = AR.augment_case_reference(c)
    g = Guarded()
    d_x, d_p = g.inp(x, off[0], "x"), g.inp(P, off[1], "params")
    d_o = g.out(x.shape, torch.float32, off[2], "out")
    plan = assert_path(lib, "augment", c)
    assert (plan.grid_x, plan.grid_y, plan.block) == ((-(-h * w // 256), n, 256) if n else (0, 0, 0))
    ok(lib, lib.ocl_scr_augment(vp(d_x), vp(d_o), n, h, w, vp(d_p), stream()), name)
    g.check(name)
    got = d_o.cpu().numpy()
    assert Guarded.is_poison(got[n:]).all(), "%s: output rows past n written" % name
    if n == 0:
        return
    assert ops.scr_augment(d_x[:n], d_p[:n]).cpu().numpy().tobytes() == got[:n].tobytes()
    got = got[:n]
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    err = float(np.abs(got.astype(np.float64) - r64).max())
    AUG_REPORT.append(("augment/" + name, "%dx%d" % (h, w), n, E, tol, err))
    print("augment/%s: float32 restatement E %.4g, tolerance %.4g, device error %.4g" % (name, E, tol, err))
    exact = 0
    for i in range(n):
        if AR.flags_only(P[i], h, w):
            want = x[i][:, :, ::-1] if P[i, 4] > 0.5 else x[i]
            assert got[i].tobytes() == np.ascontiguousarray(want).tobytes(), "%s: row %d (flags only) is not its input bit for bit" % (name, i)
            exact += 1
    if c["kind"] == "geometry":
        assert exact == 2
    i = np.unravel_index(int(np.abs(got.astype(np.float64) - r64).argmax()), got.shape)
    assert err <= tol, "%s: error %.4g against float64 at image %d channel %d pixel (%d, %d) exceeds %.4g (float32 restatement: %.4g)" % ((name, err) + tuple(i) + (tol, E))


@case_of("aug_params")
def test_scr_augment_parameters_against_float64(lib, name):
    """ocl_scr_augment_uniform's parameter kernel against ref_aug_params: on the rows whose rounding decisions are all further than 2^-18
    relative (32 float32 ulp, far above what expf and sqrtf differ by) from a boundary the integers are equal and the jitter factors within 2
    float32 spacings (augment_ref.factor_ulps); every row's box lies inside the image.  The fused call's image is ocl_scr_augment on the
    parameters it returned, bit for bit; ops.scr_augment_uniform returns the same; the parameter rows past n are left alone."""
    from ocl_amd import ops
    c = find("aug_params", name)
    n, h, w = c["n"], c["h"], c["w"]
    cfg = AR.aug_params_config(c)
    u = AR.aug_params_case_inputs(c)
    x = np.random.default_rng(c["seed"] + 1000).random((n, 3, h, w)).astype(np.float32)
    g = Guarded()
    d_x, d_u = g.inp(x, 0, "x"), g.inp(u, 0, "u")
    d_o, d_par = g.out(x.shape, torch.float32, 0, "out"), g.out((n + 3, AR.NPARAM), torch.float32, 0, "params")
    plan = assert_path(lib, "aug_params", c)
    assert (plan.grid_x, plan.block) == (-(-n // 64), 64)
    ok(lib, lib.ocl_scr_augment_uniform(vp(d_x), vp(d_o), n, h, w, vp(d_u), (C.c_double * 12)(*cfg), vp(d_par), stream()), name)
    g.check(name)
    assert Guarded.is_poison(d_par[n:]).all(), "%s: parameter rows past n written" % name
    got = d_par.cpu().numpy().astype(np.float64)[:n]
    P, D = AR.ref_aug_params(u, cfg, h, w)
    rows = AR.comparable(D)
    assert (~rows).sum() <= 0.01 * n
    inside = AR.box_inside_image(got, h, w)
    assert inside.all(), "%s: rows %s: crop box outside the image, or a flag / order out of range" % (name, np.nonzero(~inside)[0][:8])
    ints = [0, 1, 2, 3, 4, 5, 10, 11]
    bad = np.nonzero((got[:, ints] != P[:, ints]).any(1) & rows)[0]
    assert len(bad) == 0, "%s: rows %s differ from float64: %s, reference %s" % (name, bad[:8], got[bad[:3]], P[bad[:3]])
    ferr = np.abs(got[rows][:, 6:10] - P[rows][:, 6:10]) / AR.factor_ulps(cfg)
    AUG_REPORT.append(("aug_params/" + name, "%dx%d" % (h, w), n, int(rows.sum()), 2.0, float(ferr.max())))
    print("aug_params/%s: %d of %d rows compared exactly, largest jitter-factor difference %.3g float32 spacings" % (name, rows.sum(), n, ferr.max()))
    assert ferr.max() <= 2.0
    assert torch.equal(ops.scr_augment(d_x, d_par[:n]), d_o), "%s: the fused call's image is not ocl_scr_augment on its own parameters" % name
    out2, par2 = ops.scr_augment_uniform(d_x, d_u, cfg, want_params=True)
    assert torch.equal(out2, d_o) and torch.equal(par2, d_par[:n])


def test_scr_augment_pieces_equal_the_concatenated_call(lib):
    """ScrAugment.apply_parts -- the call the agent makes: one draw, one launch pair per piece at its row offset into the draws (7 rows of
    30 floats: not 16-byte aligned) -- against the single-tensor call on the concatenation under the same seed, bit for bit."""
    from ocl_amd.agents.scr import ScrAugment
    rng = np.random.default_rng(77)
    a, b = (torch.from_numpy(rng.random((k, 3, 17, 23)).astype(np.float32)).cuda() for k in (7, 3))
    empty = torch.empty((0, 3, 17, 23), dtype=torch.float32, device=a.device)
    torch.manual_seed(3)
    parts = ScrAugment((17, 23))((a, b, empty))
    torch.manual_seed(3)
    whole = ScrAugment((17, 23))(torch.cat((a, b)))
    torch.cuda.synchronize()
    assert parts.shape == whole.shape == (10, 3, 17, 23)
    assert torch.equal(parts, whole)
    assert not torch.equal(whole, torch.cat((a, b)))


# the per-case tests of every op of the table (tests/test_cpu_small_ops.py checks their parametrisation against the table)
CASE_TESTS = {
    "augment": [test_scr_augment_against_float64], "aug_params": [test_scr_augment_parameters_against_float64],
    "rows": [test_gather_rows_is_exact, test_scatter_rows_is_exact_and_leaves_other_rows], "pair": [test_gather_pair_is_exact],
    "u8": [test_gather_u8_images_is_exact], "sgd": [test_sgd_is_exact_on_integers], "cosine": [test_cosine_max], "ce": [test_cross_entropy],
    "ce_seg": [test_cross_entropy_segmented], "kd": [test_kd_loss], "mir": [test_mir_scores], "supcon": [test_supcon],
    "knn": [test_knn_sv_on_integer_features], "col_reduce": [test_col_reduce], "aser": [test_aser_score], "argsort": [test_argsort_desc_order],
    "ncm_means": [test_ncm_class_means], "ncm_predict": [test_ncm_predict],
    "gemm": [test_gemm_small_is_exact_on_integers, test_gemm_small_random_within_fp32_bound],
}


# ==========================================================================================================================================
# the NaN leg: one case per distinct path code of the table
# ==========================================================================================================================================
def nan_leg_cases():
    """(op, case name): the first case of the table for every distinct `path` code."""
    seen, rows = set(), []
    for op, cases in SC.CASES.items():
        for c in cases:
            if c["path"] not in seen:
                seen.add(c["path"])
                rows.append((op, c["name"]))
    return rows


@pytest.mark.parametrize("op,name", nan_leg_cases(), ids=lambda v: v)
def test_nan_leg_equals_the_finite_leg(lib, op, name):
    """The case's tests once more with every output, workspace and guard region holding 0xFFFFFFFF (integer tensors: their minimum) instead
    of -7777 / 4096 (guarded.run_both_legs): the tests' own assertions hold, and every output is bit-identical in the two legs.  A kernel
    that reads what it has not written -- a workspace assumed zero, an element past a tensor's end times zero -- differs there."""
    from guarded import run_both_legs
    n0, n1 = len(REPORT), len(AUG_REPORT)
    try:
        for fn in CASE_TESTS[op]:
            run_both_legs(lambda: fn(lib, name), "%s/%s/%s" % (op, name, fn.__name__))
    finally:
        del REPORT[n0:], AUG_REPORT[n1:]       # (the parity report holds the module's own run of the case, once)


def test_the_nan_leg_sees_a_read_of_unwritten_memory(cuda):
    """guarded.run_both_legs on two stand-in "kernels": one that stores its output passes; one that forms 0 * (what the output held) + x
    -- right over -7777, NaN over 0xFFFFFFFF -- is reported, as is one that leaves a cell unwritten in one leg only."""
    from guarded import run_both_legs

    def body(kind):
        g = Guarded()
        x, o = g.inp(np.arange(8, dtype=np.float32), 3, "x"), g.out((8,), torch.float32, 1, "o")
        if kind == "stores":
            o.copy_(x)
        elif kind == "reads":
            o.mul_(0.0).add_(x)
        elif Guarded.LEG == "nan":
            o[:4].copy_(x[:4])
        g.check(kind)

    run_both_legs(lambda: body("stores"), "stores")
    for kind in ("reads", "one_leg"):
        with pytest.raises(AssertionError, match="differs between the legs"):
            run_both_legs(lambda: body(kind), kind)
