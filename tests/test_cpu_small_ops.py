"""CPU: the parity suite of the small kernels (tests/test_gpu_small_ops.py) covers what csrc/small_ops.hip can do.

* every __global__ kernel of the file and every path code ocl_test_small_op_path can return (the very functions the entry points launch
  from) is claimed by a case of tests/small_op_cases.py, and every case still reaches the path it claims;
* the GPU file parametrizes every case of the table, unsliced;
* the float64 reference functions of the GPU file reproduce the reference project's own fp32 results stored in tests/golden/ (so the
  references the kernels are judged against are themselves pinned)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import small_op_cases as SC
from conftest import ROOT, gold
import ocl_amd  # noqa: F401
from ocl_amd import ffi

PFX = "OCL" + "_PATH_"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return ffi.lib()


def header_paths():
    txt = open(os.path.join(ROOT, "include", "ocl_hip.h")).read()
    return {name: int(v) for name, v in re.findall(PFX + r"([A-Z0-9_]+)\s*=\s*(\d+)", txt)}


def path_of(lib, op, case, ptrs=None):
    args = SC.plan_args(op, case, ptrs)
    plan = ffi.SmallOpPlan()
    code = lib.ocl_test_small_op_path(SC.OPS[op][0], (ffi.i64 * len(args))(*args), len(args), C.byref(plan))
    assert code == plan.path
    return code, plan


def test_every_kernel_of_the_file_is_claimed():
    src = open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", "small_ops.hip")).read()
    kernels = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?(\w+)\s*\(", src))
    assert len(kernels) == 22, sorted(kernels)
    claimed = {k for op, (_, ks) in SC.OPS.items() if SC.CASES[op] for k in ks}
    assert kernels - claimed == set(SC.EXEMPT_KERNELS), sorted(kernels - claimed)
    assert claimed <= kernels, sorted(claimed - kernels)
    assert set(SC.OPS) == set(SC.CASES)


def test_every_path_code_is_claimed_and_every_case_reaches_its_path(lib):
    paths = header_paths()
    assert len(paths) >= 45 and len(set(paths.values())) == len(paths)
    # the plan functions return these constants only (the size / form variants of the cosine and SupCon paths by offset from the first,
    # pinned by static_asserts there): a new branch needs a new constant here, and a constant needs a case below
    src = open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", "small_ops.hip")).read()
    used = set(re.findall(PFX + r"([A-Z0-9_]+)", src))
    assert used <= set(paths) and set(paths) - used <= {n for n in paths if n.startswith(("COS_", "SUPCON_"))}, sorted(set(paths) ^ used)
    claimed = set()
    for op, cases in SC.CASES.items():
        names = [c["name"] for c in cases]
        assert len(names) == len(set(names)), op
        for c in cases:
            code, plan = path_of(lib, op, c)
            assert code == paths[c["path"]], "%s/%s (%s) takes path %d, not %s" % (op, c["name"], c["key"], code, c["path"])
            assert (plan.grid_x == 0) == (c["path"].endswith("REFUSED") or c.get("n") == 0 or c.get("ne") == 0), (op, c["name"])
            claimed.add(c["path"])
    assert set(paths) - claimed == set(), "path codes without a parity case: %s" % sorted(set(paths) - claimed)
    keys = [c["key"] for cases in SC.CASES.values() for c in cases]
    missing = [k for k in SC.REQUIRED_KEYS if not any(k in have for have in keys)]
    assert not missing, missing


def test_path_export_refuses_a_wrong_call(lib):
    a = (ffi.i64 * 3)(1, 2, 3)
    assert lib.ocl_test_small_op_path(99, a, 3, None) == 0
    assert lib.ocl_test_small_op_path(0, a, 3, None) == 0            # (ROWS takes four)
    assert lib.ocl_test_small_op_path(16, a, 3, None) == header_paths()["GEMM_KTAIL"]


def test_plans_are_what_the_header_documents(lib):
    """Grid, LDS and the padded power of two for a few sizes worked out by hand from the header's description."""
    def plan(op, **kw):
        c = dict(off=0)
        c.update(kw)
        return path_of(lib, op, c)[1]
    p = plan("supcon", bsz=110, n_views=2, dim=128)
    assert (p.grid_x, p.block, p.lds_bytes, p.grid2_x, p.block2, p.lds2_bytes) == (220, 256, (128 + 220 + 16) * 4, 220, 128, 220 * 4)
    p = plan("supcon", bsz=10, n_views=2, dim=128, want="loss")
    assert (p.grid_x, p.grid2_x, p.lds2_bytes) == (20, 1, 128 * 4)
    p = plan("knn", ne=7, nc=129, dim=160, k=3)
    assert (p.grid_x, p.aux, p.lds_bytes) == (7, 256, 256 * 16 + 640)
    p = plan("argsort", n=4096)
    assert (p.aux, p.lds_bytes) == (4096, 32768)
    p = plan("cosine", n=1155608, k=10, off=(0, 0))
    assert (p.grid_x, p.aux, p.grid2_x, p.block2) == (283, 283, 1, 64)
    p = plan("cosine", n=1 << 24, k=1, off=(0, 0))
    assert p.grid_x == 512
    p = plan("rows", row=21168, n=5, off=(0, 0))
    assert (p.grid_x, p.grid_y) == (5, 6)
    p = plan("sgd", n=1155608)
    assert p.grid_x == 1155608 // 4 // 256 + 2
    p = plan("gemm", m=220, n=160, k=160)
    assert (p.grid_x, p.grid_y, p.block) == (10, 14, 64)
    p = plan("ncm_predict", n=9, d=640, n_cls=100)
    assert (p.grid_x, p.lds_bytes) == (9, (640 + 100 + 16) * 4)


# the size of the table: a case that leaves it (or joins it) is a deliberate edit of this line too
CASE_COUNTS = {"rows": 9, "pair": 7, "u8": 5, "sgd": 8, "cosine": 13, "ce": 18, "ce_seg": 7, "kd": 7, "mir": 7, "supcon": 16, "knn": 11,
               "col_reduce": 7, "aser": 6, "argsort": 12, "ncm_means": 5, "ncm_predict": 7, "gemm": 56}


def test_no_case_left_the_table():
    assert {op: len(v) for op, v in SC.CASES.items()} == CASE_COUNTS


def _params(fn):
    return [m.args[1] for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"][0]


def test_the_gpu_file_runs_every_case():
    """Every case of the table is parametrized, unsliced, in its op's test of test_gpu_small_ops.py (listing a case is not enough)."""
    import test_gpu_small_ops as T
    assert set(T.CASE_TESTS) == set(SC.CASES)
    for op, fns in T.CASE_TESTS.items():
        assert fns, op
        for fn in fns:
            assert list(_params(fn)) == SC.ids(op), (op, fn.__name__)


# ---- the float64 references are pinned to the reference project's stored results -----------------------------------------------------------
# Bounds: the golden values are the reference's own fp32 arithmetic on these inputs; the float64 restatement differs from them by that
# arithmetic's round-off only.  A loss is a mean of n (<= 220) row values of magnitude L, each a log-sum-exp over c (<= 220) terms: its
# fp32 error is a few ulp of the largest intermediate (the logits, |x| / T <= 1 / 0.07 for unit features), bounded here by 4 ulp of
# max(|loss|, largest |logit|).  A gradient element is a difference of probabilities (<= 1) scaled by 1 / n or 1 / (A T): 4 ulp of the
# larger of the tensor's largest gradient magnitude and the scale factor (cancellation p - 1 at the label leaves an absolute, not a
# relative, error).  None of this looks at a kernel.
def _close(got, ref, scale, what):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
    assert err <= 4 * 2 * U * scale, "%s: fp64 restatement differs from the reference's stored result by %g (bound %g)" % (what, err, 8 * U * scale)


def test_float64_supcon_reproduces_the_reference_golden():
    import test_gpu_small_ops as T
    g = gold("supcon")
    for ci in range(int(g["n_cases"])):
        f, y, t = g["c%d_f" % ci], g["c%d_y" % ci], float(g["c%d_t" % ci])
        bsz, nv, dim = f.shape
        vm = np.ascontiguousarray(f.transpose(1, 0, 2)).reshape(nv * bsz, dim)
        loss, df = T.ref_supcon(vm.astype(np.float64), y, bsz, nv, t)
        df = df.reshape(nv, bsz, dim).transpose(1, 0, 2)
        _close(loss, g["c%d_loss" % ci], max(abs(loss), 1.0 / t), "supcon loss %d" % ci)
        _close(df, g["c%d_grad" % ci], max(np.abs(df).max(), 1.0 / (nv * bsz * t)), "supcon grad %d" % ci)


def test_float64_kd_reproduces_the_reference_golden():
    import test_gpu_small_ops as T
    g = gold("kd")
    for ci in range(int(g["n_cases"])):
        s, t, temp = g["c%d_s" % ci], g["c%d_t" % ci], float(g["c%d_T" % ci])
        loss, ds = T.ref_kd(s.astype(np.float64), t.astype(np.float64), temp)
        _close(loss, g["c%d_loss" % ci], max(abs(loss), np.abs(s).max() / temp) * temp * temp, "kd loss %d" % ci)
        _close(ds, g["c%d_grad" % ci], max(np.abs(ds).max(), temp / s.shape[0]), "kd grad %d" % ci)


def test_float64_cross_entropy_reproduces_the_reference_golden():
    """ce_tricks.npz: the labels trick (softmax over the labels present) and the separated softmax (old / new classes), both segment forms."""
    import test_gpu_small_ops as T
    g = gold("ce_tricks")
    for ci in range(int(g["n_cases"])):
        x, y = g["c%d_logits" % ci], g["c%d_y" % ci]
        c = x.shape[1]
        seg = np.full(c, -1, dtype=np.int64)
        if str(g["c%d_kind" % ci]) == "labels":
            seg[np.unique(y)] = 0
        else:
            seg[g["c%d_old" % ci]] = 0
            seg[g["c%d_new" % ci]] = 1
        loss, dx = T.ref_ce_seg(x.astype(np.float64), y, seg)
        _close(loss, g["c%d_loss" % ci], max(abs(loss), np.abs(x).max()), "ce loss %d" % ci)
        _close(dx, g["c%d_grad" % ci], max(np.abs(dx).max(), 1.0 / x.shape[0]), "ce grad %d" % ci)


def test_float64_knn_order_and_brute_force_reproduce_the_reference_golden():
    """The float64 stable distance order equals the reference's stored order wherever fp32 separates the distances, and the brute-force
    Shapley value (the definition) equals the reference's closed-form value on the small cases."""
    import test_gpu_small_ops as T
    from oracle import ocl_oracle as O
    g = gold("knn_sv")
    checked = 0
    for ci in range(int(g["n_cases"])):
        ef, cf, ey, cy, k = g["c%d_ef" % ci], g["c%d_cf" % ci], g["c%d_ey" % ci], g["c%d_cy" % ci], int(g["c%d_k" % ci])
        d64, order = T.ref_knn_order(ef, cf)
        gorder = g["c%d_order" % ci]
        for r, c in zip(*np.nonzero(order != gorder)):
            a, b = d64[r, order[r, c]], d64[r, gorder[r, c]]
            assert abs(a - b) <= 4 * ef.shape[1] * U * max(a, b), "case %d: float64 order differs from the stored one beyond fp32 round-off" % ci
        # (for k > n_cand the reference's closed form -- last factor 1 / N, aser_utils.py:46-49 -- is not the Shapley value of the 1 / k utility:
        # test_cpu_oracle_golden.py; the kernels follow the reference there, so the definition is only compared where k <= n_cand)
        if cf.shape[0] <= 12 and k <= cf.shape[0]:
            for r in range(ef.shape[0]):
                if not np.array_equal(order[r], gorder[r]):
                    continue
                bf = T.shapley_subsets(d64[r], cy == ey[r], k)
                assert np.abs(bf - g["c%d_sv" % ci][r]).max() <= cf.shape[0] * 2.0 ** -23, ci
                if cf.shape[0] <= 7:      # the permutation form of the definition (n! terms) agrees with the subset form
                    assert np.abs(bf - O.knn_shapley_bruteforce(d64[r], cy == ey[r], k)).max() <= 1e-12
                checked += 1
    assert checked >= 5
