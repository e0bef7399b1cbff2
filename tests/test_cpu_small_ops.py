"""CPU: the parity suite of the small kernels (tests/test_gpu_small_ops.py) covers what the small-op files of csrc/ can do (small_op_cases.SOURCES:
one file per kernel family, its launch plan, kernels and entry points side by side).

* every __global__ kernel of those files (each defined in one of them; the few that belong to another suite are named, with that suite)
  and every path code ocl_test_small_op_path can return (the very functions the entry points launch from) is claimed by a case of tests/small_op_cases.py, and every case still reaches the path it claims;
* the GPU file parametrizes every case of the table, unsliced;
* the float64 reference functions of the GPU file reproduce the reference project's own fp32 results stored in tests/golden/ (so the
  references the kernels are judged against are themselves pinned);
* the float64 statement of the SCR augmentation (tests/augment_ref.py) is pinned too -- its HSV pair to colorsys, its crop to bilinear
  interpolation, identity parameters to the input -- its cases tell every observable mutant of it from the reference by 100 times their
  tolerance, the 24 jitter orders apart wherever the contract does, and at most 1 % of a parameter case's rows sit on a rounding boundary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import augment_ref as AR
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


def sources():
    """file name -> text, of every file of SC.SOURCES."""
    return {f: open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", f)).read() for f in SC.SOURCES}


def test_every_kernel_of_the_file_is_claimed():
    found = [(k, f) for f, src in sources().items()
             for k in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\(", src)]
    # a kernel of these files belongs to the table or, by name, to another suite that exists: nothing is let off by the file it is in
    assert set(SC.OTHER_SUITES) <= {k for k, _ in found}, sorted(SC.OTHER_SUITES)
    for module in SC.OTHER_SUITES.values():
        assert os.path.exists(os.path.join(ROOT, "tests", module)), module
    table = [(k, f) for k, f in found if k not in SC.OTHER_SUITES]
    kernels = {k for k, _ in table}
    assert len(table) == len(kernels), "a kernel is defined in two files: %s" % sorted(table)
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
    used = {name for src in sources().values() for name in re.findall(PFX + r"([A-Z0-9_]+)", src)}
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
    p = plan("augment", n=20, h=84, w=84)                       # one thread per pixel in workgroups of 256, one grid row per image
    assert (p.grid_x, p.grid_y, p.block, p.lds_bytes) == (28, 20, 256, 0)
    p = plan("augment", n=65535, h=17, w=23)
    assert (p.grid_x, p.grid_y) == (2, 65535)
    assert plan("augment", n=65536, h=17, w=23).grid_x == 0 and plan("augment", n=1, h=46341, w=46341).grid_x == 0      # refused
    p = plan("augment", n=1, h=46340, w=46340)                  # the largest square whose pixel indices fit an int
    assert (p.grid_x, p.grid_y) == (-(-46340 * 46340 // 256), 1)
    p = plan("aug_params", n=110)                               # one thread per image in workgroups of 64
    assert (p.grid_x, p.grid_y, p.block) == (2, 1, 64)


# the size of the table: a case that leaves it (or joins it) is a deliberate edit of this line too
CASE_COUNTS = {"rows": 9, "pair": 7, "u8": 5, "sgd": 8, "cosine": 13, "ce": 20, "ce_seg": 8, "kd": 7, "mir": 8, "supcon": 16, "knn": 20,
               "col_reduce": 7, "aser": 6, "argsort": 12, "ncm_means": 5, "ncm_predict": 10, "gemm": 56, "augment": 16, "aug_params": 17}


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


# ---- the SCR augmentation: the float64 statement of the K13 contract (tests/augment_ref.py) is pinned, and the cases tell a wrong kernel ----
def _aug_cases(run_only=True):
    return [c for c in SC.CASES["augment"] if not (run_only and (c["kind"] == "refuse" or c["n"] == 0))]


def _aug_case(name):
    return [c for c in SC.CASES["augment"] if c["name"] == name][0]


def test_augment_reference_hsv_pair_is_colorsys():
    """rgb2hsv / hsv2rgb of the reference against the standard library, on the hand-picked pixels of the hsv_sectors case (which cover the
    three maximum-channel branches, the negative-hue wrap, the ties, gray, 0, 1) and, for the way back, at every hue shift of the case (which
    together reach the six sectors)."""
    import colorsys
    px = AR.hsv_sector_pixels().astype(np.float64)
    h, s, v = AR.rgb2hsv(px[:, 0], px[:, 1], px[:, 2])
    assert ((h >= 0) & (h < 1)).all()
    branches = set()
    for i, (r, g, b) in enumerate(px):
        assert np.abs(np.array(colorsys.rgb_to_hsv(r, g, b)) - np.array([h[i], s[i], v[i]])).max() <= 1e-12, (i, r, g, b)
        mx = max(r, g, b)
        branches.add("gray" if mx == min(r, g, b) else "r_wrap" if mx == r and g < b else "r" if mx == r else "g" if mx == g else "b")
    assert branches == {"gray", "r", "r_wrap", "g", "b"}
    sectors = set()
    for d in AR.HUE_SHIFTS:
        rgb = AR.hsv2rgb(h + d, s, v)
        for i in range(len(px)):
            hh = (h[i] + d) % 1.0
            assert np.abs(np.array(colorsys.hsv_to_rgb(hh, s[i], v[i])) - np.array([rgb[0][i], rgb[1][i], rgb[2][i]])).max() <= 1e-12, (d, i)
            if s[i] > 0 and v[i] > 0:
                sectors.add(int(hh * 6.0) % 6)
    assert sectors == set(range(6))


def test_augment_reference_crop_is_bilinear_interpolation():
    """The crop-and-resize of the reference against torch.nn.functional.interpolate(bilinear, align_corners=False) in float64, on integer
    crops, in the interior (output pixels whose two source rows and columns lie inside the box: at the box's edge interpolate clamps to the
    box, the contract to the image); flipped, against the mirrored interpolation."""
    import torch
    rng = np.random.default_rng(7)
    for h, w, (y0, x0, ch, cw) in [(32, 32, (8, 4, 16, 16)), (17, 23, (3, 5, 9, 14)), (84, 84, (10, 20, 33, 57)), (5, 7, (1, 2, 3, 4)), (17, 23, (0, 0, 17, 23))]:
        x = rng.random((1, 3, h, w))
        want = torch.nn.functional.interpolate(torch.from_numpy(x[:, :, y0:y0 + ch, x0:x0 + cw]), size=(h, w), mode="bilinear", align_corners=False).numpy()
        sy = (np.arange(h) + 0.5) * ch / h - 0.5
        sx = (np.arange(w) + 0.5) * cw / w - 0.5
        iy, ix = (sy >= 0) & (sy <= ch - 1), (sx >= 0) & (sx <= cw - 1)
        assert iy.sum() >= h // 2 and ix.sum() >= w // 2
        for flip in (0, 1):
            p = np.array([[y0, x0, ch, cw, flip, 0, 1, 1, 1, 0, 0, 0]], dtype=np.float32)
            got = AR.ref_augment(x, p, np.float64)
            exp = want[:, :, :, ::-1] if flip else want
            keep = ix[::-1] if flip else ix
            assert np.abs(got[:, :, iy][:, :, :, keep] - exp[:, :, iy][:, :, :, keep]).max() <= 1e-12, (h, w, flip)


def test_augment_reference_identity_and_flags_are_exact():
    """Identity parameters return the input, flip alone the mirrored input, bit for bit, in float64 and in the float32 restatement; a
    jitter of neutral factors is the identity to round-off in every order."""
    rng = np.random.default_rng(8)
    for h, w in [(5, 7), (17, 23), (84, 84)]:
        x = rng.random((2, 3, h, w)).astype(np.float32)
        ident = np.tile(np.array([0, 0, h, w, 0, 0, 1, 1, 1, 0, 0, 0], dtype=np.float32), (2, 1))
        flip = ident.copy()
        flip[:, 4] = 1
        for T in (np.float64, np.float32):
            assert np.array_equal(AR.ref_augment(x, ident, T), x.astype(T))
            assert np.array_equal(AR.ref_augment(x, flip, T), x.astype(T)[:, :, :, ::-1])
        for order in range(24):
            neutral = ident.copy()
            neutral[:, 5], neutral[:, 10] = 1, order
            assert np.abs(AR.ref_augment(x, neutral, np.float64) - x).max() <= 1e-12, order


# the case of the table that tells each mutant of tests/augment_ref.py from the reference (None: see the test)
MUTANT_CAUGHT_BY = {
    "order_decode_13": "orders_same_image", "hsv2rgb_sector3_qt": "hsv_sectors", "rgb2hsv_no_wrap": None, "clamp_to_crop": "geometry_5x7",
    "flip_after_coordinate": "geometry_17x23", "gray_before_jitter": "gray",
}


@pytest.mark.parametrize("mutant", sorted(AR.MUTANTS))
def test_augment_cases_catch_every_mutant(mutant):
    """A kernel carrying one of these errors would miss the named case by more than 100 times its tolerance.

    rgb2hsv_no_wrap is the exception, and not for want of a case: it is no error.  Without the wrap rgb2hsv returns a hue in (-1/6, 0) for
    the pixels whose maximum is red and g < b -- one full turn below the right one (asserted here, and it is what the colorsys pin above
    catches) -- and the only consumer of that hue, hsv2rgb, takes the fractional part first (it must: the hue shift may be any real
    number).  The image is the same: on every case of the table the mutant is within 1e-12 of the reference (largest difference 1.8e-15,
    orders_mixed), so no case can be asked to catch it, and `if (h < 0.f) h += 6.f` in the kernel is not observable through the entry point."""
    assert set(MUTANT_CAUGHT_BY) == set(AR.MUTANTS)
    name = MUTANT_CAUGHT_BY[mutant]
    if name is None:
        px = AR.hsv_sector_pixels().astype(np.float64)
        h, _, _ = AR.rgb2hsv(px[:, 0], px[:, 1], px[:, 2])
        hm, _, _ = AR.rgb2hsv(px[:, 0], px[:, 1], px[:, 2], wrap=False)
        neg = (px[:, 0] >= px[:, 1]) & (px[:, 0] >= px[:, 2]) & (px[:, 1] < px[:, 2])
        assert neg.sum() >= 5 and np.abs((h - hm)[neg] - 1.0).max() <= 1e-12 and np.array_equal(h[~neg], hm[~neg])
        for c in _aug_cases():
            x, P, r64, _, _ = AR.augment_case_reference(c)
            assert np.abs(AR.ref_augment(x[:c["n"]], P[:c["n"]], np.float64, mutant=mutant) - r64).max() <= 1e-12, c["name"]
        return
    c = _aug_case(name)
    x, P, r64, E, tol = AR.augment_case_reference(c)
    d = float(np.abs(AR.ref_augment(x[:c["n"]], P[:c["n"]], np.float64, mutant=mutant) - r64).max())
    print("%s: %s differs from the reference by %.3g on %s (tolerance %.3g)" % (mutant, AR.MUTANTS[mutant], d, name, tol))
    assert d > 100 * tol, (mutant, name, d, tol)


@pytest.mark.parametrize("name, classes", [("orders_same_image", 8), ("orders_same_image_clamped", 18)])
def test_augment_orders_of_one_image_are_pairwise_distinct(name, classes):
    """One image, identical parameters but the order index (brightness 1.3, saturation 1.35, hue 0.08; contrast 0.75, or 1.4).  Any two orders
    give images further apart than 100 times the case's tolerance, so a decode that took one for the other would show -- except where the
    contract itself gives two orders the same image, for every input (AR.same_image_orders: saturation and hue commute; a contrast <= 1
    never clamps and commutes with both).  Those pairs are asserted equal (within 1e-12) rather than distinct: with contrast 0.75 the 24
    orders are 8 distinct images (largest difference inside a class 6.7e-16), which is why the case has a twin whose contrast of 1.4
    reaches the clamp: 18 distinct images, the most the contract allows (the 6 pairs left differ by exchanging saturation and hue where one
    follows the other; a decode that confused those would compute the same thing for any parameters)."""
    c = _aug_case(name)
    x, P, r64, E, tol = AR.augment_case_reference(c)
    assert c["n"] == 24 and np.array_equal(P[:, 10], np.arange(24)) and (np.delete(P, 10, axis=1) == np.delete(P, 10, axis=1)[0]).all() and (x == x[0]).all()
    assert (c["h"] * c["w"]) % 256 != 0 and c["h"] * c["w"] > 256
    assert [float(v) for v in P[0, 5:10]] == [float(np.float32(v)) for v in (1, 1.3, c.get("contrast", 0.75), 1.35, 0.08)]
    cls = []                         # one representative per class of orders the contract cannot tell apart
    closest, inside = np.inf, 0.0
    for i in range(24):
        if not any(AR.same_image_orders(i, j, P[0, 7]) for j in cls):
            cls.append(i)
        for j in range(i):
            d = float(np.abs(r64[i] - r64[j]).max())
            if AR.same_image_orders(i, j, P[0, 7]):
                inside = max(inside, d)
                assert d <= 1e-12, (i, j, d)
            else:
                closest = min(closest, d)
                assert d > 100 * tol, "orders %d and %d are %.3g apart (tolerance %.3g)" % (i, j, d, tol)
    assert len(cls) == classes
    print("%s: %d distinct images; closest two %.3g apart, tolerance %.3g; largest difference inside a class %.3g" % (name, len(cls), closest, tol, inside))


def test_augment_case_tolerances_are_what_float32_costs():
    """The tolerance of every case is 4 E with E the float32 restatement's own distance from float64, floor 8 * 2^-24: between one and a few
    dozen float32 roundings of a value in [0, 1] at these sizes -- never wide enough to hide a wrong pixel."""
    for c in _aug_cases():
        x, P, r64, E, tol = AR.augment_case_reference(c)
        assert r64.shape == (c["n"], 3, c["h"], c["w"]) and r64.min() >= 0 and r64.max() <= 1
        assert tol == max(4 * E, 8 * U) and E > 0 and tol < 1e-4, (c["name"], E)
    geo = _aug_case("geometry_84x84")
    assert (geo["h"] * geo["w"]) % 256 != 0
    _, P, _, _, _ = AR.augment_case_reference(geo)
    assert (P[:, :4] != np.floor(P[:, :4])).any(1).sum() >= 4 and P[:, 4].sum() == len(P) // 2            # fractional boxes; half flipped


@pytest.mark.parametrize("name", SC.ids("aug_params"))
def test_aug_params_reference_and_its_exclusions(name):
    """ref_aug_params against the host statement (ScrAugment.params_from_uniform, torch fp32) on every row whose rounding decisions are all
    further than 2^-18 relative from their boundaries: integers equal, jitter factors within 2 float32 spacings.  At most 1 % of a case's
    rows are excluded (a condition on the seeds, met by the reference alone).  Every row's box lies inside the image."""
    import torch
    from ocl_amd.agents.scr import ScrAugment
    c = [c for c in SC.CASES["aug_params"] if c["name"] == name][0]
    cfg = AR.aug_params_config(c)
    aug = ScrAugment((c["h"], c["w"]), scale=c["scale"])
    assert [float(v) for v in aug.config()] == cfg
    u = AR.aug_params_case_inputs(c)
    assert u.shape == (c["n"], AR.NUNIFORM) and u.min() >= 0 and u.max() <= 1 - U
    P, D = AR.ref_aug_params(u, cfg, c["h"], c["w"])
    ok = AR.comparable(D)
    assert (~ok).sum() <= 0.01 * c["n"], "%d of %d rows on a rounding boundary" % ((~ok).sum(), c["n"])
    assert AR.box_inside_image(P, c["h"], c["w"]).all()
    host = aug.params_from_uniform(torch.from_numpy(u)).numpy().astype(np.float64)
    assert AR.box_inside_image(host, c["h"], c["w"]).all()
    ints = [0, 1, 2, 3, 4, 5, 10, 11]
    assert np.array_equal(host[ok][:, ints], P[ok][:, ints])
    assert (np.abs(host[ok][:, 6:10] - P[ok][:, 6:10]) <= 2 * AR.factor_ulps(cfg)).all()
    if c["h"] != c["w"]:                      # no attempt fits: the fallback crop, ratio clamped to 4/3 (wide) or 3/4 (tall)
        assert (P[:, 2:4] == ([16, 21] if c["w"] > c["h"] else [21, 16])).all() and not np.isfinite(D[:, 60:62]).any()
    if c.get("special") == "extremes":
        assert (u[0] == 0).all() and (u[1] == np.float32(1 - U)).all() and (u[2, 20:] == 0).all() and (u[3, 20:] == np.float32(1 - U)).all()
        assert ok[0] and ok[2] and P[0, 10] == 0 and P[3, 10] == 23 and P[2, 0] == 0 and P[3, 0] + P[3, 2] == c["h"]


# ---- kNN-Shapley: the sort's total order replayed on the host, and the conditions of the non-finite and the real-valued cases ----------------
def _replay(lib, keys):
    """ocl_test_knn_order on every row of keys [m, n]: the kernel's padding, network and comparator, run on the host."""
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    m, n = keys.shape
    out = np.full((m, n), -1, dtype=np.int64)
    pk, po = keys.ctypes.data, out.ctypes.data
    for i in range(m):
        assert lib.ocl_test_knn_order(pk + 4 * n * i, n, po + 8 * n * i) == 0
    return out


def _torch_stable(keys):
    import torch
    return torch.argsort(torch.from_numpy(np.ascontiguousarray(keys, dtype=np.float32)), dim=1, stable=True).numpy()


def _assert_order(lib, keys, what):
    got, exp = _replay(lib, keys), _torch_stable(keys)
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.size == 0, "%s: %d of %d vectors are not in the stable order; first: keys %s give %s, not %s" % (
        what, bad.size, len(keys), keys[bad[0]].tolist(), got[bad[0]].tolist(), exp[bad[0]].tolist())


def test_knn_order_replay_is_the_stable_argsort_exhaustively(lib):
    """Every key vector of length 1 to 8 over {0, 1, +inf, -inf, NaN} (488280 vectors; lengths 3, 5, 6, 7 are padded, with +inf keys that tie
    with the padding's): the kernel's network with its comparator returns torch.argsort(keys, stable=True) -- numbers ascending with ties by
    index, then the NaNs by index, the padding never among the first n.  (With the earlier comparator, under which NaN compares false both ways,
    the smallest failure was n = 3: [0.0027, 0.857, NaN] -> [0, 1, 2147483647].)"""
    alphabet = np.array([0.0, 1.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    for n in range(1, 9):
        digits = (np.arange(5 ** n)[:, None] // 5 ** np.arange(n)[None, :]) % 5
        _assert_order(lib, alphabet[digits], "alphabet vectors of length %d" % n)


@pytest.mark.parametrize("n", [3, 5, 33, 100, 150, 257, 2047, 2048])
def test_knn_order_replay_on_random_keys(lib, n):
    """Seeded random keys (distinct normals, or few distinct values: ties; some with +-inf) with no NaN, one NaN, many NaNs (up to a third, and
    all but one) and the all-NaN vector, at the sizes ASER draws (100, 150), just past a power of two, and at and just under the cap."""
    rng = np.random.default_rng(1000 + n)
    rows = []
    for rep in range(24 if n <= 257 else 6):
        v = rng.standard_normal(n).astype(np.float32) ** 2
        if rep % 3 == 1:
            v = rng.integers(0, 4, n).astype(np.float32)
        if rep % 3 == 2:
            v[rng.integers(0, n, max(1, n // 8))] = np.inf
            v[rng.integers(0, n, max(1, n // 16))] = -np.inf
        for nans in (0, 1, max(2, n // 3), n - 1, n):
            w = v.copy()
            w[rng.permutation(n)[:nans]] = np.nan
            assert int(np.isnan(w).sum()) == min(nans, n)
            rows.append(w)
    _assert_order(lib, np.stack(rows), "random keys, n = %d" % n)


def test_knn_order_replay_refuses_a_wrong_call(lib):
    k = np.zeros(4, dtype=np.float32)
    o = np.zeros(4, dtype=np.int64)
    assert lib.ocl_test_knn_order(k.ctypes.data, 0, o.ctypes.data) != 0
    assert lib.ocl_test_knn_order(k.ctypes.data, 2049, o.ctypes.data) != 0
    assert lib.ocl_test_knn_order(None, 4, o.ctypes.data) != 0 and lib.ocl_test_knn_order(k.ctypes.data, 4, None) != 0


def _knn_cases(**kw):
    return [c for c in SC.CASES["knn"] if all(c.get(k) == v for k, v in kw.items())]


def test_knn_nonfinite_cases_have_a_determined_order(lib):
    """The five non-finite cases: every key is an exact integer, +inf or NaN; row 0 has a NaN key and a +inf key among finite ones, row 1 only
    +inf and NaN keys, row 2 only NaN keys; and the host replay of the kernel's sort puts the float32 keys in the stable order the GPU test
    expects of the kernel (this runs before any of these cases is sent to a device)."""
    import knn_ref as KR
    cases = _knn_cases(special="nonfinite")
    assert sorted((c["nc"], c["dim"], c["path"]) for c in cases) == [(3, 4, "KNN_VEC_REM"), (4, 8, "KNN_VEC_REM"), (5, 6, "KNN_WAVE"),
                                                                       (9, 20, "KNN_VEC_BOTH"), (129, 16, "KNN_VEC_UNROLL")]
    for c in cases:
        ef, ey, cf, cy = KR.nonfinite_inputs(c)
        d = KR.keys64(ef, cf)
        fin = np.isfinite(d)
        assert (d[fin] == np.floor(d[fin])).all() and d[fin].max() < 2 ** 24
        n_nan = 1 if c["nc"] < 9 else 2
        assert np.isnan(d[0]).sum() == n_nan and np.isinf(d[0]).sum() == n_nan and fin[0].sum() == c["nc"] - 2 * n_nan
        assert np.isnan(d[1]).sum() == 2 * n_nan and np.isinf(d[1]).sum() == c["nc"] - 2 * n_nan
        assert np.isnan(d[2]).all()
        order = KR.stable_order(d)
        assert np.array_equal(order[2], np.arange(c["nc"]))
        for r in range(3):      # K10 in words: numbers ascending (+inf one of them), then the NaNs; ties by index
            assert order[r].tolist() == sorted(range(c["nc"]), key=lambda j: (bool(np.isnan(d[r, j])), 0.0 if np.isnan(d[r, j]) else d[r, j], j))
        with np.errstate(invalid="ignore", over="ignore"):
            k32 = d.astype(np.float32)
        assert np.array_equal(_replay(lib, k32), order), c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES["knn"] if c.get("data") == "real"])
def test_knn_real_cases_test_the_order_and_not_the_tolerance(name):
    """Per kind of data, from the reference alone: a float32 restatement of the case's distance path, in the kernel's order of operations, gives
    an order whose adjacent pairs float64 orders the other way are all inside 1.01 K 2^-24 (d_a + d_b) (knn_ref.path_k: the bound is what the
    arithmetic costs), and they are at most 5 % of the adjacent pairs (else the case would test the tolerance); the planted near ties are one
    to four float32 ulps apart and the clustered data is as ill-conditioned as it claims."""
    import knn_ref as KR
    c = [c for c in SC.CASES["knn"] if c["name"] == name][0]
    K = KR.path_k(c["path"], c["dim"])
    assert K == {"real_d12": 7, "real_d70": 10, "real_d36": 13, "real_d160": 44}[name]
    for kind in KR.KINDS:
        ef, ey, cf, cy = KR.real_inputs(c, kind)
        assert ef.dtype == cf.dtype == np.float32 and ef.shape == (c["ne"], c["dim"]) and cf.shape == (c["nc"], c["dim"])
        d64 = KR.keys64(ef, cf)
        k32 = KR.restate32(c["path"], ef, cf)
        assert k32.dtype == np.float32 and np.abs(k32 - d64).max() <= (1.01 * K * U * d64).max()
        n_inv, n_pairs, gap, bound = KR.inverted_pairs(np.argsort(k32, axis=1, kind="stable"), d64, K)
        print("%s/%s: K = %d, %d of %d adjacent pairs inverted, worst gap %.3g against %.3g" % (name, kind, K, n_inv, n_pairs, gap, bound))
        assert gap <= bound, (name, kind, gap, bound)
        assert n_inv <= 0.05 * n_pairs, (name, kind, n_inv, n_pairs)
        if kind == "near_tie":
            ulps = KR.near_tie_ulps(c, ef, cf)
            assert len(ulps) == c["pairs"] >= 1 and all(1.0 <= u <= 4.0 for u in ulps), ulps
        if kind == "clustered":
            assert d64.max() < 1e-4 * c["dim"] and (ef.astype(np.float64) ** 2).sum(1).min() > 9e3 * c["dim"]
