"""The parity cases of the small kernels (one file of csrc/ per family, SOURCES below: gather / scatter, SGD, cosine-max, cross-entropy and its
relatives, SupCon, kNN-Shapley, column reductions, argsort, NCM, the small MFMA GEMM, the SCR augmentation), shared by tests/test_cpu_small_ops.py (every kernel and every path
code of ocl_test_small_op_path is claimed by a case that still reaches it; no GPU) and tests/test_gpu_small_ops.py (runs every case).

Plain data.  A case is a dict:
  name   unique within its op (the pytest id)
  key    the path key it is there for: "<op>:<what>", free text for people and for REQUIRED_KEYS
  path   the path code (include/ocl_hip.h, without its prefix) the entry point must take with the case's sizes and base offsets
  off    base-pointer offset(s) in ELEMENTS from a 16-byte aligned address (0, or an odd count to break 16-byte alignment)
  seed   of the case's random generator
  ...    the op's sizes
`plan_args(op, case, ...)` turns a case into the argument vector of ocl_test_small_op_path."""

ALIGNED = 1 << 20          # a 16-byte aligned stand-in address for the CPU test (the export looks at alignment only)

# the files of csrc/ that hold the kernels of OPS, each family's launch plan, kernels and entry points side by side
SOURCES = ["buffer_rows.hip", "loader.hip", "optim.hip", "cosine.hip", "row_losses.hip", "supcon.hip", "aser.hip", "ncm.hip", "augment.hip",
           "gemm_small.hip"]
# the other __global__ kernels of those files -> the test module whose cases run them
OTHER_SUITES = {
    "adam_flat_kernel": "test_gpu_adam.py",
    "gather_f32_hwc_f32_chw_kernel": "test_gpu_datasets.py",
    "gather_f32_hwc_f32_chw_scalar_kernel": "test_gpu_datasets.py",
}

# op name -> (op code of include/ocl_hip.h, the __global__ kernels of SOURCES its cases run)
OPS = {
    "rows": (0, ["rows_copy16", "rows_copy4"]),
    "pair": (1, ["rows_gather_pair"]),
    "u8": (2, ["gather_u8_hwc_f32_chw"]),
    "sgd": (3, ["sgd_flat"]),
    "cosine": (4, ["cosine_partial_kernel", "cosine_finish_kernel"]),
    "ce": (5, ["ce_kernel"]),
    "ce_seg": (6, ["ce_seg_kernel"]),
    "kd": (7, ["kd_kernel"]),
    "mir": (8, ["mir_kernel"]),
    "supcon": (9, ["supcon_rows", "supcon_grad"]),
    "knn": (10, ["knn_sv_kernel"]),
    "col_reduce": (11, ["col_reduce_kernel"]),
    "aser": (12, ["aser_score_kernel"]),
    "argsort": (13, ["argsort_desc_kernel"]),
    "ncm_means": (14, ["ncm_means_kernel"]),
    "ncm_predict": (15, ["ncm_predict_kernel"]),
    "gemm": (16, ["gemm_small_kernel"]),
    "augment": (17, ["augment_kernel"]),
    "aug_params": (18, ["aug_params_kernel"]),
}
# no kernel of the file is exempt.  (kornia's random DRAWS stay unpinned; what the two augmentation kernels do with
# given draws / parameters is their own contract, include/ocl_hip.h K13, stated in float64 by tests/augment_ref.py)
EXEMPT_KERNELS = []


def bad_labels(n, c):
    """(row, label) of a bad_labels case: c, c + 5 and -1 in the first, a middle and the last row."""
    return [(0, c), (n // 2, c + 5), (n - 1, -1)]


def _c(name, key, path, seed, **kw):
    d = dict(name=name, key=key, path=path, seed=seed, off=0)
    d.update(kw)
    return d


# ---- gather / scatter: rows of `row` float32 out of R, n indices; off = (source, destination) ---------------------------------------
ROWS = [
    _c("cifar", "rows:copy16", "ROWS_COPY16", 1, R=50, n=20, row=3072, off=(0, 0), idx="rand"),
    _c("mini84_y6", "rows:copy16_grid_y", "ROWS_COPY16", 2, R=9, n=5, row=21168, off=(0, 0), idx="rand"),
    _c("repeat", "rows:repeated_indices", "ROWS_COPY16", 3, R=7, n=33, row=8, off=(0, 0), idx="repeat"),
    _c("ycap16", "rows:copy16_ycap", "ROWS_COPY16_YCAP", 4, R=6, n=4, row=32772, off=(0, 0), idx="rand"),
    _c("row12", "rows:copy4_rowsize", "ROWS_COPY4", 5, R=40, n=17, row=3, off=(0, 0), idx="rand"),
    _c("src_mis", "rows:copy4_misaligned", "ROWS_COPY4", 6, R=40, n=17, row=8, off=(1, 0), idx="rand"),
    _c("dst_mis", "rows:copy4_misaligned_dst", "ROWS_COPY4", 7, R=12, n=12, row=3072, off=(0, 3), idx="rand"),
    _c("ycap4", "rows:copy4_ycap", "ROWS_COPY4_YCAP", 8, R=5, n=3, row=7173, off=(0, 0), idx="rand"),
    _c("n0", "rows:n0", "ROWS_COPY16", 9, R=5, n=0, row=8, off=(0, 0), idx="rand"),
]
# ---- pair gather: a rows of `row_a` float32, b rows of `row_b` 4-byte units, index vector on the host or the device; off: a's source --
PAIR = [
    _c("host_idx", "pair:host_index", "PAIR_FUSED", 11, R=60, n=20, row_a=3072, row_b=2, off=0, idx="host"),
    _c("dev_idx", "pair:device_index", "PAIR_FUSED", 12, R=60, n=20, row_a=3072, row_b=2, off=0, idx="dev"),
    _c("mini84", "pair:grid_y", "PAIR_FUSED", 13, R=9, n=6, row_a=21168, row_b=2, off=0, idx="host"),
    _c("b300", "pair:units_b>256", "PAIR_FUSED_BLOOP", 14, R=20, n=9, row_a=64, row_b=300, off=0, idx="dev"),
    _c("mis", "pair:fallback", "PAIR_FALLBACK", 15, R=30, n=11, row_a=3072, row_b=2, off=1, idx="host"),
    _c("row24", "pair:fallback_rowsize", "PAIR_FALLBACK", 16, R=30, n=11, row_a=6, row_b=1, off=0, idx="dev"),
    _c("n0", "pair:n0", "PAIR_FUSED", 17, R=5, n=0, row_a=8, row_b=2, off=0, idx="host"),
]
U8 = [
    _c("cifar", "u8:one_block", "U8_GATHER", 21, R=20, n=7, h=32, w=32, c=3),
    _c("mini84", "u8:grid_y", "U8_GATHER", 22, R=6, n=3, h=84, w=84, c=3),
    _c("y16", "u8:grid_y_cap", "U8_GATHER", 23, R=3, n=2, h=128, w=128, c=3),
    _c("odd", "u8:odd_base", "U8_GATHER", 24, R=4, n=5, h=5, w=7, c=1, off=1),
    _c("n0", "u8:n0", "U8_GATHER", 25, R=4, n=0, h=5, w=7, c=1),
]
# ---- SGD: in place and with `out`; off: the parameter pointer ------------------------------------------------------------------------
SGD = [_c("n%d" % n, "sgd:n=%d" % n, path, 30 + i, n=n)
       for i, (n, path) in enumerate([(1, "SGD_TAIL"), (3, "SGD_TAIL"), (4, "SGD_VEC"), (5, "SGD_TAIL"), (1003, "SGD_TAIL"),
                                      (1155608, "SGD_VEC"), (2048 * 256 * 4 + 1029, "SGD_GRID_CAP")])] + \
      [_c("misaligned", "sgd:refuse_misaligned", "SGD_REFUSED", 39, n=1003, off=1)]
# ---- cosine-max: k rows of n; off = (mem, g); special: zero_row / zero_g / max_last ---------------------------------------------------
COSINE = [
    _c("n1", "cosine:n<4", "COS_SCALAR_ONE", 41, n=1, k=1, off=(0, 0)),
    _c("n3_k10", "cosine:scalar", "COS_SCALAR_ONE", 42, n=3, k=10, off=(0, 0)),
    _c("n4", "cosine:vec", "COS_VEC_ONE", 43, n=4, k=1, off=(0, 0)),
    _c("n1003_k65", "cosine:k>64", "COS_SCALAR_ONE", 44, n=1003, k=65, off=(0, 0)),
    _c("n8192_k130", "cosine:k>128", "COS_VEC_MULTI", 45, n=8192, k=130, off=(0, 0)),
    _c("params_k10", "cosine:vec_multi", "COS_VEC_MULTI", 46, n=1155608, k=10, off=(0, 0)),
    _c("params_mis_mem", "cosine:scalar_misaligned_mem", "COS_SCALAR_MULTI", 47, n=1155608, k=2, off=(1, 0)),
    _c("g_mis", "cosine:scalar_misaligned_g", "COS_SCALAR_ONE", 48, n=1000, k=3, off=(0, 1)),
    _c("cap_scalar", "cosine:blocks_cap", "COS_SCALAR_CAP", 49, n=2097152 + 4096 + 1, k=1, off=(0, 0)),
    _c("cap_vec", "cosine:blocks_cap_vec", "COS_VEC_CAP", 50, n=2097152 + 4096, k=2, off=(0, 0)),
    _c("zero_row", "cosine:eps_zero_row", "COS_VEC_ONE", 51, n=1000, k=3, off=(0, 0), special="zero_row"),
    _c("zero_g", "cosine:eps_zero_g", "COS_VEC_ONE", 52, n=1000, k=3, off=(0, 0), special="zero_g"),
    _c("max_last", "cosine:max_in_last_row", "COS_SCALAR_MULTI", 53, n=5001, k=66, off=(0, 0), special="max_last"),
]
# ---- cross-entropy family: n rows of c logits times `scale`; the last two rows are one dominant logit and all-equal logits ---------------
_CE_SHAPES = [(1, 5, 1), (3, 10, 30), (4, 64, 1), (5, 100, 300), (10, 100, 1), (10, 128, 30), (37, 200, 1), (7, 1000, 300), (64, 63, 1)]
CE = [_c("%s_n%d_c%d_s%d" % (red, n, c, s), "ce:%s n=%d c=%d scale=%d" % (red, n, c, s), "CE_" + red.upper(), 60 + i, n=n, c=c, scale=s, red=red)
      for i, (n, c, s) in enumerate(_CE_SHAPES) for red in ("mean", "none")] + \
     [_c("%s_label_outside" % red, "ce:label_outside %s" % red, "CE_" + red.upper(), 70 + i, n=7, c=70, scale=1, red=red, bad_labels=True)
      for i, red in enumerate(("mean", "none"))]
# bad_labels: the labels of the first, a middle and the last row are c, c + 5 and -1 (bad_labels()): outside the row, inside the test's guard regions
# seg: number of segments; a quarter of the columns (random positions) are -1
CE_SEG = [_c("n%d_c%d_s%d_g%d" % (n, c, s, g), "ce_seg: n=%d c=%d scale=%d segments=%d" % (n, c, s, g), "CE_SEG", 80 + i, n=n, c=c, scale=s, seg=g)
          for i, (n, c, s, g) in enumerate([(1, 5, 1, 1), (3, 10, 30, 2), (4, 64, 1, 2), (10, 100, 300, 3), (37, 200, 1, 2), (7, 1000, 30, 4), (10, 128, 1, 1)])] + \
         [_c("label_outside", "ce_seg:label_outside", "CE_SEG", 88, n=7, c=70, scale=1, seg=2, bad_labels=True)]
KD = [_c("n%d_c%d_s%d_T%g" % (n, c, s, T), "kd: n=%d c=%d scale=%d T=%g" % (n, c, s, T), "KD", 90 + i, n=n, c=c, scale=s, T=T)
      for i, (n, c, s, T) in enumerate([(1, 5, 1, 2.0), (3, 10, 30, 1.0), (4, 64, 1, 4.0), (10, 100, 300, 2.0), (37, 200, 1, 0.5), (7, 1000, 30, 3.0), (10, 128, 1, 2.0)])]
MIR = [_c("n%d_c%d_s%d" % (n, c, s), "mir: n=%d c=%d scale=%d" % (n, c, s), "MIR", 100 + i, n=n, c=c, scale=s)
       for i, (n, c, s) in enumerate([(1, 5, 1), (3, 10, 30), (4, 64, 1), (50, 100, 300), (37, 200, 1), (7, 1000, 30), (9, 128, 1)])] + \
      [_c("label_outside", "mir:label_outside", "MIR", 108, n=7, c=70, scale=1, bad_labels=True)]
# ---- SupCon: view-major features [n_views * bsz, dim]; off: the feature pointer; want: full (gradient) or loss only ------------------
SUPCON = [
    _c("A4_d4", "supcon/rows:vec A=4", "SUPCON_VEC_TAIL", 111, bsz=2, n_views=2, dim=4, T=0.07),
    _c("A16_d6", "supcon/rows:scalar supcon/grad:no_tail A<128", "SUPCON_SCALAR_NOTAIL", 112, bsz=8, n_views=2, dim=6, T=0.07),
    _c("A100_d128", "supcon/grad:tail A<128", "SUPCON_VEC_TAIL", 113, bsz=50, n_views=2, dim=128, T=0.5),
    _c("A128_d130", "supcon/rows:scalar dim%4!=0 A=128", "SUPCON_SCALAR_NOTAIL", 114, bsz=64, n_views=2, dim=130, T=0.07),
    _c("A220_d128", "supcon:product_shape", "SUPCON_VEC_TAIL", 115, bsz=110, n_views=2, dim=128, T=0.07),
    _c("A220_d128_mis", "supcon/rows:scalar misaligned", "SUPCON_SCALAR_TAIL", 116, bsz=110, n_views=2, dim=128, T=0.07, off=1),
    _c("A256_d640", "supcon/grad:no_tail A>220 dim=640", "SUPCON_VEC_NOTAIL", 117, bsz=128, n_views=2, dim=640, T=0.5),
    _c("A2048_v1", "supcon:n_views=1 A=2048", "SUPCON_VEC_NOTAIL", 118, bsz=2048, n_views=1, dim=128, T=0.07),
    _c("A120_v3", "supcon:n_views=3", "SUPCON_VEC_TAIL", 119, bsz=40, n_views=3, dim=128, T=0.07),
    _c("A100_v1_d6", "supcon:n_views=1 scalar", "SUPCON_SCALAR_TAIL", 120, bsz=100, n_views=1, dim=6, T=0.5),
    _c("loss_only_vec", "supcon/grad:loss_only", "SUPCON_VEC_LOSS", 121, bsz=110, n_views=2, dim=128, T=0.07, want="loss"),
    _c("loss_only_scalar", "supcon/grad:loss_only scalar", "SUPCON_SCALAR_LOSS", 122, bsz=30, n_views=3, dim=130, T=0.5, want="loss"),
    _c("cap_A8192", "supcon:cap_A", "SUPCON_VEC_NOTAIL", 123, bsz=8192, n_views=1, dim=8, T=0.5),
    _c("cap_d4096", "supcon:cap_dim", "SUPCON_VEC_TAIL", 124, bsz=4, n_views=2, dim=4096, T=0.07),
    _c("refuse_A8193", "supcon:refuse_A", "SUPCON_REFUSED", 125, bsz=8193, n_views=1, dim=8, T=0.5),
    _c("refuse_d4097", "supcon:refuse_dim", "SUPCON_REFUSED", 126, bsz=4, n_views=2, dim=4097, T=0.07),
]
# ---- kNN-Shapley: integer-valued features; off: the candidate features -------------------------------------------------------------------
KNN = [
    _c("d20", "knn:vec_both d4n=5", "KNN_VEC_BOTH", 131, ne=3, nc=9, dim=20, k=3),
    _c("d24", "knn:vec_both d4n=6", "KNN_VEC_BOTH", 132, ne=5, nc=100, dim=24, k=3),
    _c("d28", "knn:vec_both d4n=7", "KNN_VEC_BOTH", 133, ne=4, nc=33, dim=28, k=5),
    _c("d16", "knn:vec_unroll", "KNN_VEC_UNROLL", 134, ne=6, nc=129, dim=16, k=7),
    _c("d160_full", "knn:vec_unroll n_cand=2048", "KNN_VEC_UNROLL", 135, ne=3, nc=2048, dim=160, k=3),
    _c("d8", "knn:vec_rem", "KNN_VEC_REM", 136, ne=2, nc=12, dim=8, k=2),
    _c("d6", "knn:wave dim%4!=0 k>=n_cand", "KNN_WAVE", 137, ne=2, nc=5, dim=6, k=7),
    _c("d16_mis", "knn:wave misaligned", "KNN_WAVE", 138, ne=5, nc=65, dim=16, k=3, off=1),
    _c("k_ge_n", "knn:k>=n_cand larger", "KNN_VEC_BOTH", 139, ne=3, nc=257, dim=20, k=300),
    _c("nc1", "knn:n_cand=1", "KNN_VEC_REM", 140, ne=2, nc=1, dim=4, k=3),
    _c("refuse", "knn:refuse_n_cand", "KNN_REFUSED", 141, ne=1, nc=2049, dim=8, k=3),
    # special="nonfinite": integer-valued features with a NaN in one candidate row, +inf in another candidate (its key +inf ties with the
    # padding's key), and per evaluation row: 0 plain, 1 +inf in that candidate's dimension (inf - inf: its key is NaN, every other +inf),
    # 2 a NaN (every key NaN: the index order).  The keys are exact, +inf or NaN, so the order is fully determined (K10's total order)
    _c("nf_d4_p4", "knn:nonfinite vec_rem n_cand=3 P=4", "KNN_VEC_REM", 142, ne=3, nc=3, dim=4, k=2, special="nonfinite"),
    _c("nf_d6", "knn:nonfinite wave", "KNN_WAVE", 143, ne=3, nc=5, dim=6, k=3, special="nonfinite"),
    _c("nf_d20", "knn:nonfinite vec_both", "KNN_VEC_BOTH", 144, ne=3, nc=9, dim=20, k=3, special="nonfinite"),
    _c("nf_d16_p256", "knn:nonfinite vec_unroll n_cand=129 P=256", "KNN_VEC_UNROLL", 145, ne=3, nc=129, dim=16, k=7, special="nonfinite"),
    _c("nf_d8_nopad", "knn:nonfinite no_padding n_cand=4", "KNN_VEC_REM", 146, ne=3, nc=4, dim=8, k=2, special="nonfinite"),
    # data="real": the four distance paths on real-valued features (standard normal, clustered 100 + 1e-3 normal, near ties of one to four
    # float32 ulps), judged against float64 by the derived bound of the path (tests/knn_ref.py); pairs: the near-tie pairs planted
    _c("real_d12", "knn:real vec_rem", "KNN_VEC_REM", 147, ne=3, nc=37, dim=12, k=3, data="real", pairs=1),
    _c("real_d70", "knn:real wave two trips", "KNN_WAVE", 148, ne=3, nc=50, dim=70, k=3, data="real", pairs=2),
    _c("real_d36", "knn:real vec_both", "KNN_VEC_BOTH", 149, ne=3, nc=100, dim=36, k=5, data="real", pairs=4),
    _c("real_d160", "knn:real vec_unroll aser shape", "KNN_VEC_UNROLL", 150, ne=3, nc=150, dim=160, k=3, data="real", pairs=6),
]
COL_REDUCE = [_c("r%d_c%d" % (r, c), "col_reduce: rows=%d cols=%d" % (r, c), "COL_REDUCE", 150 + i, rows=r, cols=c)
              for i, (r, c) in enumerate([(97, 100), (3, 100), (8, 64), (16, 1), (64, 2048), (1, 33), (128, 96)])]
ASER = [_c("a%d_c%d_n%d" % (a, c, n), "aser: n_adv=%d n_coop=%d n_cand=%d" % (a, c, n), "ASER_SCORE", 160 + i, n_adv=a, n_coop=c, n_cand=n)
        for i, (a, c, n) in enumerate([(10, 10, 100), (3, 5, 100), (8, 16, 64), (16, 4, 1), (64, 32, 2048), (1, 1, 33)])]
# data: rand (distinct), ties (few distinct values), zeros (+0.0 / -0.0), inf (+-inf among finite), equal, nan, nan_inf
ARGSORT = [_c("n%d_%s" % (n, d), "argsort: n=%d %s" % (n, d), "ARGSORT_FULL" if n & (n - 1) == 0 else "ARGSORT_PADDED", 170 + i, n=n, data=d)
           for i, (n, d) in enumerate([(1, "rand"), (2, "zeros"), (3, "inf"), (255, "ties"), (256, "rand"), (257, "zeros"), (4095, "inf"),
                                       (4096, "ties"), (100, "equal"), (64, "nan"), (100, "nan_inf")])] + \
          [_c("refuse", "argsort:refuse", "ARGSORT_REFUSED", 189, n=4097, data="rand")]
# ---- NCM: `absent` classes have no sample (their mean row must stay untouched) ------------------------------------------------------------
NCM_MEANS = [_c("n%d_d%d_c%d" % (n, d, c), "ncm_means: n=%d d=%d n_cls=%d absent=%d" % (n, d, c, a), "NCM_MEANS", 190 + i, n=n, d=d, n_cls=c, absent=a)
             for i, (n, d, c, a) in enumerate([(50, 160, 10, 0), (30, 640, 5, 1), (7, 100, 1, 0), (40, 300, 4, 2), (5, 7, 2, 0)])]
NCM_PREDICT = [_c("n%d_d%d_c%d%s" % (n, d, c, "_ties" if t else ""), "ncm_predict: n=%d d=%d n_cls=%d ties=%d" % (n, d, c, t), "NCM_PREDICT", 200 + i,
                  n=n, d=d, n_cls=c, ties=t)
               for i, (n, d, c, t) in enumerate([(50, 160, 10, 0), (30, 640, 100, 0), (7, 100, 1, 0), (40, 300, 7, 0), (20, 160, 10, 1), (9, 640, 6, 1), (0, 16, 3, 0)])] + \
              [_c("nan_" + w, "ncm_predict:nan " + what, "NCM_PREDICT", 207 + i, n=9, d=100, n_cls=6, ties=0, nan=w)
               for i, (w, what) in enumerate([("mean", "one class mean (not class 0)"), ("feat", "one feature row: every distance"),
                                              ("two_means", "two class means: the first wins")])]
# ---- small GEMM: c[m, n] (+)= a b (+ bias) (relu).  at / bt: the operand is stored transposed.  The engine's forms (csrc/net.hip):
# heads y = x W^T + b (bt, bias, relu 0 / 1); dW (+)= dy^T x (at, accumulate 0 / 1); dx = dy W (neither).  pad: c_rs - n ----------------
_G_K = [16, 17, 19, 4, 15, 640, 1, 160]        # k % 16 in {0, 1..3, 4, 15}, the feature widths 160 / 640
_G_FORMS = [("head", dict(at=0, bt=1, bias=1, relu=0, acc=0, pad=0)), ("head_relu", dict(at=0, bt=1, bias=1, relu=1, acc=0, pad=0)),
            ("dw", dict(at=1, bt=0, bias=0, relu=0, acc=0, pad=0)), ("dw_acc", dict(at=1, bt=0, bias=0, relu=0, acc=1, pad=0)),
            ("dx", dict(at=0, bt=0, bias=0, relu=0, acc=0, pad=0)), ("acc_relu", dict(at=0, bt=1, bias=1, relu=1, acc=1, pad=0)),
            ("c_rs", dict(at=0, bt=0, bias=1, relu=0, acc=1, pad=5))]
_G_MN = [(10, 100), (16, 16), (37, 53), (1, 1), (20, 160), (33, 15), (128, 5), (17, 31)]


def _gemm_path(k):
    return "GEMM_K16" if k % 16 == 0 else "GEMM_KTAIL" if k < 16 else "GEMM_KBOTH"


GEMM = [_c("%s_m%d_n%d_k%d" % (fname, m, n, k), "gemm:%s k%%16=%d" % ({"dw": "a_transposed", "dw_acc": "a_transposed+accumulate", "acc_relu": "accumulate+relu",
                                                                      "c_rs": "c_rs>n"}.get(fname, fname), k % 16),
           _gemm_path(k), 210 + fi * 8 + ki, m=m, n=n, k=k, **form)
        for fi, (fname, form) in enumerate(_G_FORMS) for ki, (k, (m, n)) in enumerate(zip(_G_K, _G_MN[fi:] + _G_MN[:fi]))]

# ---- SCR augmentation, image kernel: n images of h x w (one thread per pixel, workgroups of 256: 5x7 is under one, 17x23 = 391 and
# 84x84 = 7056 end in a partial one); kind: how tests/augment_ref.py::augment_case_inputs builds pixels and parameters; off = (x, params,
# out); extra: rows allocated past n (sentinels: the kernel must leave them alone) ----------------------------------------------------------
AUGMENT = [
    _c("orders_same_image", "augment:orders one image in the 24 orders augment:partial_block 17x23", "AUGMENT", 301, n=24, h=17, w=23, kind="orders_same"),
    # (a contrast of 0.75 never clamps and so commutes with saturation and hue: 8 distinct images.  1.4 clamps: 18, all the contract allows)
    _c("orders_same_image_clamped", "augment:orders one image in the 24 orders, contrast 1.4 reaches the clamp", "AUGMENT", 317, n=24, h=17, w=23,
       kind="orders_same", contrast=1.4),
    _c("orders_mixed","augment:orders one per image, random crops and factors", "AUGMENT", 302, n=24, h=32, w=32, kind="orders_mixed"),
    _c("hsv_sectors", "augment:hsv_sectors branches, ties, sectors; hue shifts and saturation factors", "AUGMENT", 303, n=10, h=5, w=7, kind="hsv"),
    _c("clamps", "augment:clamps brightness / contrast at 0 and 1", "AUGMENT", 304, n=4, h=5, w=7, kind="clamps"),
] + [_c("geometry_%dx%d" % (h, w), "augment:fractional_crop augment:geometry %dx%d corners, 1x1, tall, wide, flip%s" % (h, w, " augment:partial_block" if h * w % 256 else ""),
        "AUGMENT", 305 + i, n=20, h=h, w=w, kind="geometry") for i, (h, w) in enumerate([(5, 7), (17, 23), (32, 32), (84, 84)])] + [
    _c("gray", "augment:gray alone and after jitter, h != w", "AUGMENT", 310, n=3, h=17, w=23, kind="gray"),
    _c("n1", "augment:n=1", "AUGMENT", 311, n=1, h=5, w=7, kind="random"),
    _c("n0", "augment:n0", "AUGMENT", 312, n=0, h=5, w=7, kind="random", extra=1),
    _c("misaligned", "augment:misaligned x, params, out", "AUGMENT", 313, n=5, h=17, w=23, kind="random", off=(1, 3, 1)),
    _c("guard", "augment:guard rows past n untouched", "AUGMENT", 314, n=3, h=17, w=23, kind="random", extra=2),
    _c("refuse_n", "augment:refuse grid.y", "AUGMENT_REFUSED", 315, n=65536, h=1, w=1, kind="refuse"),
    _c("refuse_hw", "augment:refuse int pixel index", "AUGMENT_REFUSED", 316, n=1, h=46341, w=46341, kind="refuse"),
]
# ---- SCR augmentation, parameter kernel: n rows of 30 draws (one thread per row, workgroups of 64), image size h x w, crop scale range;
# every case's parameter buffer has sentinel rows past n.  (16, 64) and (64, 16) with scale (0.99, 1): no attempt fits, the two fallback
# crops with the clamped aspect ratio.  The seeds are chosen so that at most 1 % of a case's rows have a rounding decision on a boundary
# (tests/test_cpu_small_ops.py asserts it, from the float64 reference alone) ---------------------------------------------------------------
_AP_SIZES = [((32, 32), (0.2, 1.0)), ((84, 84), (0.2, 1.0)), ((16, 64), (0.99, 1.0)), ((64, 16), (0.99, 1.0))]
AUG_PARAMS = [_c("%dx%d_n%d" % (h, w, n), "aug_params:%s %dx%d n=%d%s" % ("partial_block" if n % 64 else "full_blocks", h, w, n, " fallback crop" if h != w else ""),
                 "AUG_PARAMS", 330 + 4 * i + j, n=n, h=h, w=w, scale=sc)
              for i, ((h, w), sc) in enumerate(_AP_SIZES) for j, n in enumerate([1, 63, 65, 110])] + \
             [_c("extremes", "aug_params:extremes draws of exactly 0 and 1 - 2^-24", "AUG_PARAMS", 350, n=256, h=32, w=32, scale=(0.2, 1.0), special="extremes")]

CASES = {"rows": ROWS, "pair": PAIR, "u8": U8, "sgd": SGD, "cosine": COSINE, "ce": CE, "ce_seg": CE_SEG, "kd": KD, "mir": MIR, "supcon": SUPCON,
         "knn": KNN, "col_reduce": COL_REDUCE, "aser": ASER, "argsort": ARGSORT, "ncm_means": NCM_MEANS, "ncm_predict": NCM_PREDICT,
         "gemm": GEMM, "augment": AUGMENT, "aug_params": AUG_PARAMS}

# the path keys the suite must keep (a case may be renamed, these substrings must stay claimed)
REQUIRED_KEYS = [
    "supcon/rows:scalar", "supcon/grad:no_tail", "supcon/grad:tail", "supcon/grad:loss_only", "supcon:cap_A", "supcon:cap_dim", "supcon:refuse_A",
    "supcon:refuse_dim", "supcon:n_views=1", "supcon:n_views=3", "cosine:scalar", "cosine:k>64", "cosine:n<4", "cosine:blocks_cap", "cosine:eps_zero_row",
    "cosine:eps_zero_g", "rows:copy4_misaligned", "rows:copy16_ycap", "pair:host_index", "pair:device_index", "pair:fallback", "pair:units_b>256",
    "sgd:refuse_misaligned", "gemm:a_transposed", "gemm:a_transposed+accumulate", "gemm:accumulate+relu", "gemm:c_rs>n", "knn:vec_both d4n=5",
    "knn:vec_both d4n=6", "knn:vec_both d4n=7", "knn:wave misaligned", "knn:k>=n_cand larger", "ncm_means: n=30 d=640", "ncm_predict: n=20 d=160 n_cls=10 ties=1",
    "col_reduce: rows=3 ", "col_reduce: rows=8 cols=64", "col_reduce: rows=16 cols=1", "col_reduce: rows=64 cols=2048", "argsort: n=2 zeros", "argsort: n=3 inf",
    "argsort: n=64 nan", "augment:orders", "augment:hsv_sectors", "augment:partial_block", "augment:fractional_crop", "augment:clamps", "augment:gray",
    "knn:nonfinite vec_rem n_cand=3 P=4", "knn:nonfinite wave", "knn:nonfinite vec_both", "knn:nonfinite vec_unroll n_cand=129 P=256",
    "knn:nonfinite no_padding", "knn:real vec_rem", "knn:real wave", "knn:real vec_both", "knn:real vec_unroll", "ce:label_outside mean",
    "ce:label_outside none", "ce_seg:label_outside", "mir:label_outside", "ncm_predict:nan one class mean", "ncm_predict:nan one feature row",
    "ncm_predict:nan two class means", "augment:misaligned", "augment:guard", "augment:refuse", "aug_params:partial_block", "aug_params:extremes",
]


def ids(op):
    return [c["name"] for c in CASES[op]]


def plan_args(op, c, ptrs=None):
    """The int64 argument vector of ocl_test_small_op_path for case c.  ptrs: the real device addresses, in the order the op's `off`
    lists them (the GPU test); None: stand-in addresses ALIGNED + 4 * off (the CPU test; every offset is in 4-byte elements but u8's)."""
    off = c["off"] if isinstance(c["off"], tuple) else (c["off"],)
    if ptrs is None:
        ptrs = [ALIGNED + (1 if op == "u8" else 4) * o for o in off]
    if op == "rows":
        return [ptrs[0], ptrs[1], c["row"] * 4, c["n"]]
    if op == "pair":
        return [ptrs[0], ALIGNED, c["row_a"] * 4, c["row_b"] * 4, c["n"]]
    if op == "u8":
        return [c["n"], c["h"], c["w"], c["c"]]
    if op == "sgd":
        return [ptrs[0], ALIGNED, 0, c["n"]]
    if op == "cosine":
        return [ptrs[0], ptrs[1], c["k"], c["n"]]
    if op == "ce":
        return [c["n"], c["c"], 1 if c["red"] == "mean" else 0]
    if op in ("ce_seg", "kd", "mir"):
        return [c["n"], c["c"]]
    if op == "supcon":
        return [ptrs[0], c["bsz"], c["n_views"], c["dim"], 0 if c.get("want") == "loss" else 1]
    if op == "knn":
        return [ptrs[0], c["ne"], c["nc"], c["dim"], c["k"]]
    if op == "col_reduce":
        return [c["rows"], c["cols"]]
    if op == "aser":
        return [c["n_cand"]]
    if op == "argsort":
        return [c["n"]]
    if op == "ncm_means":
        return [c["d"], c["n_cls"]]
    if op == "ncm_predict":
        return [c["n"], c["d"], c["n_cls"]]
    if op == "gemm":
        return [c["m"], c["n"], c["k"]]
    if op == "augment":
        return [c["n"], c["h"], c["w"]]
    if op == "aug_params":
        return [c["n"]]
    raise KeyError(op)
