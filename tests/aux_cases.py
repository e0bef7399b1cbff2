"""The parity cases of the glue kernels (csrc/conv_aux.hip: weight packing, NCHW -> NHWC4 input conversion, average pool, L2 normalisation, ReLU
backward, column sum, fill), of bn_fold_kernel / bn_apply_saved_kernel (csrc/bn.hip) and of the head chain net.hip builds from them (head_forward,
head_backward), shared by tests/test_cpu_aux.py (every kernel and every required key is claimed, the "above the cap" cases exceed the launchers'
grid caps as parsed from the sources; no GPU) and tests/test_gpu_aux.py (runs every case).

Plain data.  A case is a dict:
  name     unique within its op (the pytest id)
  key      what it is there for: "<op>:<what>", free text for people and for REQUIRED_KEYS
  also     further keys the case claims (the rows / columns its data holds), matched exactly like `key`
  kernels  the __global__ kernels the case reaches
  seed     of the case's random generator
  ...      the op's sizes
A case with `cap` = (launcher, work items) claims to launch more work than the launcher's capped grid covers in one stride."""

# op name -> op code of ocl_test_aux (include/ocl_hip.h); None: a hook of its own (ocl_test_pack_all, ocl_test_head)
OPS = {"layout": 0, "avgpool": (1, 2), "l2norm": (3, 4), "relu_bwd": 5, "colsum": 6, "fill": 7, "bn_fold": 8, "bn_apply_saved": 9,
       "pack_all": None, "head": None}
# the kernels of csrc/bn.hip this suite owns (the others are tests/test_gpu_layers.py's)
BN_KERNELS = ["bn_fold_kernel", "bn_apply_saved_kernel"]
EXEMPT_KERNELS = []


def _c(name, key, kernels, seed, **kw):
    d = dict(name=name, key=key, kernels=list(kernels), seed=seed, also=[])
    d.update(kw)
    return d


PLAIN, SEG = ["nchw3_to_nhwc4_kernel"], ["nchw3_to_nhwc4_seg_kernel"]
# ---- layout: ns = images per segment (one segment: the plain kernel, as in the engine) ------------------------------------------------
LAYOUT = [
    _c("one32", "layout:1_segment", PLAIN, 1, hw=32, ns=(3,)),
    _c("one84", "layout:1_segment_84", PLAIN, 2, hw=84, ns=(2,)),
    _c("n1", "layout:n=1", PLAIN, 3, hw=32, ns=(1,)),
    _c("two", "layout:2_segments(1,5)", SEG, 4, hw=32, ns=(1, 5)),
    _c("three", "layout:3_segments(10,10,1)", SEG, 5, hw=32, ns=(10, 10, 1)),
    _c("three84", "layout:3_segments_84", SEG, 6, hw=84, ns=(2, 1, 3)),
    _c("eight", "layout:8_segments_uneven", SEG, 7, hw=32, ns=(1, 3, 1, 2, 5, 1, 4, 1)),
    _c("eight84", "layout:8_segments_uneven_84", SEG, 8, hw=84, ns=(2, 1, 1, 3, 1, 2, 1, 1)),
    _c("cap_plain", "layout:above_cap_plain", PLAIN, 9, hw=32, ns=(513,), cap=("launch_nchw3_to_nhwc4", 513 * 32 * 32)),
    _c("cap_seg", "layout:above_cap_seg", SEG, 10, hw=84, ns=(30, 1, 44), cap=("launch_nchw3_to_nhwc4_segments", 75 * 84 * 84)),
]
# ---- avg_pool2d(4): (n, H, W, C); 11 x 11 crops to 8 x 8 (backward: zeros in rows / columns 8..10); ygrid: the backward's grid rows ----
POOL_K = ["avgpool_fwd_kernel", "avgpool_bwd_kernel"]
AVGPOOL = [
    _c("4x4_n1", "avgpool:4x4_ygrid2", POOL_K, 11, n=1, h=4, w=4, c=160, ygrid=2),
    _c("4x4_n3", "avgpool:4x4_n3", POOL_K, 12, n=3, h=4, w=4, c=160, ygrid=2),
    _c("11x11_n1", "avgpool:11x11_crop_ygrid_cap8", POOL_K, 13, n=1, h=11, w=11, c=160, ygrid=8),
    _c("11x11_n3", "avgpool:11x11_crop_n3", POOL_K, 14, n=3, h=11, w=11, c=160, ygrid=8),
]
# ---- l2norm: rows of d; the last three rows of n = 7: all zero (clamped), magnitude 1e-20 (clamped), magnitude 1e15 (squares near the top)
L2_K = ["l2norm_fwd_kernel", "l2norm_bwd_kernel"]
L2_ROWS = ["l2norm:zero_row", "l2norm:1e-20_row", "l2norm:1e15_row"]       # what every n = 7 case holds
L2NORM = [_c("d%d_n%d" % (d, n), "l2norm:d=%d,n=%d" % (d, n), L2_K, 20 + i, n=n, d=d, also=["l2norm:out2_null_and_given"] + (L2_ROWS if n == 7 else []))
          for i, (d, n) in enumerate([(128, 1), (128, 7), (160, 1), (160, 7), (640, 1), (640, 7), (10, 1), (10, 7)])]
# ---- relu_bwd -------------------------------------------------------------------------------------------------------------------------
RELU_BWD = [
    _c("n1", "relu_bwd:n=1", ["relu_bwd_kernel"], 31, n=1),
    _c("n255", "relu_bwd:n=255", ["relu_bwd_kernel"], 32, n=255),
    _c("n257", "relu_bwd:n=257", ["relu_bwd_kernel"], 33, n=257),
    _c("cap", "relu_bwd:above_cap", ["relu_bwd_kernel"], 34, n=1024 * 256 + 257, cap=("launch_relu_bwd", 1024 * 256 + 257)),
]
# ---- colsum ---------------------------------------------------------------------------------------------------------------------------
COLSUM = [_c("%dx%d" % rc, "colsum:%dx%d" % rc, ["colsum_kernel"], 40 + i, rows=rc[0], cols=rc[1])
          for i, rc in enumerate([(1, 1), (7, 33), (8, 32), (9, 100), (220, 128), (20, 640), (3, 10)])]
# ---- fill -----------------------------------------------------------------------------------------------------------------------------
FILL = [
    _c("n0", "fill:n=0", [], 50, n=0),
    _c("n1", "fill:n=1", ["fill_kernel"], 51, n=1),
    _c("n257", "fill:n=257", ["fill_kernel"], 52, n=257),
    _c("cap", "fill:above_cap", ["fill_kernel"], 53, n=1024 * 256 + 3, cap=("launch_fill", 1024 * 256 + 3)),
]
# ---- bn_fold: the whole network's BatchNorm list ----------------------------------------------------------------------------------------
BN_FOLD = [
    _c("net32", "bn_fold:whole_network", ["bn_fold_kernel"], 61, hw=32, nf=20),
    _c("net84", "bn_fold:whole_network_84", ["bn_fold_kernel"], 62, hw=84, nf=20),
]
# ---- bn_apply_saved: (m_per_group, G, C) ----------------------------------------------------------------------------------------------
BN_APPLY = [
    _c("m1", "bn_apply_saved:m=1", ["bn_apply_saved_kernel"], 71, m=1, g=1, c=20),
    _c("m1023_g2", "bn_apply_saved:m=1023,G=2", ["bn_apply_saved_kernel"], 72, m=1023, g=2, c=20),
    _c("m256_c160", "bn_apply_saved:C=160", ["bn_apply_saved_kernel"], 73, m=256, g=1, c=160),
    _c("cap", "bn_apply_saved:above_cap", ["bn_apply_saved_kernel"], 74, m=209716, g=1, c=20, cap=("launch_bn_apply_saved", 209716 * 5)),
]
# ---- pack_all: mask 1 forward packs, 2 data-gradient packs, 3 both; clear: the two regions the launch's extra grid row zeroes -------------
PACK_ALL = [_c("hw%d_%s_%s" % (hw, mn, "clear" if clear else "noclear"), "pack_all:hw=%d,mask=%s,clear=%d" % (hw, mn, clear),
               ["pack_weights_kernel"], 80 + i, hw=hw, nf=20, mask=mask, clear=clear)
            for i, (hw, (mn, mask), clear) in enumerate((hw, m, cl) for hw in (32, 84) for m in (("TF", 1), ("TD", 2), ("ALL", 3))
                                                        for cl in (0, 1))]
# ---- head: kind 0 classifier, 1 MLP, 2 linear projection, 3 none; n = "side": the smallest n whose dW / db go to the side stream ---------
HEAD_K = {0: ["colsum_kernel"],
          1: ["l2norm_fwd_kernel", "l2norm_bwd_kernel", "relu_bwd_kernel", "colsum_kernel", "fill_kernel"],
          2: ["l2norm_fwd_kernel", "l2norm_bwd_kernel", "colsum_kernel", "fill_kernel"],
          3: ["l2norm_fwd_kernel", "l2norm_bwd_kernel", "fill_kernel"]}
HEAD = [_c("k%d_hw%d_n%d_acc%d" % (k, hw, n, acc), "head:kind=%d,hw=%d,n=%d,acc=%d" % (k, hw, n, acc), HEAD_K[k] if not acc or k == 0
           else [x for x in HEAD_K[k] if x != "fill_kernel"], 100 + i, kind=k, hw=hw, n=n, acc=acc, n_classes=100 if n in (2, 20) else 10,
           feat_dim=128, also=(["head:zero_feat_row"] if k in (2, 3) and n >= 2 else []) + (["head:dead_h1_columns"] if k == 1 else []))
        for i, (k, hw, n, acc) in enumerate((k, hw, n, acc) for k in range(4) for hw in (32, 84) for n in (1, 2, 7, 20) for acc in (0, 1))]
HEAD += [_c("k1_hw%d_side_acc%d" % (hw, acc), "head:side_stream,hw=%d,acc=%d" % (hw, acc), HEAD_K[1][:4] + (["fill_kernel"] if not acc else []),
            170 + 2 * j + acc, kind=1, hw=hw, n="side", acc=acc, n_classes=10, feat_dim=128, also=["head:dead_h1_columns"])
         for j, hw in enumerate((32, 84)) for acc in (0, 1)]
# (kinds 2, 3 with n >= 2: feat row 1 is all zero; kind 1: three columns of h1 are dead for every row -- the cases' `also` keys)

CASES = {"layout": LAYOUT, "avgpool": AVGPOOL, "l2norm": L2NORM, "relu_bwd": RELU_BWD, "colsum": COLSUM, "fill": FILL, "bn_fold": BN_FOLD,
         "bn_apply_saved": BN_APPLY, "pack_all": PACK_ALL, "head": HEAD}

REQUIRED_KEYS = [
    "layout:1_segment", "layout:2_segments(1,5)", "layout:3_segments(10,10,1)", "layout:8_segments_uneven", "layout:n=1", "layout:1_segment_84",
    "layout:3_segments_84", "layout:above_cap_plain", "layout:above_cap_seg",
    "avgpool:4x4_ygrid2", "avgpool:4x4_n3", "avgpool:11x11_crop_ygrid_cap8", "avgpool:11x11_crop_n3",
    "l2norm:d=128,n=1", "l2norm:d=128,n=7", "l2norm:d=160,n=7", "l2norm:d=640,n=7", "l2norm:d=10,n=7", "l2norm:d=10,n=1",
    "l2norm:zero_row", "l2norm:1e-20_row", "l2norm:1e15_row", "l2norm:out2_null_and_given",
    "relu_bwd:n=1", "relu_bwd:n=255", "relu_bwd:n=257", "relu_bwd:above_cap",
    "colsum:1x1", "colsum:7x33", "colsum:8x32", "colsum:9x100", "colsum:220x128", "colsum:20x640", "colsum:3x10",
    "fill:n=0", "fill:n=1", "fill:n=257", "fill:above_cap",
    "bn_fold:whole_network", "bn_apply_saved:m=1", "bn_apply_saved:m=1023,G=2", "bn_apply_saved:C=160", "bn_apply_saved:above_cap",
] + ["pack_all:hw=%d,mask=%s,clear=%d" % (hw, m, cl) for hw in (32, 84) for m in ("TF", "TD", "ALL") for cl in (0, 1)] \
  + ["head:kind=%d,hw=%d,n=%d,acc=%d" % (k, hw, n, acc) for k in range(4) for hw in (32, 84) for n in (1, 2, 7, 20) for acc in (0, 1)] \
  + ["head:side_stream,hw=%d,acc=%d" % (hw, acc) for hw in (32, 84) for acc in (0, 1)] + ["head:zero_feat_row", "head:dead_h1_columns"]


def all_keys():
    """Every key a case claims (its own and its `also` list)."""
    return [k for cases in CASES.values() for c in cases for k in [c["key"]] + c["also"]]


def ids(op):
    return [c["name"] for c in CASES[op]]


def find(op, name):
    return [c for c in CASES[op] if c["name"] == name][0]
