"""The cases of the BatchNorm conditioning suite, shared by tests/test_cpu_bn_cond.py (regimes realised, every call site claimed, the bounds
can be met; no GPU) and tests/test_gpu_bn_cond.py (runs them).  Plain data and the generators of the cases' inputs (numpy / torch CPU).

A channel regime is (name, mu, sigma, kind); channel c of a case takes regime c mod 10, so every C = 20 .. 160 holds every regime.  r = 1e4 is
left out on purpose: fp32 data of that kind carries three digits of its spread, and a float64 reference of the fp32 values is no longer the
quantity of interest.

A site is (file, enclosing kernel or function, what): what = "fx" for a call of fx_add / fx_fetch_add outside conv_stats_dev.h (a producer of
batch sums), "ss" for a call of bn_scale_shift (a place that forms the scale / shift the ReLU decision is taken with)."""
import numpy as np
import torch
import torch.nn.functional as F

CONST = float(np.float32(1000.1))
REGIMES = [
    ("r0", 0.0, 1.0, "normal"),
    ("r1", 1.0, 1.0, "normal"),
    ("r10", 10.0, 1.0, "normal"),
    ("r100", 100.0, 1.0, "normal"),
    ("r1000", 1000.0, 1.0, "normal"),
    ("rneg100", -100.0, 1.0, "normal"),
    ("dead", 0.0, 0.0, "const"),
    ("const", CONST, 0.0, "const"),
    ("tiny", 0.0, 1e-4, "normal"),
    ("big", 0.0, 1e3, "normal"),
]
NAMES = [r[0] for r in REGIMES]


def regime_of(c):
    return REGIMES[c % len(REGIMES)]


def regime_tensor(rng, n, hw, c):
    """y [n, hw, hw, c] of fp32 values (as float64): channel j drawn from its regime."""
    y = np.empty((n, hw, hw, c), np.float32)
    for j in range(c):
        _, mu, sigma, kind = regime_of(j)
        y[..., j] = mu if kind == "const" else (mu + sigma * rng.standard_normal((n, hw, hw))).astype(np.float32)
    return y.astype(np.float64)


def affine(rng, c):
    """gamma, beta (fp32 values as float64): beta of both signs and one exact zero per ten channels."""
    gamma = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32).astype(np.float64)
    beta = (0.5 * rng.standard_normal(c)).astype(np.float32).astype(np.float64)
    beta[3::10] = 0.0
    return gamma, beta


# ---- producers: a regime realised through a convolution --------------------------------------------------------------------------------
def const_channel(cin):
    return 2 if cin == 3 else cin - 1


def producer_inputs(dims, groups, seed, act=None):
    """dims = (n, hin, win, cin, cout, k, stride).  Returns (x [n, hin, win, cinT], w [cout, cin, k, k]) as float64 tensors of fp32 values.

    One input channel is the constant 1 (+1 in the images of BatchNorm group 0, -1 in group 1); output channel c's weight on the centre tap of
    that channel carries mu_c (the centre tap never meets padding: every output pixel gets exactly the offset); the other weights are random,
    rescaled per output row in float64 so that the output spread is sigma_c, and the row's offset also takes out the mean of that random
    part.  With two groups the images of group 1 are the negated images of group 0: the random part of group 1 is the negative of group 0's, so
    group 1 realises (-mu_c, sigma_c) exactly as group 0 realises (mu_c, sigma_c), and a pixel booked to the wrong group moves a sum by 2 mu_c.
    dead and const rows have all other weights zero.
    act: for the input-transform forms, the activation [n, hin, win, cinT] the consuming convolution stages (its constant channel is 1: a
    raw-output channel with gamma = 0, beta = 1); x is then ignored and only w is built from it.  ReLU'd activations cannot be mirrored: with
    two groups both realise (+mu_c, sigma_c), up to the difference of the two groups' sample means of the random part."""
    n, hin, win, cin, cout, k, stride = dims
    cin_t = 4 if cin == 3 else cin
    rng = np.random.default_rng(seed)
    cc = const_channel(cin)
    if act is None:
        assert n % groups == 0 and groups in (1, 2, 3)
        per = n // groups
        x = rng.standard_normal((per, hin, win, cin_t)).astype(np.float32).astype(np.float64)
        x[..., cc] = 1.0
        if cin == 3:
            x[..., 3] = 0.0
        if groups > 1:      # (a third group holds the images of group 0 again: every neighbour of a group is its mirror image)
            x = np.concatenate([x if g % 2 == 0 else -x for g in range(groups)], axis=0)
    else:
        x = np.asarray(act, np.float64)
    w = rng.standard_normal((cout, cin, k, k))
    w[:, cc] = 0.0
    for c in range(cout):
        if regime_of(c)[3] == "const":
            w[c] = 0.0
    pad, mid = (1 if k == 3 else 0), k // 2
    per = n if act is not None else n // groups     # (act: no mirrored group, the rows are scaled and centred over all images)
    xt = torch.from_numpy(np.ascontiguousarray(x[:per, ..., :cin].transpose(0, 3, 1, 2)))
    yr = F.conv2d(xt, torch.from_numpy(w), stride=stride, padding=pad).numpy()      # the random part of group 0: [per, cout, ho, wo]
    for c in range(cout):
        _, mu, sigma, kind = regime_of(c)
        if kind == "const":
            w[c, cc, mid, mid] = mu
            continue
        s = sigma / yr[:, c].std()
        w[c] *= s
        w[c, cc, mid, mid] = mu - s * yr[:, c].mean()
    w = w.astype(np.float32).astype(np.float64)
    return torch.from_numpy(x), torch.from_numpy(w)


def conv64(x, w, stride):
    """float64 convolution of x NHWC [n, h, w, cinT] with w [cout, cin, k, k] -> NHWC."""
    k, cin = w.shape[-1], w.shape[1]
    y = F.conv2d(x[..., :cin].permute(0, 3, 1, 2), w, stride=stride, padding=1 if k == 3 else 0)
    return y.permute(0, 2, 3, 1).contiguous()


T, Q, S, WX, BN, WG, SD = "conv_t_kernel.h", "conv_q.hip", "conv_s.hip", "convw.hip", "bn.hip", "wgrad.hip", "conv_stats_dev.h"

# (a) producers: layer_forms.COVERED key -> sites.  The cheapest key that reaches each stats epilogue; the .../stats_xf keys also reach the
# family's bn_scale_shift (the input transform's table).
PRODUCERS = [
    dict(key="t1x1.res.c1.pf4/stats", sites=[(T, "conv_t_kernel", "fx")]),
    dict(key="q2.pf4/stats", sites=[(Q, "conv_q_kernel", "fx")]),
    dict(key="s1/stats", sites=[(S, "conv_s_kernel", "fx")]),
    dict(key="s2/stats", sites=[(S, "conv_s_kernel", "fx")]),
    dict(key="wx1x1/stats", sites=[(WX, "conv_wx_kernel", "fx")]),
    dict(key="wx3x1/stats", sites=[(WX, "conv_wx_kernel", "fx")]),
    dict(key="t1x1.res.c1.pf4/stats_xf", sites=[(T, "conv_t_kernel", "ss"), (T, "conv_t_kernel", "fx")]),
    dict(key="q2.pf12/stats_xf", sites=[(Q, "conv_q_kernel", "ss"), (Q, "conv_q_kernel", "fx")]),
    dict(key="s1/stats_xf", sites=[(S, "conv_s_kernel", "ss"), (S, "conv_s_kernel", "fx")]),
]

# conv_w_kernel: reached only with OCL_CONV_WX=0 (read once per process): the layer of a covered conv_wx key, in a child process
SWITCH_PRODUCER = dict(key="wx3x1/stats", want="w3x1/stats", force=dict(force_cw=1), env=dict(OCL_CONV_WX="0"),
                       test="test_conv_w_kernel_producer_in_a_fresh_process", sites=[(WX, "conv_w_kernel", "fx")])

# (b) - (d): the BatchNorm kernels and the recomputed ReLU decision: name, the test of tests/test_gpu_bn_cond.py that runs it, sites
CONSUMERS = [
    dict(name="bn_fwd", test="test_six_places_take_one_relu_decision", sites=[(BN, "bn_fwd_kernel", "ss")]),
    dict(name="bn_apply_saved", test="test_six_places_take_one_relu_decision", sites=[(BN, "bn_apply_saved_kernel", "ss")]),
    dict(name="conv_xf_identity", test="test_six_places_take_one_relu_decision", sites=[(T, "conv_t_kernel", "ss")]),
    dict(name="conv_xf_consumer", test="test_input_transform_of_exact_cells_on_ill_conditioned_channels",
         sites=[(T, "conv_t_kernel", "ss"), (S, "conv_s_kernel", "ss"), (Q, "conv_q_kernel", "ss")]),
    dict(name="wgrad_xf", test="test_six_places_take_one_relu_decision", sites=[(WG, "conv_wgrad_body", "ss")]),
    dict(name="bnb_no_z", test="test_six_places_take_one_relu_decision", sites=[(SD, "bnb_table", "ss")]),
    dict(name="bn_bwd_chan", test="test_mask_from_y_of_every_backward_path_is_the_exact_decision", sites=[(BN, "bn_bwd_chan_kernel", "ss")]),
    dict(name="bn_bwd_fused", test="test_mask_from_y_of_every_backward_path_is_the_exact_decision", sites=[(BN, "bn_bwd_fused_kernel", "ss"), (BN, "bn_bwd_fused_kernel", "fx")]),
    dict(name="bn_bwd_two_kernel", test="test_mask_from_y_of_every_backward_path_is_the_exact_decision", sites=[(BN, "bn_bwd_reduce_kernel", "ss"), (BN, "bn_bwd_apply_kernel", "ss"), (BN, "bn_bwd_reduce_kernel", "fx")]),
]

# (b) the convolution's input transform as a consumer of exact cells: (n, hw, C, groups, the family the planner gives a C -> C 3x3 convolution of
# this pass; the GPU test asserts it): conv_t, conv_s and conv_q, each at one or two groups, and conv_t at three (the third row of the
# [groups][Cin/4][2][4] table and of the saved statistics, the third running update)
# (conv_q takes a C -> C convolution only from 64 images of 32 x 32 on: above the n <= 12 of the other consumer cases)
XF_CONSUMERS = [(10, 32, 20, 2, "t"), (6, 16, 40, 1, "t"), (12, 8, 160, 2, "s"), (5, 4, 80, 1, "s"), (64, 32, 20, 2, "q"), (6, 16, 40, 3, "t")]

# (c) the ladder cases of the six places: (n, hw, C, groups); every group holds at least 129 pixels
LADDERS = [(4, 16, 40, 1), (4, 16, 20, 2)]
# mask_from_y through every backward kernel that honours it: (n, hw, c, groups, one_pass, the path code ocl_test_bn_bwd reports)
# (layer_api allows mask_from_y with one set only: the codes are 1011, 2031, 2061, 2121, 3001.  2121 = bn_bwd_fused_kernel<12, 1> has no case: it
# needs more than 6 units per thread on 256 workgroups -- 40 images of 32 x 32 -- beyond the n <= 12 of these cases, and it is the same template
# code as 2031 / 2061 with a longer register array; its arithmetic is held by BWD_PATHS' 2121 case)
# frozen = 1 reaches the two-kernel path only (launch_bn_bwd sends frozen launches past the chan and fused kernels), so the other paths run
# unfrozen and show their mask through dbeta = sum(mask * dz): powers of two on the ladder rungs, twelve per group and launch, and dz = 1 for
# a per-channel count over all elements.  Elements outside the ladders are thus held as a count only, and the apply-side use of the mask in
# the fused and chan kernels (the same registers d[e] the sums were taken from) is not observed element by element.
MASK_PATHS = [
    (9, 4, 160, 1, 1, 1011),     # bn_bwd_chan_kernel<1, 1> (144 pixels: the small-map gate is 512)
    (4, 16, 40, 1, 1, 2031),     # bn_bwd_fused_kernel<3, 1>
    (6, 16, 40, 2, 1, 2061),     # bn_bwd_fused_kernel<6, 1>
    (10, 32, 20, 2, 0, 3001),    # bn_bwd_reduce_kernel + bn_bwd_apply_kernel
]
# (d) every path code of test_bn_backward_paths_against_float64: (n, hw, c, groups, nsets, one_pass, path)
# (2121 needs 40 images of 32 x 32: above the n <= 12 of the other backward cases, the smallest pass that reaches that path code)
BWD_PATHS = [
    (4, 4, 160, 2, 1, 1, 1011), (8, 4, 160, 1, 2, 1, 1012),
    (4, 16, 40, 1, 1, 1, 2031), (4, 16, 40, 1, 2, 1, 2032),
    (6, 16, 40, 2, 1, 1, 2061), (10, 32, 20, 2, 2, 1, 2062),
    (40, 32, 20, 2, 1, 1, 2121),
    (10, 32, 20, 2, 1, 0, 3001), (10, 16, 40, 2, 2, 0, 3002),
]
# the scales of dz per channel (cyclic, period 4 against the regimes' period 10: every pairing occurs within C = 20 only partly, within 40
# fully); "cancel": dz = 5 + 0.01 randn, so that d - k1 cancels
DZ_SCALES = [1.0, 1e-4, 1e3, "cancel"]

# sites no case of this suite reaches, with the reason (tests/test_cpu_bn_cond.py: every parsed site is required, every required site is
# claimed by a case or listed here with its reason)
EXEMPT_SITES = {
    (WX, "conv_w_kernel", "ss"): "conv_w_kernel runs only with OCL_CONV_WX=0, and the planner gives the conv_w / conv_wx families no input-transform form (no .../stats_xf key in COVERED)",
    (WX, "conv_wx_kernel", "ss"): "the planner gives conv_wx no input-transform form (no wx.../stats_xf key in layer_forms.COVERED)",
}

# every call site of fx_add / fx_fetch_add outside conv_stats_dev.h ("fx") and of bn_scale_shift ("ss"), as (file, enclosing function, what)
REQUIRED_SITES = [
    (T, "conv_t_kernel", "fx"), (Q, "conv_q_kernel", "fx"), (S, "conv_s_kernel", "fx"), (WX, "conv_w_kernel", "fx"), (WX, "conv_wx_kernel", "fx"),
    (BN, "bn_bwd_reduce_kernel", "fx"), (BN, "bn_bwd_fused_kernel", "fx"),
    (T, "conv_t_kernel", "ss"), (Q, "conv_q_kernel", "ss"), (S, "conv_s_kernel", "ss"), (WX, "conv_w_kernel", "ss"), (WX, "conv_wx_kernel", "ss"),
    (WG, "conv_wgrad_body", "ss"), (SD, "bnb_table", "ss"),
    (BN, "bn_fwd_kernel", "ss"), (BN, "bn_apply_saved_kernel", "ss"), (BN, "bn_bwd_reduce_kernel", "ss"), (BN, "bn_bwd_apply_kernel", "ss"),
    (BN, "bn_bwd_fused_kernel", "ss"), (BN, "bn_bwd_chan_kernel", "ss"),
]
