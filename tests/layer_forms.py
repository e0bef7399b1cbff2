"""Shared by tests/test_gpu_layers.py and tests/test_cpu_forms.py (a plain helper module, not a conftest): the names of the kernel forms
the network engine plans, the pass grid that crosses every planner threshold, and the single-layer parity cases that cover those forms.

A form is one compiled kernel the engine launches for a layer: the family and its template parameters (conv_t_kernel's MT, NT, weight
schedule, class count and patch prefetch depth; conv_q_kernel's pixel sets and prefetch depth; conv_s_kernel's pixel tiles; conv_w /
conv_wx's tiles; conv_wgrad_kernel's MTW, NTW and prefetch depth, its 4x4x1 form, the variants of conv_wgrad_multi_kernel), together
with the epilogue the engine runs it with (train forward: batch statistics, with the producer's BatchNorm + ReLU applied while staging
for the second convolution of a block; eval forward: folded BatchNorm; data gradient: plain, or feeding a BatchNorm backward)."""
import ctypes as C

FAMILIES = ("t", "q", "s", "w", "wx")
CONV_FAMILY = {0: "conv_t", 1: "conv_q", 2: "conv_s", 3: "conv_w", 4: "conv_wx"}

# train passes: every batch size up to 64 (the replay-sized passes and their thresholds), then the large passes; eval passes as the engine
# plans them (rounded up to 4 images up to 16, to 16 above)
TRAIN_N = list(range(1, 65)) + [100, 110, 128, 160, 220, 256, 300]
EVAL_N = [4, 8, 12, 16] + list(range(32, 417, 16))
HW = (32, 84)


def conv_key(form, epi):
    """epi: 'stats' / 'stats_xf' (train forward), 'affine' (eval forward), 'plain' / 'bnb' (data gradient)."""
    fam = FAMILIES[form.family]
    if form.family == 0:
        sched = "ring" if form.pipe else ("res" if form.wres else "two")
        body = "t%dx%d.%s.c%d.pf%d" % (form.mt, form.nt, sched, form.ncls, form.pf)
    elif form.family == 1:
        body = "q%d.pf%d" % (form.q4, form.pf)
    elif form.family == 2:
        body = "s%d" % form.nt
    else:
        body = "%s%dx%d" % (fam, form.mt, form.nt)
    return body + "/" + epi


def wgrad_key(wform, xf, merged):
    body = ("wgq%d" % wform.q_rgw) if wform.q_rgw else ("wg%dx%d" % (wform.mtw, wform.ntw))
    body += ".pf%d" % wform.pf
    if merged and wform.multi >= 0:
        body += ".m%d" % wform.multi
    return body + ("/xf" if xf else "/plain")


def net_forms(lib, hw, n, groups, train):
    """[(key, entry)] for every launch geometry of one pass, entry: the ocl_test_net_form (a copy)."""
    from ocl_amd import ffi
    cap = 256
    arr = (ffi.TestNetForm * cap)()
    cnt = lib.ocl_test_net_forms(hw, 20, n, groups, train, arr, cap)
    assert 0 < cnt <= cap, (hw, n, groups, train, cnt, lib.ocl_last_error())
    out = []
    for i in range(cnt):
        e = ffi.TestNetForm()
        C.memmove(C.addressof(e), C.addressof(arr[i]), C.sizeof(e))
        if e.dir == 0:
            epi = ("stats_xf" if e.desc.xf else "stats") if train else "affine"
            out.append((conv_key(e.form, epi), e))
        elif e.dir == 1:
            out.append((conv_key(e.form, "bnb" if e.desc.bnb else "plain"), e))
        else:
            out.append((wgrad_key(e.wform, e.wdesc.xf_groups > 0, e.wg_merged), e))
    return out


def pass_grid():
    for hw in HW:
        for n in TRAIN_N:
            for g in (1, 2):
                if n % g == 0:
                    yield hw, n, g, 1
        for n in EVAL_N:
            yield hw, n, 1, 0


def entry_cost(hw, n, e):
    d = e.desc if e.dir < 2 else e.wdesc
    return n * d.hin * d.win * max(d.cin, 4) * d.cout


def enumerate_forms(lib):
    """{key: (hw, n, groups, train, entry)}: every form of the grid with the cheapest pass / layer that reaches it."""
    best = {}
    for hw, n, g, train in pass_grid():
        for key, e in net_forms(lib, hw, n, g, train):
            c = entry_cost(hw, n, e)
            if key not in best or c < best[key][0]:
                best[key] = (c, (hw, n, g, train, e))
    return {k: v[1] for k, v in best.items()}


# The single-layer parity cases of tests/test_gpu_layers.py that reach each form: key -> (hw, n, groups, layer index, direction).  The
# layer index is the conv's position in module order (0 stem, then conv1, conv2[, shortcut] of each block); the GPU test re-derives the
# layer's description through ocl_test_net_forms and asserts that the hook reports this very form.  Regenerate with
# `python tests/layer_forms.py` after a planner change (and add parity cases for the new forms).
COVERED = {
    'q1.pf12/affine': (84, 8, 1, 1, 0),
    'q1.pf12/bnb': (84, 5, 1, 1, 1),
    'q1.pf12/plain': (84, 24, 1, 1, 1),
    'q1.pf12/stats': (84, 5, 1, 1, 0),
    'q1.pf12/stats_xf': (84, 5, 1, 2, 0),
    'q2.pf12/affine': (32, 64, 1, 1, 0),
    'q2.pf12/bnb': (32, 64, 1, 1, 1),
    'q2.pf12/plain': (32, 220, 1, 1, 1),
    'q2.pf12/stats': (32, 64, 1, 1, 0),
    'q2.pf12/stats_xf': (32, 64, 1, 2, 0),
    'q2.pf4/affine': (32, 64, 1, 0, 0),
    'q2.pf4/stats': (32, 64, 1, 0, 0),
    's1/affine': (32, 4, 1, 11, 0),
    's1/bnb': (32, 1, 1, 11, 1),
    's1/plain': (32, 1, 1, 13, 1),
    's1/stats': (32, 1, 1, 13, 0),
    's1/stats_xf': (32, 1, 1, 11, 0),
    's2/affine': (32, 48, 1, 11, 0),
    's2/bnb': (32, 40, 1, 11, 1),
    's2/plain': (32, 40, 1, 13, 1),
    's2/stats': (32, 40, 1, 13, 0),
    's2/stats_xf': (32, 40, 1, 11, 0),
    't1x1.res.c1.pf4/affine': (32, 4, 1, 0, 0),
    't1x1.res.c1.pf4/bnb': (32, 1, 1, 1, 1),
    't1x1.res.c1.pf4/plain': (32, 1, 1, 7, 1),
    't1x1.res.c1.pf4/stats': (32, 1, 1, 0, 0),
    't1x1.res.c1.pf4/stats_xf': (32, 1, 1, 2, 0),
    't1x1.res.c1.pf8/affine': (32, 4, 1, 6, 0),
    't1x1.res.c1.pf8/bnb': (32, 1, 1, 6, 1),
    't1x1.res.c1.pf8/plain': (32, 1, 1, 8, 1),
    't1x1.res.c1.pf8/stats': (32, 1, 1, 8, 0),
    't1x1.res.c1.pf8/stats_xf': (32, 1, 1, 6, 0),
    't1x1.res.c4.pf4/plain': (32, 1, 1, 5, 1),
    't1x1.res.c4.pf8/plain': (32, 1, 1, 10, 1),
    't1x1.ring.c1.pf4/stats': (84, 1, 1, 5, 0),
    't1x1.ring.c1.pf8/affine': (32, 4, 1, 10, 0),
    't1x1.ring.c1.pf8/bnb': (84, 1, 1, 6, 1),
    't1x1.ring.c1.pf8/plain': (84, 1, 1, 8, 1),
    't1x1.ring.c1.pf8/stats': (32, 1, 1, 10, 0),
    't1x1.ring.c1.pf8/stats_xf': (84, 1, 1, 6, 0),
    't1x1.ring.c4.pf4/plain': (32, 1, 1, 15, 1),
    't1x1.ring.c4.pf8/plain': (32, 2, 1, 15, 1),
    't1x1.two.c1.pf8/affine': (84, 8, 1, 10, 0),
    't1x1.two.c1.pf8/stats': (84, 8, 1, 10, 0),
    't1x1.two.c4.pf8/plain': (32, 220, 1, 15, 1),
    't2x1.res.c1.pf4/affine': (32, 16, 1, 0, 0),
    't2x1.res.c1.pf4/bnb': (32, 13, 1, 1, 1),
    't2x1.res.c1.pf4/plain': (32, 50, 1, 7, 1),
    't2x1.res.c1.pf4/stats': (32, 13, 1, 0, 0),
    't2x1.res.c1.pf4/stats_xf': (32, 13, 1, 2, 0),
    't2x1.res.c1.pf8/affine': (84, 4, 1, 1, 0),
    't2x1.res.c1.pf8/bnb': (84, 2, 1, 1, 1),
    't2x1.res.c1.pf8/plain': (32, 25, 1, 8, 1),
    't2x1.res.c1.pf8/stats': (84, 2, 1, 1, 0),
    't2x1.res.c1.pf8/stats_xf': (84, 2, 1, 2, 0),
    't2x1.res.c4.pf4/plain': (32, 50, 1, 5, 1),
    't2x1.res.c4.pf8/plain': (84, 8, 1, 5, 1),
    't2x1.ring.c1.pf4/affine': (84, 4, 1, 5, 0),
    't2x1.ring.c1.pf4/stats': (84, 4, 1, 5, 0),
    't2x1.ring.c1.pf8/affine': (84, 4, 1, 6, 0),
    't2x1.ring.c1.pf8/bnb': (84, 4, 1, 6, 1),
    't2x1.ring.c1.pf8/plain': (84, 4, 1, 8, 1),
    't2x1.ring.c1.pf8/stats': (84, 4, 1, 8, 0),
    't2x1.ring.c1.pf8/stats_xf': (84, 4, 1, 6, 0),
    't2x1.ring.c4.pf8/plain': (32, 100, 1, 10, 1),
    't2x1.two.c1.pf8/stats': (84, 13, 1, 10, 0),
    't2x2.two.c1.pf8/plain': (84, 100, 1, 7, 1),
    't3x1.res.c1.pf8/affine': (32, 64, 1, 6, 0),
    't3x1.res.c1.pf8/bnb': (32, 50, 1, 6, 1),
    't3x1.res.c1.pf8/plain': (32, 50, 1, 8, 1),
    't3x1.res.c1.pf8/stats': (32, 50, 1, 8, 0),
    't3x1.res.c1.pf8/stats_xf': (32, 50, 1, 6, 0),
    't3x1.ring.c1.pf4/affine': (84, 8, 1, 5, 0),
    't3x1.ring.c1.pf4/stats': (84, 8, 1, 5, 0),
    't3x1.ring.c1.pf8/affine': (84, 8, 1, 6, 0),
    't3x1.ring.c1.pf8/bnb': (84, 8, 1, 6, 1),
    't3x1.ring.c1.pf8/plain': (84, 8, 1, 8, 1),
    't3x1.ring.c1.pf8/stats': (84, 8, 1, 8, 0),
    't3x1.ring.c1.pf8/stats_xf': (84, 8, 1, 6, 0),
    't3x1.ring.c4.pf8/plain': (84, 29, 1, 10, 1),
    't3x2.two.c1.pf4/affine': (84, 80, 1, 5, 0),
    't3x2.two.c1.pf4/stats': (84, 100, 1, 5, 0),
    't3x2.two.c1.pf8/affine': (84, 80, 1, 6, 0),
    't3x2.two.c1.pf8/bnb': (84, 100, 1, 6, 1),
    't3x2.two.c1.pf8/plain': (84, 100, 1, 8, 1),
    't3x2.two.c1.pf8/stats': (84, 100, 1, 8, 0),
    't3x2.two.c1.pf8/stats_xf': (84, 100, 1, 6, 0),
    't4x1.ring.c1.pf8/affine': (32, 272, 1, 17, 0),
    't4x1.ring.c1.pf8/stats': (84, 34, 1, 17, 0),
    't4x1.two.c1.pf8/affine': (32, 352, 1, 17, 0),
    't5x1.ring.c1.pf8/affine': (32, 208, 1, 11, 0),
    't5x1.ring.c1.pf8/bnb': (84, 29, 1, 11, 1),
    't5x1.ring.c1.pf8/plain': (84, 29, 1, 13, 1),
    't5x1.ring.c1.pf8/stats': (84, 29, 1, 13, 0),
    't5x1.ring.c1.pf8/stats_xf': (84, 29, 1, 11, 0),
    't5x1.two.c1.pf8/affine': (32, 272, 1, 11, 0),
    't5x1.two.c1.pf8/bnb': (84, 37, 1, 11, 1),
    't5x1.two.c1.pf8/plain': (84, 37, 1, 13, 1),
    't5x1.two.c1.pf8/stats': (84, 37, 1, 13, 0),
    't5x1.two.c1.pf8/stats_xf': (84, 37, 1, 11, 0),
    't5x2.two.c1.pf8/affine': (84, 304, 1, 11, 0),
    't5x2.two.c1.pf8/bnb': (84, 300, 1, 11, 1),
    't5x2.two.c1.pf8/plain': (84, 300, 1, 13, 1),
    't5x2.two.c1.pf8/stats': (84, 300, 1, 13, 0),
    't5x2.two.c1.pf8/stats_xf': (84, 300, 1, 11, 0),
    'wg1x2.pf4.m0/plain': (32, 1, 1, 0, 2),
    'wg1x2.pf4/plain': (32, 48, 1, 0, 2),
    'wg1x2.pf8.m1/plain': (32, 1, 1, 1, 2),
    'wg1x2.pf8.m1/xf': (32, 1, 1, 2, 2),
    'wg1x3.pf4.m2/plain': (32, 1, 1, 17, 2),
    'wg1x3.pf4/plain': (84, 7, 1, 5, 2),
    'wg1x3.pf8.m3/plain': (32, 1, 1, 8, 2),
    'wg1x3.pf8.m3/xf': (32, 1, 1, 6, 2),
    'wg1x3.pf8/plain': (84, 7, 1, 18, 2),
    'wg1x3.pf8/xf': (84, 7, 1, 16, 2),
    'wg1x5.pf4/plain': (32, 48, 1, 13, 2),
    'wg1x5.pf4/xf': (32, 48, 1, 11, 2),
    'wg1x5.pf8/plain': (32, 48, 1, 18, 2),
    'wg1x5.pf8/xf': (32, 48, 1, 16, 2),
    'wg2x2.pf8/plain': (84, 10, 1, 1, 2),
    'wg2x2.pf8/xf': (84, 10, 1, 2, 2),
    'wg2x3.pf8/plain': (32, 48, 1, 8, 2),
    'wg2x3.pf8/xf': (32, 48, 1, 6, 2),
    'wg3x2.pf8/plain': (32, 48, 1, 1, 2),
    'wg3x2.pf8/xf': (32, 48, 1, 2, 2),
    'wgq3.pf8/plain': (84, 28, 1, 1, 2),
    'wgq3.pf8/xf': (84, 28, 1, 2, 2),
    'wx1x1/affine': (32, 112, 1, 13, 0),
    'wx1x1/bnb': (32, 110, 1, 11, 1),
    'wx1x1/plain': (32, 110, 1, 13, 1),
    'wx1x1/stats': (32, 110, 1, 13, 0),
    'wx3x1/affine': (32, 128, 1, 8, 0),
    'wx3x1/bnb': (32, 128, 1, 6, 1),
    'wx3x1/plain': (32, 128, 1, 8, 1),
    'wx3x1/stats': (32, 128, 1, 8, 0),
}


# how tests/test_gpu_layers.py runs the cases (tests/test_cpu_forms.py checks that together they are every key of COVERED and that the GPU
# file parametrizes its tests with exactly these lists): integer-exact conv cases, the input-transform cases (tier 2 against float64
# BatchNorm), the integer-exact weight-gradient cases
EXACT_CONV_KEYS = sorted(k for k in COVERED if not k.startswith("wg") and not k.endswith("/stats_xf"))
XF_KEYS = sorted(k for k in COVERED if k.endswith("/stats_xf"))
WGRAD_KEYS = sorted(k for k in COVERED if k.startswith("wg"))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi
    forms = enumerate_forms(ffi.lib())
    print("COVERED = {")
    for k in sorted(forms):
        hw, n, g, train, e = forms[k]
        print("    %r: (%d, %d, %d, %d, %d)," % (k, hw, n, g, e.layer, e.dir))
    print("}")
