"""Shared by tests/test_gpu_layers.py, tests/test_gpu_form_grid.py, tests/test_cpu_forms.py and tests/test_cpu_form_grid.py (a plain helper
module, not a conftest): the names of the kernel forms the network engine plans, the dense pass grid -- every pass the engine accepts by
default: 32 x 32, 50 x 50, 84 x 84 and 128 x 128 inputs, every train pass of 1 .. resnet._default_max_batch images in one and two BatchNorm
groups, every eval pass the engine's rounding can plan, plus the passes above the defaults that earlier cases rest on -- the single-layer
parity cases that cover those forms (COVERED), and the edge sizes of every form (EDGE_CASES).

A form is one compiled kernel the engine launches for a layer: the family and its template parameters (conv_t_kernel's MT, NT, weight
schedule, class count and patch prefetch depth; conv_q_kernel's pixel sets and prefetch depth; conv_s_kernel's pixel tiles; conv_w /
conv_wx's tiles; conv_wgrad_kernel's MTW, NTW and prefetch depth, its 4x4x1 form, the variants of conv_wgrad_multi_kernel), together
with the epilogue the engine runs it with (train forward: batch statistics, with the producer's BatchNorm + ReLU applied while staging
for the second convolution of a block; eval forward: folded BatchNorm; data gradient: plain, or feeding a BatchNorm backward)."""
import ctypes as C

FAMILIES = ("t", "q", "s", "w", "wx")
CONV_FAMILY = {0: "conv_t", 1: "conv_q", 2: "conv_s", 3: "conv_w", 4: "conv_wx"}

HW = (32, 50, 84, 128)
GROUPS = (1, 2)
# passes above the default max_batch (a user may raise model.max_batch): 300 train images and eval passes of 272 .. 416 at 32 x 32 and
# 84 x 84 -- the parity cases of the t5x2.* forms lie there (inside the defaults those forms are planned at 128 images of 128 x 128 only)
EXTRA_TRAIN = {32: (300,), 84: (300,)}
EXTRA_EVAL = {32: tuple(range(272, 417, 16)), 84: tuple(range(272, 417, 16))}


def max_batch(hw):
    from ocl_amd.resnet import _default_max_batch
    return _default_max_batch(hw, hw)


def eval_sizes(mb):
    """Every size ocl_net_forward plans an eval pass of N = 1 .. mb images at: N rounded up to 4 images up to 16, to 16 above, capped."""
    return sorted({min(mb, (N + 3) // 4 * 4 if N <= 16 else (N + 15) // 16 * 16) for N in range(1, mb + 1)})


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


def is_train(key):
    """The pass kind that plans a key: '/affine' is the eval forward's epilogue, every other one belongs to a train pass."""
    return 0 if key.endswith("/affine") else 1


def _entry_key(e, train):
    if e.dir == 0:
        return conv_key(e.form, ("stats_xf" if e.desc.xf else "stats") if train else "affine")
    if e.dir == 1:
        return conv_key(e.form, "bnb" if e.desc.bnb else "plain")
    return wgrad_key(e.wform, e.wdesc.xf_groups > 0, e.wg_merged)


def _net_entries(lib, hw, n, groups, train):
    """The ocl_test_net_form array of one pass (overwritten by the next call's owner: read or copy before going on)."""
    from ocl_amd import ffi
    cap = 256
    arr = (ffi.TestNetForm * cap)()
    cnt = lib.ocl_test_net_forms(hw, 20, n, groups, train, arr, cap)
    assert 0 < cnt <= cap, (hw, n, groups, train, cnt, lib.ocl_last_error())
    return arr, cnt


def net_forms(lib, hw, n, groups, train):
    """[(key, entry)] for every launch geometry of one pass, entry: the ocl_test_net_form (a copy)."""
    from ocl_amd import ffi
    arr, cnt = _net_entries(lib, hw, n, groups, train)
    out = []
    for i in range(cnt):
        e = ffi.TestNetForm()
        C.memmove(C.addressof(e), C.addressof(arr[i]), C.sizeof(e))
        out.append((_entry_key(e, train), e))
    return out


def dense_grid():
    """(hw, n, groups, train) of every pass the engine accepts with its default max_batch; an eval pass has one BatchNorm group."""
    for hw in HW:
        mb = max_batch(hw)
        for n in range(1, mb + 1):
            for g in GROUPS:
                if n % g == 0:
                    yield hw, n, g, 1
        for n in eval_sizes(mb):
            yield hw, n, 1, 0


def pass_grid():
    """The dense grid and the explicit passes above the defaults."""
    seen = set(dense_grid())
    for p in sorted(seen):
        yield p
    for hw in HW:
        for n in EXTRA_TRAIN.get(hw, ()):
            for g in GROUPS:
                if n % g == 0 and (hw, n, g, 1) not in seen:
                    yield hw, n, g, 1
        for n in EXTRA_EVAL.get(hw, ()):
            if (hw, n, 1, 0) not in seen:
                yield hw, n, 1, 0


def entry_cost(hw, n, e):
    d = e.desc if e.dir < 2 else e.wdesc
    return n * d.hin * d.win * max(d.cin, 4) * d.cout


_SWEEP = {}


def sweep(lib):
    """{key: [(hw, n, groups, layer, direction, cost, k)]}: every entry of every pass of pass_grid() (computed once per process)."""
    if "all" not in _SWEEP:
        out = {}
        for hw, n, g, train in pass_grid():
            arr, cnt = _net_entries(lib, hw, n, g, train)
            for i in range(cnt):
                e = arr[i]
                k = (e.desc if e.dir < 2 else e.wdesc).k
                out.setdefault(_entry_key(e, train), []).append((hw, n, g, e.layer, e.dir, entry_cost(hw, n, e), k))
        _SWEEP["all"] = out
    return _SWEEP["all"]


def _cheapest(rows):
    return min(rows, key=lambda r: (r[5], r[1], r[0], r[2], r[3], r[4]))


def enumerate_forms(lib):
    """{key: (hw, n, groups, layer, direction)}: every form of the grid with the cheapest pass / layer that reaches it."""
    return {k: _cheapest(rows)[:5] for k, rows in sweep(lib).items()}


def plans(lib, key, case):
    """Does the planner give `key` at case = (hw, n, groups, layer, direction)?"""
    hw, n, g, layer, dr = case
    train = is_train(key)
    arr, cnt = _net_entries(lib, hw, n, g, train)
    return any(arr[i].layer == layer and arr[i].dir == dr and _entry_key(arr[i], train) == key for i in range(cnt))


def find_case(lib, key, case):
    """The entry (a copy) of case = (hw, n, groups, layer, direction), which must plan `key`."""
    hw, n, g, layer, dr = case
    for k, e in net_forms(lib, hw, n, g, is_train(key)):
        if k == key and e.layer == layer and e.dir == dr:
            return e
    raise AssertionError("the planner no longer gives %s at %r: regenerate the tables of tests/layer_forms.py" % (key, case))


def parity_case(key):
    """The single-layer parity case of a key: COVERED, or datasets_cases.NEW_FORMS for the forms only the 50 / 128 inputs bring."""
    if key in COVERED:
        return COVERED[key]
    import datasets_cases
    return datasets_cases.NEW_FORMS[key]


def regenerate_covered(lib):
    """COVERED for the present planner: an entry whose case still plans its key stays; a form new to the grid (and absent from
    datasets_cases.NEW_FORMS) gets the cheapest pass / layer that reaches it; a form the grid no longer holds leaves."""
    import datasets_cases
    out = {}
    for k, case in enumerate_forms(lib).items():
        if k in datasets_cases.NEW_FORMS:
            continue
        out[k] = COVERED[k] if k in COVERED and plans(lib, k, COVERED[k]) else case
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# edge sizes
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_work(key, row):
    """Multiply-adds of float64 reference one case costs: the layer's (entry_cost * k * k) times the float64 convolutions its check
    computes (tier 1: one; the input-transform check: four -- result, magnitude, terms, ambiguity)."""
    return row[5] * row[6] * row[6] * (4 if key.endswith("/stats_xf") else 1)


def edge_cases(lib):
    """{key: [(kind, hw, n, groups, layer, direction)]} by the rule above EDGE_CASES."""
    out = {}
    for key, rows in sorted(sweep(lib).items()):
        base = parity_case(key)
        picked = []
        largest = min(rows, key=lambda r: (-r[1], r[5], r[0], r[2], r[3], r[4]))
        picked.append(("largest", largest[:5]))
        odd = [r for r in rows if (r[1] // r[2]) % 2 == 1]
        if odd:
            o = min(odd, key=lambda r: (-r[1], r[5], r[0], r[2], r[3], r[4]))
            if o[:5] != largest[:5]:
                picked.append(("odd", o[:5]))
        have = {base[0]} | {c[0] for _, c in picked}
        for hw in HW:
            at = [r for r in rows if r[0] == hw]
            if at and hw not in have:
                picked.append(("lattice", _cheapest(at)[:5]))
        picked = [(kind, c) for kind, c in picked if c != tuple(base)]
        if picked:
            out[key] = [(kind,) + c for kind, c in picked]
    return out


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
    't2x1.two.c1.pf8/bnb': (50, 100, 1, 16, 1),
    't2x1.two.c1.pf8/stats': (84, 13, 1, 10, 0),
    't2x1.two.c1.pf8/stats_xf': (50, 100, 2, 16, 0),
    't2x1.two.c4.pf8/plain': (32, 341, 1, 15, 1),
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
    't3x2.two.c1.pf4/stats_xf': (32, 512, 1, 6, 0),
    't3x2.two.c1.pf8/affine': (84, 80, 1, 6, 0),
    't3x2.two.c1.pf8/bnb': (84, 100, 1, 6, 1),
    't3x2.two.c1.pf8/plain': (84, 100, 1, 8, 1),
    't3x2.two.c1.pf8/stats': (84, 100, 1, 8, 0),
    't3x2.two.c1.pf8/stats_xf': (84, 100, 1, 6, 0),
    't4x1.ring.c1.pf8/affine': (32, 272, 1, 17, 0),
    't4x1.ring.c1.pf8/stats': (84, 34, 1, 17, 0),
    't4x1.two.c1.pf8/affine': (32, 352, 1, 17, 0),
    't4x1.two.c1.pf8/stats': (32, 338, 2, 17, 0),
    't5x1.res.c1.pf8/plain': (50, 200, 1, 15, 1),
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
    't5x1.two.c4.pf8/plain': (128, 65, 1, 15, 1),
    't5x2.two.c1.pf8/affine': (84, 304, 1, 11, 0),
    't5x2.two.c1.pf8/bnb': (84, 300, 1, 11, 1),
    't5x2.two.c1.pf8/plain': (84, 300, 1, 13, 1),
    't5x2.two.c1.pf8/stats': (84, 300, 1, 13, 0),
    't5x2.two.c1.pf8/stats_xf': (84, 300, 1, 11, 0),
    'wg1x2.pf4.m0/plain': (32, 1, 1, 0, 2),
    'wg1x2.pf4/plain': (32, 48, 1, 0, 2),
    'wg1x2.pf8.m1/plain': (32, 1, 1, 1, 2),
    'wg1x2.pf8.m1/xf': (32, 1, 1, 2, 2),
    'wg1x2.pf8/plain': (50, 26, 1, 1, 2),
    'wg1x2.pf8/xf': (50, 26, 1, 2, 2),
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


# The edge sizes of every form: key -> [(kind, hw, n, groups, layer index, direction)], generated by edge_cases() from the grid (regenerate
# with `python tests/layer_forms.py`; tests/test_cpu_form_grid.py re-derives the table from the planner).  Of all the entries of the grid that
# plan a key:
#   largest   the one with the most images (ties: the cheaper layer by entry_cost) -- the most tiles per workgroup, a saturated grid;
#   odd       the one with the most images among those with an odd number of images per BatchNorm group, if it is another one -- a
#             partial last tile, an odd image pairing;
#   lattice   for every input size at which the key is planned and neither its parity case (COVERED / datasets_cases.NEW_FORMS) nor the
#             two above lie: the cheapest entry at that size -- the 7 x 7 / 13 x 13 / 11 x 11 lattices of the other inputs.
# An entry that is the key's parity case is left out.  No case was replaced by a cheaper one: the dearest float64 reference of the table
# (ref_work: 3.0e10 multiply-adds, the input-transform check of layer 1 at 300 images of 84 x 84) takes under ten seconds on 16 threads.
EDGE_CASES = {
    'q1.pf12/affine': [('largest', 84, 416, 1, 1, 0), ('lattice', 50, 16, 1, 1, 0), ('lattice', 128, 4, 1, 1, 0)],
    'q1.pf12/bnb': [('largest', 84, 300, 1, 2, 1), ('odd', 50, 255, 1, 2, 1), ('lattice', 128, 2, 1, 1, 1)],
    'q1.pf12/plain': [('largest', 32, 512, 1, 7, 1), ('odd', 32, 511, 1, 7, 1), ('lattice', 50, 66, 1, 1, 1),
        ('lattice', 128, 11, 1, 1, 1)],
    'q1.pf12/stats': [('largest', 84, 300, 1, 1, 0), ('odd', 50, 255, 1, 1, 0), ('lattice', 128, 2, 1, 1, 0)],
    'q1.pf12/stats_xf': [('largest', 84, 300, 1, 2, 0), ('odd', 50, 255, 1, 2, 0), ('lattice', 128, 2, 1, 2, 0)],
    'q2.pf12/affine': [('largest', 32, 512, 1, 1, 0)],
    'q2.pf12/bnb': [('largest', 32, 512, 1, 2, 1), ('odd', 32, 511, 1, 2, 1)],
    'q2.pf12/plain': [('largest', 32, 512, 1, 1, 1), ('odd', 32, 511, 1, 1, 1)],
    'q2.pf12/stats': [('largest', 32, 512, 1, 1, 0), ('odd', 32, 511, 1, 1, 0)],
    'q2.pf12/stats_xf': [('largest', 32, 512, 1, 2, 0), ('odd', 32, 511, 1, 2, 0)],
    'q2.pf4/affine': [('largest', 32, 512, 1, 0, 0), ('lattice', 50, 32, 1, 0, 0), ('lattice', 84, 12, 1, 0, 0),
        ('lattice', 128, 4, 1, 0, 0)],
    'q2.pf4/stats': [('largest', 32, 512, 1, 0, 0), ('odd', 32, 511, 1, 0, 0), ('lattice', 50, 26, 1, 0, 0), ('lattice', 84, 10, 1, 0, 0),
        ('lattice', 128, 4, 1, 0, 0)],
    's1/affine': [('largest', 32, 512, 1, 16, 0), ('lattice', 50, 4, 1, 11, 0), ('lattice', 84, 4, 1, 11, 0),
        ('lattice', 128, 4, 1, 16, 0)],
    's1/bnb': [('largest', 32, 512, 1, 16, 1), ('odd', 32, 511, 1, 16, 1), ('lattice', 50, 1, 1, 11, 1), ('lattice', 84, 1, 1, 11, 1),
        ('lattice', 128, 1, 1, 11, 1)],
    's1/plain': [('largest', 32, 512, 1, 18, 1), ('odd', 32, 511, 1, 18, 1), ('lattice', 50, 1, 1, 13, 1), ('lattice', 84, 1, 1, 13, 1),
        ('lattice', 128, 1, 1, 13, 1)],
    's1/stats': [('largest', 32, 512, 1, 18, 0), ('odd', 32, 511, 1, 18, 0), ('lattice', 50, 1, 1, 13, 0), ('lattice', 84, 1, 1, 13, 0),
        ('lattice', 128, 1, 1, 13, 0)],
    's1/stats_xf': [('largest', 32, 512, 1, 16, 0), ('odd', 32, 511, 1, 16, 0), ('lattice', 50, 1, 1, 11, 0), ('lattice', 84, 1, 1, 11, 0),
        ('lattice', 128, 1, 1, 11, 0)],
    's2/affine': [('largest', 32, 192, 1, 11, 0), ('lattice', 50, 16, 1, 11, 0), ('lattice', 84, 8, 1, 11, 0),
        ('lattice', 128, 4, 1, 11, 0)],
    's2/bnb': [('largest', 32, 102, 1, 11, 1), ('odd', 32, 102, 2, 11, 1), ('lattice', 50, 15, 1, 11, 1), ('lattice', 84, 6, 1, 11, 1),
        ('lattice', 128, 3, 1, 11, 1)],
    's2/plain': [('largest', 50, 199, 1, 15, 1), ('lattice', 84, 6, 1, 13, 1), ('lattice', 128, 3, 1, 13, 1)],
    's2/stats': [('largest', 32, 102, 1, 13, 0), ('odd', 32, 102, 2, 13, 0), ('lattice', 50, 15, 1, 13, 0), ('lattice', 84, 6, 1, 13, 0),
        ('lattice', 128, 3, 1, 13, 0)],
    's2/stats_xf': [('largest', 32, 199, 1, 11, 0), ('lattice', 50, 15, 1, 11, 0), ('lattice', 84, 6, 1, 11, 0),
        ('lattice', 128, 3, 1, 11, 0)],
    't1x1.res.c1.pf4/affine': [('largest', 32, 12, 1, 0, 0), ('lattice', 50, 4, 1, 0, 0)],
    't1x1.res.c1.pf4/bnb': [('largest', 32, 12, 1, 1, 1), ('odd', 32, 11, 1, 1, 1)],
    't1x1.res.c1.pf4/plain': [('largest', 32, 49, 1, 7, 1), ('lattice', 50, 1, 1, 7, 1)],
    't1x1.res.c1.pf4/stats': [('largest', 32, 12, 1, 0, 0), ('odd', 32, 11, 1, 0, 0), ('lattice', 50, 1, 1, 0, 0),
        ('lattice', 84, 1, 1, 0, 0)],
    't1x1.res.c1.pf4/stats_xf': [('largest', 32, 12, 1, 2, 0), ('odd', 32, 11, 1, 2, 0)],
    't1x1.res.c1.pf8/affine': [('largest', 32, 16, 1, 6, 0), ('lattice', 50, 4, 1, 1, 0)],
    't1x1.res.c1.pf8/bnb': [('largest', 32, 24, 1, 6, 1), ('odd', 32, 23, 1, 6, 1), ('lattice', 50, 1, 1, 1, 1),
        ('lattice', 84, 1, 1, 1, 1)],
    't1x1.res.c1.pf8/plain': [('largest', 32, 99, 1, 12, 1), ('lattice', 50, 1, 1, 8, 1), ('lattice', 84, 1, 1, 7, 1),
        ('lattice', 128, 1, 1, 7, 1)],
    't1x1.res.c1.pf8/stats': [('largest', 32, 24, 1, 8, 0), ('odd', 32, 23, 1, 8, 0), ('lattice', 50, 1, 1, 1, 0),
        ('lattice', 84, 1, 1, 1, 0), ('lattice', 128, 1, 1, 7, 0)],
    't1x1.res.c1.pf8/stats_xf': [('largest', 32, 24, 1, 6, 0), ('odd', 32, 23, 1, 6, 0), ('lattice', 50, 1, 1, 2, 0),
        ('lattice', 84, 1, 1, 2, 0)],
    't1x1.res.c4.pf4/plain': [('largest', 32, 49, 1, 5, 1)],
    't1x1.res.c4.pf8/plain': [('largest', 32, 99, 1, 10, 1), ('lattice', 50, 1, 1, 5, 1), ('lattice', 84, 1, 1, 5, 1),
        ('lattice', 128, 1, 1, 5, 1)],
    't1x1.ring.c1.pf4/affine': [('largest', 50, 8, 1, 5, 0), ('lattice', 128, 4, 1, 10, 0)],
    't1x1.ring.c1.pf4/stats': [('largest', 50, 9, 1, 5, 0), ('lattice', 128, 1, 1, 5, 0)],
    't1x1.ring.c1.pf8/affine': [('largest', 32, 96, 1, 17, 0), ('lattice', 50, 4, 1, 10, 0), ('lattice', 84, 4, 1, 10, 0),
        ('lattice', 128, 4, 1, 12, 0)],
    't1x1.ring.c1.pf8/bnb': [('largest', 84, 3, 1, 6, 1), ('lattice', 128, 1, 1, 6, 1)],
    't1x1.ring.c1.pf8/plain': [('largest', 32, 264, 1, 17, 1), ('odd', 32, 263, 1, 17, 1), ('lattice', 50, 1, 1, 10, 1),
        ('lattice', 128, 1, 1, 8, 1)],
    't1x1.ring.c1.pf8/stats': [('largest', 32, 100, 1, 17, 0), ('odd', 32, 99, 1, 17, 0), ('lattice', 50, 1, 1, 10, 0),
        ('lattice', 84, 1, 1, 8, 0), ('lattice', 128, 1, 1, 8, 0)],
    't1x1.ring.c1.pf8/stats_xf': [('largest', 84, 3, 1, 6, 0), ('lattice', 128, 1, 1, 6, 0)],
    't1x1.ring.c4.pf8/plain': [('largest', 32, 204, 1, 15, 1), ('odd', 32, 203, 1, 15, 1), ('lattice', 84, 1, 1, 10, 1),
        ('lattice', 128, 1, 1, 10, 1)],
    't1x1.two.c1.pf8/affine': [('largest', 32, 144, 1, 17, 0)],
    't1x1.two.c1.pf8/stats': [('largest', 32, 156, 1, 17, 0), ('odd', 32, 155, 1, 17, 0)],
    't1x1.two.c4.pf8/plain': [('largest', 32, 264, 1, 15, 1), ('odd', 32, 263, 1, 15, 1), ('lattice', 128, 13, 1, 15, 1)],
    't2x1.res.c1.pf4/affine': [('largest', 32, 48, 1, 0, 0), ('lattice', 50, 8, 1, 0, 0), ('lattice', 84, 4, 1, 0, 0)],
    't2x1.res.c1.pf4/bnb': [('largest', 32, 63, 1, 1, 1)],
    't2x1.res.c1.pf4/plain': [('largest', 32, 127, 1, 7, 1), ('lattice', 50, 20, 1, 7, 1)],
    't2x1.res.c1.pf4/stats': [('largest', 32, 63, 1, 0, 0), ('lattice', 50, 5, 1, 0, 0), ('lattice', 84, 2, 1, 0, 0),
        ('lattice', 128, 1, 1, 0, 0)],
    't2x1.res.c1.pf4/stats_xf': [('largest', 32, 63, 1, 2, 0)],
    't2x1.res.c1.pf8/affine': [('largest', 32, 48, 1, 6, 0), ('lattice', 50, 8, 1, 1, 0)],
    't2x1.res.c1.pf8/bnb': [('largest', 32, 49, 1, 6, 1), ('lattice', 50, 5, 1, 1, 1)],
    't2x1.res.c1.pf8/plain': [('largest', 32, 199, 1, 12, 1), ('lattice', 50, 10, 1, 8, 1), ('lattice', 84, 8, 1, 7, 1),
        ('lattice', 128, 4, 1, 7, 1)],
    't2x1.res.c1.pf8/stats': [('largest', 32, 49, 1, 8, 0), ('lattice', 50, 5, 1, 1, 0), ('lattice', 128, 2, 1, 7, 0)],
    't2x1.res.c1.pf8/stats_xf': [('largest', 32, 49, 1, 6, 0), ('lattice', 50, 5, 1, 2, 0)],
    't2x1.res.c4.pf4/plain': [('largest', 32, 512, 1, 5, 1), ('odd', 32, 511, 1, 5, 1)],
    't2x1.res.c4.pf8/plain': [('largest', 84, 300, 1, 5, 1), ('odd', 50, 255, 1, 5, 1), ('lattice', 128, 4, 1, 5, 1)],
    't2x1.ring.c1.pf4/affine': [('largest', 50, 16, 1, 5, 0)],
    't2x1.ring.c1.pf4/stats': [('largest', 50, 19, 1, 5, 0), ('lattice', 128, 1, 1, 1, 0)],
    't2x1.ring.c1.pf8/affine': [('largest', 32, 192, 1, 17, 0), ('lattice', 50, 32, 1, 10, 0), ('lattice', 128, 12, 1, 17, 0)],
    't2x1.ring.c1.pf8/bnb': [('largest', 84, 99, 1, 16, 1), ('lattice', 128, 2, 1, 6, 1)],
    't2x1.ring.c1.pf8/plain': [('largest', 32, 396, 1, 17, 1), ('odd', 32, 395, 1, 17, 1), ('lattice', 50, 34, 1, 10, 1),
        ('lattice', 128, 2, 1, 8, 1)],
    't2x1.ring.c1.pf8/stats': [('largest', 50, 199, 1, 18, 0), ('lattice', 32, 67, 1, 10, 0), ('lattice', 128, 2, 1, 8, 0)],
    't2x1.ring.c1.pf8/stats_xf': [('largest', 50, 199, 1, 16, 0), ('lattice', 128, 2, 1, 6, 0)],
    't2x1.ring.c4.pf8/plain': [('largest', 32, 340, 1, 15, 1), ('odd', 32, 339, 1, 15, 1), ('lattice', 84, 15, 1, 10, 1),
        ('lattice', 128, 7, 1, 10, 1)],
    't2x1.two.c1.pf8/bnb': [('largest', 50, 199, 1, 16, 1)],
    't2x1.two.c1.pf8/stats': [('largest', 84, 14, 1, 10, 0), ('odd', 84, 14, 2, 10, 0)],
    't2x1.two.c1.pf8/stats_xf': [('largest', 50, 198, 2, 16, 0)],
    't2x1.two.c4.pf8/plain': [('largest', 32, 396, 1, 15, 1), ('odd', 32, 395, 1, 15, 1), ('lattice', 128, 22, 1, 15, 1)],
    't2x2.two.c1.pf8/plain': [('largest', 84, 300, 1, 7, 1), ('odd', 84, 255, 1, 7, 1)],
    't3x1.res.c1.pf8/affine': [('largest', 32, 496, 1, 6, 0), ('lattice', 50, 32, 1, 6, 0), ('lattice', 128, 4, 1, 7, 0)],
    't3x1.res.c1.pf8/bnb': [('largest', 32, 127, 1, 6, 1)],
    't3x1.res.c1.pf8/plain': [('largest', 32, 512, 1, 12, 1), ('odd', 32, 511, 1, 12, 1), ('lattice', 50, 20, 1, 8, 1),
        ('lattice', 84, 29, 1, 12, 1), ('lattice', 128, 13, 1, 12, 1)],
    't3x1.res.c1.pf8/stats': [('largest', 32, 511, 1, 5, 0), ('lattice', 50, 20, 1, 8, 0), ('lattice', 128, 4, 1, 7, 0)],
    't3x1.res.c1.pf8/stats_xf': [('largest', 32, 511, 1, 6, 0), ('lattice', 50, 20, 1, 6, 0)],
    't3x1.ring.c1.pf4/affine': [('largest', 50, 192, 1, 5, 0), ('lattice', 128, 4, 1, 5, 0)],
    't3x1.ring.c1.pf4/bnb': [('largest', 50, 204, 1, 6, 1), ('odd', 50, 203, 1, 6, 1)],
    't3x1.ring.c1.pf4/stats': [('largest', 50, 204, 1, 5, 0), ('odd', 50, 203, 1, 5, 0), ('lattice', 128, 4, 1, 5, 0)],
    't3x1.ring.c1.pf4/stats_xf': [('largest', 50, 204, 2, 6, 0), ('odd', 50, 202, 2, 6, 0)],
    't3x1.ring.c1.pf8/affine': [('largest', 32, 256, 1, 17, 0), ('lattice', 50, 48, 1, 10, 0), ('lattice', 128, 4, 1, 6, 0)],
    't3x1.ring.c1.pf8/bnb': [('largest', 84, 73, 1, 6, 1), ('lattice', 128, 4, 1, 6, 1)],
    't3x1.ring.c1.pf8/plain': [('largest', 32, 512, 1, 17, 1), ('odd', 32, 511, 1, 17, 1), ('lattice', 50, 67, 1, 10, 1),
        ('lattice', 128, 4, 1, 8, 1)],
    't3x1.ring.c1.pf8/stats': [('largest', 32, 264, 1, 17, 0), ('odd', 32, 263, 1, 17, 0), ('lattice', 50, 34, 1, 10, 0),
        ('lattice', 128, 4, 1, 8, 0)],
    't3x1.ring.c1.pf8/stats_xf': [('largest', 84, 73, 1, 6, 0), ('lattice', 128, 4, 1, 6, 0)],
    't3x1.ring.c4.pf8/plain': [('largest', 32, 512, 1, 10, 1), ('odd', 32, 511, 1, 10, 1), ('lattice', 128, 13, 1, 10, 1)],
    't3x2.two.c1.pf4/affine': [('largest', 32, 512, 1, 6, 0), ('lattice', 50, 208, 1, 5, 0), ('lattice', 128, 32, 1, 5, 0)],
    't3x2.two.c1.pf4/stats': [('largest', 32, 512, 1, 5, 0), ('odd', 50, 255, 1, 5, 0), ('lattice', 128, 32, 1, 5, 0)],
    't3x2.two.c1.pf8/affine': [('largest', 84, 416, 1, 6, 0), ('lattice', 50, 208, 1, 6, 0), ('lattice', 128, 32, 1, 6, 0)],
    't3x2.two.c1.pf8/bnb': [('largest', 84, 300, 1, 6, 1), ('odd', 50, 255, 1, 6, 1), ('lattice', 128, 32, 1, 6, 1)],
    't3x2.two.c1.pf8/plain': [('largest', 84, 300, 1, 8, 1), ('odd', 50, 255, 1, 8, 1), ('lattice', 128, 32, 1, 8, 1)],
    't3x2.two.c1.pf8/stats': [('largest', 84, 300, 1, 8, 0), ('odd', 50, 255, 1, 8, 0), ('lattice', 128, 32, 1, 8, 0)],
    't3x2.two.c1.pf8/stats_xf': [('largest', 84, 300, 1, 6, 0), ('odd', 50, 255, 1, 6, 0), ('lattice', 128, 32, 1, 6, 0)],
    't4x1.ring.c1.pf8/affine': [('largest', 32, 336, 1, 17, 0), ('lattice', 50, 80, 1, 17, 0), ('lattice', 84, 48, 1, 17, 0)],
    't4x1.ring.c1.pf8/stats': [('largest', 32, 340, 1, 17, 0), ('odd', 32, 339, 1, 17, 0), ('lattice', 50, 67, 1, 17, 0),
        ('lattice', 128, 17, 1, 17, 0)],
    't4x1.two.c1.pf8/affine': [('largest', 32, 384, 1, 17, 0)],
    't4x1.two.c1.pf8/stats': [('largest', 32, 396, 1, 17, 0), ('odd', 32, 395, 1, 17, 0)],
    't5x1.res.c1.pf8/plain': [('largest', 50, 256, 1, 15, 1), ('odd', 50, 255, 1, 15, 1)],
    't5x1.ring.c1.pf4/stats': [('odd', 128, 15, 1, 10, 0)],
    't5x1.ring.c1.pf8/affine': [('largest', 32, 512, 1, 17, 0), ('lattice', 50, 80, 1, 11, 0), ('lattice', 84, 32, 1, 11, 0),
        ('lattice', 128, 16, 1, 11, 0)],
    't5x1.ring.c1.pf8/bnb': [('largest', 50, 85, 1, 11, 1), ('lattice', 128, 13, 1, 11, 1)],
    't5x1.ring.c1.pf8/plain': [('largest', 50, 256, 1, 15, 1), ('odd', 50, 255, 1, 15, 1), ('lattice', 128, 13, 1, 13, 1)],
    't5x1.ring.c1.pf8/stats': [('largest', 32, 512, 1, 17, 0), ('odd', 32, 511, 1, 17, 0), ('lattice', 50, 67, 1, 13, 0),
        ('lattice', 128, 13, 1, 13, 0)],
    't5x1.ring.c1.pf8/stats_xf': [('largest', 32, 256, 1, 11, 0), ('odd', 32, 255, 1, 11, 0), ('lattice', 50, 67, 1, 11, 0),
        ('lattice', 128, 13, 1, 11, 0)],
    't5x1.ring.c4.pf8/plain': [('largest', 128, 64, 1, 15, 1), ('odd', 128, 63, 1, 15, 1)],
    't5x1.two.c1.pf4/affine': [('largest', 128, 112, 1, 10, 0)],
    't5x1.two.c1.pf4/stats': [('largest', 128, 127, 1, 10, 0)],
    't5x1.two.c1.pf8/affine': [('largest', 32, 512, 1, 11, 0), ('lattice', 50, 96, 1, 11, 0), ('lattice', 84, 48, 1, 11, 0),
        ('lattice', 128, 32, 1, 11, 0)],
    't5x1.two.c1.pf8/bnb': [('largest', 84, 300, 1, 16, 1), ('odd', 50, 255, 1, 11, 1), ('lattice', 128, 17, 1, 11, 1)],
    't5x1.two.c1.pf8/plain': [('largest', 84, 300, 1, 18, 1), ('odd', 50, 255, 1, 13, 1), ('lattice', 128, 17, 1, 13, 1)],
    't5x1.two.c1.pf8/stats': [('largest', 32, 512, 1, 10, 0), ('odd', 32, 511, 1, 10, 0), ('lattice', 50, 86, 1, 13, 0),
        ('lattice', 128, 17, 1, 13, 0)],
    't5x1.two.c1.pf8/stats_xf': [('largest', 32, 512, 1, 11, 0), ('odd', 32, 511, 1, 11, 0), ('lattice', 50, 86, 1, 11, 0),
        ('lattice', 128, 17, 1, 11, 0)],
    't5x1.two.c4.pf8/plain': [('largest', 128, 128, 1, 15, 1), ('odd', 128, 127, 1, 15, 1)],
    't5x2.two.c1.pf8/affine': [('largest', 84, 416, 1, 11, 0), ('lattice', 128, 128, 1, 11, 0)],
    't5x2.two.c1.pf8/bnb': [('lattice', 128, 128, 1, 11, 1)],
    't5x2.two.c1.pf8/plain': [('lattice', 128, 128, 1, 13, 1)],
    't5x2.two.c1.pf8/stats': [('lattice', 128, 128, 1, 13, 0)],
    't5x2.two.c1.pf8/stats_xf': [('lattice', 128, 128, 1, 11, 0)],
    'wg1x2.pf4.m0/plain': [('largest', 32, 47, 1, 0, 2), ('lattice', 50, 1, 1, 0, 2), ('lattice', 84, 1, 1, 0, 2),
        ('lattice', 128, 1, 1, 0, 2)],
    'wg1x2.pf4.m0/xf': [('largest', 128, 2, 1, 2, 2), ('odd', 128, 2, 2, 2, 2)],
    'wg1x2.pf4/plain': [('largest', 32, 512, 1, 0, 2), ('odd', 32, 511, 1, 0, 2), ('lattice', 50, 20, 1, 0, 2), ('lattice', 84, 7, 1, 0, 2),
        ('lattice', 128, 3, 1, 0, 2)],
    'wg1x2.pf4/xf': [('largest', 128, 128, 1, 2, 2), ('odd', 128, 127, 1, 2, 2)],
    'wg1x2.pf8.m1/plain': [('largest', 32, 47, 1, 1, 2), ('lattice', 50, 1, 1, 1, 2), ('lattice', 84, 1, 1, 1, 2)],
    'wg1x2.pf8.m1/xf': [('largest', 32, 47, 1, 2, 2), ('lattice', 50, 1, 1, 2, 2), ('lattice', 84, 1, 1, 2, 2)],
    'wg1x2.pf8/plain': [('largest', 32, 71, 1, 1, 2)],
    'wg1x2.pf8/xf': [('largest', 32, 71, 1, 2, 2)],
    'wg1x3.pf4.m2/plain': [('largest', 84, 6, 1, 5, 2), ('odd', 84, 6, 2, 5, 2), ('lattice', 128, 1, 1, 5, 2)],
    'wg1x3.pf4/plain': [('largest', 84, 300, 1, 5, 2), ('odd', 84, 255, 1, 5, 2), ('lattice', 128, 3, 1, 5, 2)],
    'wg1x3.pf8.m3/plain': [('largest', 32, 47, 1, 8, 2), ('lattice', 50, 1, 1, 8, 2), ('lattice', 84, 1, 1, 8, 2),
        ('lattice', 128, 1, 1, 8, 2)],
    'wg1x3.pf8.m3/xf': [('largest', 32, 47, 1, 6, 2), ('lattice', 50, 1, 1, 6, 2), ('lattice', 84, 1, 1, 6, 2),
        ('lattice', 128, 1, 1, 6, 2)],
    'wg1x3.pf8/plain': [('largest', 32, 512, 1, 7, 2), ('odd', 32, 511, 1, 7, 2), ('lattice', 50, 22, 1, 13, 2),
        ('lattice', 128, 3, 1, 18, 2)],
    'wg1x3.pf8/xf': [('largest', 32, 190, 1, 6, 2), ('odd', 32, 190, 2, 6, 2), ('lattice', 50, 22, 1, 11, 2),
        ('lattice', 128, 3, 1, 16, 2)],
    'wg1x5.pf4/plain': [('largest', 32, 512, 1, 13, 2), ('odd', 32, 511, 1, 13, 2), ('lattice', 50, 48, 1, 13, 2),
        ('lattice', 128, 48, 1, 18, 2)],
    'wg1x5.pf4/xf': [('largest', 32, 512, 1, 11, 2), ('odd', 32, 511, 1, 11, 2), ('lattice', 50, 48, 1, 11, 2),
        ('lattice', 128, 48, 1, 16, 2)],
    'wg1x5.pf8/plain': [('largest', 32, 512, 1, 18, 2), ('odd', 32, 511, 1, 18, 2), ('lattice', 50, 48, 1, 18, 2),
        ('lattice', 84, 48, 1, 13, 2), ('lattice', 128, 48, 1, 13, 2)],
    'wg1x5.pf8/xf': [('largest', 32, 512, 1, 16, 2), ('odd', 32, 511, 1, 16, 2), ('lattice', 50, 48, 1, 16, 2),
        ('lattice', 84, 48, 1, 11, 2), ('lattice', 128, 48, 1, 11, 2)],
    'wg2x2.pf8/plain': [('largest', 32, 143, 1, 1, 2), ('lattice', 50, 29, 1, 1, 2)],
    'wg2x2.pf8/xf': [('largest', 32, 143, 1, 2, 2), ('lattice', 50, 29, 1, 2, 2)],
    'wg2x3.pf8/plain': [('largest', 32, 512, 1, 8, 2), ('odd', 32, 511, 1, 8, 2), ('lattice', 50, 20, 1, 8, 2), ('lattice', 84, 7, 1, 8, 2),
        ('lattice', 128, 3, 1, 8, 2)],
    'wg2x3.pf8/xf': [('largest', 32, 512, 1, 6, 2), ('odd', 32, 511, 1, 6, 2), ('lattice', 50, 20, 1, 6, 2), ('lattice', 84, 7, 1, 6, 2),
        ('lattice', 128, 3, 1, 6, 2)],
    'wg3x2.pf8/plain': [('largest', 32, 191, 1, 1, 2), ('lattice', 50, 20, 1, 1, 2), ('lattice', 84, 7, 1, 1, 2)],
    'wg3x2.pf8/xf': [('largest', 32, 191, 1, 2, 2), ('lattice', 50, 20, 1, 2, 2), ('lattice', 84, 7, 1, 2, 2)],
    'wgq3.pf8/plain': [('largest', 32, 512, 1, 1, 2), ('odd', 32, 511, 1, 1, 2), ('lattice', 50, 77, 1, 1, 2)],
    'wgq3.pf8/xf': [('largest', 32, 512, 1, 2, 2), ('odd', 32, 511, 1, 2, 2), ('lattice', 50, 77, 1, 2, 2)],
    'wx1x1/affine': [('largest', 32, 512, 1, 13, 0)],
    'wx1x1/bnb': [('largest', 32, 512, 1, 11, 1), ('odd', 32, 511, 1, 11, 1)],
    'wx1x1/plain': [('largest', 32, 512, 1, 13, 1), ('odd', 32, 511, 1, 13, 1)],
    'wx1x1/stats': [('largest', 32, 512, 1, 13, 0), ('odd', 32, 511, 1, 13, 0)],
    'wx3x1/affine': [('largest', 32, 512, 1, 8, 0)],
    'wx3x1/bnb': [('largest', 32, 512, 1, 6, 1), ('odd', 32, 511, 1, 6, 1)],
    'wx3x1/plain': [('largest', 32, 512, 1, 8, 1), ('odd', 32, 511, 1, 8, 1)],
    'wx3x1/stats': [('largest', 32, 512, 1, 8, 0), ('odd', 32, 511, 1, 8, 0)],
}


# ---------------------------------------------------------------------------------------------------------------------------------
# passes of three to eight BatchNorm groups
# ---------------------------------------------------------------------------------------------------------------------------------
# model.forward_views hands len(views) to the engine as the group count and ocl_net_forward takes up to eight.  GROUPS, COVERED and EDGE_CASES
# above stay the one- and two-group grid; this is a second sweep beside it.
MANY_GROUPS = (3, 4, 5, 6, 7, 8)
GROUP_EPILOGUES = ("/stats", "/stats_xf", "/xf")     # the forms whose epilogue or staging reads a tile's group


def group_grid():
    """(hw, n, groups, 1) of every train pass of g .. max_batch(hw) images in g = 3 .. 8 equal BatchNorm groups."""
    for hw in HW:
        mb = max_batch(hw)
        for n in range(1, mb + 1):
            for g in MANY_GROUPS:
                if n >= g and n % g == 0:
                    yield hw, n, g, 1


def group_sweep(lib):
    """sweep() over group_grid()."""
    if "groups" not in _SWEEP:
        out = {}
        for hw, n, g, train in group_grid():
            arr, cnt = _net_entries(lib, hw, n, g, train)
            for i in range(cnt):
                e = arr[i]
                k = (e.desc if e.dir < 2 else e.wdesc).k
                out.setdefault(_entry_key(e, train), []).append((hw, n, g, e.layer, e.dir, entry_cost(hw, n, e), k))
        _SWEEP["groups"] = out
    return _SWEEP["groups"]


def group_cases(lib):
    """{key: [(kind, hw, n, groups, layer, direction)]} by the rule above GROUP_CASES."""
    out = {}
    for key, rows in sorted(group_sweep(lib).items()):
        gmax = max(r[2] for r in rows)
        picked = [("most", _cheapest([r for r in rows if r[2] == gmax])[:5])]
        if key.endswith(GROUP_EPILOGUES):
            c = _cheapest(rows)[:5]
            if c != picked[0][1]:
                picked.append(("cheapest", c))
        out[key] = [(kind,) + c for kind, c in picked]
    return out


# The many-group cases of every form a pass of 3 .. 8 BatchNorm groups plans: key -> [(kind, hw, n, groups, layer index, direction)], generated
# by group_cases() from group_grid() (regenerate with `python tests/layer_forms.py groups`; tests/test_cpu_form_grid.py re-derives the table
# from the planner).  Of all the entries of that grid that plan a key:
#   most      the cheapest (entry_cost) among those with the most groups -- the most group boundaries inside a workgroup's tile range, the
#             highest index into the per-group tables;
#   cheapest  for the forms whose epilogue or staging reads the group (GROUP_EPILOGUES), the cheapest of all when it is another one -- the
#             fewest images per group the form is planned at.
# Being the cheapest with its property, no case can be replaced by a cheaper one; the bounds of ref_work are those of EDGE_CASES.
GROUP_CASES = {
    'q1.pf12/plain': [('most', 50, 16, 8, 1, 1)],
    'q1.pf12/stats': [('most', 50, 16, 8, 1, 0), ('cheapest', 50, 14, 7, 1, 0)],
    'q1.pf12/stats_xf': [('most', 50, 16, 8, 2, 0), ('cheapest', 50, 14, 7, 2, 0)],
    'q2.pf12/plain': [('most', 32, 64, 8, 1, 1)],
    'q2.pf12/stats': [('most', 32, 64, 8, 1, 0), ('cheapest', 32, 64, 4, 1, 0)],
    'q2.pf12/stats_xf': [('most', 32, 64, 8, 2, 0), ('cheapest', 32, 64, 4, 2, 0)],
    'q2.pf4/stats': [('most', 32, 64, 8, 0, 0), ('cheapest', 128, 4, 4, 0, 0)],
    's1/plain': [('most', 32, 8, 8, 11, 1)],
    's1/stats': [('most', 32, 8, 8, 13, 0), ('cheapest', 32, 3, 3, 13, 0)],
    's1/stats_xf': [('most', 32, 8, 8, 11, 0), ('cheapest', 32, 3, 3, 11, 0)],
    's2/plain': [('most', 32, 40, 8, 11, 1)],
    's2/stats': [('most', 32, 40, 8, 13, 0), ('cheapest', 50, 15, 3, 13, 0)],
    's2/stats_xf': [('most', 32, 40, 8, 11, 0), ('cheapest', 50, 15, 3, 11, 0)],
    't1x1.res.c1.pf4/plain': [('most', 32, 8, 8, 1, 1)],
    't1x1.res.c1.pf4/stats': [('most', 32, 8, 8, 0, 0), ('cheapest', 32, 3, 3, 0, 0)],
    't1x1.res.c1.pf4/stats_xf': [('most', 32, 8, 8, 2, 0), ('cheapest', 32, 3, 3, 2, 0)],
    't1x1.res.c1.pf8/plain': [('most', 32, 8, 8, 6, 1)],
    't1x1.res.c1.pf8/stats': [('most', 32, 8, 8, 8, 0), ('cheapest', 32, 3, 3, 8, 0)],
    't1x1.res.c1.pf8/stats_xf': [('most', 32, 8, 8, 6, 0), ('cheapest', 32, 3, 3, 6, 0)],
    't1x1.res.c4.pf4/plain': [('most', 32, 8, 8, 5, 1)],
    't1x1.res.c4.pf8/plain': [('most', 32, 8, 8, 10, 1)],
    't1x1.ring.c1.pf4/stats': [('most', 50, 8, 8, 5, 0), ('cheapest', 50, 3, 3, 5, 0)],
    't1x1.ring.c1.pf8/plain': [('most', 32, 8, 8, 17, 1)],
    't1x1.ring.c1.pf8/stats': [('most', 32, 8, 8, 10, 0), ('cheapest', 32, 3, 3, 10, 0)],
    't1x1.ring.c1.pf8/stats_xf': [('most', 84, 3, 3, 6, 0)],
    't1x1.ring.c4.pf8/plain': [('most', 32, 8, 8, 15, 1)],
    't1x1.two.c1.pf8/stats': [('most', 84, 8, 8, 10, 0), ('cheapest', 84, 8, 4, 10, 0)],
    't1x1.two.c4.pf8/plain': [('most', 32, 208, 8, 15, 1)],
    't2x1.res.c1.pf4/plain': [('most', 32, 16, 8, 1, 1)],
    't2x1.res.c1.pf4/stats': [('most', 32, 16, 8, 0, 0), ('cheapest', 50, 5, 5, 0, 0)],
    't2x1.res.c1.pf4/stats_xf': [('most', 32, 16, 8, 2, 0), ('cheapest', 32, 14, 7, 2, 0)],
    't2x1.res.c1.pf8/plain': [('most', 50, 8, 8, 1, 1)],
    't2x1.res.c1.pf8/stats': [('most', 50, 8, 8, 1, 0), ('cheapest', 50, 5, 5, 1, 0)],
    't2x1.res.c1.pf8/stats_xf': [('most', 50, 8, 8, 2, 0), ('cheapest', 50, 5, 5, 2, 0)],
    't2x1.res.c4.pf4/plain': [('most', 32, 56, 8, 5, 1)],
    't2x1.res.c4.pf8/plain': [('most', 84, 8, 8, 5, 1)],
    't2x1.ring.c1.pf4/stats': [('most', 50, 16, 8, 5, 0), ('cheapest', 50, 10, 5, 5, 0)],
    't2x1.ring.c1.pf8/plain': [('most', 50, 40, 8, 10, 1)],
    't2x1.ring.c1.pf8/stats': [('most', 50, 24, 8, 10, 0), ('cheapest', 84, 4, 4, 8, 0)],
    't2x1.ring.c1.pf8/stats_xf': [('most', 84, 7, 7, 6, 0), ('cheapest', 84, 4, 4, 6, 0)],
    't2x1.ring.c4.pf8/plain': [('most', 32, 104, 8, 10, 1)],
    't2x1.two.c1.pf8/stats': [('most', 84, 14, 7, 10, 0)],
    't2x1.two.c1.pf8/stats_xf': [('most', 50, 104, 8, 16, 0), ('cheapest', 50, 100, 4, 16, 0)],
    't2x1.two.c4.pf8/plain': [('most', 32, 344, 8, 15, 1)],
    't2x2.two.c1.pf8/plain': [('most', 84, 80, 8, 7, 1)],
    't3x1.res.c1.pf8/plain': [('most', 32, 56, 8, 6, 1)],
    't3x1.res.c1.pf8/stats': [('most', 32, 56, 8, 8, 0), ('cheapest', 50, 20, 4, 8, 0)],
    't3x1.res.c1.pf8/stats_xf': [('most', 32, 56, 8, 6, 0), ('cheapest', 32, 50, 5, 6, 0)],
    't3x1.ring.c1.pf4/stats': [('most', 84, 8, 8, 5, 0), ('cheapest', 50, 20, 4, 5, 0)],
    't3x1.ring.c1.pf4/stats_xf': [('most', 50, 24, 8, 6, 0), ('cheapest', 50, 20, 4, 6, 0)],
    't3x1.ring.c1.pf8/plain': [('most', 84, 8, 8, 6, 1)],
    't3x1.ring.c1.pf8/stats': [('most', 84, 8, 8, 8, 0), ('cheapest', 84, 8, 4, 8, 0)],
    't3x1.ring.c1.pf8/stats_xf': [('most', 84, 8, 8, 6, 0), ('cheapest', 84, 8, 4, 6, 0)],
    't3x1.ring.c4.pf8/plain': [('most', 32, 200, 8, 10, 1)],
    't3x2.two.c1.pf4/stats': [('most', 50, 208, 8, 5, 0), ('cheapest', 50, 205, 5, 5, 0)],
    't3x2.two.c1.pf4/stats_xf': [('most', 32, 512, 8, 6, 0), ('cheapest', 32, 512, 4, 6, 0)],
    't3x2.two.c1.pf8/plain': [('most', 50, 208, 8, 6, 1)],
    't3x2.two.c1.pf8/stats': [('most', 50, 208, 8, 8, 0), ('cheapest', 50, 205, 5, 8, 0)],
    't3x2.two.c1.pf8/stats_xf': [('most', 50, 208, 8, 6, 0), ('cheapest', 50, 205, 5, 6, 0)],
    't4x1.ring.c1.pf8/stats': [('most', 50, 72, 8, 17, 0), ('cheapest', 50, 68, 4, 17, 0)],
    't4x1.two.c1.pf8/stats': [('most', 32, 328, 8, 17, 0)],
    't5x1.res.c1.pf8/plain': [('most', 50, 200, 8, 15, 1)],
    't5x1.ring.c1.pf4/stats': [('most', 128, 16, 8, 10, 0), ('cheapest', 128, 14, 7, 10, 0)],
    't5x1.ring.c1.pf4/stats_xf': [('most', 32, 200, 8, 11, 0)],
    't5x1.ring.c1.pf8/plain': [('most', 50, 72, 8, 11, 1)],
    't5x1.ring.c1.pf8/stats': [('most', 50, 72, 8, 13, 0), ('cheapest', 50, 68, 4, 13, 0)],
    't5x1.ring.c1.pf8/stats_xf': [('most', 50, 72, 8, 11, 0), ('cheapest', 50, 68, 4, 11, 0)],
    't5x1.ring.c4.pf8/plain': [('most', 128, 56, 8, 15, 1)],
    't5x1.two.c1.pf4/stats': [('most', 128, 24, 8, 10, 0), ('cheapest', 128, 18, 3, 10, 0)],
    't5x1.two.c1.pf8/plain': [('most', 50, 88, 8, 11, 1)],
    't5x1.two.c1.pf8/stats': [('most', 50, 88, 8, 13, 0), ('cheapest', 50, 87, 3, 13, 0)],
    't5x1.two.c1.pf8/stats_xf': [('most', 50, 88, 8, 11, 0), ('cheapest', 50, 87, 3, 11, 0)],
    't5x1.two.c4.pf8/plain': [('most', 128, 72, 8, 15, 1)],
    't5x2.two.c1.pf8/plain': [('most', 128, 128, 8, 11, 1)],
    't5x2.two.c1.pf8/stats': [('most', 128, 128, 8, 13, 0), ('cheapest', 128, 128, 4, 13, 0)],
    't5x2.two.c1.pf8/stats_xf': [('most', 128, 128, 8, 11, 0), ('cheapest', 128, 128, 4, 11, 0)],
    'wg1x2.pf4.m0/plain': [('most', 32, 8, 8, 0, 2)],
    'wg1x2.pf4/plain': [('most', 32, 48, 8, 0, 2)],
    'wg1x2.pf4/xf': [('most', 128, 8, 8, 2, 2), ('cheapest', 128, 3, 3, 2, 2)],
    'wg1x2.pf8.m1/plain': [('most', 32, 8, 8, 1, 2)],
    'wg1x2.pf8.m1/xf': [('most', 32, 8, 8, 2, 2), ('cheapest', 32, 3, 3, 2, 2)],
    'wg1x2.pf8/plain': [('most', 50, 28, 7, 1, 2)],
    'wg1x2.pf8/xf': [('most', 50, 28, 7, 2, 2), ('cheapest', 32, 65, 5, 2, 2)],
    'wg1x3.pf4.m2/plain': [('most', 84, 6, 6, 5, 2)],
    'wg1x3.pf4/plain': [('most', 84, 8, 8, 5, 2)],
    'wg1x3.pf8.m3/plain': [('most', 32, 8, 8, 8, 2)],
    'wg1x3.pf8.m3/xf': [('most', 32, 8, 8, 6, 2), ('cheapest', 32, 3, 3, 6, 2)],
    'wg1x3.pf8/plain': [('most', 50, 24, 8, 13, 2)],
    'wg1x3.pf8/xf': [('most', 50, 24, 8, 11, 2), ('cheapest', 128, 3, 3, 16, 2)],
    'wg1x5.pf4/plain': [('most', 32, 48, 8, 13, 2)],
    'wg1x5.pf4/xf': [('most', 32, 48, 8, 11, 2), ('cheapest', 32, 48, 3, 11, 2)],
    'wg1x5.pf8/plain': [('most', 32, 48, 8, 18, 2)],
    'wg1x5.pf8/xf': [('most', 32, 56, 8, 16, 2), ('cheapest', 32, 48, 3, 16, 2)],
    'wg2x2.pf8/plain': [('most', 32, 72, 8, 1, 2)],
    'wg2x2.pf8/xf': [('most', 32, 72, 8, 2, 2), ('cheapest', 84, 10, 5, 2, 2)],
    'wg2x3.pf8/plain': [('most', 32, 48, 8, 8, 2)],
    'wg2x3.pf8/xf': [('most', 32, 48, 8, 6, 2), ('cheapest', 128, 3, 3, 6, 2)],
    'wg2x5.pf8/xf': [('most', 32, 48, 8, 16, 2)],
    'wg3x2.pf8/plain': [('most', 32, 48, 8, 1, 2)],
    'wg3x2.pf8/xf': [('most', 32, 48, 8, 2, 2), ('cheapest', 32, 48, 3, 2, 2)],
    'wgq3.pf8/plain': [('most', 32, 192, 8, 1, 2)],
    'wgq3.pf8/xf': [('most', 32, 192, 8, 2, 2), ('cheapest', 50, 77, 7, 2, 2)],
    'wx1x1/plain': [('most', 32, 104, 8, 11, 1)],
    'wx1x1/stats': [('most', 32, 104, 8, 13, 0), ('cheapest', 32, 104, 4, 13, 0)],
    'wx3x1/plain': [('most', 32, 128, 8, 6, 1)],
    'wx3x1/stats': [('most', 32, 128, 8, 8, 0), ('cheapest', 32, 128, 4, 8, 0)],
}


GROUP_LIST = [(k, c[0], tuple(c[1:])) for k in sorted(GROUP_CASES) for c in GROUP_CASES[k]]
GROUP_CONV = [c for c in GROUP_LIST if not c[0].startswith("wg") and not c[0].endswith("/stats_xf")]
GROUP_XF = [c for c in GROUP_LIST if c[0].endswith("/stats_xf")]
GROUP_WGRAD = [c for c in GROUP_LIST if c[0].startswith("wg")]


# how tests/test_gpu_layers.py runs the cases (tests/test_cpu_forms.py checks that together they are every key of COVERED and that the GPU
# file parametrizes its tests with exactly these lists): integer-exact conv cases, the input-transform cases (tier 2 against float64
# BatchNorm), the integer-exact weight-gradient cases
EXACT_CONV_KEYS = sorted(k for k in COVERED if not k.startswith("wg") and not k.endswith("/stats_xf"))
XF_KEYS = sorted(k for k in COVERED if k.endswith("/stats_xf"))
WGRAD_KEYS = sorted(k for k in COVERED if k.startswith("wg"))
# the edge cases, flat: (key, kind, (hw, n, groups, layer, direction)), split the same way (tests/test_gpu_form_grid.py)
EDGE_LIST = [(k, c[0], tuple(c[1:])) for k in sorted(EDGE_CASES) for c in EDGE_CASES[k]]
EDGE_CONV = [c for c in EDGE_LIST if not c[0].startswith("wg") and not c[0].endswith("/stats_xf")]
EDGE_XF = [c for c in EDGE_LIST if c[0].endswith("/stats_xf")]
EDGE_WGRAD = [c for c in EDGE_LIST if c[0].startswith("wg")]


def format_tables(lib):
    """The text of COVERED and EDGE_CASES for the present planner."""
    cov = regenerate_covered(lib)
    COVERED.clear()
    COVERED.update(cov)
    out = ["COVERED = {"]
    out += ["    %r: %r," % (k, tuple(cov[k])) for k in sorted(cov)]
    out += ["}", ""]
    return "\n".join(out + _format_case_table("EDGE_CASES", edge_cases(lib)))


def format_group_cases(lib):
    """The text of GROUP_CASES for the present planner."""
    return "\n".join(_format_case_table("GROUP_CASES", group_cases(lib)))


def _format_case_table(name, ec):
    out = ["%s = {" % name]
    for k in sorted(ec):
        line = "    %r: [" % k
        for i, c in enumerate(ec[k]):
            item = repr(tuple(c)) + ("," if i + 1 < len(ec[k]) else "],")
            if len(line) + 1 + len(item) > 140:
                out.append(line)
                line = "       "
            line += item if line.endswith("[") else " " + item
        out.append(line)
    out.append("}")
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi
    print(format_group_cases(ffi.lib()) if sys.argv[1:] == ["groups"] else format_tables(ffi.lib()))
