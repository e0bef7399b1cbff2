"""Shared by tests/test_gpu_datasets.py and tests/test_cpu_datasets.py (a plain helper module, not a conftest): the pass grid of the 50 x 50
(openloris) and 128 x 128 (core50) inputs, and the single-layer parity cases for the kernel forms the planner gives there that
layer_forms.COVERED does not contain.  (The dense grid of tests/layer_forms.py covers these input sizes too, up to the default max_batch;
a form it finds is accepted with a case in either table, and its edge sizes are in layer_forms.EDGE_CASES.)"""
import layer_forms as LF

HW = (50, 128)
N = (1, 2, 3, 4, 8, 10, 16, 20, 32, 50, 64)


def pass_grid():
    """hw x n x groups {1, 2} x train {0, 1}; an eval pass has one BatchNorm group (ocl_test_net_forms refuses two)."""
    for hw in HW:
        for n in N:
            for g in (1, 2):
                if n % g:
                    continue
                for train in ((0, 1) if g == 1 else (1,)):
                    yield hw, n, g, train


def new_forms(lib):
    """{key: (hw, n, groups, train, entry)}: every form of the grid above that layer_forms.COVERED lacks, at the cheapest pass / layer."""
    best = {}
    for hw, n, g, train in pass_grid():
        for key, e in LF.net_forms(lib, hw, n, g, train):
            if key in LF.COVERED:
                continue
            c = LF.entry_cost(hw, n, e)
            if key not in best or c < best[key][0]:
                best[key] = (c, (hw, n, g, train, e))
    return {k: v[1] for k, v in best.items()}


# key -> (hw, n, groups, layer index, direction), as layer_forms.COVERED.  Regenerate with `python tests/datasets_cases.py` after a planner
# change; tests/test_cpu_datasets.py fails when the planner gives a form at these sizes that neither table holds.
NEW_FORMS = {
    't1x1.ring.c1.pf4/affine': (50, 1, 1, 5, 0),
    't2x1.ring.c1.pf4/bnb': (128, 1, 1, 1, 1),
    't2x1.ring.c1.pf4/stats_xf': (128, 1, 1, 2, 0),
    't3x1.ring.c1.pf4/bnb': (50, 20, 1, 6, 1),
    't3x1.ring.c1.pf4/stats_xf': (50, 20, 2, 6, 0),
    't5x1.ring.c1.pf4/affine': (128, 16, 1, 10, 0),
    't5x1.ring.c1.pf4/stats': (128, 16, 1, 10, 0),
    't5x1.ring.c4.pf8/plain': (128, 50, 1, 15, 1),
    't5x1.two.c1.pf4/affine': (128, 20, 1, 10, 0),
    't5x1.two.c1.pf4/stats': (128, 20, 1, 10, 0),
    'wg1x2.pf4.m0/xf': (128, 1, 1, 2, 2),
    'wg1x2.pf4/xf': (128, 3, 1, 2, 2),
}

EXACT_CONV_KEYS = sorted(k for k in NEW_FORMS if not k.startswith("wg") and not k.endswith("/stats_xf"))
XF_KEYS = sorted(k for k in NEW_FORMS if k.endswith("/stats_xf"))
WGRAD_KEYS = sorted(k for k in NEW_FORMS if k.startswith("wg"))


def find_entry(lib, key):
    hw, n, g, layer, dr = NEW_FORMS[key]
    train = 0 if key.endswith("/affine") else 1
    for k, e in LF.net_forms(lib, hw, n, g, train):
        if k == key and e.layer == layer and e.dir == dr:
            return e
    raise AssertionError("the planner no longer gives %s at %r: regenerate datasets_cases.NEW_FORMS" % (key, NEW_FORMS[key]))


# Single layers at the lattices the new inputs bring: (cin, cout, k, stride, input size).  50 -> 25 -> 13 -> 7 is odd at every level (a
# stride-2 layer's last output row and column read the padding), 7 x 7 is the map avg_pool2d(4) crops, 128 x 128 the longest rows.
LATTICE_SHAPES = [
    (3, 20, 3, 1, 50), (3, 20, 3, 1, 128),           # the 3-channel stem
    (20, 20, 3, 1, 128),                             # 128 x 128, stride 1, Cin 20
    (20, 40, 3, 2, 50), (20, 40, 1, 2, 50),          # 50 -> 25
    (40, 80, 3, 2, 25), (40, 80, 1, 2, 25),          # 25 -> 13
    (80, 160, 3, 2, 13), (80, 160, 1, 2, 13),        # 13 -> 7
    (160, 160, 3, 1, 7),                             # 7 x 7, stride 1
]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi
    forms = new_forms(ffi.lib())
    print("NEW_FORMS = {")
    for k in sorted(forms):
        hw, n, g, train, e = forms[k]
        print("    %r: (%d, %d, %d, %d, %d)," % (k, hw, n, g, e.layer, e.dir))
    print("}")
