"""GPU: every kernel form of the convolution, data-gradient and weight-gradient families at the edge sizes of the planner's domain
(layer_forms.EDGE_CASES: per form the pass with the most images, the largest pass with an odd number of images per BatchNorm group, and
the cheapest pass at every input size the form's other cases do not lie at), one layer at a time, through the case bodies of
tests/test_gpu_layers.py:

* convolution and data-gradient forms: tier 1 (integers in -2 .. 2, bit equality with float64, the hook reports the named form, the slack
  behind the output untouched); '/stats' and '/bnb' cases compare the accumulator cells as well;
* '/stats_xf' forms: tier 2 against float64 BatchNorm, with that test's bound;
* weight-gradient forms: tier 1 as a launch of their own and, for the forms of conv_wgrad_multi_kernel, inside the merged launch;
* the sentinel pass of tests/test_gpu_layers.py at 67 images in one group and 70 in two (the first sizes above the range that file walks).

The nine forms the dense grid added to layer_forms.COVERED run in the per-form tests of tests/test_gpu_layers.py; the whole passes at 67,
70 and 342 images are cases of tests/test_gpu_net.py::test_train_forward_backward_vs_oracle.

The same three bodies run the cases of layer_forms.GROUP_CASES: every form a pass of three to eight BatchNorm groups plans, at the cheapest
pass with the most groups and, where the epilogue or the staging reads the group, at the cheapest pass of all.  The bodies take the group
count from the layer's description and compare every group's accumulator cells.

With OCL_PARITY_REPORT=<file> the tier-2 margins and every case's wall time go to form_grid_parity.txt next to it
(profiles/form_grid_parity.txt), those of the many-group cases to many_groups_form_parity.txt (a section of
profiles/many_groups_parity.txt)."""
import os
import time

import pytest
import torch

import layer_forms as LF
import test_gpu_layers as TL

pytestmark = pytest.mark.gpu

REPORT = []
GROUP_REPORT = []


def _id(c):
    key, kind, (hw, n, g, layer, dr) = c
    return "%s-%s-hw%d-n%d-g%d-l%d" % (key, kind, hw, n, g, layer)


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    yield L
    L.ocl_set_deterministic(0)
    total = time.perf_counter() - t0
    path = os.environ.get("OCL_PARITY_REPORT")
    if path and REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "form_grid_parity.txt"), "w") as f:
            f.write("# the edge sizes of every kernel form (tests/test_gpu_form_grid.py, layer_forms.EDGE_CASES): tier 1 cases are bit-equal or fail;\n"
                    "# tier 2 (/stats_xf) cases give their worst error / bound (must be < 1); seconds are wall time, float64 reference included\n")
            f.write("# %d cases, %.1f s in all (slowest %.2f s)\n" % (len(REPORT), total, max(r[2] for r in REPORT)))
            f.write("%-72s %-8s %8s %8s\n" % ("case", "tier", "seconds", "ratio"))
            for case, tier, sec, ratio in REPORT:
                f.write("%-72s %-8s %8.2f %8s\n" % (case, tier, sec, "" if ratio is None else "%.3f" % ratio))
    if path and GROUP_REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "many_groups_form_parity.txt"), "w") as f:
            f.write("# every form a pass of 3 .. 8 BatchNorm groups plans (layer_forms.GROUP_CASES): tier 1 cases are bit-equal or fail; tier 2\n"
                    "# (/stats_xf) cases give their worst error / bound (must be < 1); seconds are wall time, float64 reference included\n")
            f.write("# %d cases, slowest %.2f s\n" % (len(GROUP_REPORT), max(r[2] for r in GROUP_REPORT)))
            f.write("%-72s %-8s %8s %8s\n" % ("case", "tier", "seconds", "ratio"))
            for case, tier, sec, ratio in GROUP_REPORT:
                f.write("%-72s %-8s %8.2f %8s\n" % (case, tier, sec, "" if ratio is None else "%.3f" % ratio))


@pytest.fixture
def at(monkeypatch, lib):
    """The case bodies of tests/test_gpu_layers.py look their layer up through find_entry: point it at one edge case."""
    def use(case):
        monkeypatch.setattr(TL, "find_entry", lambda L, key: LF.find_case(L, key, case))
    return use


@pytest.mark.parametrize("case", LF.EDGE_CONV, ids=_id)
def test_edge_conv_form_is_exact(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    TL._conv_form_is_exact(lib, key, 0)
    REPORT.append((_id(case), "1", time.perf_counter() - t0, None))


@pytest.mark.parametrize("case", LF.EDGE_XF, ids=_id)
def test_edge_input_transform_against_float64_batchnorm(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    ratio = TL._input_transform_against_float64_batchnorm(lib, key, 0)
    REPORT.append((_id(case), "2", time.perf_counter() - t0, ratio))


@pytest.mark.parametrize("case", LF.EDGE_WGRAD, ids=_id)
def test_edge_wgrad_form_is_exact(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    TL._wgrad_form_is_exact(lib, key, False)
    if ".m" in key:
        TL._wgrad_form_is_exact(lib, key, True)
    REPORT.append((_id(case), "1", time.perf_counter() - t0, None))


@pytest.mark.parametrize("case", LF.GROUP_CONV, ids=_id)
def test_group_conv_form_is_exact(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    TL._conv_form_is_exact(lib, key, 0)
    GROUP_REPORT.append((_id(case), "1", time.perf_counter() - t0, None))


@pytest.mark.parametrize("case", LF.GROUP_XF, ids=_id)
def test_group_input_transform_against_float64_batchnorm(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    ratio = TL._input_transform_against_float64_batchnorm(lib, key, 0)
    GROUP_REPORT.append((_id(case), "2", time.perf_counter() - t0, ratio))


@pytest.mark.parametrize("case", LF.GROUP_WGRAD, ids=_id)
def test_group_wgrad_form_is_exact(lib, at, case):
    key, kind, where = case
    at(where)
    t0 = time.perf_counter()
    TL._wgrad_form_is_exact(lib, key, False)
    if ".m" in key:
        TL._wgrad_form_is_exact(lib, key, True)
    GROUP_REPORT.append((_id(case), "1", time.perf_counter() - t0, None))


@pytest.mark.parametrize("kind", ["last_image", "last_pixel"])
@pytest.mark.parametrize("n,groups", [(67, 1), (70, 2)])
def test_sentinels_one_image_above_the_dense_range(lib, kind, n, groups):
    """tests/test_gpu_layers.py::test_sentinels_every_layer_shape at the passes of 65 .. 71 images (SCR with eps_mem_batch 25: 70 views in two
    groups; ER with batch 10 and 57 memory images: 67 in one), where layer 1's weight gradient is wg1x2.pf8."""
    t0 = time.perf_counter()
    TL.test_sentinels_every_layer_shape(lib, kind, n, groups)
    REPORT.append(("sentinels-%s-n%d-g%d" % (kind, n, groups), "1", time.perf_counter() - t0, None))
