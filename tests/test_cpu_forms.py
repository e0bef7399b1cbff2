"""CPU: every kernel form the network engine plans (ocl_test_net_forms: the very function the engine's plan cache calls) over the dense
grid of layer_forms.pass_grid -- 32 x 32, 50 x 50, 84 x 84 and 128 x 128, every train pass of 1 .. resnet._default_max_batch images in
one and two BatchNorm groups, every eval pass the engine's rounding can plan, and the passes above the defaults (300 train images, eval
passes up to 416 at 32 x 32 and 84 x 84) -- must have a single-layer parity case in tests/test_gpu_layers.py (layer_forms.COVERED) or
tests/test_gpu_datasets.py (datasets_cases.NEW_FORMS).  A planner change that reaches a new form without a parity case fails here; the
grid itself and the edge sizes of every form (layer_forms.EDGE_CASES) are checked in tests/test_cpu_form_grid.py."""
import ctypes as C

import pytest

import layer_forms as LF
import ocl_amd  # noqa: F401
from ocl_amd import ffi


@pytest.fixture(scope="module")
def lib():
    return ffi.lib()


def test_every_planned_form_has_a_parity_case(lib):
    import datasets_cases as DC
    forms = LF.enumerate_forms(lib)
    missing = sorted(set(forms) - set(LF.COVERED) - set(DC.NEW_FORMS))
    assert not missing, "forms without a case in layer_forms.COVERED / datasets_cases.NEW_FORMS: %s" % missing
    assert len(forms) >= 100
    # every case still reaches its form where the list says
    stale = [k for k, case in LF.COVERED.items() if not LF.plans(lib, k, case)]
    assert not stale, stale


def _params(fn):
    return [m.args[1] for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"][0]


def test_the_gpu_file_runs_every_covered_key():
    """Every key of COVERED is parametrized, unsliced, in one of test_gpu_layers.py's per-form tests (listing a key is not enough)."""
    import test_gpu_layers as T
    assert set(LF.EXACT_CONV_KEYS) | set(LF.XF_KEYS) | set(LF.WGRAD_KEYS) == set(LF.COVERED)
    exact = {k for k, det in _params(T.test_conv_form_is_exact) if det == 0}
    assert exact == set(LF.EXACT_CONV_KEYS)
    assert set(_params(T.test_input_transform_against_float64_batchnorm)) == set(LF.XF_KEYS)
    assert set(_params(T.test_wgrad_form_is_exact)) == set(LF.WGRAD_KEYS)


def test_forms_of_a_pass_are_what_the_hook_plans(lib):
    """ocl_test_conv_plan on the description a pass entry carries plans the entry's form (the GPU cases reproduce layers this way)."""
    for hw, n, g, train in [(32, 220, 2, 1), (32, 20, 2, 1), (84, 15, 1, 1), (32, 416, 1, 0)]:
        ents = LF.net_forms(lib, hw, n, g, train)
        for key, e in ents:
            if e.dir == 2:
                f = ffi.TestWgradForm()
                assert lib.ocl_test_wgrad(C.byref(e.wdesc), None, 1, 0, 0, C.byref(f), None) == 0, lib.ocl_last_error()
                assert LF.wgrad_key(f, e.wdesc.xf_groups > 0, e.wg_merged) == key
                continue
            fs = (ffi.TestConvForm * 4)()
            cnt = lib.ocl_test_conv_plan(C.byref(e.desc), fs, 4)
            assert cnt in (1, 4), lib.ocl_last_error()
            epi = key.split("/")[1]
            assert key in [LF.conv_key(fs[i], epi) for i in range(cnt)]
        # one forward per conv, at least one data gradient per conv but the stem (train), one weight gradient per conv (train)
        assert sum(e.dir == 0 for _, e in ents) == 20
        if train:
            assert sum(e.dir == 2 for _, e in ents) == 20 and sum(e.dir == 1 for _, e in ents) >= 19


def _max_partial(shape_terms, mag=2 * 2):
    return shape_terms * mag


def test_tier1_integer_cases_stay_below_2_24(lib):
    """Tier 1 draws inputs, weights and gradients from {-2..2}: every partial sum of a case is bounded by (terms) * 4, which must stay below
    2^24 for the fp32 result to be exact in any summation order."""
    worst = 0
    cases = list(LF.COVERED.items()) + [(k, case) for k, _, case in LF.EDGE_LIST]
    assert len(cases) > len(LF.COVERED) + 300
    for k, (hw, n, g, layer, dr) in cases:
        for kk, e in LF.net_forms(lib, hw, n, g, 0 if k.endswith("/affine") else 1):
            if kk != k or e.layer != layer or e.dir != dr:
                continue
            if dr == 2:
                d = e.wdesc
                pad = 1 if d.k == 3 else 0
                ho = (d.hin + 2 * pad - d.k) // d.stride + 1
                terms = n * ho * ho
            else:
                d = e.desc
                terms = d.k * d.k * (d.cin if dr == 0 else d.cout)
            # (+ the epilogue's integer addends: shift <= 3, residual / accumulated value <= 2, before the ReLU)
            worst = max(worst, _max_partial(terms) + 8)
    # the fixed shapes of test_gpu_layers.py: 220-view pass wgrad of the stem (220 * 32 * 32 terms), 84 x 84 at 3 images
    worst = max(worst, _max_partial(220 * 32 * 32), _max_partial(3 * 84 * 84))
    # (the edge cases' worst are the stride-1 weight gradients over whole inputs: 128 images of 128 x 128 and 300 of 84 x 84, 8.4e6 and 8.5e6)
    assert 128 * 128 * 128 * 4 <= worst < 2 ** 24, worst
