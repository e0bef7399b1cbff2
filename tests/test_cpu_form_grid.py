"""CPU: the dense planner grid of tests/layer_forms.py is the engine's real domain, every form it reaches has a single-layer parity case,
and the committed edge sizes of every form (layer_forms.EDGE_CASES) are what the rule gives on the present planner.

The grid: 32 x 32, 50 x 50, 84 x 84 and 128 x 128 inputs; every train pass of 1 .. resnet._default_max_batch(hw, hw) images in one and two
BatchNorm groups; every eval pass ocl_net_forward's rounding (4 images up to 16, 16 above, capped at max_batch) can plan; and the passes
above the defaults that earlier cases rest on (300 train images, eval passes of 272 .. 416 at 32 x 32 and 84 x 84).  All of it is swept,
not sampled: about 1 800 calls of ocl_test_net_forms, the function the engine's plan cache calls, in well under a second.

A planner change that reaches a form without a parity case, moves a form's largest / odd / other-lattice pass, or takes a form away from
a committed case fails here, on the CPU; `python tests/layer_forms.py` prints the regenerated tables."""
import pytest

import datasets_cases as DC
import layer_forms as LF
import ocl_amd  # noqa: F401
from ocl_amd import ffi
from ocl_amd.resnet import _default_max_batch


@pytest.fixture(scope="module")
def lib():
    return ffi.lib()


def test_the_grid_is_the_engines_default_domain():
    assert LF.HW == (32, 50, 84, 128) and LF.GROUPS == (1, 2)
    dense = list(LF.dense_grid())
    assert len(dense) == len(set(dense))
    for hw in LF.HW:
        mb = _default_max_batch(hw, hw)
        train = {(n, g) for h, n, g, t in dense if h == hw and t}
        ev = sorted(n for h, n, g, t in dense if h == hw and not t)
        # the per-size maxima are the engine's default: a changed default moves the grid with it
        assert max(n for n, _ in train) == mb and max(ev) == mb
        assert train == {(n, g) for n in range(1, mb + 1) for g in (1, 2) if n % g == 0}
        # Nplan of ocl_net_forward for N = 1 .. max_batch
        assert ev == sorted({min(mb, -(-N // 4) * 4 if N <= 16 else -(-N // 16) * 16) for N in range(1, mb + 1)})
    grid = list(LF.pass_grid())
    assert len(grid) == len(set(grid)) and set(dense) <= set(grid)
    # the passes above the defaults stay, and the t5x2.* parity cases that lie there
    for hw in (32, 84):
        assert (hw, 300, 1, 1) in grid and (hw, 300, 2, 1) in grid
        assert all((hw, n, 1, 0) in grid for n in range(272, 417, 16))
    t5x2 = {k: c for k, c in LF.COVERED.items() if k.startswith("t5x2.")}
    assert len(t5x2) == 5 and all(c[0] == 84 and c[1] > _default_max_batch(84, 84) for c in t5x2.values()), t5x2
    assert all((c[0], c[1], c[2], LF.is_train(k)) in grid for k, c in LF.COVERED.items())


def test_every_form_of_the_dense_grid_has_a_parity_case(lib):
    forms = LF.enumerate_forms(lib)
    assert len(forms) >= 150
    missing = sorted(set(forms) - set(LF.COVERED) - set(DC.NEW_FORMS))
    assert not missing, "forms without a case in layer_forms.COVERED / datasets_cases.NEW_FORMS: %s" % missing
    assert not set(LF.COVERED) & set(DC.NEW_FORMS)
    # the table is what regeneration gives: no stale case, no key the grid no longer reaches, no hand-edited case
    stale = [k for k, case in LF.COVERED.items() if not LF.plans(lib, k, case)]
    assert not stale, stale
    assert LF.regenerate_covered(lib) == LF.COVERED
    assert sorted(set(forms) - set(LF.COVERED)) == sorted(DC.NEW_FORMS)


def test_edge_cases_are_what_the_rule_gives_on_this_planner(lib):
    want = LF.edge_cases(lib)
    got = {k: [tuple(c) for c in v] for k, v in LF.EDGE_CASES.items()}
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, "layer_forms.EDGE_CASES is not what edge_cases() gives: regenerate (%r)" % (sorted(diff.items())[:3],)
    sw = LF.sweep(lib)
    for key, kind, case in LF.EDGE_LIST:
        assert LF.plans(lib, key, case), (key, kind, case)
        assert case != tuple(LF.parity_case(key))
        assert kind in ("largest", "odd", "lattice")
    for key, rows in sw.items():
        kinds = [c[0] for c in LF.EDGE_CASES.get(key, [])]
        base = tuple(LF.parity_case(key))
        nmax = max(r[1] for r in rows)
        # the largest pass of every form is a case (of this table or the parity case itself)
        assert ("largest" in kinds and LF.EDGE_CASES[key][0][2] == nmax) or base[1] == nmax, key
        # every input size a form is planned at holds one of its cases
        at = {base[0]} | {c[1] for c in LF.EDGE_CASES.get(key, [])}
        assert at == {r[0] for r in rows}, key
        # a form planned at an odd group size has a case with one
        if any((r[1] // r[2]) % 2 for r in rows):
            assert any((n // g) % 2 for _, n, g, _, _ in [base] + [c[1:] for c in LF.EDGE_CASES.get(key, [])]), key


def test_no_edge_case_needs_more_than_seconds_of_reference(lib):
    """ref_work counts the float64 multiply-adds a case's check computes.  torch's float64 convolution does about 6e9 a second on eight
    threads (7.6e9 in 1.2 s: layer 1 at 300 images of 84 x 84), so the table's dearest case, 3.0e10, stays under ten seconds on 16; a
    planner change that makes a case dearer than 4e10 has to replace it by the next cheaper entry with the same property, as the table's
    comment says."""
    sw = LF.sweep(lib)
    work = {(k, kind, case): LF.ref_work(k, [r for r in sw[k] if r[:5] == case][0]) for k, kind, case in LF.EDGE_LIST}
    worst = max(work, key=work.get)
    assert work[worst] <= 4e10, (worst, work[worst])
    assert sum(work.values()) <= 1.2e12


def _params(fn):
    return [m.args[1] for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"][0]


def test_the_gpu_file_runs_every_edge_case():
    """Every entry of EDGE_CASES is parametrized, unsliced, in one of tests/test_gpu_form_grid.py's tests."""
    import test_gpu_form_grid as T
    assert len(LF.EDGE_LIST) == sum(len(v) for v in LF.EDGE_CASES.values()) == len(set(LF.EDGE_LIST))
    assert sorted(LF.EDGE_CONV + LF.EDGE_XF + LF.EDGE_WGRAD) == sorted(LF.EDGE_LIST)
    assert _params(T.test_edge_conv_form_is_exact) == LF.EDGE_CONV
    assert _params(T.test_edge_input_transform_against_float64_batchnorm) == LF.EDGE_XF
    assert _params(T.test_edge_wgrad_form_is_exact) == LF.EDGE_WGRAD
    assert sorted(_params(T.test_sentinels_one_image_above_the_dense_range)) == [(67, 1), (70, 2)]
    assert len(set(map(T._id, LF.EDGE_LIST))) == len(LF.EDGE_LIST)


def test_the_whole_passes_of_the_new_sizes_are_cases_of_the_net_test():
    import test_gpu_net as TN
    for case in (("ER", "cifar100", None, 67, 1), ("SCR", "cifar100", "mlp", 70, 2), ("ER", "cifar100", None, 342, 1)):
        assert case in TN.CASES
    sw = LF.sweep(ffi.lib())
    at = lambda key: {(r[0], r[1], r[2]) for r in sw[key]}
    assert (32, 67, 1) in at("wg1x2.pf8/plain") and (32, 70, 2) in at("wg1x2.pf8/xf")
    assert (32, 342, 1) in at("t4x1.two.c1.pf8/stats") and (32, 342, 1) in at("t2x1.two.c4.pf8/plain")
