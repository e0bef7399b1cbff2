"""GPU: the arg-max and class-score kernel (csrc/rowstats.hip: ocl_row_argmax_groupsum; ops.row_argmax_groupsum), the host bookkeeping
built on it (error_analysis.py) and evaluate() with params.error_analysis (agents/base.py), against the float64 statements of
tests/error_analysis_ref.py (pinned on the CPU by tests/test_cpu_error_analysis.py) and the run recorded from the reference
(tests/golden/error_analysis.npz).

The arg-max is exact.  A row's sum is judged by parity_bounds.check_derived against 1.01 * c * 2^-53 * sum|x_j| over the selected columns:
the round-off of a float64 sum of c terms in any order.  Observed margins: profiles/error_analysis_parity.txt (written by this module's
report when PARITY_REPORT_DIR names a directory)."""
import copy
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set
from conftest import gold
from guarded import Guarded
from oracle.synth import make_stream
import parity_bounds
import error_analysis_ref as E
from error_analysis_ref import ref_row_argmax_groupsum, ref_error_analysis, ref_norms

pytestmark = pytest.mark.gpu

REPORT = []
SHAPES = [
    (1, 1), (1, 2), (3, 10), (5, 64), (4, 65),        # the smallest; one lane; both sides of 64 lanes
    (5, 256), (4, 257),                               # the two sides of the register form
    (6, 300), (16, 100), (128, 100),                  # the strided form; a partial and a full test batch
    (130, 100),                                       # the rows do not divide by the rows per workgroup
    (100, 160), (100, 640),                           # the last layer's weight
]
SCALES = [1e-3, 1.0, 1e3]
POISON = -7777


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    """After the module's tests: the rows parity_bounds recorded, as a table, into $PARITY_REPORT_DIR/error_analysis_parity.txt."""
    yield
    out = os.environ.get("PARITY_REPORT_DIR")
    if out and REPORT:
        with open(os.path.join(out, "error_analysis_parity.txt"), "w") as f:
            f.write("%-52s %-8s %-12s %-12s %-12s %s\n" % ("case", "tensor", "kernel err", "torch32 err", "bound", "err/bound"))
            for case, tensor, err, e_ref, bound, ratio in REPORT:
                f.write("%-52s %-8s %-12.4g %-12s %-12.4g %.3f\n" % (case, tensor, err, e_ref, bound, ratio))
            f.write("worst err/bound %.3f over %d rows\n" % (max(r[5] for r in REPORT), len(REPORT)))


def _x(n, c, scale):
    rng = np.random.default_rng(7000 + 131 * n + 17 * c)
    return (rng.standard_normal((n, c)) * scale).astype(np.float32)


def _groups(c):
    """(name, table or None, sel): all 0, all 1, mixed with -1 (either selection), an empty selection, no table."""
    mixed = np.random.default_rng(50 + c).integers(-1, 2, c).astype(np.int32)
    return [("all0", np.zeros(c, dtype=np.int32), 0), ("all1", np.ones(c, dtype=np.int32), 1), ("mixed/0", mixed, 0), ("mixed/1", mixed, 1),
            ("empty", mixed, 5), ("null", None, 0)]


@pytest.fixture(scope="module")
def kernel_results(cuda):
    """Every (shape, group, scale) case through the C entry point once, on guarded tensors: {(n, c, group name, scale): (argmax, sums) as
    device tensors}, with the inputs they came from.  Shared by the parity, single-row and repeat tests."""
    from ocl_amd import ffi
    lib = ffi.lib()
    res = {}
    for n, c in SHAPES:
        for scale in SCALES:
            x = _x(n, c, scale)
            for name, group, sel in _groups(c):
                g = Guarded()
                d_x = g.inp(x, 0, "x")
                d_g = g.inp(group, 0, "col_group") if group is not None else None
                d_am, d_sm = g.out((n,), torch.int64, 0, "argmax_out"), g.out((n,), torch.float64, 0, "sum_out")
                rc = lib.ocl_row_argmax_groupsum(ffi.ptr(d_x), n, c, ffi.ptr(d_g), sel, ffi.ptr(d_am), ffi.ptr(d_sm), ffi.stream())
                assert rc == 0, lib.ocl_last_error()
                g.check("row_argmax_groupsum %s" % ((n, c, name, scale),))
                res[(n, c, name, scale)] = SimpleNamespace(x=x, d_x=d_x, group=group, d_g=d_g, sel=sel, am=d_am, sm=d_sm)
    return res


# ---- 1. the kernel against the float64 statement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,c", SHAPES)
def test_row_argmax_groupsum_vs_float64_reference(kernel_results, n, c):
    for scale in SCALES:
        for name, group, sel in _groups(c):
            r = kernel_results[(n, c, name, scale)]
            want_am, want_sm = ref_row_argmax_groupsum(r.x, group, sel)
            assert not E.top2_tie(r.x).any()
            assert np.array_equal(_host(r.am), want_am), (n, c, name, scale)
            parity_bounds.check_derived(REPORT, "rowstats n=%d c=%d group=%s scale=%g" % (n, c, name, scale), "sums", _host(r.sm), want_sm,
                                        E.sum_bound(r.x, group, sel))
            if name == "empty":
                assert not bool(_bits(r.sm).any()), "an empty group does not give +0.0"


@pytest.mark.parametrize("n,c", SHAPES)
def test_a_row_alone_gives_the_bits_it_gives_in_the_batch_and_two_runs_are_identical(cuda, kernel_results, n, c):
    from ocl_amd import ops
    for name in ("mixed/1", "null"):
        r = kernel_results[(n, c, name, 1.0)]
        am2, sm2 = ops.row_argmax_groupsum(r.d_x, r.d_g, r.sel)
        assert torch.equal(am2, r.am) and torch.equal(_bits(sm2), _bits(r.sm)), "two runs differ"
        for row in sorted({0, n // 2, n - 1, min(n - 1, 4), min(n - 1, 127)}):
            am1, sm1 = ops.row_argmax_groupsum(r.d_x[row:row + 1].clone(), r.d_g, r.sel)
            assert torch.equal(am1, r.am[row:row + 1]) and torch.equal(_bits(sm1), _bits(r.sm[row:row + 1])), (name, row)
        # each output alone: the same bits
        am_only, none = ops.row_argmax_groupsum(r.d_x, r.d_g, r.sel, want_sum=False)
        none2, sm_only = ops.row_argmax_groupsum(r.d_x, r.d_g, r.sel, want_argmax=False)
        assert none is None and none2 is None and torch.equal(am_only, r.am) and torch.equal(_bits(sm_only), _bits(r.sm))


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------

def _check_argmax(cuda, x, want):
    from ocl_amd import ops
    am, _ = ops.row_argmax_groupsum(_dev(x, cuda))
    got = _host(am).tolist()
    assert got == want, (got, want)
    assert got == ref_row_argmax_groupsum(x, None, 0)[0].tolist() == torch.max(torch.from_numpy(x), 1)[1].tolist()


@pytest.mark.parametrize("c", [256, 300])
def test_ties_nans_and_signed_zeros(cuda, c):
    """Ties planted at lanes 0 / 63 / 64 and (c = 300: the strided form) at columns 255 / 256: the smaller index wins, within a lane, across
    lanes and across the register groups.  A NaN beats everything, +Inf included, and the first NaN wins.  -0.0 and +0.0 are equal."""
    pairs = [(0, 63), (63, 64), (64, 128), (0, 64), (1, 255), (191, 255), (62, 63)] + ([(255, 256), (256, 299), (0, 256), (63, 299), (64, 256)] if c > 256 else [])
    rng = np.random.default_rng(c)
    base = rng.standard_normal((len(pairs), c)).astype(np.float32)
    x = base.copy()
    for r, (a, b) in enumerate(pairs):
        x[r, a] = x[r, b] = 50.0
    _check_argmax(cuda, x, [a for a, _ in pairs])
    x = base.copy()
    for r, (a, b) in enumerate(pairs):            # the later column holds the first NaN's rival: a second NaN, or +Inf
        x[r, a], x[r, b] = np.nan, (np.nan if r % 2 else np.inf)
    _check_argmax(cuda, x, [a for a, _ in pairs])
    x = base.copy()
    for r, (a, b) in enumerate(pairs):            # +Inf first, the NaN later: the NaN
        x[r, a], x[r, b] = np.inf, np.nan
    _check_argmax(cuda, x, [b for _, b in pairs])
    x = -np.abs(base) - 1.0
    for r, (a, b) in enumerate(pairs):
        x[r, a], x[r, b] = (-0.0, 0.0) if r % 2 else (0.0, -0.0)
    _check_argmax(cuda, x, [a for a, _ in pairs])
    _check_argmax(cuda, np.full((3, c), -np.inf, dtype=np.float32), [0, 0, 0])
    _check_argmax(cuda, np.full((3, c), 2.5, dtype=np.float32), [0, 0, 0])


@pytest.mark.parametrize("n,c", [(3, 10), (4, 65), (5, 256), (6, 300), (128, 100)])
def test_nan_and_inf_outside_the_group_leave_the_sums_bits_alone(cuda, n, c):
    from ocl_amd import ops
    x0 = _x(n, c, 1.0)
    group = np.random.default_rng(c).integers(-1, 2, c).astype(np.int32)
    group[0], group[c - 1] = 1, 0
    for sel in (0, 1):
        out = group != sel
        x1 = x0.copy()
        x1[:, out] = np.nan
        x1[::2, out] = np.inf
        x1[1::3, out] = -np.inf
        x00 = x0.copy()
        x00[:, out] = 0.0
        _, s0 = ops.row_argmax_groupsum(_dev(x0, cuda), _dev(group, cuda, np.int32), sel, want_argmax=False)
        _, s1 = ops.row_argmax_groupsum(_dev(x1, cuda), _dev(group, cuda, np.int32), sel, want_argmax=False)
        _, s00 = ops.row_argmax_groupsum(_dev(x00, cuda), _dev(group, cuda, np.int32), sel, want_argmax=False)
        assert bool(torch.isfinite(s1).all()) and torch.equal(_bits(s0), _bits(s1)) and torch.equal(_bits(s0), _bits(s00))


def test_outputs_go_into_a_row_block_of_a_larger_buffer_and_leave_the_rest(cuda):
    from ocl_amd import ops
    n, c = 16, 100
    x, group = _dev(_x(n, c, 1.0), cuda), _dev(np.arange(c) % 3 - 1, cuda, np.int32)
    big_am = torch.full((3 * n,), POISON, dtype=torch.int64, device=cuda)
    big_sm = torch.full((3 * n + 5,), float(POISON), dtype=torch.float64, device=cuda)
    am, sm = ops.row_argmax_groupsum(x, group, 1, argmax_out=big_am[n:2 * n], sum_out=big_sm[n + 5:2 * n + 5])
    want_am, want_sm = ops.row_argmax_groupsum(x, group, 1)
    assert am.data_ptr() == big_am[n:2 * n].data_ptr() and sm.data_ptr() == big_sm[n + 5:2 * n + 5].data_ptr()
    assert torch.equal(am, want_am) and torch.equal(_bits(sm), _bits(want_sm))
    assert bool((big_am[:n] == POISON).all()) and bool((big_am[2 * n:] == POISON).all())
    assert bool((big_sm[:n + 5] == POISON).all()) and bool((big_sm[2 * n + 5:] == POISON).all())
    # one int64 table holding the predictions and, behind them, the sums' bits (error_analysis.py's loader table)
    table = torch.full((2 * n,), POISON, dtype=torch.int64, device=cuda)
    ops.row_argmax_groupsum(x, group, 1, argmax_out=table[:n], sum_out=table[n:].view(torch.float64))
    assert torch.equal(table[:n], want_am) and torch.equal(table[n:], _bits(want_sm))
    for bad in (dict(argmax_out=big_am[:n + 1]), dict(argmax_out=big_am[:2 * n:2]), dict(argmax_out=big_am[:n].int()), dict(argmax_out=big_am[:n].cpu()),
                dict(sum_out=big_sm[:n - 1]), dict(sum_out=big_sm[:n].float()), dict(sum_out=big_sm[:n].cpu()), dict(col_group=group.cpu()),
                dict(col_group=group[:50]), dict(col_group=group.long())):
        kw = dict(col_group=group)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="row_argmax_groupsum"):
            ops.row_argmax_groupsum(x, sel=1, **kw)


# ---- 3. refused arguments ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from ocl_amd import ffi
    lib = ffi.lib()
    n, c = 4, 8
    x = torch.full((n, c), 1.0, device=cuda)
    group = torch.full((c,), 1, dtype=torch.int32, device=cuda)
    am = torch.full((n,), POISON, dtype=torch.int64, device=cuda)
    sm = torch.full((n,), float(POISON), dtype=torch.float64, device=cuda)

    def call(**over):
        kw = dict(x=x.data_ptr(), n=n, c=c, group=group.data_ptr(), sel=1, am=am.data_ptr(), sm=sm.data_ptr())
        kw.update(over)
        rc = lib.ocl_row_argmax_groupsum(ffi.vp(kw["x"]), kw["n"], kw["c"], ffi.vp(kw["group"]), kw["sel"], ffi.vp(kw["am"]), ffi.vp(kw["sm"]),
                                         ffi.stream())
        return rc, lib.ocl_last_error()

    for over in (dict(x=0), dict(am=0, sm=0), dict(n=0), dict(n=-1), dict(c=0), dict(c=-5),
                 dict(am=x.data_ptr()), dict(am=x.data_ptr() + 4 * (n * c - 1)), dict(sm=x.data_ptr() + 64), dict(am=group.data_ptr()),
                 dict(sm=group.data_ptr() + 8), dict(sm=am.data_ptr()), dict(sm=am.data_ptr() + 8 * (n - 1)), dict(am=sm.data_ptr() + 8)):
        rc, msg = call(**over)
        assert rc == -1 and msg.startswith(b"row_argmax_groupsum:"), (over, rc, msg)
        if set(over) & {"am", "sm"} and len(over) == 1:
            assert b"overlap" in msg, (over, msg)
    torch.cuda.synchronize()
    assert bool((am == POISON).all()) and bool((sm == POISON).all()) and bool((x == 1.0).all()) and bool((group == 1).all())
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert am.tolist() == [0] * n and sm.tolist() == [8.0] * n
    rc, msg = call(group=0, sel=3, am=0)        # no table: every column, whatever sel says; no arg-max
    assert rc == 0, msg


# ---- 4. the pipeline on the recorded logits ----------------------------------------------------------------------------------------------

def _drive(ea, batches, bk, weight, bias, cuda):
    ea.begin(bk["old_labels"], bk["new_labels_zombie"], bk["class_task_map"], bk["task_seen"], weight.shape[0], cuda)
    acc = np.zeros(bk["n_loaders"])
    for task in range(bk["n_loaders"]):
        mine = [(l, y) for t, l, y in batches if t == task]
        ea.begin_loader(task, sum(len(y) for _, y in mine))
        for l, y in mine:
            ea.batch(_dev(l, cuda), y)
        acc[task] = E._avg([(c / n, n) for c, n in ea.end_loader()])
    return acc, ea.end(SimpleNamespace(weight=_dev(weight, cuda), bias=_dev(bias, cuda)))


def test_recorded_logits_through_the_pipeline_reproduce_the_recorded_outputs(cuda):
    """tests/golden/error_analysis.npz: the reference's own logits, uploaded and fed batch by batch through error_analysis.py.  Tuples,
    confusion lists and accuracies exact (the fixture has no top-2 tie); scores and norms within the bound of the reference's float32
    means."""
    from ocl_amd import error_analysis as EA
    g = gold("error_analysis")
    for e in range(int(g["n_evaluates"])):
        batches, bk, weight, bias, out = E.golden_evaluate(g, e)
        ea = EA.ErrorAnalysis()
        acc, norms = _drive(ea, batches, bk, weight, bias, cuda)
        assert ea.error_tuple() == out["error"] == E.EA_RECORDED_TUPLES[e]
        assert [ea.correct_lb, ea.predict_lb] == out["confusion"] and np.array_equal(acc, out["acc"])
        for which, got in (("new", ea.new_class_score.avg()), ("old", ea.old_class_score.avg())):
            want, bound = out[which + "_class_score"], E.score_bound(batches, bk, which)
            print("evaluate %d %s score %.9g recorded %.9g |diff| %.3g bound %.3g" % (e, which, got, want, abs(got - want), bound))
            assert E.close(got, want, bound), (e, which, got, want, bound)
        bounds = E.norm_bounds(weight, bias, bk)
        for k in bounds:
            print("evaluate %d %s %.9g recorded %.9g |diff| %.3g bound %.3g" % (e, k, norms[k], out[k], abs(norms[k] - out[k]), bounds[k]))
            assert E.close(norms[k], out[k], bounds[k]), (e, k, norms[k], out[k], bounds[k])


# ---- 5. the agent ---------------------------------------------------------------------------------------------------------------------

LISTS = ("error_list", "new_class_score", "old_class_score", "fc_norm_new", "fc_norm_old", "bias_norm_new", "bias_norm_old")


@pytest.fixture(scope="module")
def agent_run(cuda, tmp_path_factory):
    """ER on the engine through the three tasks of the recorded case's stream with error_analysis on.  After each task, from the same
    host RNG state (the test loaders shuffle): evaluate() with the fused path (its kernel calls, copies and batches recorded), the
    batches forwarded a second time, evaluate() with the flag off, and evaluate() with the torch-statement leg."""
    from ocl_amd import ops, error_analysis as EA
    from ocl_amd.data import setup_test_loader
    cfg = E.EA_CASE
    params, model, _, agent = build_agent(cfg, test_batch=E.EA_TEST_BATCH, error_analysis=True)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    launches, copies, items, seen, forwards = [], [], [], [], []
    recs = []
    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(tmp_path_factory.mktemp("error_analysis"))
        inner_op, inner_copy, inner_item, inner_batch, inner_forward = ops.row_argmax_groupsum, EA.to_host, EA.item, EA.ErrorAnalysis.batch, model.forward
        mp.setattr(ops, "row_argmax_groupsum", lambda *a, **k: (launches.append(tuple(a[0].shape)), inner_op(*a, **k))[1])
        mp.setattr(EA, "to_host", lambda t: (copies.append(tuple(t.shape)), inner_copy(t))[1])
        mp.setattr(EA, "item", lambda t: (items.append(1), inner_item(t))[1])

        def batch(self, logits, y_host):
            seen.append((self.task, logits.clone(), np.asarray(y_host).copy()))
            return inner_batch(self, logits, y_host)

        def forward(x):
            out = inner_forward(x)
            if not model.training:
                forwards.append((x.clone(), out.clone()))
            return out

        mp.setattr(EA.ErrorAnalysis, "batch", batch)
        mp.setattr(model, "forward", forward)
        for x, y in tasks:
            agent.train_learner(x, y)
            for buf in (launches, copies, items, seen, forwards):
                del buf[:]
            st = _rng_get()
            acc = agent.evaluate(loaders)
            rec = SimpleNamespace(acc=acc, launches=list(launches), copies=list(copies), items=len(items), seen=list(seen),
                                  fused={k: copy.deepcopy(getattr(agent, k)) for k in LISTS}, confusion=copy.deepcopy(agent.confusion),
                                  pickled=pickle.load(open("confusion", "rb")), task_seen=agent.task_seen, n_forwards=len(forwards),
                                  bk=dict(old_labels=list(agent.old_labels), new_labels_zombie=list(agent.new_labels_zombie),
                                          class_task_map=dict(agent.class_task_map), task_seen=agent.task_seen, n_loaders=len(loaders)),
                                  weight=_host(model.linear.weight), bias=_host(model.linear.bias))
            # a second eval forward over the same batches: the same bits
            assert not model.training
            rec.again = [inner_forward(x_) for x_, _ in forwards]
            rec.first = [out for _, out in forwards]
            saved = {k: copy.deepcopy(getattr(agent, k)) for k in LISTS}
            # the flag off, from the same RNG state
            n_launches = len(launches)
            _rng_set(st)
            params.error_analysis = False
            try:
                rec.acc_off = agent.evaluate(loaders)
            finally:
                params.error_analysis = True
            rec.off_launches = len(launches) - n_launches
            rec.off_lists = {k: copy.deepcopy(getattr(agent, k)) for k in LISTS}
            # the torch-statement leg, from the same RNG state
            _rng_set(st)
            n_launches, n_copies = len(launches), len(copies)
            del items[:]
            agent._force_torch_error_analysis = True
            try:
                rec.acc_torch = agent.evaluate(loaders)
            finally:
                agent._force_torch_error_analysis = False
            rec.torch = {k: copy.deepcopy(getattr(agent, k)) for k in LISTS}
            rec.torch_confusion = copy.deepcopy(agent.confusion)
            rec.torch_launches, rec.torch_copies, rec.torch_items = len(launches) - n_launches, len(copies) - n_copies, len(items)
            for k in LISTS:                     # the comparator's appends are taken back: the next task sees the fused path's lists
                getattr(agent, k)[:] = saved[k]
            recs.append(rec)
    return recs


def test_evaluate_equals_the_float64_statement_on_the_engines_own_logits(agent_run):
    """After each task: the second eval forward gives the bits of the first, those logits hold no exact top-2 tie, and evaluate()'s
    outputs are ref_error_analysis of them: the tuple (Python ints), the confusion lists and acc_array exact; the scores and norms within
    twice the round-off of a float64 mean (both sides sum the same terms in double, in different orders)."""
    for t, rec in enumerate(agent_run):
        assert rec.task_seen == t + 1 and rec.n_forwards == len(rec.seen) == 9
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rec.first, rec.again)), "a second eval forward gives other bits"
        assert all(torch.equal(_bits(l), _bits(f)) for (_, l, _), f in zip(rec.seen, rec.first))
        batches = [(task, _host(l), y) for task, l, y in rec.seen]
        assert [len(y) for _, _, y in batches] == [16, 16, 8] * 3 and [b[0] for b in batches] == [0] * 3 + [1] * 3 + [2] * 3
        assert not any(E.top2_tie(l).any() for _, l, _ in batches), "the engine's logits hold an exact top-2 tie"
        tup, new_s, old_s, confusion, acc = ref_error_analysis(batches, rec.bk)
        got = rec.fused
        assert all(len(got[k]) == t + 1 for k in LISTS)
        assert got["error_list"][-1] == tup and all(type(v) is int for v in got["error_list"][-1])
        assert rec.confusion == confusion and np.array_equal(rec.acc, acc)
        for which, want in (("new", new_s), ("old", old_s)):
            bound = 2 * E.score_bound(batches, rec.bk, which, u=E.U64)
            print("task %d %s score %.12g statement %.12g |diff| %.3g bound %.3g" % (t, which, got[which + "_class_score"][-1], want,
                                                                                      abs(got[which + "_class_score"][-1] - want), bound))
            assert E.close(got[which + "_class_score"][-1], want, bound)
        norms, bounds = ref_norms(rec.weight, rec.bias, rec.bk), E.norm_bounds(rec.weight, rec.bias, rec.bk, u=E.U64)
        for k, want in norms.items():
            assert E.close(got[k][-1], want, 2 * bounds[k]), (t, k, got[k][-1], want, bounds[k])
    first = agent_run[0].fused
    assert np.isnan(first["fc_norm_old"][0]) and np.isnan(first["bias_norm_old"][0]) and first["old_class_score"][0] == 0
    assert first["error_list"][0][2:] == (0, 0)


def test_acc_array_is_bit_equal_to_the_flag_off_path_which_launches_nothing_new(agent_run):
    for t, rec in enumerate(agent_run):
        assert rec.acc.tobytes() == rec.acc_off.tobytes() == rec.acc_torch.tobytes(), (t, rec.acc, rec.acc_off)
        assert rec.off_launches == 0, "the flag-off path launched the error analysis' kernel"
        assert rec.off_lists["error_list"] == rec.fused["error_list"], "the flag-off path appended to the result lists"
        assert all(np.array_equal(rec.off_lists[k], rec.fused[k], equal_nan=True) for k in LISTS if k != "error_list")


def test_fused_path_and_torch_statement_leg_agree(agent_run):
    """Counts and confusion lists exactly; scores and norms within the bound of the comparator's float32 means."""
    for t, rec in enumerate(agent_run):
        batches = [(task, _host(l), y) for task, l, y in rec.seen]
        a, b = rec.fused, rec.torch
        assert all(len(b[k]) == len(a[k]) + 1 for k in LISTS), "the comparator appended nothing"
        assert b["error_list"][-1] == a["error_list"][-1] and rec.torch_confusion == rec.confusion
        assert E.close(b["new_class_score"][-1], a["new_class_score"][-1], E.score_bound(batches, rec.bk, "new"))
        assert E.close(b["old_class_score"][-1], a["old_class_score"][-1], E.score_bound(batches, rec.bk, "old"))
        bounds = E.norm_bounds(rec.weight, rec.bias, rec.bk)
        for k in bounds:
            assert E.close(b[k][-1], a[k][-1], bounds[k]), (t, k, b[k][-1], a[k][-1], bounds[k])
        assert rec.torch_launches == 0 and rec.torch_copies == 0, "the comparator went through the fused path"
        # one read per predicted label and one per batch's correct count at the least; then the wrong-prediction counts, the means, the norms
        assert rec.torch_items >= 120 + 9 + 4, "the comparator reads its values through the host one by one"


def test_one_launch_per_batch_and_one_copy_per_loader(agent_run):
    """One kernel per test batch plus one per evaluate (the last layer's weight); one device-to-host copy per loader plus one at the end;
    no value read through the host one by one."""
    for t, rec in enumerate(agent_run):
        assert rec.launches == [(16, 10), (16, 10), (8, 10)] * 3 + [(10, 160)], rec.launches
        assert rec.copies == [(80,) if task <= t else (40,) for task in range(3)] + [(20,)], rec.copies
        assert rec.items == 0


def test_the_confusion_file_unpickles_to_the_agents_confusion(agent_run):
    for rec in agent_run:
        assert rec.pickled == rec.confusion and len(rec.confusion) == 2 and len(rec.confusion[0]) == len(rec.confusion[1]) == 120
        assert rec.confusion[0] == [0] * 40 + [1] * 40 + [2] * 40 and set(rec.confusion[1]) <= set(range(rec.task_seen))
