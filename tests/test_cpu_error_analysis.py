"""CPU: the host side of evaluate()'s error analysis (the argument checks of csrc/rowstats.hip's entry point and of
ops.row_argmax_groupsum, the constructor's rules, the kernel's use of scratch, error_analysis.py's bookkeeping driven with a stand-in for
the op) and the references the GPU tests rely on (tests/error_analysis_ref.py): the float64 statement of the kernel on rows made by hand,
and the restatement of the reference's branch against its recorded run (tests/golden/error_analysis.npz) and against the reference
itself."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from ocl_amd.agents.base import ContinualLearner
from conftest import gold, ROOT
from oracle import ref_import
import error_analysis_ref as E
from error_analysis_ref import ref_row_argmax_groupsum, ref_error_analysis, ref_norms

OCL_ERR_ARG = -1    # include/ocl_hip.h
HIPCC = "/opt/rocm/bin/hipcc"
TRICK = {'labels_trick': False, 'kd_trick': False, 'separated_softmax': False, 'review_trick': False, 'ncm_trick': False,
         'kd_trick_star': False}


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # a host address: never dereferenced, every case below is refused first
MB = 1 << 24
N, CC = 4, 8
X_BYTES, G_BYTES, OUT_BYTES = N * CC * 4, CC * 4, N * 8


def _call(**over):
    kw = dict(x=A, n=N, c=CC, group=A + MB, sel=0, am=A + 2 * MB, sm=A + 3 * MB)
    kw.update(over)
    for out in ("am", "sm"):
        if out + "_at" in kw:              # an output placed relative to another array (an id must not carry a process address)
            kw[out] = kw[kw[out + "_at"][0]] + kw[out + "_at"][1]
    rc = ffi.lib().ocl_row_argmax_groupsum(ffi.vp(kw["x"]), kw["n"], kw["c"], ffi.vp(kw["group"]), kw["sel"], ffi.vp(kw["am"]), ffi.vp(kw["sm"]),
                                           ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signature_is_registered_and_declared():
    vp, i = ffi.vp, C.c_int
    assert ffi.SIGNATURES["ocl_row_argmax_groupsum"] == (C.c_int, [vp, i, i, vp, i, vp, vp, vp])
    header = open(ROOT + "/include/ocl_hip.h").read()
    assert hasattr(ffi.lib(), "ocl_row_argmax_groupsum") and re.search(r"\bocl_row_argmax_groupsum\(", header)
    assert "rowstats.hip" in open(ROOT + "/online-continual-learning_amd/csrc/Makefile").read()


@pytest.mark.parametrize("over", [
    dict(x=0), dict(am=0, sm=0),
    dict(n=0), dict(n=-3), dict(c=0), dict(c=-1),
    dict(am_at=("x", 0)), dict(am_at=("x", X_BYTES - 4)), dict(am_at=("x", 4 - OUT_BYTES)),             # on, ending inside, starting inside
    dict(sm_at=("x", 0)), dict(sm_at=("x", X_BYTES - 4)), dict(sm_at=("x", 4 - OUT_BYTES)),
    dict(am_at=("group", 0)), dict(am_at=("group", G_BYTES - 4)), dict(am_at=("group", 4 - OUT_BYTES)),
    dict(sm_at=("group", 0)), dict(sm_at=("group", G_BYTES - 4)), dict(sm_at=("group", 4 - OUT_BYTES)),
    dict(sm_at=("am", 0)), dict(sm_at=("am", OUT_BYTES - 4)), dict(sm_at=("am", 4 - OUT_BYTES)),
    dict(sm=0, am_at=("x", 8)), dict(am=0, sm_at=("group", 8)),
], ids=lambda o: ",".join("%s=%s" % (k, "%s%+d" % v if isinstance(v, tuple) else v) for k, v in o.items()))
def test_entry_point_refuses_bad_arguments_without_a_device(over):
    rc, msg = _call(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("row_argmax_groupsum:"), msg
    for out, name in (("am", "argmax_out"), ("sm", "sum_out")):
        if out + "_at" in over:
            other = {"x": "x", "group": "col_group", "am": "argmax_out"}[over[out + "_at"][0]]
            assert "overlaps" in msg and name in msg and other in msg, msg


def test_ops_wrapper_refuses_wrong_dtype_shape_layout_and_device_without_a_device():
    """Every check of ops.row_argmax_groupsum comes before the library is initialised: CPU tensors are enough to reach each of them (a
    well-formed set of CPU tensors is refused for its device)."""
    from ocl_amd import ops
    x, g = torch.zeros(4, 8), torch.zeros(8, dtype=torch.int32)
    wide = torch.zeros(4, 16)
    bad = [
        ("x dtype", dict(x=x.double())), ("x rank", dict(x=x.reshape(-1))), ("x layout", dict(x=wide[:, :8])), ("x transposed", dict(x=torch.zeros(8, 4).t())),
        ("x rows", dict(x=torch.zeros(0, 8))), ("x columns", dict(x=torch.zeros(4, 0), col_group=None)), ("x not a tensor", dict(x=np.zeros((4, 8), np.float32))),
        ("col_group dtype", dict(col_group=g.long())), ("col_group shape", dict(col_group=torch.zeros(7, dtype=torch.int32))),
        ("col_group rank", dict(col_group=g.reshape(1, 8))), ("col_group layout", dict(col_group=torch.zeros(16, dtype=torch.int32)[::2])),
        ("nothing asked for", dict(want_argmax=False, want_sum=False)),
        ("argmax_out dtype", dict(argmax_out=torch.zeros(4, dtype=torch.int32))), ("argmax_out shape", dict(argmax_out=torch.zeros(5, dtype=torch.int64))),
        ("argmax_out layout", dict(argmax_out=torch.zeros(8, dtype=torch.int64)[::2])),
        ("sum_out dtype", dict(sum_out=torch.zeros(4))), ("sum_out shape", dict(sum_out=torch.zeros(3, dtype=torch.float64))),
        ("sum_out layout", dict(sum_out=torch.zeros(8, dtype=torch.float64)[::2])),
    ]
    for what, over in bad:
        kw = dict(x=x, col_group=g)
        kw.update(over)
        with pytest.raises(RuntimeError, match="row_argmax_groupsum"):
            ops.row_argmax_groupsum(**kw)
    for kw in (dict(), dict(col_group=g), dict(argmax_out=torch.zeros(4, dtype=torch.int64), sum_out=torch.zeros(4, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="GPU"):
            ops.row_argmax_groupsum(x, **kw)


# ---- the float64 statement on rows made by hand -------------------------------------------------------------------------------------------

def test_float64_statement_on_hand_made_rows():
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, 5.0, 5.0, 2.0],           # a tie: the first of the maxima
                  [nan, 9.0, nan, 1.0],           # a NaN first
                  [3.0, inf, nan, nan],           # a NaN later: above +inf, the first of the NaNs
                  [-0.0, 0.0, -1.0, -0.0],        # the signed zeros are equal: the first
                  [0.0, -0.0, -1.0, -2.0],
                  [-inf, -inf, -inf, -inf]], dtype=np.float32)
    am, sums = ref_row_argmax_groupsum(x, None, 0)
    assert am.tolist() == [1, 0, 2, 0, 0, 0] and am.dtype == np.int64 and sums.dtype == np.float64
    assert sums[0] == 13.0 and np.isnan(sums[1]) and np.isnan(sums[2]) and sums[3] == -1.0 and sums[4] == -3.0 and sums[5] == -inf
    # groups: the columns outside the selection are not looked at, NaN and Inf included
    group = np.array([0, 1, -1, 0], dtype=np.int32)
    am_g, s0 = ref_row_argmax_groupsum(x, group, 0)
    _, s1 = ref_row_argmax_groupsum(x, group, 1)
    assert np.array_equal(am_g, am), "the arg-max does not depend on the group table"
    assert s0[0] == 3.0 and s1[0] == 5.0
    assert np.isnan(s0[1]) and s1[1] == 9.0               # row 1: the NaN of column 0 is in group 0; group 1 holds 9 alone
    assert np.isnan(s0[2]) and s1[2] == inf               # row 2: column 3's NaN is in group 0; the NaN of column 2 (group -1) touches neither
    _, s_m1 = ref_row_argmax_groupsum(x, group, -1)
    assert s_m1[0] == 5.0 and np.isnan(s_m1[1]) and s_m1[3] == -1.0
    # an empty group: +0.0
    _, s_e = ref_row_argmax_groupsum(x, group, 7)
    assert np.array_equal(s_e, np.zeros(6)) and not np.signbit(s_e).any()
    # c = 1
    am1, s1c = ref_row_argmax_groupsum(np.array([[2.5], [nan], [-inf]], dtype=np.float32), None, 0)
    assert am1.tolist() == [0, 0, 0] and s1c[0] == 2.5 and np.isnan(s1c[1]) and s1c[2] == -inf
    # the sum is a float64 sum of the float32 values: 2^24 + 1 + 1 is exact there and not in float32
    _, s_big = ref_row_argmax_groupsum(np.array([[2.0 ** 24, 1.0, 1.0]], dtype=np.float32), None, 0)
    assert s_big[0] == 2.0 ** 24 + 2.0
    assert E.top2_tie(x).tolist() == [True, False, False, True, True, True] and not E.top2_tie(np.array([[1.0, 2.0]])).any()


def test_statement_agrees_with_torch_max_on_the_cpu():
    """torch.max(x, 1) on the CPU is the order the kernel restates (NaN largest, the first of equals)."""
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (200, 9)).astype(np.float32)      # small integers: plenty of ties, and both zeros
    x[x == 0] = rng.choice([0.0, -0.0], int((x == 0).sum()))
    x[rng.random(x.shape) < 0.03] = np.nan
    x[rng.random(x.shape) < 0.03] = np.inf
    am, _ = ref_row_argmax_groupsum(x, None, 0)
    assert np.array_equal(am, torch.max(torch.from_numpy(x), 1)[1].numpy())


# ---- the restatement against the recorded run and the reference ---------------------------------------------------------------------------

def _check_against_recorded(batches, bk, weight, bias, out):
    tup, new_s, old_s, confusion, acc = ref_error_analysis(batches, bk)
    assert not any(E.top2_tie(l).any() for _, l, _ in batches), "the fixture has an exact tie between a row's two largest logits"
    assert tup == out["error"] and confusion == out["confusion"] and np.array_equal(acc, out["acc"])
    for which, got in (("new", new_s), ("old", old_s)):
        want, bound = out[which + "_class_score"], E.score_bound(batches, bk, which)
        print("%s score %.9g recorded %.9g  |diff| %.3g  bound %.3g" % (which, got, want, abs(got - want), bound))
        assert E.close(got, want, bound), (which, got, want, bound)
    norms, bounds = ref_norms(weight, bias, bk), E.norm_bounds(weight, bias, bk)
    for k, got in norms.items():
        print("%s %.9g recorded %.9g  |diff| %.3g  bound %.3g" % (k, got, out[k], abs(got - out[k]), bounds[k]))
        assert E.close(got, out[k], bounds[k]), (k, got, out[k], bounds[k])


def test_ref_error_analysis_reproduces_the_recorded_reference_run():
    g = gold("error_analysis")
    assert int(g["n_evaluates"]) == 3 and int(g["n_loaders"]) == 3
    tuples = []
    for e in range(3):
        batches, bk, weight, bias, out = E.golden_evaluate(g, e)
        assert [len(y) for _, _, y in batches] == [16, 16, 8] * 3 and [t for t, _, _ in batches] == [0] * 3 + [1] * 3 + [2] * 3
        assert bk["task_seen"] == e + 1 and weight.shape == (10, 160) and weight.dtype == np.float32
        _check_against_recorded(batches, bk, weight, bias, out)
        tuples.append(out["error"])
    assert tuples == E.EA_RECORDED_TUPLES
    first = E.golden_evaluate(g, 0)[4]
    assert np.isnan(first["fc_norm_old"]) and np.isnan(first["bias_norm_old"]) and first["old_class_score"] == 0


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_ref_error_analysis_equals_the_reference_agent_on_a_second_seed():
    sys.path.insert(0, ROOT + "/scripts")
    try:
        import make_error_analysis_golden as M
    finally:
        sys.path.remove(ROOT + "/scripts")
    torch.set_num_threads(1)
    recs = M.run_reference_case(dict(E.EA_CASE, seed=E.LIVE_SEED))
    assert len(recs) == 3
    g = {"e%d_%s" % (e, k): v for e, r in enumerate(recs) for k, v in r.items()}
    g["n_loaders"] = 3
    for e in range(3):
        _check_against_recorded(*E.golden_evaluate(g, e))


# ---- the constructor ----------------------------------------------------------------------------------------------------------------------

class _Learner(ContinualLearner):
    def train_learner(self, x_train, y_train):
        pass


def _params(**over):
    p = dict(agent="ER", data="cifar10", cuda=False, epoch=1, batch=10, verbose=False, error_analysis=True, trick=dict(TRICK))
    p.update(over)
    return SimpleNamespace(**p)


def test_constructor_accepts_the_flag_and_refuses_it_with_ncm_prediction():
    model = torch.nn.Linear(2, 2)
    a = _Learner(model, None, _params())
    for name in ("error_list", "new_class_score", "old_class_score", "fc_norm_new", "fc_norm_old", "bias_norm_new", "bias_norm_old"):
        assert getattr(a, name) == [], name
    assert len({id(getattr(a, n)) for n in ("error_list", "new_class_score", "old_class_score", "fc_norm_new", "fc_norm_old", "bias_norm_new",
                                            "bias_norm_old")}) == 7
    assert ContinualLearner._force_torch_error_analysis is False
    for over in (dict(trick=dict(TRICK, ncm_trick=True)), dict(agent="ICARL"), dict(agent="SCR"), dict(agent="SCP")):
        with pytest.raises(NotImplementedError, match="nearest-class-mean"):
            _Learner(model, None, _params(**over))
        _Learner(model, None, _params(error_analysis=False, **over))       # without the flag nothing is refused
    for trick in ("labels_trick", "separated_softmax", "kd_trick", "kd_trick_star", "review_trick"):
        _Learner(model, None, _params(trick=dict(TRICK, **{trick: True})))


# ---- error_analysis.py driven with a stand-in for the op ----------------------------------------------------------------------------------

def _stub_op(monkeypatch):
    """ops.row_argmax_groupsum and ops.upload on CPU tensors, from the float64 statement; returns the list of calls."""
    from ocl_amd import ops
    calls = []

    def row_argmax_groupsum(x, col_group=None, sel=0, want_argmax=True, want_sum=True, argmax_out=None, sum_out=None):
        am, sums = ref_row_argmax_groupsum(x.numpy(), None if col_group is None else col_group.numpy(), sel)
        calls.append((tuple(x.shape), col_group is not None, sel, argmax_out is not None, sum_out is not None))
        if argmax_out is not None:
            argmax_out.copy_(torch.from_numpy(am))
        if sum_out is not None:
            sum_out.copy_(torch.from_numpy(sums))
        return argmax_out, sum_out

    monkeypatch.setattr(ops, "row_argmax_groupsum", row_argmax_groupsum)
    monkeypatch.setattr(ops, "upload", lambda t, device: t.clone())
    return calls


def _drive(ea, batches, bk, weight, bias):
    ea.begin(bk["old_labels"], bk["new_labels_zombie"], bk["class_task_map"], bk["task_seen"], weight.shape[0], torch.device("cpu"))
    acc = np.zeros(bk["n_loaders"])
    for task in range(bk["n_loaders"]):
        mine = [(l, y) for t, l, y in batches if t == task]
        ea.begin_loader(task, sum(len(y) for _, y in mine))
        for l, y in mine:
            ea.batch(torch.from_numpy(np.ascontiguousarray(l)), y)
        pairs = ea.end_loader()
        acc[task] = E._avg([(c / n, n) for c, n in pairs])
    linear = SimpleNamespace(weight=torch.from_numpy(weight), bias=torch.from_numpy(bias))
    return acc, ea.end(linear)


@pytest.mark.parametrize("leg", ["fused", "torch"])
def test_host_bookkeeping_reproduces_the_recorded_run(monkeypatch, leg):
    """Both legs of error_analysis.py on the recorded logits (the fused one over a stand-in for the kernel): tuples, confusion lists and
    accuracies exact, scores and norms within the bound of the reference's float32 means.  The fused leg: one op call per batch and one
    per evaluate, one copy per loader and one at the end."""
    from ocl_amd import error_analysis as EA
    calls = _stub_op(monkeypatch)
    copies = []
    inner = EA.to_host
    monkeypatch.setattr(EA, "to_host", lambda t: (copies.append(tuple(t.shape)), inner(t))[1])
    g = gold("error_analysis")
    for e in range(3):
        batches, bk, weight, bias, out = E.golden_evaluate(g, e)
        del calls[:], copies[:]
        ea = EA.ErrorAnalysis() if leg == "fused" else EA.TorchErrorAnalysis()
        acc, norms = _drive(ea, batches, bk, weight, bias)
        assert ea.error_tuple() == out["error"] and all(type(v) is int for v in ea.error_tuple())
        assert [ea.correct_lb, ea.predict_lb] == out["confusion"] and np.array_equal(acc, out["acc"])
        assert E.close(ea.new_class_score.avg(), out["new_class_score"], E.score_bound(batches, bk, "new"))
        assert E.close(ea.old_class_score.avg(), out["old_class_score"], E.score_bound(batches, bk, "old"))
        bounds = E.norm_bounds(weight, bias, bk)
        for k in bounds:
            assert E.close(norms[k], out[k], bounds[k]), (k, norms[k], out[k])
        if leg == "fused":
            assert len(calls) == 9 + 1 and len(copies) == 3 + 1
            # loaders of tasks not trained yet: the arg-max alone, no group table; the last call: the weight's row sums alone
            for (shape, has_group, sel, has_am, has_sum), (t, l, _) in zip(calls[:9], batches):
                kind = 0 if t < e else (1 if t == e else None)
                assert shape == l.shape and has_am and has_sum == (kind is not None) == has_group and sel == (kind or 0)
            assert calls[9] == ((10, 160), False, 0, False, True)
            assert copies == [(80,) if t <= e else (40,) for t in range(3)] + [(20,)]
        else:
            assert not calls and not copies


def test_a_prediction_of_an_unseen_class_raises_key_error(monkeypatch):
    """The reference's class_task_map[pred] raises KeyError(label) for a class no task has introduced; here at the loader's one
    synchronisation."""
    from ocl_amd import error_analysis as EA
    _stub_op(monkeypatch)
    for ea in (EA.ErrorAnalysis(), EA.TorchErrorAnalysis()):
        ea.begin([0, 1, 2, 3], [2, 3], {0: 0, 1: 0, 2: 1, 3: 1}, 2, 6, torch.device("cpu"))
        assert ea.group_host.tolist() == [0, 0, 1, 1, -1, -1] and ea.group_host.dtype == np.int32
        ea.begin_loader(0, 3)
        logits = torch.tensor([[5.0, 0, 0, 0, 0, 0], [0, 0, 0, 6.0, 0, 0], [0, 0, 0, 0, 0, 7.0]])
        with pytest.raises(KeyError) as err:
            ea.batch(logits, np.array([0, 0, 0]))
            ea.end_loader()
        assert err.value.args == (5,)


# ---- the kernels use no scratch ----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_rowstats_kernels_use_no_scratch_and_spill_nothing():
    """csrc/rowstats.hip for gfx950 with the compiler's resource remarks, parsed as tests/test_cpu_icarl.py parses icarl.hip's: both
    instantiations (row in registers or strided); no LDS (there is no cross-wave reduction)."""
    src = ROOT + "/online-continual-learning_amd/csrc/rowstats.hip"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            cur = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur).replace("void ", "").replace("ocl::", "")
            res[cur] = {}
        elif cur:
            for key in ("ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size"):
                if t.startswith(key):
                    res[cur][key] = int(re.search(r":\s*(\d+)", t).group(1))
    hits = {k: v for k, v in res.items() if re.fullmatch(r"row_argmax_groupsum_kernel<(true|false)>", k)}
    assert len(hits) == 2 and len(res) == 2, sorted(res)
    for k, v in hits.items():
        assert v == {"ScratchSize": 0, "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size": 0}, (k, v)
