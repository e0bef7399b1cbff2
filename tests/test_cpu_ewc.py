"""CPU: the host side of the EWC++ agent (the argument checks of csrc/ewc.hip's three entry points, the registries, the kernels' use of
scratch) and the references the GPU tests rely on (tests/ewc_ref.py): the float64 accumulate step with its round-off bound, the float32
statements of the moving average and the normalisation against torch running the reference's own expressions, and the restatement of
the reference's loop against the reference itself and against its recorded run (tests/golden/ewc.npz)."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from conftest import gold, ROOT
from oracle import ref_import
from oracle.synth import make_stream, seed_all
from test_cpu_adam import make_grads
import ewc_ref
from ewc_ref import EWC_CASE, EWC_LOOPS_CASE, GOLDEN_KEYS, FISHER_KEYS

OCL_ERR_ARG = -1    # include/ocl_hip.h
HIPCC = "/opt/rocm/bin/hipcc"


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # 16-byte aligned host address: never dereferenced, every case below is refused first
MB = 1 << 24
ARRAYS = ("g", "t", "p", "q", "f")


def _id_value(v):
    """A case value for a pytest id: addresses as their offset from A (A itself differs from process to process, and an id must not)."""
    return "A+0x%x" % (v - A) if v >= A else str(v)


def _accumulate(**over):
    kw = dict(g=A, t=A + MB, p=A + 2 * MB, q=A + 3 * MB, f=A + 4 * MB, n=16, scale=2.0, ws=A + 5 * MB, ws_doubles=2, pen=A + 6 * MB)
    kw.update(over)
    rc = ffi.lib().ocl_ewc_accumulate(ffi.vp(kw["g"]), ffi.vp(kw["t"]), ffi.vp(kw["p"]), ffi.vp(kw["q"]), ffi.vp(kw["f"]), kw["n"], kw["scale"],
                                      ffi.vp(kw["ws"]), kw["ws_doubles"], ffi.vp(kw["pen"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def _ema(**over):
    kw = dict(r=A, t=A + MB, n=16)
    kw.update(over)
    rc = ffi.lib().ocl_ewc_fisher_ema(ffi.vp(kw["r"]), ffi.vp(kw["t"]), kw["n"], 0.1, 0.45, ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def _normalize(**over):
    kw = dict(r=A, f=A + MB, n=16, ws=A + 5 * MB, ws_floats=4, mm=A + 6 * MB)
    kw.update(over)
    rc = ffi.lib().ocl_ewc_fisher_normalize(ffi.vp(kw["r"]), ffi.vp(kw["f"]), kw["n"], ffi.vp(kw["ws"]), kw["ws_floats"], ffi.vp(kw["mm"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signatures_are_registered():
    vp, i64, f32 = ffi.vp, ffi.i64, C.c_float
    assert ffi.SIGNATURES["ocl_ewc_workspace_doubles"] == (i64, [i64])
    assert ffi.SIGNATURES["ocl_ewc_accumulate"] == (C.c_int, [vp, vp, vp, vp, vp, i64, f32, vp, i64, vp, vp])
    assert ffi.SIGNATURES["ocl_ewc_fisher_ema"] == (C.c_int, [vp, vp, i64, f32, f32, vp])
    assert ffi.SIGNATURES["ocl_ewc_fisher_normalize"] == (C.c_int, [vp, vp, i64, vp, i64, vp, vp])
    header = open(ROOT + "/include/ocl_hip.h").read()
    for name in ("ocl_ewc_workspace_doubles", "ocl_ewc_accumulate", "ocl_ewc_fisher_ema", "ocl_ewc_fisher_normalize"):
        assert hasattr(ffi.lib(), name) and re.search(r"\b%s\(" % name, header), name


@pytest.mark.parametrize("over", [
    dict(g=0), dict(t=0), dict(p=0),
    dict(q=0), dict(f=0),                               # one of the pair null, the other set
    dict(ws=0),                                         # penalty_out given: the workspace is needed
    dict(n=0), dict(n=-16),
    dict(ws_doubles=0), dict(n=4096, ws_doubles=3), dict(n=1 << 22, ws_doubles=511),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_accumulate_refuses_bad_arguments_without_a_device(over):
    rc, msg = _accumulate(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("ewc:"), msg


@pytest.mark.parametrize("which", ARRAYS)
def test_accumulate_refuses_each_array_misaligned_or_overlapping_without_a_device(which):
    base = dict(g=A, t=A + MB, p=A + 2 * MB, q=A + 3 * MB, f=A + 4 * MB)
    for shift in (4, 8):
        rc, msg = _accumulate(**{which: base[which] + shift})
        assert rc == OCL_ERR_ARG and msg.startswith("ewc:") and "aligned" in msg, (which, shift, rc, msg)
    for other in ARRAYS:
        if other == which:
            continue
        for at in (base[other], base[other] + 48, base[other] - 16):      # on it, inside it, ending inside it
            rc, msg = _accumulate(**{which: at})
            assert rc == OCL_ERR_ARG and msg.startswith("ewc:") and "overlap" in msg, (which, other, rc, msg)
    rc, msg = _accumulate(**{which: A + 5 * MB - 16})                     # ends inside the workspace
    assert rc == OCL_ERR_ARG and msg.startswith("ewc:") and "overlap" in msg, (which, rc, msg)
    rc, msg = _accumulate(ws=A + 5 * MB + 4)
    assert rc == OCL_ERR_ARG and msg.startswith("ewc:") and "aligned" in msg, (rc, msg)


@pytest.mark.parametrize("call,over", [
    (_ema, dict(r=0)), (_ema, dict(t=0)), (_ema, dict(n=0)), (_ema, dict(n=-1)), (_ema, dict(r=A + 4)), (_ema, dict(t=A + MB + 8)),
    (_ema, dict(t=A)), (_ema, dict(t=A + 48)), (_ema, dict(r=A + MB - 16)),
    (_normalize, dict(r=0)), (_normalize, dict(f=0)), (_normalize, dict(ws=0)), (_normalize, dict(n=0)), (_normalize, dict(n=-1)),
    (_normalize, dict(r=A + 4)), (_normalize, dict(f=A + MB + 8)), (_normalize, dict(ws=A + 5 * MB + 2)), (_normalize, dict(f=A)),
    (_normalize, dict(f=A + 48)), (_normalize, dict(ws=A + 32)), (_normalize, dict(mm=A + 16)),
    (_normalize, dict(ws_floats=1)), (_normalize, dict(n=4096, ws_floats=7)), (_normalize, dict(n=1 << 22, ws_floats=1023)),
], ids=lambda v: v.__name__ if callable(v) else ",".join("%s=%s" % (k, _id_value(x)) for k, x in v.items()))
def test_ema_and_normalize_refuse_bad_arguments_without_a_device(call, over):
    rc, msg = call(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("ewc:"), msg


def test_workspace_size_is_small_even_positive_and_monotone():
    """One double per block for the penalty's partials; even, so that the same workspace read as floats holds whole [min, max] pairs
    of doubles' width; at most 512 blocks."""
    f = ffi.lib().ocl_ewc_workspace_doubles
    sizes = [1, 2, 3, 4, 5, 1003, 1024, 1025, 4099, 65536, 524288, 524289, 1094750, 1109240, 1 << 24, 1 << 31, 1 << 40]
    got = [f(n) for n in sizes]
    assert all(0 < w <= 512 and w % 2 == 0 for w in got), got
    assert got == sorted(got) and got[0] == 2 and got[-1] == 512, got
    assert f(0) > 0 and f(-5) > 0


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_ewc_is_a_regularization_agent_and_the_other_tables_are_unchanged():
    from ocl_amd import name_match
    from ocl_amd.agents.agem import AGEM
    from ocl_amd.agents.ewc_pp import EWC_pp
    from ocl_amd.agents.exp_replay import ExperienceReplay
    from ocl_amd.agents.scr import SupContrastReplay
    assert set(name_match.regularization_agents.keys()) == {"EWC"}
    assert name_match.get_agent("EWC") is EWC_pp is name_match.regularization_agents["EWC"]
    assert set(name_match.agents.keys()) == {"ER", "SCR"} and set(name_match.extra_agents.keys()) == {"AGEM"}
    assert name_match.get_agent("ER") is ExperienceReplay and name_match.get_agent("SCR") is SupContrastReplay and name_match.get_agent("AGEM") is AGEM
    with pytest.raises(KeyError):
        name_match.get_agent("nope")
    assert EWC_pp._force_torch_bookkeeping is False
    assert ExperienceReplay._kd_mix is EWC_pp._kd_mix and ExperienceReplay._kd_weight is EWC_pp._kd_weight


@pytest.mark.parametrize("trick,want", [({}, [1.0, 1.0, 1.0]), (dict(kd_trick=True), [1.0, 1 / 2, 1 / 3]),
                                        (dict(kd_trick_star=True), [1.0, 1 / 2 ** 0.5, 1 / 3 ** 0.5]),
                                        (dict(kd_trick=True, kd_trick_star=True), [1.0, 1 / 2 * (1 / 2 ** 0.5), 1 / 3 * (1 / 3 ** 0.5)])])
def test_kd_weight_is_the_factor_kd_mix_puts_on_the_loss(trick, want):
    """_kd_mix with a zero distillation term (no teacher) only scales: its factor is _kd_weight()."""
    from types import SimpleNamespace
    from ocl_amd.agents.base import ContinualLearner
    full = {k: False for k in ('labels_trick', 'kd_trick', 'separated_softmax', 'review_trick', 'ncm_trick', 'kd_trick_star')}
    full.update(trick)
    for t, w in enumerate(want):
        me = SimpleNamespace(params=SimpleNamespace(trick=full), task_seen=t, kd_manager=SimpleNamespace(get_kd_loss=lambda logits, x: 0.0))
        assert ContinualLearner._kd_weight(me) == pytest.approx(w, rel=1e-15)
        assert ContinualLearner._kd_mix(me, 3.0, None, None) == pytest.approx(3.0 * ContinualLearner._kd_weight(me), rel=1e-15)


# ---- the float64 accumulate step and its bound -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("n", [1, 3, 5, 1003, 100003])
def test_fp32_emulation_of_the_accumulate_step_stays_inside_the_bound(n, prev):
    """numpy float32 in the kernel's order of roundings, without and with the products fused into the sums the way an fma would (formed
    in float64 and rounded once): within 1 x accumulate_bounds; without prev, g is untouched."""
    rng = np.random.default_rng(300 + n)
    c = ewc_ref.make_case(rng, n, make_grads, prev=prev)
    for scale in ((0.0, 2.0, 200.0) if prev else (0.0,)):
        ref = ewc_ref.ref_accumulate(c.g, c.t, c.p, c.q, c.f, scale)
        assert ref.has_prev == (prev and scale != 0)
        if ref.has_prev:
            d = c.p - c.q
            sf = np.float32(scale) * c.f
            g1 = c.g + sf * d
            g1_fma = (c.g.astype(np.float64) + sf.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
        else:
            g1 = g1_fma = c.g
        for g_got in (g1, g1_fma):
            t1 = c.t + g_got * g_got
            t1_fma = (c.t.astype(np.float64) + g_got.astype(np.float64) ** 2).astype(np.float32)
            assert g_got.dtype == t1.dtype == np.float32
            for t_got in (t1, t1_fma):
                rg, rt = ewc_ref.worst_ratios(g_got, t_got, ref)
                print("fp32 emulation n=%d prev=%d scale=%g: worst |err| / bound g %.3f tmp %.3f" % (n, prev, scale, rg, rt))
                assert rg <= 1.0 and rt <= 1.0, (rg, rt)
        if prev:
            assert n < 3 or (ref.penalty > 0 and (c.f == 0).any() and (c.f == 1).any())
        else:
            assert ref.penalty == 0.0 and np.array_equal(ref.g1, c.g.astype(np.float64))


# ---- the float32 statements against torch running the reference's expressions --------------------------------------------------------

@pytest.mark.parametrize("alpha,fua", [(0.9, 2), (0.9, 50), (0.5, 3), (0.3, 7), (1.0, 1), (0.0, 1)])
def test_ema_float32_statement_equals_torch_on_the_reference_expression(alpha, fua):
    """ewc_pp.py:99-100 on float tensors and Python scalars: torch rounds each scalar to float32 and each of the three operations once.
    0-dim tensors (the scalar path) and a vector (the vectorised path) both."""
    rng = np.random.default_rng(int(alpha * 10) + fua)
    r = (make_grads(rng, 257, 1).astype(np.float64) ** 2).astype(np.float32)
    t = (make_grads(rng, 257, 1).astype(np.float64) ** 2).astype(np.float32)
    keep, gain = 1. - alpha, 1. / fua * alpha
    want = ewc_ref.ema_f32(r, t, keep, gain)
    rt, tt = torch.from_numpy(r), torch.from_numpy(t)
    got_vec = (1. - alpha) * rt + 1. / fua * alpha * tt
    got_0d = np.array([float((1. - alpha) * rt[i] + 1. / fua * alpha * tt[i]) for i in range(64)], dtype=np.float32)
    assert got_vec.dtype == torch.float32 and rt[0].dim() == 0
    assert np.array_equal(got_vec.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_0d.view(np.uint32), want[:64].view(np.uint32))
    exact, bound = ewc_ref.ref_ema(r, t, keep, gain)
    assert (np.abs(want.astype(np.float64) - exact) <= bound).all()


@pytest.mark.parametrize("kind", ["random", "zero", "constant", "nan"])
def test_normalize_float32_statement_equals_torch_on_the_reference_expression(kind):
    """ewc_pp.py:77-80 with min and max as 0-dim float tensors and 1e-32 as a Python scalar."""
    rng = np.random.default_rng(5)
    r = (make_grads(rng, 1003, 1).astype(np.float64) ** 2).astype(np.float32)
    if kind == "zero":
        r[:] = 0.0
    elif kind == "constant":
        r[:] = 0.37
    elif kind == "nan":
        r[500] = np.nan
    want, mm = ewc_ref.normalize_f32(r)
    rt = torch.from_numpy(r)
    pieces = [rt[:400], rt[400:900], rt[900:]]
    if kind == "nan":        # the builtin max() / min() over a list depend on where the NaN sits; within a tensor torch keeps it
        max_fisher, min_fisher = torch.max(rt), torch.min(rt)
        assert torch.isnan(max_fisher) and torch.isnan(min_fisher)
    else:
        max_fisher = max([torch.max(m) for m in pieces])
        min_fisher = min([torch.min(m) for m in pieces])
    assert max_fisher.dim() == 0 and max_fisher.dtype == torch.float32
    got = torch.cat([(p - min_fisher) / (max_fisher - min_fisher + 1e-32) for p in pieces]).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or (kind == "nan" and np.isnan(got).all() and np.isnan(want).all())
    assert np.array_equal(mm, np.array([float(min_fisher), float(max_fisher)], dtype=np.float32), equal_nan=True)
    if kind in ("zero", "constant"):
        assert not want.any()
    if kind == "random":
        assert want.min() == 0.0 and want.max() == 1.0
        exact, bound = ewc_ref.ref_normalize(r)
        assert (np.abs(want.astype(np.float64) - exact) <= bound).all()


# ---- the restatement against the reference and its recorded run ------------------------------------------------------------------------

def _assert_equals_reference(n_tasks):
    torch.set_num_threads(1)
    cfg = EWC_CASE
    ref_import.activate()
    params = ref_import.default_params(**ewc_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = ref_import.build_agent(params)
    tasks, _ = make_stream(cfg)
    with ref_import.quiet():
        for x, y in tasks[:n_tasks]:
            agent.train_learner(x, y)
    rng_ref = (torch.get_rng_state(), np.random.get_state())
    seed_all(cfg["seed"])
    ag = ewc_ref.EwcOracle(cfg)
    for x, y in tasks[:n_tasks]:
        ag.train_learner(x, y)
    assert torch.equal(rng_ref[0], torch.get_rng_state()), "torch's host RNG stream"
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(rng_ref[1], np.random.get_state())), "numpy's RNG stream"
    sd = model.state_dict()
    assert list(sd.keys()) == list(ag.state.keys())
    for k, v in sd.items():
        assert torch.equal(v, ag.state[k].detach()), k
    for which, theirs in zip(FISHER_KEYS, (agent.running_fisher, agent.tmp_fisher, agent.normalized_fisher, agent.prev_params)):
        mine = getattr(ag.ewc, which)
        assert list(theirs.keys()) == list(mine.keys()) == ag.names, which
        for k in theirs:
            assert torch.equal(theirs[k], mine[k]), (which, k)
    assert len(ag.log) == 6 * n_tasks and [e["ema"] for e in ag.log] == [False, True] * (3 * n_tasks)
    return ag


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_ewc_oracle_equals_the_reference_agent_over_task_one():
    ag = _assert_equals_reference(1)
    assert all(e["penalty"] == 0.0 for e in ag.log) and any(float(v.max()) > 0 for v in ag.ewc.normalized.values())


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_ewc_oracle_equals_the_reference_agent_over_all_three_tasks():
    ag = _assert_equals_reference(3)
    assert sum(e["penalty"] > 0 for e in ag.log) == 10


def test_ewc_oracle_free_run_reproduces_the_recorded_reference_run():
    """The weights are bit-equal only on a CPU whose float32 convolution and matrix kernels add in the order of the recording machine's,
    and they follow a chaotic trajectory: they get the sanity band of test_cpu_agem's free run, as the GPU free run does.  What does not
    depend on the trajectory is exact: the penalty is zero through the first task and on the first step of every later one (p == prev),
    positive otherwise, and lambda_ times it stays well below the cross-entropy."""
    g = gold("ewc")
    recs, ag = ewc_ref.run_oracle_case()
    assert len(recs) == int(g["ewc_c10_ntasks"]) == 3
    assert set(GOLDEN_KEYS) == {"acc", "state", "minmax", "running", "tmp", "normalized", "prev"}
    for t, rec in enumerate(recs):
        for k in ("state",) + FISHER_KEYS:
            ds, gs = rec[k], g["ewc_c10_t%d_%s" % (t, k)]
            assert ds.shape == gs.shape, (t, k)
            rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
            ratio = np.sqrt((ds[:, 1] ** 2).sum() / max((gs[:, 1] ** 2).sum(), 1e-300))
            print("ewc_c10 oracle", t, k, "digest rel err", rel, "norm ratio", ratio)
            assert np.isfinite(ds).all() and rel < 3.0, (t, k, rel)
            if k != "tmp":                       # (the temporary Fisher at a task's end is one step's squared gradient: no average to band)
                assert 0.5 < ratio < 2.0, (t, k, ratio)
        lo, hi = rec["minmax"]
        glo, ghi = g["ewc_c10_t%d_minmax" % t]
        print("ewc_c10 oracle", t, "running Fisher min / max", lo, hi, "recorded", glo, ghi, "acc", rec["acc"], g["ewc_c10_t%d_acc" % t])
        assert 0.0 <= lo < hi and 0.5 < hi / ghi < 2.0
        assert rec["acc"].shape == g["ewc_c10_t%d_acc" % t].shape and (rec["acc"] >= 0).all() and (rec["acc"] <= 1).all()
    ce, pen = np.array([e["ce"] for e in ag.log]), np.array([e["penalty"] for e in ag.log])
    assert len(ag.log) == 18 and g["ewc_c10_penalty"].shape == (18,)
    zero = [i in (0, 1, 2, 3, 4, 5, 6, 12) for i in range(18)]          # steps 1-7 and 13
    for name, p in (("recorded", g["ewc_c10_penalty"]), ("this machine", pen)):
        assert [(v == 0.0) for v in p] == zero and (p >= 0).all(), (name, p)
    lam = EWC_CASE["lambda_"]
    assert (lam * pen[~np.array(zero)] < ce[~np.array(zero)]).all() and (lam * pen).max() > 0.01
    assert np.abs(ce - g["ewc_c10_ce"]).max() < 1.0


# ---- the kernels use no scratch ----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_ewc_kernels_use_no_scratch():
    """csrc/ewc.hip for gfx950 with the compiler's resource remarks, parsed as tests/test_cpu_kernel_resources.py parses them: every
    kernel of the file, every instantiation."""
    src = ROOT + "/online-continual-learning_amd/csrc/ewc.hip"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    scratch, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            cur = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur).replace("void ", "").replace("ocl::", "")
        elif cur and t.startswith("ScratchSize"):
            scratch[cur] = int(re.search(r":\s*(\d+)", t).group(1))
    for pat, count in ((r"ewc_accumulate_kernel<(true|false), (true|false), (true|false)>", 5), (r"ewc_penalty_kernel", 1),
                       (r"ewc_fisher_ema_kernel", 1), (r"ewc_minmax_kernel", 1), (r"ewc_normalize_kernel", 1)):
        hits = {k: v for k, v in scratch.items() if re.fullmatch(pat, k)}
        assert len(hits) == count, (pat, sorted(scratch))
    assert len(scratch) == 9, sorted(scratch)
    bad = {k: v for k, v in scratch.items() if v}
    assert not bad, "scratch in an EWC++ kernel: %s" % bad


def test_ewc_oracle_two_epochs_reproduce_the_recorded_schedule_and_forward_counts():
    """ewc_loops (epoch 2, three batches per epoch, fisher_update_after 2): the reference's counter runs across the epochs
    (ewc_pp.py:41), so the running Fisher is updated at the task's iterations 1, 3, 5 -- i = 1 in the first epoch, i = 0 and 2 in the
    second -- and not at i = 1 twice.  The sequence and num_batches_tracked are exact against the reference's recording."""
    g = gold("ewc")
    recs, ag = ewc_ref.run_oracle_case(EWC_LOOPS_CASE)
    assert len(recs) == int(g["ewc_loops_ntasks"]) == 2
    for t, rec in enumerate(recs):
        assert np.array_equal(rec["ema_at"], g["ewc_loops_t%d_ema_at" % t]) and rec["ema_at"].tolist() == [1, 3, 5]
        assert np.array_equal(rec["nbt"], g["ewc_loops_t%d_nbt" % t]) and rec["nbt"].tolist() == [6 * (t + 1)] * 20
    assert [e["ema"] for e in ag.log] == [False, True, False, True, False, True] * 2
    assert "ewc_c10_t0_ema_at" not in g.files and "ewc_c10_t0_nbt" not in g.files
