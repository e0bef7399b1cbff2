"""CPU: the host side of the LwF agent (the argument checks of csrc/distill.hip's entry point and of ops.ce_kd_blend, the registries, the
kernels' use of scratch) and the references the GPU tests rely on (tests/lwf_ref.py): the float64 statement of the blended loss on cases
worked out by hand, the plain float32 statement against it, and the restatement of the reference's loop against the reference itself and
against its recorded run (tests/golden/lwf.npz)."""
import ctypes as C
import math
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
import lwf_ref
from lwf_ref import LWF_CASE, GOLDEN_KEYS, ref_blend, torch32_blend

OCL_ERR_ARG = -1    # include/ocl_hip.h
HIPCC = "/opt/rocm/bin/hipcc"


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # a host address: never dereferenced, every case below is refused first
MB = 1 << 24
N, CC = 4, 8
BYTES = N * CC * 4


def _blend(**over):
    kw = dict(logits=A, y=A + MB, teacher=A + 2 * MB, n=N, c=CC, T=2.0, w_new=0.5, w_old=0.5, loss=A + 3 * MB, dl=A + 4 * MB)
    kw.update(over)
    if "dl_at" in kw:                      # dlogits placed relative to another array (an id must not carry a process address)
        kw["dl"] = kw[kw["dl_at"][0]] + kw["dl_at"][1]
    rc = ffi.lib().ocl_ce_kd_blend_fwd_bwd(ffi.vp(kw["logits"]), ffi.vp(kw["y"]), ffi.vp(kw["teacher"]), kw["n"], kw["c"], kw["T"], kw["w_new"],
                                           kw["w_old"], ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signature_is_registered_and_declared():
    vp, f32 = ffi.vp, C.c_float
    assert ffi.SIGNATURES["ocl_ce_kd_blend_fwd_bwd"] == (C.c_int, [vp, vp, vp, C.c_int, C.c_int, f32, f32, f32, vp, vp, vp])
    header = open(ROOT + "/include/ocl_hip.h").read()
    assert hasattr(ffi.lib(), "ocl_ce_kd_blend_fwd_bwd") and re.search(r"\bocl_ce_kd_blend_fwd_bwd\(", header)
    assert "distill.hip" in open(ROOT + "/online-continual-learning_amd/csrc/Makefile").read()


@pytest.mark.parametrize("over", [
    dict(logits=0), dict(y=0), dict(loss=0),
    dict(n=0), dict(n=-3), dict(c=0), dict(c=-1),
    dict(T=0.0), dict(T=-2.0), dict(T=math.inf), dict(T=math.nan),
    dict(w_new=math.nan), dict(w_new=math.inf), dict(w_old=math.nan), dict(w_old=-math.inf),
    dict(dl_at=("logits", 0)), dict(dl_at=("logits", BYTES - 4)), dict(dl_at=("logits", 4 - BYTES)),     # on, ending inside, starting inside
    dict(dl_at=("teacher", 0)), dict(dl_at=("teacher", BYTES - 4)), dict(dl_at=("teacher", 4 - BYTES)),
], ids=lambda o: ",".join("%s=%s" % (k, "%s%+d" % v if isinstance(v, tuple) else v) for k, v in o.items()))
def test_entry_point_refuses_bad_arguments_without_a_device(over):
    rc, msg = _blend(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("ce_kd_blend:"), msg
    if "dl_at" in over:
        assert "overlaps " + over["dl_at"][0] in msg, msg


def test_ops_wrapper_refuses_wrong_dtype_shape_layout_and_device_without_a_device():
    """Every check of ops.ce_kd_blend comes before the library is initialised: CPU tensors are enough to reach each of them (a
    well-formed set of CPU tensors is refused for its device)."""
    from ocl_amd import ops
    s, y, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 8)
    wide = torch.zeros(4, 16)
    bad = [
        ("logits dtype", (s.double(), y, t)), ("logits rank", (s.reshape(-1), y, t)), ("logits layout", (wide[:, :8], y, t)),
        ("y dtype", (s, y.int(), t)), ("y shape", (s, y[:3], t)), ("y rank", (s, y.reshape(4, 1), t)), ("y layout", (s, torch.zeros(8, dtype=torch.int64)[::2], t)),
        ("teacher dtype", (s, y, t.double())), ("teacher shape", (s, y, torch.zeros(4, 7))), ("teacher layout", (s, y, wide[:, 8:])),
        ("teacher transposed", (s, y, torch.zeros(8, 4).t())),
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError, match="ce_kd_blend"):
            ops.ce_kd_blend(*args, 2.0, 0.5, 0.5)
    for what, dl in (("dl_out dtype", torch.zeros(4, 8, dtype=torch.float64)), ("dl_out shape", torch.zeros(5, 8)), ("dl_out layout", wide[:, :8])):
        with pytest.raises(RuntimeError, match="dl_out"):
            ops.ce_kd_blend(s, y, t, 2.0, 0.5, 0.5, dl_out=dl)
    for teacher in (t, None):
        with pytest.raises(RuntimeError, match="GPU"):
            ops.ce_kd_blend(s, y, teacher, 2.0, 0.5, 0.5)


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_lwf_resolves_by_name_and_the_baseline_table_is_unchanged():
    from ocl_amd import name_match
    from ocl_amd.agents.lwf import Lwf
    from ocl_amd.agents.base import ContinualLearner
    assert name_match.get_agent("LWF") is Lwf and issubclass(Lwf, ContinualLearner)
    assert "LWF" not in name_match.agents and set(name_match.agents.keys()) == {"ER", "SCR"}
    assert set(name_match.distillation_agents.keys()) == {"LWF"} and name_match.distillation_agents["LWF"] is Lwf
    assert Lwf._force_autograd is False and Lwf.T == 2.0
    assert "LWF" not in " ".join(ffi.KNOWN_ENV)


def test_kd_manager_hands_out_the_teachers_logits_without_a_node_and_none_before_the_first_snapshot():
    from ocl_amd.kd_manager import KdManager

    class Owner:
        def __init__(self):
            self.flat, self.seen = torch.arange(3.0), []

        def flat_params(self):
            return self.flat

        def forward_with_params(self, x, flat):
            self.seen.append((x, flat, torch.is_grad_enabled()))
            return x * 2

    km, owner, x = KdManager(), Owner(), torch.ones(2)
    assert km.teacher_logits(x) is None and km.get_kd_loss(None, x) == 0 and not owner.seen
    km.update_teacher(owner)
    owner.flat += 1                                   # the snapshot is a copy
    out = km.teacher_logits(x)
    assert torch.equal(out, x * 2) and len(owner.seen) == 1
    assert owner.seen[0][0] is x and owner.seen[0][1] is km.teacher_model and owner.seen[0][2] is False
    assert torch.equal(km.teacher_model, torch.arange(3.0))


# ---- the float64 statement on cases worked out by hand ---------------------------------------------------------------------------------

def test_float64_statement_on_one_row_of_two_logits():
    """s = [0, log 3], y = 0: softmax(s) = [1/4, 3/4], ce = log 4.  t = [log 4, 0], T = 1: softmax(t) = [4/5, 1/5],
    kd = -(4/5 log 1/4 + 1/5 log 3/4).  dl = w_new ([1/4, 3/4] - [1, 0]) + w_old ([1/4, 3/4] - [4/5, 1/5])."""
    s, t = np.array([[0.0, math.log(3.0)]]), np.array([[math.log(4.0), 0.0]])
    w_new, w_old = 0.25, 0.75
    loss3, dl = ref_blend(s, [0], t, 1.0, w_new, w_old)
    ce, kd = math.log(4.0), -(0.8 * math.log(0.25) + 0.2 * math.log(0.75))
    assert loss3 == pytest.approx([w_new * ce + w_old * kd, ce, kd], rel=1e-14)
    assert dl == pytest.approx(np.array([[w_new * -0.75 + w_old * (0.25 - 0.8), w_new * 0.75 + w_old * (0.75 - 0.2)]]), rel=1e-13)
    # T = 2 on the same row: softmax(s / 2) = [1, sqrt 3] / (1 + sqrt 3), softmax(t / 2) = [2, 1] / 3; the gradient's KD term carries T / n = 2
    loss3, dl = ref_blend(s, [0], t, 2.0, 0.0, 1.0)
    ps, pt = np.array([1.0, math.sqrt(3.0)]) / (1.0 + math.sqrt(3.0)), np.array([2.0, 1.0]) / 3.0
    assert loss3[2] == pytest.approx(-(pt * np.log(ps)).sum() * 4.0, rel=1e-14) and loss3[0] == loss3[2] and loss3[1] == pytest.approx(ce)
    assert dl == pytest.approx(((ps - pt) * 2.0)[None], rel=1e-13)
    # no teacher: kd = 0 and the CE term alone, whatever w_old
    loss3, dl = ref_blend(s, [0], None, 2.0, 1.0, 0.7)
    assert loss3.tolist() == [loss3[1], loss3[1], 0.0] and dl == pytest.approx(np.array([[-0.75, 0.75]]), rel=1e-14)


@pytest.mark.parametrize("n,c,T", [(1, 2, 2.0), (3, 10, 1.0), (5, 100, 4.0), (4, 7, 0.5)])
def test_float64_statement_on_all_equal_logits(n, c, T):
    """Every softmax is uniform: ce = log c, kd = T^2 log c, the KD gradient vanishes and the CE gradient is (1/c - onehot) / n."""
    s, t = np.full((n, c), 1.25), np.full((n, c), -3.0)
    y = np.arange(n) % c
    loss3, dl = ref_blend(s, y, t, T, 1 / 3, 1 - 1 / 3)
    w_new, w_old = float(np.float32(1 / 3)), float(np.float32(1 - 1 / 3))
    assert loss3[1] == pytest.approx(math.log(c), rel=1e-14) and loss3[2] == pytest.approx(T * T * math.log(c), rel=1e-14)
    assert loss3[0] == pytest.approx(w_new * math.log(c) + w_old * T * T * math.log(c), rel=1e-14)
    want = np.full((n, c), 1.0 / c)
    want[np.arange(n), y] -= 1.0
    assert dl == pytest.approx(w_new * want / n, rel=1e-13, abs=1e-18)


def test_float64_statement_with_the_teacher_equal_to_the_student():
    """softmax(s / T) - softmax(t / T) is exactly 0: the gradient is the CE term, bit for bit the w_old = 0 one; kd is the entropy of
    softmax(s / T) times T^2."""
    rng = np.random.default_rng(5)
    s = lwf_ref.logits_for(rng, 6, 33, 3.0)
    y = rng.integers(0, 33, 6)
    loss3, dl = ref_blend(s, y, s.copy(), 3.0, 0.5, 0.5)
    loss3_0, dl_0 = ref_blend(s, y, s.copy(), 3.0, 0.5, 0.0)
    _, dl_none = ref_blend(s, y, None, 3.0, 0.5, 0.5)
    assert np.array_equal(dl, dl_0) and np.array_equal(dl, dl_none)
    p = np.exp(lwf_ref._log_softmax64(s.astype(np.float64) / 3.0))
    assert loss3[2] == pytest.approx(float(-(p * np.log(np.maximum(p, 1e-300))).sum(axis=1).mean() * 9.0), rel=1e-12)
    assert loss3[1] == loss3_0[1] and loss3_0[0] == 0.5 * loss3_0[1]


@pytest.mark.parametrize("n,c,scale,T", [(1, 5, 1, 2.0), (10, 100, 1, 2.0), (10, 128, 30, 3.0), (7, 1000, 30, 3.0)])
def test_plain_float32_statement_agrees_with_the_float64_one(n, c, scale, T):
    """The e_ref of the GPU parity test is the round-off of torch's float32 statements, not a difference of formulas: a few 1e-7
    relative to the largest element."""
    rng = np.random.default_rng(n * 1000 + c)
    s, t = lwf_ref.logits_for(rng, n, c, scale), lwf_ref.logits_for(rng, n, c, scale)
    y = rng.integers(0, c, n)
    for teacher in (t, None):
        l64, g64 = ref_blend(s, y, teacher, T, 1 / 3, 1 - 1 / 3)
        l32, g32 = torch32_blend(s, y, teacher, T, 1 / 3, 1 - 1 / 3)
        assert l32.dtype == g32.dtype == np.float32
        assert np.abs(l32 - l64).max() <= 2e-6 * max(1.0, np.abs(l64).max()), (l32, l64)
        assert np.abs(g32 - g64).max() <= 2e-6 * np.abs(g64).max(), np.abs(g32 - g64).max()
        if teacher is None:
            assert l64[2] == 0.0 and l32[2] == 0.0


# ---- the restatement against the reference and its recorded run ------------------------------------------------------------------------

@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_lwf_oracle_equals_the_reference_agent_over_all_three_tasks():
    torch.set_num_threads(1)
    cfg = LWF_CASE
    ref_import.activate()
    params = ref_import.default_params(**lwf_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = ref_import.build_agent(params)
    tasks, _ = make_stream(cfg)
    teachers = []
    with ref_import.quiet():
        for x, y in tasks:
            agent.train_learner(x, y)
            teachers.append({k: v.clone() for k, v in agent.kd_manager.teacher_model.state_dict().items()})
    rng_ref = (torch.get_rng_state(), np.random.get_state())
    seed_all(cfg["seed"])
    ag = lwf_ref.LwfOracle(cfg)
    for t, (x, y) in enumerate(tasks):
        ag.train_learner(x, y)
        for k, v in teachers[t].items():
            assert torch.equal(v, ag.teacher[k]), "the teacher after task %d: %s" % (t, k)
    assert torch.equal(rng_ref[0], torch.get_rng_state()), "torch's host RNG stream"
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(rng_ref[1], np.random.get_state())), "numpy's RNG stream"
    sd = model.state_dict()
    assert list(sd.keys()) == list(ag.state.keys())
    for k, v in sd.items():
        assert torch.equal(v, ag.state[k].detach()), k
    assert agent.task_seen == ag.task_seen == 3 and agent.old_labels == ag.old_labels
    assert len(ag.log) == 18 and [e["teacher"] for e in ag.log] == [False] * 6 + [True] * 12


def test_lwf_oracle_free_run_reproduces_the_recorded_reference_run():
    """The weights are bit-equal only on a CPU whose float32 convolution and matrix kernels add in the order of the recording machine's,
    and they follow a chaotic trajectory: they get the sanity band of test_cpu_agem's free run, as the GPU free run does.  What does not
    depend on the trajectory is exact: loss_old is zero through the first task and positive from then on.  The first step of the run
    starts from the seeded initial weights on every machine: its cross-entropy is the recorded one to float32 round-off."""
    g = gold("lwf")
    recs, ag = lwf_ref.run_oracle_case()
    assert len(recs) == int(g["lwf_c10_ntasks"]) == 3 and int(g["lwf_c10_steps_per_task"]) == 6
    assert set(GOLDEN_KEYS) == {"acc", "state"}
    for t, rec in enumerate(recs):
        ds, gs = rec["state"], g["lwf_c10_t%d_state" % t]
        assert ds.shape == gs.shape, t
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / max((gs[:, 1] ** 2).sum(), 1e-300))
        print("lwf_c10 oracle", t, "digest rel err", rel, "norm ratio", ratio, "acc", rec["acc"], g["lwf_c10_t%d_acc" % t])
        assert np.isfinite(ds).all() and rel < 3.0 and 0.5 < ratio < 2.0, (t, rel, ratio)
        assert rec["acc"].shape == g["lwf_c10_t%d_acc" % t].shape and (rec["acc"] >= 0).all() and (rec["acc"] <= 1).all()
    want = g["lwf_c10_losses"]
    got = lwf_ref.recorded_losses(ag.log, 6)
    assert want.shape == got.shape == (3, lwf_ref.RECORDED_STEPS, 2)
    print("lwf_c10 oracle losses (new, old) per task\n", got, "\nrecorded\n", want)
    for name, a in (("recorded", want), ("this machine", got)):
        assert (a[0, :, 1] == 0.0).all() and (a[1:, :, 1] > 0.0).all() and (a[:, :, 0] > 0.0).all() and np.isfinite(a).all(), (name, a)
    assert abs(got[0, 0, 0] - want[0, 0, 0]) < 1e-4
    assert [e["teacher"] for e in ag.log] == [False] * 6 + [True] * 12
    assert all(e["loss_old"] == 0.0 for e in ag.log[:6]) and all(e["loss_old"] > 0.0 for e in ag.log[6:])


# ---- the kernels use no scratch ----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_distill_kernels_use_no_scratch_and_spill_nothing():
    """csrc/distill.hip for gfx950 with the compiler's resource remarks, parsed as tests/test_cpu_ewc.py parses ewc.hip's: every
    instantiation (row in registers or strided, with and without a teacher); LDS holds the per-wave partials alone."""
    src = ROOT + "/online-continual-learning_amd/csrc/distill.hip"
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
    hits = {k: v for k, v in res.items() if re.fullmatch(r"ce_kd_blend_kernel<(true|false), (true|false)>", k)}
    assert len(hits) == 4 and len(res) == 4, sorted(res)
    for k, v in hits.items():
        assert v == {"ScratchSize": 0, "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size": 32}, (k, v)
