"""CPU: the host side of the iCaRL agent (the argument checks of csrc/icarl.hip's entry point and of ops.bce_distill, the registries, the
kernels' use of scratch) and the references the GPU tests rely on (tests/icarl_ref.py): the float64 statement of the loss on cases
worked out by hand, the plain float32 statement against it, and the restatement of the reference's loop against the reference itself and
against its recorded run (tests/golden/icarl.npz)."""
import ctypes as C
import math
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi, name_match
from ocl_amd.agents.icarl import Icarl
from conftest import gold, ROOT
from oracle import ref_import
from oracle.synth import make_stream, seed_all
import icarl_ref
from icarl_ref import ICARL_CASE, GOLDEN_KEYS, ref_bce_distill, torch32_bce_distill

OCL_ERR_ARG = -1    # include/ocl_hip.h
HIPCC = "/opt/rocm/bin/hipcc"


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # a host address: never dereferenced, every case below is refused first
MB = 1 << 24
N, NS, CC = 4, 2, 8
BYTES = N * CC * 4


def _bce(**over):
    kw = dict(logits=A, teacher=A + MB, pos=A + 2 * MB, n=N, n_stream=NS, c=CC, n_cls=6, n_old=4, loss=A + 3 * MB, dl=A + 4 * MB)
    kw.update(over)
    if "dl_at" in kw:                      # dlogits placed relative to another array (an id must not carry a process address)
        kw["dl"] = kw[kw["dl_at"][0]] + kw["dl_at"][1]
    rc = ffi.lib().ocl_bce_distill_fwd_bwd(ffi.vp(kw["logits"]), ffi.vp(kw["teacher"]), ffi.vp(kw["pos"]), kw["n"], kw["n_stream"], kw["c"],
                                           kw["n_cls"], kw["n_old"], ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signature_is_registered_and_declared():
    vp, i = ffi.vp, C.c_int
    assert ffi.SIGNATURES["ocl_bce_distill_fwd_bwd"] == (C.c_int, [vp, vp, vp, i, i, i, i, i, vp, vp, vp])
    header = open(ROOT + "/include/ocl_hip.h").read()
    assert hasattr(ffi.lib(), "ocl_bce_distill_fwd_bwd") and re.search(r"\bocl_bce_distill_fwd_bwd\(", header)
    assert "icarl.hip" in open(ROOT + "/online-continual-learning_amd/csrc/Makefile").read()


@pytest.mark.parametrize("over", [
    dict(logits=0), dict(pos=0), dict(loss=0),
    dict(n=0), dict(n=-3), dict(c=0), dict(c=-1),
    dict(n_stream=0), dict(n_stream=-1), dict(n_stream=N + 1),
    dict(n_old=-1), dict(n_old=7), dict(n_cls=CC + 1), dict(n_cls=-1, n_old=-1), dict(n_cls=3),
    dict(teacher=0), dict(teacher=0, n_old=1),
    dict(dl_at=("logits", 0)), dict(dl_at=("logits", BYTES - 4)), dict(dl_at=("logits", 4 - BYTES)),     # on, ending inside, starting inside
    dict(dl_at=("teacher", 0)), dict(dl_at=("teacher", BYTES - 4)), dict(dl_at=("teacher", 4 - BYTES)),
    dict(dl_at=("pos", 0)), dict(dl_at=("pos", 8 * NS - 4)), dict(dl_at=("pos", 4 - BYTES)),
], ids=lambda o: ",".join("%s=%s" % (k, "%s%+d" % v if isinstance(v, tuple) else v) for k, v in o.items()))
def test_entry_point_refuses_bad_arguments_without_a_device(over):
    rc, msg = _bce(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("bce_distill:"), msg
    if "dl_at" in over:
        assert "overlaps " + over["dl_at"][0] in msg, msg
    if over.get("teacher") == 0:
        assert "teacher" in msg, msg


def test_ops_wrapper_refuses_wrong_dtype_shape_layout_and_device_without_a_device():
    """Every check of ops.bce_distill comes before the library is initialised: CPU tensors are enough to reach each of them (a
    well-formed set of CPU tensors is refused for its device)."""
    from ocl_amd import ops
    s, t, p = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(2, dtype=torch.int64)
    wide = torch.zeros(4, 16)
    good = (2, 6, 4)
    bad = [
        ("logits dtype", (s.double(), t, p) + good), ("logits rank", (s.reshape(-1), t, p) + good), ("logits layout", (wide[:, :8], t, p) + good),
        ("pos dtype", (s, t, p.int()) + good), ("pos shape", (s, t, torch.zeros(3, dtype=torch.int64)) + good),
        ("pos rank", (s, t, p.reshape(2, 1)) + good), ("pos layout", (s, t, torch.zeros(4, dtype=torch.int64)[::2]) + good),
        ("teacher dtype", (s, t.double(), p) + good), ("teacher shape", (s, torch.zeros(4, 7), p) + good),
        ("teacher layout", (s, wide[:, 8:], p) + good), ("teacher transposed", (s, torch.zeros(8, 4).t(), p) + good),
        ("n_stream 0", (s, t, p[:0], 0, 6, 4)), ("n_stream > n", (s, t, torch.zeros(5, dtype=torch.int64), 5, 6, 4)),
        ("n_old > n_cls", (s, t, p, 2, 4, 6)), ("n_cls > c", (s, t, p, 2, 9, 4)), ("n_old < 0", (s, t, p, 2, 6, -1)),
        ("n_old without a teacher", (s, None, p, 2, 6, 4)),
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError, match="bce_distill"):
            ops.bce_distill(*args)
    for what, dl in (("dl_out dtype", torch.zeros(4, 8, dtype=torch.float64)), ("dl_out shape", torch.zeros(5, 8)), ("dl_out layout", wide[:, :8])):
        with pytest.raises(RuntimeError, match="dl_out"):
            ops.bce_distill(s, t, p, *good, dl_out=dl)
    for teacher, n_old in ((t, 4), (None, 0)):
        with pytest.raises(RuntimeError, match="GPU"):
            ops.bce_distill(s, teacher, p, 2, 6, n_old)


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_icarl_resolves_by_name_and_every_other_table_keeps_its_keys():
    from ocl_amd.agents.base import ContinualLearner
    assert name_match.get_agent("ICARL") is Icarl and Icarl is name_match.exemplar_agents["ICARL"] and issubclass(Icarl, ContinualLearner)
    assert set(name_match.exemplar_agents.keys()) == {"ICARL"}
    assert set(name_match.agents.keys()) == {"ER", "SCR"}
    assert set(name_match.extra_agents.keys()) == {"AGEM"}
    assert set(name_match.regularization_agents.keys()) == {"EWC"}
    assert set(name_match.distillation_agents.keys()) == {"LWF"}
    assert set(name_match.offline_agents.keys()) == {"GDUMB"}
    assert Icarl._force_autograd is False
    assert "ICARL" not in " ".join(ffi.KNOWN_ENV)
    with pytest.raises(KeyError):
        name_match.get_agent("CNDPM")


def test_positions_follow_the_reference_and_an_unknown_label_raises_value_error():
    """len(old_labels) + new_labels.index(y), on the host; list.index's ValueError for a label outside the task's new labels."""
    me = Icarl.__new__(Icarl)
    me.__dict__.update(old_labels=[7, 3, 9], new_labels=[5, 2])
    assert Icarl._positions(me, np.array([2, 5, 5, 2])) == [4, 3, 3, 4]
    with pytest.raises(ValueError):
        Icarl._positions(me, np.array([5, 7]))          # an old label is not a new one


# ---- the float64 statement on cases worked out by hand ---------------------------------------------------------------------------------

def test_float64_statement_on_one_row_of_two_logits():
    """s = [log 3, -log 3]: sig(s) = [3/4, 1/4].  No teacher, pos = 0: l = [-log 3/4, -log 3/4], dl = [-1/4, 1/4].  With a teacher
    t = [log 4, .] on one old column: z = [4/5, 0] whatever pos says about column 0; l_0 = -(4/5 log 3/4 + 1/5 log 1/4)."""
    s = np.array([[math.log(3.0), -math.log(3.0)]])
    loss3, dl = ref_bce_distill(s, None, [0], 1, 2, 0)
    assert loss3 == pytest.approx([-2 * math.log(0.75), 0.0, -2 * math.log(0.75)], rel=1e-14) and loss3[1] == 0.0
    assert dl == pytest.approx(np.array([[-0.25, 0.25]]), rel=1e-14)
    t = np.array([[math.log(4.0), np.nan]])            # the teacher's column 1 is not an old column: never looked at
    for pos in ([0], [1], [5], [-1]):
        loss3, dl = ref_bce_distill(s, t, pos, 1, 2, 1)
        z1 = 1.0 if pos == [1] else 0.0
        old = -(0.8 * math.log(0.75) + 0.2 * math.log(0.25))
        new = -math.log(0.25) if z1 else -math.log(0.75)
        assert loss3 == pytest.approx([old + new, old, new], rel=1e-14)
        assert dl == pytest.approx(np.array([[0.75 - 0.8, 0.25 - z1]]), rel=1e-13)
    # a dead column (c = 3 > n_cls = 2) holds anything: gradient 0 there
    loss3a, dla = ref_bce_distill(s, t, [1], 1, 2, 1)
    loss3b, dlb = ref_bce_distill(np.array([[math.log(3.0), -math.log(3.0), np.inf]]), t, [1], 1, 2, 1)
    assert np.array_equal(loss3a, loss3b) and np.array_equal(dla, dlb[:, :2])
    assert dlb[0, 2] == 0.0 and not np.signbit(dlb[0, 2]) and np.isfinite(loss3b).all()


@pytest.mark.parametrize("n,n_stream,c,n_cls", [(1, 1, 2, 2), (3, 3, 10, 10), (20, 10, 100, 6), (4, 2, 7, 5)])
def test_float64_statement_on_all_zero_logits_with_one_hot_targets(n, n_stream, c, n_cls):
    """s = 0: every element's loss is log 2 whatever its target, so loss = n_cls log 2; dl = (1/2 - z) / n."""
    pos = np.arange(n_stream) % n_cls
    loss3, dl = ref_bce_distill(np.zeros((n, c)), None, pos, n_stream, n_cls, 0)
    assert loss3 == pytest.approx([n_cls * math.log(2.0), 0.0, n_cls * math.log(2.0)], rel=1e-14)
    want = np.zeros((n, c))
    want[:, :n_cls] = 0.5
    want[np.arange(n_stream), pos] -= 1.0
    assert np.array_equal(dl, want / n)


def test_float64_statement_with_the_teacher_equal_to_the_student():
    """sig(s) - sig(t) is exactly 0 on the old columns; the old loss is the summed binary entropy of sig(s) there; the new columns do
    not see the teacher."""
    rng = np.random.default_rng(5)
    s = (rng.standard_normal((6, 33)) * 3.0).astype(np.float32)     # (no saturated logit: the entropy below is written with plain logs)
    pos = rng.integers(20, 30, 3)
    loss3, dl = ref_bce_distill(s, s.copy(), pos, 3, 30, 20)
    assert np.array_equal(dl[:, :20], np.zeros((6, 20)))
    p = icarl_ref._sigmoid64(s.astype(np.float64)[:, :20])
    assert loss3[1] == pytest.approx(float(-(p * np.log(p) + (1 - p) * np.log1p(-p)).sum() / 6), rel=1e-12)
    other = rng.standard_normal((6, 33)).astype(np.float32)
    loss3_o, dl_o = ref_bce_distill(s, other, pos, 3, 30, 20)
    assert np.array_equal(dl[:, 20:], dl_o[:, 20:]) and loss3[2] == loss3_o[2] and loss3[1] != loss3_o[1]
    # the memory rows (r >= n_stream) have all-zero new targets: sig(s) / n
    assert np.array_equal(dl[3:, 20:30], icarl_ref._sigmoid64(s.astype(np.float64)[3:, 20:30]) / 6)


@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old,scale", [(1, 1, 2, 2, 0, 1), (20, 10, 100, 100, 90, 1), (20, 10, 100, 65, 64, 30),
                                                            (6, 3, 300, 100, 50, 30), (20, 10, 10, 4, 2, 300)])
def test_plain_float32_statement_agrees_with_the_float64_one(n, n_stream, c, n_cls, n_old, scale):
    """The e_ref of the GPU parity test is the round-off of torch's float32 statements, not a difference of formulas: a few 1e-7
    relative to the largest element."""
    rng = np.random.default_rng(n * 1000 + c)
    s, t = icarl_ref.logits_for(rng, n, c, scale), icarl_ref.logits_for(rng, n, c, scale)
    pos = rng.integers(n_old, n_cls, n_stream)
    teacher = t if n_old else None
    l64, g64 = ref_bce_distill(s, teacher, pos, n_stream, n_cls, n_old)
    l32, g32 = torch32_bce_distill(s, teacher, pos, n_stream, n_cls, n_old)
    assert l32.dtype == g32.dtype == np.float32 and g32.shape == (n, c)
    assert np.abs(l32 - l64).max() <= 2e-6 * max(1.0, np.abs(l64).max()), (l32, l64)
    assert np.abs(g32 - g64).max() <= 2e-6 * np.abs(g64).max(), np.abs(g32 - g64).max()
    assert np.array_equal(g32[:, n_cls:], np.zeros((n, c - n_cls), dtype=np.float32))
    if not n_old:
        assert l64[1] == 0.0 and l32[1] == 0.0


# ---- the restatement against the reference and its recorded run ------------------------------------------------------------------------

@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_icarl_oracle_equals_the_reference_agent_over_all_three_tasks():
    torch.set_num_threads(1)
    cfg = ICARL_CASE
    ref_import.activate()
    params = ref_import.default_params(**icarl_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = ref_import.build_agent(params)
    tasks, _ = make_stream(cfg)
    teachers = []
    with ref_import.quiet():
        for x, y in tasks:
            agent.train_learner(x, y)
            teachers.append({k: v.clone() for k, v in agent.prev_model.state_dict().items()})
    rng_ref = (torch.get_rng_state(), np.random.get_state())
    seed_all(cfg["seed"])
    ag = icarl_ref.IcarlOracle(cfg)
    for t, (x, y) in enumerate(tasks):
        ag.train_learner(x, y)
        for k, v in teachers[t].items():
            if v.is_floating_point() and "running" not in k:     # (the reference's copy updates its own running statistics: unused in train mode)
                assert torch.equal(v, ag.teacher[k]), "the teacher after task %d: %s" % (t, k)
    assert torch.equal(rng_ref[0], torch.get_rng_state()), "torch's host RNG stream"
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(rng_ref[1], np.random.get_state())), "numpy's RNG stream"
    sd = model.state_dict()
    assert list(sd.keys()) == list(ag.state.keys())
    for k, v in sd.items():
        assert torch.equal(v, ag.state[k].detach()), k
    assert agent.task_seen == ag.task_seen == 3 and agent.old_labels == ag.old_labels
    assert torch.equal(agent.buffer.buffer_label, ag.buf.label) and torch.equal(agent.buffer.buffer_img, ag.buf.img)
    assert agent.buffer.current_index == ag.buf.current_index == 50 and agent.buffer.n_seen_so_far == ag.buf.n_seen_so_far == 180
    assert len(ag.log) == 18 and [e["teacher"] for e in ag.log] == [False] * 6 + [True] * 12
    assert [(e["rows"], e["n_cls"]) for e in ag.log] == [(10, 2)] * 6 + [(20, 4)] * 6 + [(20, 6)] * 6


def test_icarl_oracle_free_run_reproduces_the_recorded_reference_run():
    """The weights are bit-equal only on a CPU whose float32 convolution and matrix kernels add in the order of the recording machine's,
    and they follow a chaotic trajectory: they get the sanity band of test_cpu_lwf's free run.  What does not depend on the trajectory
    is exact: the retrievals (host RNG and the reservoir's slots alone), the number of excluded slots, the shapes.  The first step of
    the run starts from the seeded initial weights on every machine: its loss is the recorded one to float32 round-off."""
    g = gold("icarl")
    recs, ag = icarl_ref.run_oracle_case()
    assert len(recs) == int(g["icarl_c10_ntasks"]) == 3 and int(g["icarl_c10_steps_per_task"]) == 6
    assert set(GOLDEN_KEYS) == {"acc", "state"}
    for t, rec in enumerate(recs):
        ds, gs = rec["state"], g["icarl_c10_t%d_state" % t]
        assert ds.shape == gs.shape, t
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / max((gs[:, 1] ** 2).sum(), 1e-300))
        print("icarl_c10 oracle", t, "digest rel err", rel, "norm ratio", ratio, "acc", rec["acc"], g["icarl_c10_t%d_acc" % t])
        assert np.isfinite(ds).all() and rel < 3.0 and 0.5 < ratio < 2.0, (t, rel, ratio)
        assert rec["acc"].shape == g["icarl_c10_t%d_acc" % t].shape and (rec["acc"] >= 0).all() and (rec["acc"] <= 1).all()
    want = g["icarl_c10_losses"]
    got = icarl_ref.recorded_losses([e["loss"] for e in ag.log], 6)
    assert want.shape == got.shape == (3, icarl_ref.RECORDED_STEPS)
    print("icarl_c10 oracle losses per task\n", got, "\nrecorded\n", want)
    assert np.isfinite(got).all() and (got > 0).all() and (want > 0).all()
    assert abs(got[0, 0] - want[0, 0]) < 1e-4
    retrievals = icarl_ref.retrieval_table([e["indices"] for e in ag.log if e["indices"] is not None], 10)
    assert np.array_equal(retrievals, g["icarl_c10_retrievals"]) and retrievals.shape == (12, 10)
    n_excl = [len(e["excl"]) for e in ag.log if e["teacher"]]
    assert n_excl == g["icarl_c10_n_excluded"].tolist() and max(n_excl) > 0
    assert all(not set(e["indices"].tolist()) & set(e["excl"]) for e in ag.log if e["teacher"])
    assert [e["teacher"] for e in ag.log] == [False] * 6 + [True] * 12


# ---- the kernels use no scratch ----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_icarl_kernels_use_no_scratch_and_spill_nothing():
    """csrc/icarl.hip for gfx950 with the compiler's resource remarks, parsed as tests/test_cpu_lwf.py parses distill.hip's: every
    instantiation (row in registers or strided, with and without a teacher); LDS holds the per-wave partials alone (2 x 4 doubles)."""
    src = ROOT + "/online-continual-learning_amd/csrc/icarl.hip"
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
    hits = {k: v for k, v in res.items() if re.fullmatch(r"bce_distill_kernel<(true|false), (true|false)>", k)}
    assert len(hits) == 4 and len(res) == 4, sorted(res)
    for k, v in hits.items():
        assert v == {"ScratchSize": 0, "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size": 64}, (k, v)
