"""GPU: the BCE-distillation kernel (csrc/icarl.hip: ocl_bce_distill_fwd_bwd; ops.bce_distill) and the iCaRL agent built on it
(agents/icarl.py), against the float64 statement of the loss, the plain float32 statement, and the restatement of the reference's loop
(tests/icarl_ref.py, all pinned on the CPU by tests/test_cpu_icarl.py).

The kernel is judged by parity_bounds.check_vs_torch32, the project's rule for transcendental kernels: its error against float64 is at
most max(4 x the error of torch's own float32 statements on the same inputs, 4 ulp of the largest reference element), for each of the
three losses and for the gradient.  Observed values: profiles/icarl_parity.txt (written by this module's report when PARITY_REPORT_DIR
names a directory)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from conftest import gold
from guarded import Guarded
from oracle.synth import make_stream, seed_all, digest_state
import parity_bounds
import icarl_ref
from icarl_ref import ICARL_CASE, ref_bce_distill, torch32_bce_distill, logits_for

pytestmark = pytest.mark.gpu

_build_agent = functools.partial(build_agent, extra=icarl_ref.ref_params)

REPORT = []
# (n, n_stream, c, n_cls, n_old)
SHAPES = [
    (1, 1, 2, 2, 0),                                                  # smallest, no teacher
    (2, 1, 4, 4, 2),                                                  # one stream row, one memory row
    (4, 2, 10, 6, 4), (5, 3, 10, 6, 4),                               # both sides of four waves
    (20, 10, 10, 4, 2),                                               # dead columns
    (20, 10, 100, 100, 90),                                           # the workload's last task
    (20, 10, 100, 64, 63), (20, 10, 100, 65, 64),                     # the 64-lane boundary, in n_cls and in n_old
    (6, 3, 256, 256, 128), (6, 3, 257, 257, 128), (6, 3, 300, 100, 50),   # both sides of the register threshold; dead columns on the strided path
    (10, 10, 100, 10, 0),                                             # first task, no teacher
]
SCALES = [1, 30, 300]


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    """After the module's tests: the rows parity_bounds recorded, as a table, into $PARITY_REPORT_DIR/icarl_parity.txt."""
    yield
    out = os.environ.get("PARITY_REPORT_DIR")
    if out and REPORT:
        with open(os.path.join(out, "icarl_parity.txt"), "w") as f:
            f.write("%-52s %-8s %-12s %-12s %-12s %s\n" % ("case", "tensor", "kernel err", "torch32 err", "bound", "err/bound"))
            for case, tensor, err, e_ref, bound, ratio in REPORT:
                f.write("%-52s %-8s %-12.4g %-12s %-12.4g %.3f\n" % (case, tensor, err, e_ref, bound, ratio))
            f.write("worst err/bound %.3f over %d rows\n" % (max(r[5] for r in REPORT), len(REPORT)))


def _case(n, n_stream, c, n_cls, n_old, scale):
    """Student and teacher logits, and the stream rows' columns: new columns, except that (where there are rows enough) one lies below
    n_old (the teacher's value overwrites it) and one outside [0, n_cls) (no target)."""
    rng = np.random.default_rng(9000 + 131 * n + 17 * c + n_cls + n_old)
    s, t = logits_for(rng, n, c, scale), logits_for(rng, n, c, scale)
    pos = rng.integers(n_old, n_cls, n_stream).astype(np.int64)
    if n_stream >= 3:
        pos[1] = rng.integers(0, n_old) if n_old else pos[1]
        pos[2] = n_cls + 3
    return s, t, pos


# ---- 1. the kernel against the float64 statement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old", SHAPES)
def test_bce_distill_vs_float64_reference(cuda, n, n_stream, c, n_cls, n_old, scale):
    from ocl_amd import ffi
    lib = ffi.lib()
    s, t, pos = _case(n, n_stream, c, n_cls, n_old, scale)
    teacher = t if n_old else None
    l64, g64 = ref_bce_distill(s, teacher, pos, n_stream, n_cls, n_old)
    l32, g32 = torch32_bce_distill(s, teacher, pos, n_stream, n_cls, n_old)
    g = Guarded()
    d_s, d_p = g.inp(s, 0, "logits"), g.inp(pos, 0, "pos")
    d_t = g.inp(t, 0, "teacher") if n_old else None
    d_l, d_dl = g.out((3,), torch.float32, 0, "loss_out"), g.out((n, c), torch.float32, 0, "dlogits")
    rc = lib.ocl_bce_distill_fwd_bwd(ffi.ptr(d_s), ffi.ptr(d_t), ffi.ptr(d_p), n, n_stream, c, n_cls, n_old, ffi.ptr(d_l), ffi.ptr(d_dl), ffi.stream())
    assert rc == 0, lib.ocl_last_error()
    g.check("bce_distill")
    got_l, got_g = _host(d_l), _host(d_dl)
    assert np.isfinite(got_l).all() and np.isfinite(got_g).all()
    name = "bce n=%d stream=%d c=%d n_cls=%d n_old=%d scale=%g" % (n, n_stream, c, n_cls, n_old, scale)
    for k, which in enumerate(("loss", "old", "new")):
        parity_bounds.check_vs_torch32(REPORT, name, which, got_l[k:k + 1], l64[k:k + 1], l32[k:k + 1])
    parity_bounds.check_vs_torch32(REPORT, name, "dlogits", got_g, g64, g32)
    assert not got_g[:, n_cls:].any() and not np.signbit(got_g[:, n_cls:]).any()


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old", [(20, 10, 10, 4, 2), (6, 3, 300, 100, 50), (20, 10, 100, 64, 63), (10, 10, 100, 10, 0)])
def test_dead_columns_are_never_read(cuda, n, n_stream, c, n_cls, n_old):
    """NaN in the logit columns from n_cls on and in the teacher's columns from n_old on, against zeros there: the three losses and
    dlogits bit for bit, and dlogits +0.0 bit for bit from n_cls on."""
    from ocl_amd import ops
    s, t, pos = _case(n, n_stream, c, n_cls, n_old, 1)
    s0, t0 = s.copy(), t.copy()
    s0[:, n_cls:], t0[:, n_old:] = 0.0, 0.0
    s1, t1 = s0.copy(), t0.copy()
    s1[:, n_cls:], t1[:, n_old:] = np.nan, np.nan
    s1[::2, n_cls:] = np.inf
    d_p = _dev(pos, cuda, np.int64)
    l0, dl0 = ops.bce_distill(_dev(s0, cuda), _dev(t0, cuda), d_p, n_stream, n_cls, n_old)
    l1, dl1 = ops.bce_distill(_dev(s1, cuda), _dev(t1, cuda), d_p, n_stream, n_cls, n_old)
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(dl1).all())
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(dl0), _bits(dl1))
    assert c == n_cls or not bool(_bits(dl1[:, n_cls:]).any()), "dlogits is not +0.0 in the columns from n_cls on"


@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old", [sh for sh in SHAPES if sh[4]])
def test_a_teacher_equal_to_the_student_gives_exactly_zero_on_the_old_columns(cuda, n, n_stream, c, n_cls, n_old):
    """sig(s) and sig(t) come from one function and are rounded before they are subtracted.  The new columns do not see the teacher:
    their gradient is, bit for bit, what the kernel without a teacher (another instantiation, n_old = 0, the old columns counted as
    new ones without a target) gives on the same logits -- the stream rows' columns here all lie in [n_old, n_cls)."""
    from ocl_amd import ops
    for scale in SCALES:
        s, _, pos = _case(n, n_stream, c, n_cls, n_old, scale)
        pos = np.where((pos >= n_old) & (pos < n_cls), pos, n_old).astype(np.int64)
        d_s, d_p = _dev(s, cuda), _dev(pos, cuda, np.int64)
        loss3, dl = ops.bce_distill(d_s, d_s.clone(), d_p, n_stream, n_cls, n_old)
        assert not bool(_bits(dl[:, :n_old]).any()), "scale %g: a gradient on an old column" % scale
        loss3_n, dl_n = ops.bce_distill(d_s, None, d_p, n_stream, n_cls, 0)
        assert torch.equal(_bits(dl[:, n_old:]), _bits(dl_n[:, n_old:])), "scale %g: the new columns depend on the teacher" % scale
        assert float(loss3[1]) >= 0.0 and float(loss3_n[1]) == 0.0


@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old", [(2, 1, 4, 4, 2), (20, 10, 100, 100, 90), (6, 3, 300, 100, 50), (5, 3, 10, 6, 4)])
def test_memory_rows_have_all_zero_new_targets(cuda, n, n_stream, c, n_cls, n_old):
    """Rows from n_stream on: the gradient on the new columns is sig(s) / n -- bit for bit what the same kernel gives for those rows
    when they are stream rows whose column lies outside [0, n_cls)."""
    from ocl_amd import ops
    s, t, pos = _case(n, n_stream, c, n_cls, n_old, 1)
    d_s, d_t = _dev(s, cuda), _dev(t, cuda)
    _, dl = ops.bce_distill(d_s, d_t, _dev(pos, cuda, np.int64), n_stream, n_cls, n_old)
    nowhere = np.concatenate([pos, np.full(n - n_stream, n_cls + 5, dtype=np.int64)])
    nowhere[n_stream::2] = -1
    _, dl_all = ops.bce_distill(d_s, d_t, _dev(nowhere, cuda, np.int64), n, n_cls, n_old)
    assert torch.equal(_bits(dl), _bits(dl_all))
    want = 1.0 / (1.0 + np.exp(-s[n_stream:, n_old:n_cls].astype(np.float64))) / n
    assert np.abs(_host(dl)[n_stream:, n_old:n_cls] - want).max() <= 4 * 2.0 ** -24 / n


@pytest.mark.parametrize("n,n_stream,c,n_cls,n_old", SHAPES)
def test_two_runs_are_bit_identical_and_the_losses_do_not_depend_on_want_grad(cuda, n, n_stream, c, n_cls, n_old):
    from ocl_amd import ops
    s, t, pos = _case(n, n_stream, c, n_cls, n_old, 30)
    d_s, d_p = _dev(s, cuda), _dev(pos, cuda, np.int64)
    d_t = _dev(t, cuda) if n_old else None
    l_a, dl_a = ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old)
    l_b, dl_b = ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old)
    l_c, dl_c = ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old, want_grad=False)
    assert dl_c is None and dl_a is not dl_b
    assert torch.equal(_bits(l_a), _bits(l_b)) and torch.equal(_bits(dl_a), _bits(dl_b)) and torch.equal(_bits(l_a), _bits(l_c))


def test_dl_out_writes_into_a_row_block_of_a_larger_buffer_and_leaves_the_rest(cuda):
    from ocl_amd import ops
    n, n_stream, c, n_cls, n_old = 20, 10, 100, 100, 90
    s, t, pos = _case(n, n_stream, c, n_cls, n_old, 1)
    d_s, d_t, d_p = _dev(s, cuda), _dev(t, cuda), _dev(pos, cuda, np.int64)
    big = torch.full((3 * n, c), -7777.0, device=cuda)
    loss3, dl = ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old, dl_out=big[n:2 * n])
    want_l, want_dl = ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old)
    assert dl.data_ptr() == big[n:2 * n].data_ptr() and torch.equal(_bits(dl), _bits(want_dl)) and torch.equal(_bits(loss3), _bits(want_l))
    assert bool((big[:n] == -7777.0).all()) and bool((big[2 * n:] == -7777.0).all())
    for bad in (big[:, :c // 2], big[:n].double(), big[:n + 1], big[:n].cpu()):
        with pytest.raises(RuntimeError):
            ops.bce_distill(d_s, d_t, d_p, n_stream, n_cls, n_old, dl_out=bad)
    with pytest.raises(RuntimeError):
        ops.bce_distill(d_s, d_t[:, :50], d_p, n_stream, n_cls, n_old)
    with pytest.raises(RuntimeError):
        ops.bce_distill(d_s, d_t, d_p.cpu(), n_stream, n_cls, n_old)


# ---- 3. refused arguments ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from ocl_amd import ffi
    lib = ffi.lib()
    n, n_stream, c = 4, 2, 8
    s, t = torch.full((n, c), 1.0, device=cuda), torch.full((n, c), 2.0, device=cuda)
    pos = torch.full((n_stream,), 5, dtype=torch.int64, device=cuda)
    loss, dl = torch.full((3,), -7777.0, device=cuda), torch.full((n, c), -7777.0, device=cuda)

    def call(**over):
        kw = dict(s=s.data_ptr(), t=t.data_ptr(), pos=pos.data_ptr(), n=n, n_stream=n_stream, c=c, n_cls=6, n_old=4, loss=loss.data_ptr(),
                  dl=dl.data_ptr())
        kw.update(over)
        rc = lib.ocl_bce_distill_fwd_bwd(ffi.vp(kw["s"]), ffi.vp(kw["t"]), ffi.vp(kw["pos"]), kw["n"], kw["n_stream"], kw["c"], kw["n_cls"],
                                         kw["n_old"], ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.stream())
        return rc, lib.ocl_last_error()

    for over in (dict(n=0), dict(n=-1), dict(c=0), dict(c=-5), dict(n_stream=0), dict(n_stream=n + 1), dict(n_old=-1), dict(n_old=7),
                 dict(n_cls=c + 1), dict(n_cls=3), dict(t=0), dict(s=0), dict(pos=0), dict(loss=0),
                 dict(dl=s.data_ptr()), dict(dl=s.data_ptr() + 4 * (n * c - 1)), dict(dl=t.data_ptr()), dict(dl=t.data_ptr() + 64),
                 dict(dl=pos.data_ptr())):
        rc, msg = call(**over)
        assert rc == -1 and msg.startswith(b"bce_distill:"), (over, rc, msg)
        if "dl" in over:
            assert b"overlap" in msg, (over, msg)
    torch.cuda.synchronize()
    assert bool((loss == -7777.0).all()) and bool((dl == -7777.0).all()) and bool((s == 1.0).all()) and bool((t == 2.0).all())
    assert bool((pos == 5).all())
    rc, msg = call()
    assert rc == 0, msg
    rc, msg = call(t=0, n_old=0, dl=0)      # both optional pointers null: the losses alone, no old part
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool((dl == -7777.0).any()) and float(loss[1]) == 0.0 and float(loss[0]) == float(loss[2])


# ---- 4. the agent ---------------------------------------------------------------------------------------------------------------------

def _spy_bce(patch):
    """Records every ops.bce_distill call; `patch(obj, name, value)` is monkeypatch.setattr or a stand-in for it."""
    from ocl_amd import ops
    calls = []
    inner = ops.bce_distill

    def bce_distill(logits, teacher_logits, pos, n_stream, n_cls, n_old, want_grad=True, dl_out=None):
        loss3, dl = inner(logits, teacher_logits, pos, n_stream, n_cls, n_old, want_grad=want_grad, dl_out=dl_out)
        calls.append(SimpleNamespace(logits=logits.clone(), teacher=teacher_logits, pos=pos.clone(), n_stream=n_stream, n_cls=n_cls, n_old=n_old,
                                     dl=dl, dl_bits=dl.clone(), loss3=loss3.clone()))
        return loss3, dl

    patch(ops, "bce_distill", bce_distill)
    return calls


def _bn_stats(state):
    return {k: v for k, v in state.items() if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


def _pieces(v):
    return tuple(v) if isinstance(v, (list, tuple)) else (v,)


def test_agent_hands_the_right_things_to_the_kernel_and_its_gradient_to_the_backward(cuda, monkeypatch):
    """Three train_learner calls of two batches each, order-independent batch sums.  One ops.bce_distill call per optimiser step, with
    n_stream = batch, n_cls = len(old) + len(new), n_old = len(old) and pos = len(old) + new.index(y) for the batch's labels.  Task 1: no
    teacher, no teacher forward, 10 rows.  Later tasks: the student's taped pass takes (stream batch, memory rows) as ONE view of two
    pieces; the teacher's logits are forward_with_params' output for the same two pieces and the snapshot taken at the end of the
    previous task (bit-equal to flat_params at that moment).  The kernel's dl is the very tensor backward_taped receives, unchanged.
    The teacher's pass leaves the student's BatchNorm running statistics alone: after a step they are the bits of a twin model that ran
    the student's forward of the same 20 images as one group only."""
    from ocl_amd import ops
    from ocl_amd.setup_elements import setup_architecture
    cfg = dict(ICARL_CASE, seed=23)
    ops.set_deterministic(True)
    try:
        params, model, opt, agent = _build_agent(cfg)
        calls = _spy_bce(monkeypatch.setattr)
        fwp, taped, backs, steps, before, updates = [], [], [], [], [], []
        inner_fwp, inner_taped, inner_back, inner_step = model.forward_with_params, model.forward_views_taped, model.backward_taped, opt.step
        inner_update = agent.buffer.update

        def forward_with_params(x, flat):
            out = inner_fwp(x, flat)
            fwp.append(SimpleNamespace(x=[p.clone() for p in _pieces(x)], flat=flat, flat_bits=flat.clone(), out=out, grad=torch.is_grad_enabled(),
                                       at=len(taped)))
            return out

        def forward_views_taped(views):
            before.append({k: v.clone() for k, v in model.state_dict().items()})
            out, tape = inner_taped(views)
            taped.append(SimpleNamespace(x=[p.clone() for p in _pieces(views[0])], n_views=len(views), out=out, tape=tape))
            return out, tape

        def backward_taped(tape, dout):
            backs.append(SimpleNamespace(tape=tape, dout=dout, bits=dout.clone(), n_calls=len(calls)))
            return inner_back(tape, dout)

        def step(*a, **k):
            out = inner_step(*a, **k)
            steps.append(SimpleNamespace(n_back=len(backs), state={k_: v.clone() for k_, v in model.state_dict().items()}))
            return out

        def update(x, y, **kw):
            updates.append(SimpleNamespace(x=x.clone(), y_host=np.asarray(kw["y_host"]).copy(), n_steps=len(steps)))
            return inner_update(x, y, **kw)

        model.forward_with_params, model.forward_views_taped, model.backward_taped, opt.step = forward_with_params, forward_views_taped, backward_taped, step
        agent.buffer.update = update
        tasks, _ = make_stream(cfg)
        pick = np.r_[0:10, 30:40]
        snaps = []
        for t in range(3):
            assert (agent.prev.teacher_model is None) == (t == 0) and agent.kd_manager.teacher_model is None
            agent.train_learner(tasks[t][0][pick], tasks[t][1][pick])
            assert agent.task_seen == t + 1 and len(calls) == len(taped) == len(backs) == len(steps) == len(updates) == 2 * (t + 1)
            teacher = agent.prev.teacher_model
            assert torch.equal(_bits(teacher), _bits(model.flat_params())) and teacher.data_ptr() != model.flat_params().data_ptr()
            snaps.append(teacher.clone())
        assert agent.prev is not agent.kd_manager and agent.kd_manager.teacher_model is None
        assert len(fwp) == 4 and [f.at for f in fwp] == [3, 4, 5, 6], "the teacher's pass follows the student's, from the second task on"
        for k, c in enumerate(calls):
            t = k // 2
            old, new = [l for task in cfg["tasks"][:t] for l in task], list(set(tasks[t][1][pick].tolist()))
            assert (c.n_stream, c.n_cls, c.n_old) == (10, len(old) + len(new), len(old))
            assert _host(c.pos).tolist() == [len(old) + new.index(y) for y in updates[k].y_host.tolist()] and updates[k].n_steps == k + 1
            rows = 10 if t == 0 else 20
            assert taped[k].n_views == 1 and len(taped[k].x) == (1 if t == 0 else 2) and all(p.shape[0] == 10 for p in taped[k].x)
            assert torch.equal(_bits(taped[k].x[0]), _bits(updates[k].x)), "the first piece is not the stream batch"
            assert c.logits.shape == (rows, 10) and torch.equal(_bits(c.logits), _bits(taped[k].out))
            assert backs[k].dout is c.dl and backs[k].tape is taped[k].tape and backs[k].n_calls == k + 1
            assert torch.equal(_bits(backs[k].bits), _bits(c.dl_bits)), "dl was changed between the kernel and the backward"
            assert steps[k].n_back == k + 1
            if t == 0:
                assert c.teacher is None and float(c.loss3[1]) == 0.0 and torch.equal(_bits(c.loss3[0]), _bits(c.loss3[2]))
            else:
                f = fwp[k - 2]
                assert c.teacher is f.out and f.grad is False and len(f.x) == 2
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(f.x, taped[k].x)), "the teacher saw other images"
                assert torch.equal(_bits(f.flat_bits), _bits(snaps[t - 1])), "the teacher is not the snapshot of the previous task's end"
                assert float(c.loss3[1]) > 0.0
            want_l, want_dl = ref_bce_distill(_host(c.logits), None if c.teacher is None else _host(c.teacher), _host(c.pos), 10, c.n_cls, c.n_old)
            assert np.abs(_host(c.loss3) - want_l).max() <= 1e-5 * max(1.0, np.abs(want_l).max())
            assert np.abs(_host(c.dl_bits) - want_dl).max() <= 1e-5 * np.abs(want_dl).max()
        # the running statistics after each step with a teacher, against a twin that ran the student's forward alone from the same state
        twin = setup_architecture(params).cuda()
        for k in (2, 3, 4, 5):
            twin.load_state_dict(before[k])
            twin.train()
            with torch.no_grad():
                twin.forward(tuple(taped[k].x))
            want, got = _bn_stats(twin.state_dict()), _bn_stats(steps[k].state)
            assert want.keys() == got.keys() and len(want) > 0
            for name in want:
                assert torch.equal(want[name], got[name]), "step %d: %s differs from the student-only forward's" % (k, name)
            assert any(not torch.equal(before[k][name], got[name]) for name in want if name.endswith("running_mean"))
    finally:
        ops.set_deterministic(False)


# ---- 5. co-simulation against IcarlOracle ----------------------------------------------------------------------------------------------

def test_cosim_icarl(cuda, monkeypatch):
    """The three tasks of the case, one train_learner call (six batches) per task; before every call the HIP model is loaded with the
    oracle's state and agent.prev.teacher_model with the oracle's teacher (the teacher's state dict loaded into the model, flat_params()
    cloned), between the steps of a call the model is loaded with the oracle's again (the per-step bounds are bounds for one step from
    the same state), and both sides consume the same host RNG streams and keep their own replay memories.  Per call: RNG state and
    memory contents equal.  Per step: the retrieved slots equal, the loss within 1e-4 * max(1, |loss|), the update within 1e-2
    norm-wise (the project's co-simulation bounds)."""
    from ocl_amd import debug
    cfg = ICARL_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = icarl_ref.IcarlOracle(cfg)
    tasks = icarl_ref.cosim_stream(cfg)
    seed_all(1000 + cfg["seed"])
    steps, ostates = [], []
    inner_step = opt.step

    def step(*a, **k):
        out = inner_step(*a, **k)
        steps.append(model.flat_params().double().cpu().numpy())
        if len(steps) < len(ostates):           # not after the call's last step: the task's end keeps the agent's own weights
            model.load_state_dict(ostates[len(steps) - 1])
        return out

    opt.step = step
    worst = dict(loss=0.0, update=0.0)
    with_teacher = 0
    for it, (x, y) in enumerate(tasks):
        if oa.teacher is None:
            assert it == 0 and agent.prev.teacher_model is None
        else:
            model.load_state_dict(oa.teacher)
            agent.prev.teacher_model = model.flat_params().detach().clone()
            assert agent.prev._owner is model
        model.load_state_dict(oa.state_dict())
        w_before = [_flat(oa.state, oa.names)]
        st = _rng_get()
        n_log = len(oa.log)
        del ostates[:]
        inner_icarl_step = icarl_ref.icarl_step

        def spy(state, names, *a, **k):
            out = inner_icarl_step(state, names, *a, **k)
            w_before.append(_flat(state, names))
            ostates.append({k_: v.detach().clone() for k_, v in state.items()})
            return out

        monkeypatch.setattr(icarl_ref, "icarl_step", spy)
        oa.train_learner(x, y)
        monkeypatch.setattr(icarl_ref, "icarl_step", inner_icarl_step)
        logs = oa.log[n_log:]
        st_o = _rng_get()
        _rng_set(st)
        del steps[:]
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        assert len(logs) == 6 and agent.task_seen == oa.task_seen == it + 1 and agent.old_labels == oa.old_labels
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged in call %d" % it
        assert agent.buffer.current_index == oa.buf.current_index and agent.buffer.n_seen_so_far == oa.buf.n_seen_so_far
        assert np.array_equal(agent.buffer.buffer_label.cpu().numpy(), oa.buf.label.numpy())
        assert torch.allclose(agent.buffer.buffer_img.cpu(), oa.buf.img, rtol=0, atol=2.0 ** -24), "the replay memories hold different images after call %d" % it
        loss, drawn = _events(ev, "icarl_loss"), _events(ev, "random_retrieve")
        assert len(loss) == 6 and len(steps) == 6 and len(w_before) == 7 and len(drawn) == (6 if it else 0)
        for k in range(6):
            ol = logs[k]
            assert ol["teacher"] == (it > 0) and ol["rows"] == (20 if it else 10)
            if it:
                assert np.array_equal(drawn[k]["indices"], ol["indices"]), (it, k)
                assert loss[k]["old"] > 0
            else:
                assert loss[k]["old"] == 0.0
            d_loss = abs(loss[k]["loss"] - ol["loss"]) / max(1.0, abs(ol["loss"]))
            dw_o = w_before[k + 1] - w_before[k]
            dw_m = steps[k] - w_before[k]
            upd = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
            print("icarl cosim call %d step %d  loss %.6f / %.6f (old %.6f, new %.6f)  update err %.2e"
                  % (it, k, loss[k]["loss"], ol["loss"], loss[k]["old"], loss[k]["new"], upd))
            worst["loss"], worst["update"] = max(worst["loss"], d_loss), max(worst["update"], upd)
            assert d_loss <= 1e-4, (it, k, loss[k], ol)
            assert abs(loss[k]["old"] + loss[k]["new"] - loss[k]["loss"]) <= 1e-5 * max(1.0, abs(loss[k]["loss"]))
            assert upd <= 1e-2, (it, k, upd)
            with_teacher += it > 0
        assert torch.equal(_bits(agent.prev.teacher_model), _bits(model.flat_params())), "the task's end did not refresh the teacher"
    print("icarl cosim: %d steps with a teacher; worst loss diff %.2e (relative above 1), update err %.2e" % (with_teacher, worst["loss"], worst["update"]))
    assert with_teacher >= 6


# ---- 6. the comparator -------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-5     # test_gpu_ewc.COMPARATOR_BOUND


def test_fused_step_against_the_autograd_statements_on_the_same_state(cuda, monkeypatch):
    """`_force_autograd` runs the reference's statements: forward of (stream batch, memory rows), the one-hot, the cat with zeros, the
    sigmoid, one column copy per old class, F.binary_cross_entropy_with_logits, autograd.  Two agents from one seed run the first task
    (one each way, from the same host RNG state, each filling its own memory); then, for the six steps of the second task, the
    comparator starts every step from the fused agent's weights, running statistics and teacher, under order-independent batch sums.
    One step's updates agree within 1e-5 norm-wise (the two differ by the float32 rounding of dL/dlogits alone: the forward and the
    backward are the same function on both sides) and the running statistics bit for bit.  The comparator calls ops.bce_distill never."""
    from ocl_amd import ops
    cfg = ICARL_CASE
    ops.set_deterministic(True)
    try:
        _, model_a, opt_a, a = _build_agent(cfg)
        _, model_b, opt_b, b = _build_agent(cfg)
        b._force_autograd = True
        calls = _spy_bce(monkeypatch.setattr)
        tasks, _ = make_stream(cfg)
        st = _rng_get()
        a.train_learner(*tasks[0])
        assert len(calls) == 6
        _rng_set(st)
        b.train_learner(*tasks[0])
        assert len(calls) == 6, "the comparator called the fused kernel"
        assert torch.equal(a.buffer.buffer_img, b.buffer.buffer_img) and torch.equal(a.buffer.buffer_label, b.buffer.buffer_label)
        model_b.load_state_dict(model_a.state_dict())
        b.prev.teacher_model.copy_(a.prev.teacher_model)
        pre, post, got = [], [], []
        inner_a, inner_b = opt_a.step, opt_b.step

        def step_a(*args, **kw):
            w0 = model_a.flat_params().double().cpu().numpy()
            out = inner_a(*args, **kw)
            pre.append(w0)
            post.append({k: v.clone() for k, v in model_a.state_dict().items()})
            return out

        def step_b(*args, **kw):
            out = inner_b(*args, **kw)
            got.append({k: v.clone() for k, v in model_b.state_dict().items()})
            if len(got) < len(post):
                model_b.load_state_dict(post[len(got) - 1])
            return out

        opt_a.step, opt_b.step = step_a, step_b
        st = _rng_get()
        a.train_learner(*tasks[1])
        _rng_set(st)
        b.train_learner(*tasks[1])
        assert len(calls) == 12 and len(pre) == len(post) == len(got) == 6 and all(c.teacher is not None and c.n_old == 2 for c in calls[6:])
        assert torch.equal(a.buffer.buffer_img, b.buffer.buffer_img) and torch.equal(a.buffer.buffer_label, b.buffer.buffer_label)
        names = [n for n, _ in model_a.named_parameters()]
        worst = 0.0
        for k in range(6):
            wa, wb = _flat(post[k], names), _flat(got[k], names)
            diff = float(np.linalg.norm((wb - pre[k]) - (wa - pre[k])) / np.linalg.norm(wa - pre[k]))
            worst = max(worst, diff)
            print("icarl comparator step %d  update difference %.2e (allowed %.0e)" % (k, diff, COMPARATOR_BOUND))
            assert diff <= COMPARATOR_BOUND, (k, diff)
            sa, sb = _bn_stats(post[k]), _bn_stats(got[k])
            assert sa.keys() == sb.keys() and all(torch.equal(sa[n], sb[n]) for n in sa), "running statistics differ at step %d" % k
        print("icarl comparator: worst norm-wise update difference over the second task %.2e" % worst)
    finally:
        ops.set_deterministic(False)


# ---- 7. a retrieval shorter than the batch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False], ids=["fused", "autograd"])
def test_a_short_retrieval_raises_value_error_before_anything_runs(cuda, monkeypatch, fused):
    """The reference pairs the memory rows with `batch` rows of zero targets, so a retrieval of fewer rows makes its BCE raise
    ValueError.  Here: past the first task, with an emptied memory (and with one of 7 slots), the next step raises ValueError naming both
    row counts; no kernel call, no forward, the parameters untouched."""
    cfg = ICARL_CASE
    params, model, opt, agent = _build_agent(cfg)
    agent._force_autograd = not fused
    tasks, _ = make_stream(cfg)
    pick = np.r_[0:10, 30:40]
    agent.train_learner(tasks[0][0][pick], tasks[0][1][pick])
    calls = _spy_bce(monkeypatch.setattr)
    forwards = []
    for name in ("forward", "forward_views_taped", "forward_with_params"):
        inner = getattr(model, name)
        monkeypatch.setattr(model, name, lambda *a, _inner=inner, _name=name, **k: (forwards.append(_name), _inner(*a, **k))[1])
    for filled, rows in ((0, 0), (7, 7)):
        agent.buffer.current_index = filled
        flat = model.flat_params().clone()
        with pytest.raises(ValueError, match=r"10 stream rows.* %d \(" % rows):
            agent.train_learner(tasks[1][0][pick], tasks[1][1][pick])
        assert not calls and not forwards and torch.equal(_bits(flat), _bits(model.flat_params()))
        agent.new_labels.clear()


# ---- 8. free run against the recorded reference run -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def free_run(cuda):
    """Whole tasks, free running with the debug trace on: what the two tests below look at."""
    from ocl_amd import debug, ops
    from ocl_amd.data import setup_test_loader
    cfg = ICARL_CASE
    params, model, opt, agent = _build_agent(cfg)
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    calls = _spy_bce(patch)
    predicts = []
    inner_predict = ops.ncm_predict
    patch(ops, "ncm_predict", lambda *a, **k: (predicts.append(len(calls)), inner_predict(*a, **k))[1])
    n_steps = []
    inner = opt.step
    opt.step = lambda *a, **k: (n_steps.append(len(calls)), inner(*a, **k))[1]
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    per_task = []
    try:
        for t, (x, y) in enumerate(tasks):
            debug.LOG = []
            try:
                agent.train_learner(x, y)
                ev = list(debug.LOG)
            finally:
                debug.LOG = None
            n_predicts = len(predicts)
            acc = agent.evaluate(loaders)
            per_task.append(SimpleNamespace(ev=ev, acc=acc, task_seen=agent.task_seen, old_labels=list(agent.old_labels), new_labels=list(agent.new_labels),
                                            class_task_map=dict(agent.class_task_map), n_steps=list(n_steps), current_index=agent.buffer.current_index,
                                            n_seen=agent.buffer.n_seen_so_far, digest=digest_state(model.state_dict()), n_predicts=len(predicts) - n_predicts,
                                            teacher_is_model=torch.equal(_bits(agent.prev.teacher_model), _bits(model.flat_params()))))
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    return SimpleNamespace(cfg=cfg, calls=calls, per_task=per_task)


def test_retrievals_avoid_the_slots_written_during_the_task_and_equal_the_recorded_ones(free_run):
    """Every traced random_retrieve of a task holds `batch` distinct filled slots, none of them written by the reservoir update earlier
    in the same train_learner call; over the run they are the indices recorded from the reference (they depend on the host RNG streams
    and on the slots alone, not on the weights).  At least one retrieval excluded something."""
    g = gold("icarl")
    drawn, n_excl = [], []
    for t, rec in enumerate(free_run.per_task):
        updated = []
        for tag, e in rec.ev:
            if tag == "random_retrieve":
                idx = e["indices"].tolist()
                assert len(idx) == 10 == len(set(idx)) and not set(idx) & set(updated), (t, idx, updated)
                drawn.append(idx)
                n_excl.append(len(updated))
            elif tag == "reservoir":
                updated += list(e["slots"])
        assert sum(tag == "random_retrieve" for tag, _ in rec.ev) == (6 if t else 0)
    assert np.array_equal(np.array(drawn), g["icarl_c10_retrievals"])
    assert n_excl == g["icarl_c10_n_excluded"].tolist() and max(n_excl) > 0


def test_free_run_vs_reference_golden(free_run):
    """Whole tasks, free running, against the run recorded from the REAL reference agent (tests/golden/icarl.npz): counters and task
    bookkeeping are exact; the weights follow a chaotic trajectory and get the sanity band of test_gpu_lwf's free run; evaluate
    classified by the nearest class mean."""
    g = gold("icarl")
    cfg, calls = free_run.cfg, free_run.calls
    assert int(g["icarl_c10_ntasks"]) == len(free_run.per_task) == 3 and int(g["icarl_c10_steps_per_task"]) == 6
    seen = []
    for t, rec in enumerate(free_run.per_task):
        seen += cfg["tasks"][t]
        assert rec.task_seen == t + 1 and sorted(rec.old_labels) == seen and rec.new_labels == []
        assert rec.class_task_map == {c: i for i, cs in enumerate(cfg["tasks"][:t + 1]) for c in cs}
        assert rec.n_steps == list(range(1, 6 * (t + 1) + 1)), "one kernel call per optimiser step"
        assert rec.current_index == 50 and rec.n_seen == 60 * (t + 1)
        assert [c.teacher is not None for c in calls[6 * t:6 * t + 6]] == [t > 0] * 6
        assert all((c.n_stream, c.n_cls, c.n_old) == (10, 2 * t + 2, 2 * t) for c in calls[6 * t:6 * t + 6])
        assert all(c.logits.shape == ((20, 10) if t else (10, 10)) for c in calls[6 * t:6 * t + 6])
        assert rec.teacher_is_model and rec.n_predicts == 3, "evaluate did not go through ops.ncm_predict once per test loader"
        pre = "icarl_c10_t%d_" % t
        ds, gs = rec.digest, g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        first = [float(c.loss3[0]) for c in calls[6 * t:6 * t + 2]]
        print("icarl_c10", t, "state digest rel err", rel, "norm ratio", ratio, "acc", rec.acc, g[pre + "acc"], "first losses", first,
              "recorded", g["icarl_c10_losses"][t].tolist())
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert rec.acc.shape == g[pre + "acc"].shape and (rec.acc >= 0).all() and (rec.acc <= 1).all()
        assert np.isfinite(first).all() and all(f > 0 for f in first)
    assert len(calls) == 18
    # the very first step starts from the seeded weights on both sides
    assert abs(float(calls[0].loss3[0]) - g["icarl_c10_losses"][0, 0]) < 1e-4
