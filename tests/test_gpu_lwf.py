"""GPU: the blended cross-entropy + distillation kernel (csrc/distill.hip: ocl_ce_kd_blend_fwd_bwd; ops.ce_kd_blend) and the LwF agent
built on it (agents/lwf.py), against the float64 statement of the loss, the plain float32 statement, and the restatement of the
reference's loop (tests/lwf_ref.py, all pinned on the CPU by tests/test_cpu_lwf.py).

The kernel is judged by parity_bounds.check_vs_torch32, the project's rule for transcendental kernels: its error against float64 is at
most max(4 x the error of torch's own float32 statements on the same inputs, 4 ulp of the largest reference element), for each of the
three losses and for the gradient.  Observed values: profiles/lwf_parity.txt."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (TRICK, build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from conftest import gold
from guarded import Guarded
from oracle.synth import make_stream, seed_all, digest_state
import parity_bounds
import lwf_ref
from lwf_ref import LWF_CASE, ref_blend, torch32_blend, logits_for

pytestmark = pytest.mark.gpu

_build_agent = functools.partial(build_agent, extra=lwf_ref.ref_params)

REPORT = []
# (n, c, logit scale, T): the CE family's shapes with the KD family's temperatures; they bracket 4 waves per block and 64 lanes per row
CASES = [(1, 5, 1, 2.0), (3, 10, 30, 1.0), (4, 64, 1, 4.0), (5, 100, 300, 2.0), (10, 100, 1, 2.0), (10, 65, 1, 2.0), (10, 128, 30, 3.0),
         (37, 200, 1, 0.5), (7, 1000, 30, 3.0), (64, 63, 1, 2.0)]
# both sides of the row length at which the kernel stops holding the row in registers (256), and the last full register
THRESHOLD_CASES = [(6, 192, 1, 2.0), (6, 193, 30, 3.0), (6, 256, 1, 2.0), (6, 257, 1, 2.0), (5, 321, 30, 3.0)]
WEIGHTS = [(1 / 2, 1 / 2), (1 / 3, 2 / 3), (1 / 10, 9 / 10)]


def _case(n, c, scale, T):
    rng = np.random.default_rng(7000 + 131 * n + c)
    s, t = logits_for(rng, n, c, scale), logits_for(rng, n, c, scale)
    return s, t, rng.integers(0, c, n).astype(np.int64)


# ---- 1. the kernel against the float64 statement ---------------------------------------------------------------------------------------

def _check_case(n, c, scale, T, w_new, w_old, with_teacher=True):
    from ocl_amd import ffi
    lib = ffi.lib()
    s, t, y = _case(n, c, scale, T)
    teacher = t if with_teacher else None
    l64, g64 = ref_blend(s, y, teacher, T, w_new, w_old)
    l32, g32 = torch32_blend(s, y, teacher, T, w_new, w_old)
    g = Guarded()
    d_s, d_y = g.inp(s, 0, "logits"), g.inp(y, 0, "y")
    d_t = g.inp(t, 0, "teacher") if with_teacher else None
    d_l, d_dl = g.out((3,), torch.float32, 0, "loss_out"), g.out((n, c), torch.float32, 0, "dlogits")
    rc = lib.ocl_ce_kd_blend_fwd_bwd(ffi.ptr(d_s), ffi.ptr(d_y), ffi.ptr(d_t), n, c, T, w_new, w_old, ffi.ptr(d_l), ffi.ptr(d_dl), ffi.stream())
    assert rc == 0, lib.ocl_last_error()
    g.check("ce_kd_blend")
    got_l, got_g = _host(d_l), _host(d_dl)
    assert np.isfinite(got_l).all() and np.isfinite(got_g).all()
    name = "blend n=%d c=%d scale=%g T=%g w=(%.3g, %.3g)%s" % (n, c, scale, T, w_new, w_old, "" if with_teacher else " no teacher")
    for k, which in enumerate(("loss", "ce", "kd")):
        parity_bounds.check_vs_torch32(REPORT, name, which, got_l[k:k + 1], l64[k:k + 1], l32[k:k + 1])
    parity_bounds.check_vs_torch32(REPORT, name, "dlogits", got_g, g64, g32)


@pytest.mark.parametrize("w_new,w_old", WEIGHTS, ids=["w1/2", "w1/3", "w1/10"])
@pytest.mark.parametrize("n,c,scale,T", CASES)
def test_blend_vs_float64_reference(cuda, n, c, scale, T, w_new, w_old):
    _check_case(n, c, scale, T, w_new, w_old)


@pytest.mark.parametrize("n,c,scale,T", THRESHOLD_CASES)
def test_blend_vs_float64_reference_around_the_register_threshold(cuda, n, c, scale, T):
    _check_case(n, c, scale, T, 1 / 3, 2 / 3)
    _check_case(n, c, scale, T, 1 / 3, 2 / 3, with_teacher=False)


@pytest.mark.parametrize("n,c,scale,T", [CASES[0], CASES[4], CASES[8]])
def test_blend_without_a_teacher_vs_float64_reference(cuda, n, c, scale, T):
    _check_case(n, c, scale, T, 1.0, 0.0, with_teacher=False)


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,c,scale,T", CASES + THRESHOLD_CASES)
def test_without_a_teacher_and_with_unit_weight_the_blend_is_the_cross_entropy_kernel_bit_for_bit(cuda, n, c, scale, T):
    from ocl_amd import ops
    s, _, y = _case(n, c, scale, T)
    d_s, d_y = _dev(s, cuda), _dev(y, cuda, np.int64)
    want_l, want_dl = ops.cross_entropy(d_s, d_y, "mean")
    for w_old in (0.0, 0.75):                 # without a teacher w_old multiplies nothing
        loss3, dl = ops.ce_kd_blend(d_s, d_y, None, T, 1.0, w_old)
        assert torch.equal(_bits(loss3[0]), _bits(want_l)) and torch.equal(_bits(loss3[1]), _bits(want_l))
        assert float(loss3[2]) == 0.0
        assert torch.equal(_bits(dl), _bits(want_dl))


@pytest.mark.parametrize("n,c,scale,T", CASES + THRESHOLD_CASES)
def test_a_teacher_equal_to_the_student_adds_exactly_nothing_to_the_gradient(cuda, n, c, scale, T):
    from ocl_amd import ops
    s, _, y = _case(n, c, scale, T)
    d_s, d_y = _dev(s, cuda), _dev(y, cuda, np.int64)
    d_t = d_s.clone()
    for w_new, w_old in WEIGHTS:
        l_a, dl_a = ops.ce_kd_blend(d_s, d_y, d_t, T, w_new, w_old)
        l_b, dl_b = ops.ce_kd_blend(d_s, d_y, d_t, T, w_new, 0.0)
        assert torch.equal(_bits(dl_a), _bits(dl_b))
        assert torch.equal(_bits(l_a[1:]), _bits(l_b[1:])) and float(l_a[2]) >= 0.0


@pytest.mark.parametrize("n,c,scale,T", CASES + THRESHOLD_CASES)
def test_two_runs_are_bit_identical_and_the_losses_do_not_depend_on_want_grad(cuda, n, c, scale, T):
    from ocl_amd import ops
    s, t, y = _case(n, c, scale, T)
    d_s, d_t, d_y = _dev(s, cuda), _dev(t, cuda), _dev(y, cuda, np.int64)
    for teacher in (d_t, None):
        l_a, dl_a = ops.ce_kd_blend(d_s, d_y, teacher, T, 1 / 3, 2 / 3)
        l_b, dl_b = ops.ce_kd_blend(d_s, d_y, teacher, T, 1 / 3, 2 / 3)
        l_c, dl_c = ops.ce_kd_blend(d_s, d_y, teacher, T, 1 / 3, 2 / 3, want_grad=False)
        assert dl_c is None and dl_a is not dl_b
        assert torch.equal(_bits(l_a), _bits(l_b)) and torch.equal(_bits(dl_a), _bits(dl_b)) and torch.equal(_bits(l_a), _bits(l_c))


def test_dl_out_writes_into_a_row_block_of_a_larger_buffer_and_leaves_the_rest(cuda):
    from ocl_amd import ops
    n, c = 10, 100
    s, t, y = _case(n, c, 1, 2.0)
    d_s, d_t, d_y = _dev(s, cuda), _dev(t, cuda), _dev(y, cuda, np.int64)
    big = torch.full((3 * n, c), -7777.0, device=cuda)
    loss3, dl = ops.ce_kd_blend(d_s, d_y, d_t, 2.0, 0.5, 0.5, dl_out=big[n:2 * n])
    want_l, want_dl = ops.ce_kd_blend(d_s, d_y, d_t, 2.0, 0.5, 0.5)
    assert dl.data_ptr() == big[n:2 * n].data_ptr() and torch.equal(_bits(dl), _bits(want_dl)) and torch.equal(_bits(loss3), _bits(want_l))
    assert bool((big[:n] == -7777.0).all()) and bool((big[2 * n:] == -7777.0).all())
    for bad in (big[:, :c // 2], big[:n].double(), big[:n + 1], big[:n].cpu()):
        with pytest.raises(RuntimeError):
            ops.ce_kd_blend(d_s, d_y, d_t, 2.0, 0.5, 0.5, dl_out=bad)
    with pytest.raises(RuntimeError):
        ops.ce_kd_blend(d_s, d_y, d_t[:, :50], 2.0, 0.5, 0.5)
    with pytest.raises(RuntimeError):
        ops.ce_kd_blend(d_s, d_y.cpu(), d_t, 2.0, 0.5, 0.5)


# ---- 3. refused arguments ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from ocl_amd import ffi
    lib = ffi.lib()
    n, c = 4, 8
    s, t = torch.full((n, c), 1.0, device=cuda), torch.full((n, c), 2.0, device=cuda)
    y = torch.zeros(n, dtype=torch.int64, device=cuda)
    loss, dl = torch.full((3,), -7777.0, device=cuda), torch.full((n, c), -7777.0, device=cuda)
    nan, inf = float("nan"), float("inf")

    def call(**over):
        kw = dict(s=s.data_ptr(), y=y.data_ptr(), t=t.data_ptr(), n=n, c=c, T=2.0, w_new=0.5, w_old=0.5, loss=loss.data_ptr(), dl=dl.data_ptr())
        kw.update(over)
        rc = lib.ocl_ce_kd_blend_fwd_bwd(ffi.vp(kw["s"]), ffi.vp(kw["y"]), ffi.vp(kw["t"]), kw["n"], kw["c"], kw["T"], kw["w_new"], kw["w_old"],
                                         ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.stream())
        return rc, lib.ocl_last_error()

    for over in (dict(n=0), dict(n=-1), dict(c=0), dict(c=-5), dict(T=0.0), dict(T=-1.0), dict(T=nan), dict(T=inf), dict(w_new=nan), dict(w_new=inf),
                 dict(w_old=nan), dict(w_old=-inf), dict(s=0), dict(y=0), dict(loss=0),
                 dict(dl=s.data_ptr()), dict(dl=s.data_ptr() + 4 * (n * c - 1)), dict(dl=t.data_ptr()), dict(dl=t.data_ptr() + 64)):
        rc, msg = call(**over)
        assert rc == -1 and msg.startswith(b"ce_kd_blend:"), (over, rc, msg)
        if "dl" in over:
            assert b"overlap" in msg, (over, msg)
    torch.cuda.synchronize()
    assert bool((loss == -7777.0).all()) and bool((dl == -7777.0).all()) and bool((s == 1.0).all()) and bool((t == 2.0).all())
    rc, msg = call()
    assert rc == 0, msg
    rc, msg = call(t=0, dl=0)               # both optional pointers null: the losses alone
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool((dl == -7777.0).any()) and float(loss[2]) == 0.0


# ---- 4. the agent ---------------------------------------------------------------------------------------------------------------------

def _spy_blend(monkeypatch):
    from ocl_amd import ops
    calls = []
    inner = ops.ce_kd_blend

    def ce_kd_blend(logits, y, teacher_logits, T, w_new, w_old, want_grad=True, dl_out=None):
        loss3, dl = inner(logits, y, teacher_logits, T, w_new, w_old, want_grad=want_grad, dl_out=dl_out)
        calls.append(SimpleNamespace(logits=logits.clone(), y=y.clone(), teacher=teacher_logits, T=T, w_new=w_new, w_old=w_old, dl=dl,
                                     dl_bits=dl.clone(), loss3=loss3.clone()))
        return loss3, dl

    monkeypatch.setattr(ops, "ce_kd_blend", ce_kd_blend)
    return calls


def _bn_stats(state):
    return {k: v for k, v in state.items() if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


def test_agent_hands_the_right_things_to_the_kernel_and_its_gradient_to_the_backward(cuda, monkeypatch):
    """Three train_learner calls of two batches each, order-independent batch sums.  Task 1: no teacher, no teacher forward, weights
    (1, 0).  Task 2: the teacher's logits are forward_with_params' output for the batch and the snapshot taken at the end of task 1
    (bit-equal to flat_params at that moment), weights (1/2, 1/2).  Task 3: (1/3, 2/3), task 2's snapshot.  The kernel's dl is the very
    tensor backward_taped receives, unchanged, and the logits are those of the taped forward.  The teacher's pass leaves the student's
    BatchNorm running statistics alone: after a step they are the bits of a twin model that ran the student's forward only."""
    from ocl_amd import ops
    from ocl_amd.setup_elements import setup_architecture
    cfg = dict(LWF_CASE, seed=23)
    ops.set_deterministic(True)
    try:
        params, model, opt, agent = _build_agent(cfg)
        calls = _spy_blend(monkeypatch)
        fwp, taped, backs, steps, before = [], [], [], [], []
        inner_fwp, inner_taped, inner_back, inner_step = model.forward_with_params, model.forward_views_taped, model.backward_taped, opt.step

        def forward_with_params(x, flat):
            out = inner_fwp(x, flat)
            fwp.append(SimpleNamespace(x=x.clone(), flat=flat, flat_bits=flat.clone(), out=out, grad=torch.is_grad_enabled(), at=len(taped)))
            return out

        def forward_views_taped(views):
            before.append({k: v.clone() for k, v in model.state_dict().items()})
            out, tape = inner_taped(views)
            taped.append(SimpleNamespace(x=views[0].clone(), n_views=len(views), out=out, tape=tape))
            return out, tape

        def backward_taped(tape, dout):
            backs.append(SimpleNamespace(tape=tape, dout=dout, bits=dout.clone(), n_calls=len(calls)))
            return inner_back(tape, dout)

        def step(*a, **k):
            out = inner_step(*a, **k)
            steps.append(SimpleNamespace(n_back=len(backs), state={k_: v.clone() for k_, v in model.state_dict().items()}))
            return out

        model.forward_with_params, model.forward_views_taped, model.backward_taped, opt.step = forward_with_params, forward_views_taped, backward_taped, step
        tasks, _ = make_stream(cfg)
        pick = np.r_[0:10, 30:40]
        snaps = []
        for t in range(3):
            assert (agent.kd_manager.teacher_model is None) == (t == 0)
            agent.train_learner(tasks[t][0][pick], tasks[t][1][pick])
            assert agent.task_seen == t + 1 and len(calls) == len(taped) == len(backs) == len(steps) == 2 * (t + 1)
            teacher = agent.kd_manager.teacher_model
            assert torch.equal(_bits(teacher), _bits(model.flat_params())) and teacher.data_ptr() != model.flat_params().data_ptr()
            snaps.append(teacher.clone())
        assert len(fwp) == 4 and [f.at for f in fwp] == [3, 4, 5, 6], "the teacher's pass follows the student's, from the second task on"
        for k, c in enumerate(calls):
            t = k // 2
            assert c.T == 2.0 and np.float32(c.w_new) == np.float32(1 / (t + 1)) and np.float32(c.w_old) == np.float32(1 - 1 / (t + 1))
            assert (c.w_new, c.w_old) == ((1.0, 0.0) if t == 0 else (1 / (t + 1), 1 - 1 / (t + 1)))
            assert taped[k].n_views == 1 and c.logits.shape == (10, 10) and torch.equal(_bits(c.logits), _bits(taped[k].out))
            assert backs[k].dout is c.dl and backs[k].tape is taped[k].tape and backs[k].n_calls == k + 1
            assert torch.equal(_bits(backs[k].bits), _bits(c.dl_bits)), "dl was changed between the kernel and the backward"
            assert steps[k].n_back == k + 1
            if t == 0:
                assert c.teacher is None and float(c.loss3[2]) == 0.0 and torch.equal(_bits(c.loss3[0]), _bits(c.loss3[1]))
            else:
                f = fwp[k - 2]
                assert c.teacher is f.out and f.grad is False
                assert torch.equal(_bits(f.x), _bits(taped[k].x)), "the teacher saw another batch"
                assert torch.equal(_bits(f.flat_bits), _bits(snaps[t - 1])), "the teacher is not the snapshot of the previous task's end"
                assert float(c.loss3[2]) > 0.0
            want_l, want_dl = ref_blend(_host(c.logits), _host(c.y), None if c.teacher is None else _host(c.teacher), 2.0, c.w_new, c.w_old)
            assert np.abs(_host(c.loss3) - want_l).max() <= 1e-5 * max(1.0, np.abs(want_l).max())
            assert np.abs(_host(c.dl_bits) - want_dl).max() <= 1e-5 * np.abs(want_dl).max()
        # the running statistics after each step with a teacher, against a twin that ran the student's forward alone from the same state
        twin = setup_architecture(params).cuda()
        for k in (2, 3, 4, 5):
            twin.load_state_dict(before[k])
            twin.train()
            with torch.no_grad():
                twin.forward(taped[k].x)
            want, got = _bn_stats(twin.state_dict()), _bn_stats(steps[k].state)
            assert want.keys() == got.keys() and len(want) > 0
            for name in want:
                assert torch.equal(want[name], got[name]), "step %d: %s differs from the student-only forward's" % (k, name)
            assert any(not torch.equal(before[k][name], got[name]) for name in want if name.endswith("running_mean"))
    finally:
        ops.set_deterministic(False)


# ---- 5. co-simulation against LwfOracle ------------------------------------------------------------------------------------------------

def test_cosim_lwf(cuda, monkeypatch):
    """The three tasks of lwf_c10 concatenated, 9 sequential slices of 20, one train_learner call (two batches) per slice; before every
    call the HIP model is loaded with the oracle's state and kd_manager.teacher_model with the oracle's teacher (the teacher's state
    dict loaded into the model, flat_params() cloned), between the two steps of a call the model is loaded with the oracle's again (the
    per-step bounds are bounds for one step from the same state), and both sides consume the same host RNG streams.  Per call: RNG state
    equal.  Per step: loss_new within 1e-4 (ER's bound), loss_old within 1e-4 * max(1, |loss_old|), the update within 1e-2 norm-wise
    (ER's co-simulation bound)."""
    from ocl_amd import debug
    cfg = LWF_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = lwf_ref.LwfOracle(cfg)
    xs, ys = lwf_ref.cosim_stream(cfg)
    assert xs.shape[0] == 180
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
    worst = dict(loss_new=0.0, loss_old=0.0, update=0.0)
    with_teacher = 0
    for it in range(9):
        x, y = xs[it * 20:(it + 1) * 20], ys[it * 20:(it + 1) * 20]
        if oa.teacher is None:
            assert it == 0 and agent.kd_manager.teacher_model is None
        else:
            model.load_state_dict(oa.teacher)
            agent.kd_manager.teacher_model = model.flat_params().detach().clone()
            assert agent.kd_manager._owner is model
        model.load_state_dict(oa.state_dict())
        w_before = [_flat(oa.state, oa.names)]
        st = _rng_get()
        n_log = len(oa.log)
        del ostates[:]
        inner_lwf_step = lwf_ref.lwf_step

        def spy(state, names, *a, **k):
            out = inner_lwf_step(state, names, *a, **k)
            w_before.append(_flat(state, names))
            ostates.append({k_: v.detach().clone() for k_, v in state.items()})
            return out

        monkeypatch.setattr(lwf_ref, "lwf_step", spy)
        oa.train_learner(x, y)
        monkeypatch.setattr(lwf_ref, "lwf_step", inner_lwf_step)
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
        assert len(logs) == 2 and agent.task_seen == oa.task_seen == it + 1
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged in call %d" % it
        loss = _events(ev, "lwf_loss")
        assert len(loss) == 2 and len(steps) == 2 and len(w_before) == 3
        for k in range(2):
            ol = logs[k]
            assert ol["teacher"] == (it > 0)
            d_new = abs(loss[k]["loss_new"] - ol["loss_new"])
            d_old = abs(loss[k]["loss_old"] - ol["loss_old"]) / max(1.0, abs(ol["loss_old"]))
            d_tot = abs(loss[k]["loss"] - ol["loss"]) / max(1.0, abs(ol["loss"]))
            dw_o = w_before[k + 1] - w_before[k]
            dw_m = steps[k] - w_before[k]
            upd = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
            print("lwf cosim call %d step %d  loss_new %.6f / %.6f  loss_old %.6f / %.6f  loss %.6f / %.6f  update err %.2e"
                  % (it, k, loss[k]["loss_new"], ol["loss_new"], loss[k]["loss_old"], ol["loss_old"], loss[k]["loss"], ol["loss"], upd))
            worst["loss_new"], worst["loss_old"], worst["update"] = max(worst["loss_new"], d_new), max(worst["loss_old"], d_old), max(worst["update"], upd)
            assert d_new < 1e-4, (it, k, loss[k], ol)
            assert d_old <= 1e-4, (it, k, loss[k], ol)
            assert d_tot <= 1e-4, (it, k, loss[k], ol)
            assert upd <= 1e-2, (it, k, upd)
            assert (loss[k]["loss_old"] > 0) == (it > 0) == (ol["loss_old"] > 0)
            with_teacher += it > 0
        assert torch.equal(_bits(agent.kd_manager.teacher_model), _bits(model.flat_params())), "after_train did not refresh the teacher"
    print("lwf cosim: %d steps with a teacher; worst |loss_new diff| %.2e, loss_old diff %.2e (relative above 1), update err %.2e"
          % (with_teacher, worst["loss_new"], worst["loss_old"], worst["update"]))
    assert with_teacher >= 6


# ---- 6. the comparator -------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-5     # test_gpu_ewc.COMPARATOR_BOUND


def test_fused_step_against_the_autograd_statements_on_the_same_state(cuda, monkeypatch):
    """`_force_autograd` runs the reference's statements: forward, criterion, get_kd_loss, the blend, autograd.  Two agents from one seed
    run the first task (one each way, from the same host RNG state); then, for the six steps of the second task, the comparator starts
    every step from the fused agent's weights, running statistics and teacher, under order-independent batch sums.  One step's updates
    agree within 1e-5 norm-wise (the two differ by the float32 rounding of dL/dlogits alone: the forward and the backward are the same
    function on both sides) and the running statistics bit for bit.  The comparator calls ops.ce_kd_blend never."""
    from ocl_amd import ops
    cfg = LWF_CASE
    ops.set_deterministic(True)
    try:
        _, model_a, opt_a, a = _build_agent(cfg)
        _, model_b, opt_b, b = _build_agent(cfg)
        b._force_autograd = True
        calls = _spy_blend(monkeypatch)
        tasks, _ = make_stream(cfg)
        st = _rng_get()
        a.train_learner(*tasks[0])
        assert len(calls) == 6
        _rng_set(st)
        b.train_learner(*tasks[0])
        assert len(calls) == 6, "the comparator called the fused kernel"
        model_b.load_state_dict(model_a.state_dict())
        b.kd_manager.teacher_model.copy_(a.kd_manager.teacher_model)
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
        assert len(calls) == 12 and len(pre) == len(post) == len(got) == 6 and all(c.teacher is not None for c in calls[6:])
        names = [n for n, _ in model_a.named_parameters()]
        worst = 0.0
        for k in range(6):
            wa, wb = _flat(post[k], names), _flat(got[k], names)
            diff = float(np.linalg.norm((wb - pre[k]) - (wa - pre[k])) / np.linalg.norm(wa - pre[k]))
            worst = max(worst, diff)
            print("lwf comparator step %d  update difference %.2e (allowed %.0e)" % (k, diff, COMPARATOR_BOUND))
            assert diff <= COMPARATOR_BOUND, (k, diff)
            sa, sb = _bn_stats(post[k]), _bn_stats(got[k])
            assert sa.keys() == sb.keys() and all(torch.equal(sa[n], sb[n]) for n in sa), "running statistics differ at step %d" % k
        print("lwf comparator: worst norm-wise update difference over the second task %.2e" % worst)
    finally:
        ops.set_deterministic(False)


def test_labels_trick_takes_the_autograd_path_and_learns(cuda, monkeypatch):
    """With the labels trick the criterion is the segmented cross-entropy: the agent takes the reference's statements over autograd.  No
    ce_kd_blend call; over the first task's slice the loss is finite and ends below where it began (two separable classes, the softmax
    over those two heads alone: the first loss is about log 2); the second task runs with a teacher and stays finite."""
    from ocl_amd import debug
    cfg = LWF_CASE
    for trick in (dict(labels_trick=True), dict(separated_softmax=True)):
        params, model, opt, agent = _build_agent(cfg, trick=dict(TRICK, **trick))
        assert agent._fused() is False
        calls = _spy_blend(monkeypatch)
        tasks, _ = make_stream(cfg)
        debug.LOG = []
        try:
            agent.train_learner(*tasks[0])
            first = _events(list(debug.LOG), "lwf_loss")
            agent.train_learner(*tasks[1])
            second = _events(list(debug.LOG), "lwf_loss")[len(first):]
        finally:
            debug.LOG = None
        assert not calls and len(first) == 6 and len(second) == 6
        losses = [e["loss"] for e in first]
        print("lwf %s: first-task losses %s, second-task (loss_new, loss_old) %s" % (trick, np.round(losses, 4).tolist(),
                                                                                     [(round(e["loss_new"], 3), round(e["loss_old"], 3)) for e in second]))
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        assert all(e["loss_old"] == 0.0 and e["loss"] == e["loss_new"] for e in first)
        assert all(np.isfinite([e["loss"], e["loss_new"], e["loss_old"]]).all() and e["loss_old"] > 0.0 for e in second)
        assert bool(torch.isfinite(model.flat_params()).all())
    plain = _build_agent(cfg)[3]
    assert plain._fused() is True


# ---- 7. free run against the recorded reference run -----------------------------------------------------------------------------------

def test_free_run_vs_reference_golden(cuda, monkeypatch):
    """Whole tasks, free running, against the run recorded from the REAL reference agent (tests/golden/lwf.npz): counters and task
    bookkeeping are exact; the weights follow a chaotic trajectory and get the sanity band of test_gpu_agem's free run."""
    from ocl_amd.data import setup_test_loader
    g = gold("lwf")
    cfg = LWF_CASE
    params, model, opt, agent = _build_agent(cfg)
    calls = _spy_blend(monkeypatch)
    n_steps = []
    inner = opt.step

    def step(*a, **k):
        n_steps.append(len(calls))
        return inner(*a, **k)

    opt.step = step
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    assert int(g["lwf_c10_ntasks"]) == len(tasks) == 3 and int(g["lwf_c10_steps_per_task"]) == 6
    seen = []
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        seen += cfg["tasks"][t]
        assert agent.task_seen == t + 1 and sorted(agent.old_labels) == seen and agent.new_labels == []
        assert {k: v for k, v in agent.class_task_map.items()} == {c: i for i, cs in enumerate(cfg["tasks"][:t + 1]) for c in cs}
        assert n_steps == list(range(1, 6 * (t + 1) + 1)), "one kernel call per optimiser step"
        assert [c.teacher is not None for c in calls[6 * t:]] == [t > 0] * 6
        assert all((c.w_new, c.w_old) == (1 / (t + 1), 1 - 1 / (t + 1)) for c in calls[6 * t:])
        assert torch.equal(_bits(agent.kd_manager.teacher_model), _bits(model.flat_params()))
        pre = "lwf_c10_t%d_" % t
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        first = [[float(c.loss3[1]), float(c.loss3[2])] for c in calls[6 * t:6 * t + 2]]
        print("lwf_c10", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, g[pre + "acc"], "first losses (new, old)", first,
              "recorded", g["lwf_c10_losses"][t].tolist())
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()
        assert np.isfinite(first).all() and all((lo > 0) == (t > 0) for _, lo in first)
    # the very first step starts from the seeded weights on both sides
    assert abs(float(calls[0].loss3[1]) - g["lwf_c10_losses"][0, 0, 0]) < 1e-4
