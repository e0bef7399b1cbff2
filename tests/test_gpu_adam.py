"""GPU: the fused Adam step (csrc/optim.hip adam_flat_kernel, ocl_adam_step, optim.FusedAdam) against the float64 statement of the
update rule (tests/test_cpu_adam.py ref_adam, itself pinned against torch.optim.Adam in float64).

Every step is judged on its own from the kernel's incoming p / m / v (teacher forcing) and element by element against the first-order
propagation of fp32 round-off through the formula (adam_bounds: one half-ulp, U = 2^-24, per operation); allowed: 4 x these bounds.
The factor: torch's own fp32 Adam measures about 1 (p), 1 (m) and 2 - 2.2 (v) of them on these inputs; sqrtf and '/' may each take a
whole ulp where the bounds count a half, and the products inside v' are rounded too.  torch.optim.Adam(foreach=False) runs on the GPU
on the same inputs and is judged by the same yardstick; both worst ratios are printed per case (profiles/adam_parity.txt).

The reference is evaluated at the hyper-parameters as the kernel receives them: lr, the betas, eps, weight_decay and grad_scale cross
the C-ABI as `float`, so ref_adam (and torch) get float32(lr), float32(0.9), float32(0.999) ... -- 1 - float32(0.999) differs from 0.001
by 1.3e-5 relative, a difference of the inputs, not of the arithmetic."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import build_agent, dev as _dev, host as _host
from oracle.synth import STEP_CASES, make_stream
from test_cpu_adam import ref_adam, worst_ratios, make_grads, f32

pytestmark = pytest.mark.gpu

_build_agent = functools.partial(build_agent, optimizer="Adam", learning_rate=1e-3)

FACTOR = 4.0
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
SIZES = [1, 3, 4, 1003, 4099, 1109240, 1155608]
HYPER = [(1e-3, 0.0, 1.0), (1e-3, 1e-4, 1.0), (0.1, 1e-4, 0.1), (1e-3, 5e-4, 1.0)]


# ---- 1. the kernel against ref_adam -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lr,wd,gs", HYPER)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_vs_float64_reference_teacher_forced(cuda, n, lr, wd, gs):
    from ocl_amd import ops
    rng = np.random.default_rng(1000 + n)
    p0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    p, m, v = _dev(p0, cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    tp = torch.nn.Parameter(_dev(p0, cuda))
    topt = torch.optim.Adam([tp], lr=f32(lr), betas=(B1, B2), eps=EPS, weight_decay=f32(wd), foreach=False)
    gs_dev = torch.tensor(f32(gs), dtype=torch.float32, device=cuda)
    mine, theirs = [0.0] * 3, [0.0] * 3
    for t in range(1, 13):
        g = make_grads(rng, n, t)
        gd = _dev(g, cuda)
        # the kernel, from its own incoming state
        before = (_host(p), _host(m), _host(v))
        ops.adam_step(p, gd, m, v, t, lr, (0.9, 0.999), 1e-8, wd, gs)
        r = ref_adam(before[0], g, before[1], before[2], t, f32(lr), B1, B2, EPS, f32(wd), f32(gs))
        mine = [max(a, b) for a, b in zip(mine, worst_ratios(_host(p), _host(m), _host(v), r))]
        # torch's fp32 Adam on the same device, from ITS own incoming state
        st = topt.state.get(tp, {})
        before = (_host(tp), _host(st["exp_avg"]) if st else np.zeros(n, np.float32), _host(st["exp_avg_sq"]) if st else np.zeros(n, np.float32))
        tp.grad = gd * gs_dev
        topt.step()
        st = topt.state[tp]
        r = ref_adam(before[0], g, before[1], before[2], t, f32(lr), B1, B2, EPS, f32(wd), f32(gs))
        theirs = [max(a, b) for a, b in zip(theirs, worst_ratios(_host(tp), _host(st["exp_avg"]), _host(st["exp_avg_sq"]), r))]
    print("adam parity n=%-8d lr=%-6g wd=%-6g gs=%-4g  worst |err|/bound over 12 steps  kernel p %.2f m %.2f v %.2f   torch p %.2f m %.2f v %.2f"
          % ((n, lr, wd, gs) + tuple(mine) + tuple(theirs)))
    assert max(mine) <= FACTOR, (mine, theirs)


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------------

def _state(cuda, n, seed):
    rng = np.random.default_rng(seed)
    return (_dev(0.1 * rng.standard_normal(n), cuda), _dev(make_grads(rng, n, 1), cuda), _dev(0.01 * rng.standard_normal(n), cuda),
            _dev(1e-4 * rng.random(n), cuda))


@pytest.mark.parametrize("n,skip", [(20003, (1001, 17101)), (20003, (1002, 17103)), (4099, (4097, 4099)), (4099, (0, 5)), (64, (0, 64))])
def test_skip_range_is_untouched_and_the_rest_is_not(cuda, n, skip):
    from ocl_amd import ops
    p, g, m, v = _state(cuda, n, 7)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    q, mq, vq = p.clone(), m.clone(), v.clone()
    for t in range(1, 4):
        ops.adam_step(p, g, m, v, t, 1e-3, weight_decay=1e-4, skip=skip)
        ops.adam_step(q, g, mq, vq, t, 1e-3, weight_decay=1e-4)
    b, e = skip
    for new, old, free in ((p, p0, q), (m, m0, mq), (v, v0, vq)):
        assert torch.equal(new[b:e], old[b:e]), "an element inside the skip range changed"
        assert torch.equal(new[:b], free[:b]) and torch.equal(new[e:], free[e:]), "an element outside the skip range differs from the run without one"
        assert not torch.equal(free[b:e], old[b:e])     # (the range is not trivially constant: without it these elements move)


def test_zero_gradient_fresh_state_leaves_parameters_bit_identical(cuda):
    from ocl_amd import ops
    n = 4099
    p, _, _, _ = _state(cuda, n, 9)
    p0 = p.clone()
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    ops.adam_step(p, torch.zeros(n, device=cuda), m, v, 1, 1e-3)
    assert torch.equal(p, p0) and not m.any() and not v.any()


def test_misaligned_pointer_is_refused(cuda):
    from ocl_amd import ffi
    n = 1024
    bufs = [torch.zeros(n + 4, device=cuda) for _ in range(4)]
    for bad in range(4):
        ptrs = [ffi.vp(b.data_ptr() + (4 if i == bad else 0)) for i, b in enumerate(bufs)]
        rc = ffi.lib().ocl_adam_step(*ptrs, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0, 0, ffi.stream())
        assert rc == -1 and b"aligned" in ffi.lib().ocl_last_error()
    torch.cuda.synchronize()
    assert not any(b.any() for b in bufs)


def test_two_runs_are_bit_identical(cuda):
    from ocl_amd import ops
    n = 1155608
    outs = []
    for _ in range(2):
        p, g, m, v = _state(cuda, n, 11)
        for t in range(1, 4):
            ops.adam_step(p, g, m, v, t, 1e-3, weight_decay=1e-4, grad_scale=0.1, skip=(1001, 17101))
        outs.append((p, m, v))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 3. the optimiser object ----------------------------------------------------------------------------------------------------------

def _model(cuda, kind="ER"):
    from ocl_amd.setup_elements import setup_architecture
    torch.manual_seed(2)
    m = setup_architecture(SimpleNamespace(agent=kind, data="cifar10" if kind == "ER" else "cifar100", head="mlp")).to(cuda)
    m.train()
    return m


def _fake_backward(model, g):
    """What a backward leaves behind, without running one: gradients in the flat array, 'not fresh'."""
    model.flat_grads().copy_(g)
    model._grads_fresh = False


def test_state_dict_continues_bit_identically(cuda):
    from ocl_amd.optim import FusedAdam
    a_model = _model(cuda)
    a = FusedAdam(a_model, lr=1e-3, weight_decay=1e-4)
    n = a_model.flat_params().numel()
    rng = np.random.default_rng(4)
    grads = [_dev(make_grads(rng, n, t), cuda) for t in range(1, 6)]
    for g in grads[:3]:
        a.zero_grad()
        _fake_backward(a_model, g)
        a.step()
    assert a.step_count == 3
    b_model = _model(cuda)
    b_model.flat_params().copy_(a_model.flat_params())
    b = FusedAdam(b_model, lr=0.5)
    sd = a.state_dict()
    b.load_state_dict(sd)
    assert b.step_count == 3 and b.param_groups[0]["lr"] == 1e-3 and b.param_groups[0]["weight_decay"] == 1e-4
    assert b.exp_avg.data_ptr() != a.exp_avg.data_ptr() and sd["exp_avg"].data_ptr() != a.exp_avg.data_ptr()
    for g in grads[3:]:
        for opt, mod in ((a, a_model), (b, b_model)):
            opt.zero_grad()
            _fake_backward(mod, g)
            opt.step()
    assert a.step_count == b.step_count == 5
    assert torch.equal(a_model.flat_params(), b_model.flat_params())
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert not torch.equal(a.exp_avg, sd["exp_avg"])     # (the dictionary holds copies, not the live arrays)


def test_step_after_zero_grad_does_nothing_and_lr_is_read_every_step(cuda):
    from ocl_amd.optim import FusedAdam
    model = _model(cuda)
    opt = FusedAdam(model, lr=1e-3)
    n = model.flat_params().numel()
    g = _dev(make_grads(np.random.default_rng(6), n, 1), cuda)
    p0 = model.flat_params().clone()
    opt.zero_grad()
    opt.step()
    assert opt.step_count == 0 and opt.exp_avg is None and torch.equal(model.flat_params(), p0)
    _fake_backward(model, g)
    model._weights_dirty = False
    opt.step()
    assert opt.step_count == 1 and model._weights_dirty, "a counted step reports its write to the engine"
    p1, m1, v1 = model.flat_params().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    opt.zero_grad()
    opt.step()
    assert opt.step_count == 1 and torch.equal(model.flat_params(), p1) and torch.equal(opt.exp_avg, m1) and torch.equal(opt.exp_avg_sq, v1)
    # the same second step at two learning rates: the parameter change scales with it
    _fake_backward(model, g)
    opt.step()
    d_small = (model.flat_params() - p1).double()
    model.flat_params().copy_(p1)
    opt.exp_avg.copy_(m1)
    opt.exp_avg_sq.copy_(v1)
    opt.step_count = 1
    opt.param_groups[0]["lr"] = 1e-2
    _fake_backward(model, g)
    opt.step()
    d_large = (model.flat_params() - p1).double()
    r = ref_adam(_host(p1), _host(g), _host(m1), _host(v1), 2, f32(1e-2), B1, B2, EPS)
    assert max(worst_ratios(_host(model.flat_params()), _host(opt.exp_avg), _host(opt.exp_avg_sq), r)) <= FACTOR
    ratio = float(d_large.abs().sum() / d_small.abs().sum())
    assert 9.5 < ratio < 10.5, ratio


# ---- 4. through the agents ------------------------------------------------------------------------------------------------------------


def _record_steps(opt):
    """Wraps opt.step: per call, flat p / g / m / v and the step count before, p / m / v and the count after, and the grad_scale."""
    calls = []
    inner = opt.step

    def snap():
        z = np.zeros(opt.model.flat_params().numel(), np.float32)
        return (_host(opt.model.flat_params()).copy(), _host(opt.model.flat_grads()).copy(),
                _host(opt.exp_avg).copy() if opt.exp_avg is not None else z, _host(opt.exp_avg_sq).copy() if opt.exp_avg_sq is not None else z)

    def step(closure=None, grad_scale=1.0):
        fresh, count = opt.model._grads_fresh, opt.step_count
        before = snap()
        inner(closure, grad_scale=grad_scale)
        calls.append(SimpleNamespace(fresh=fresh, count_before=count, count_after=opt.step_count, before=before, after=snap(), gs=grad_scale))

    opt.step = step
    return calls


def _judge(call, lr, wd, skip=(0, 0)):
    p0, g, m0, v0 = call.before
    r = ref_adam(p0, g, m0, v0, call.count_after, f32(lr), B1, B2, EPS, f32(wd), f32(call.gs), skip)
    p1, _, m1, v1 = call.after
    return worst_ratios(p1, m1, v1, r)


def _task(cfg, n_train):
    tasks, _ = make_stream(dict(cfg, n_train=n_train))
    return tasks[0]


def _review_step(agent, x, y):
    """One backward on a fixed batch, then the review trick's scaled step (agents/base.py: gradients / 10)."""
    from ocl_amd.loss import unit_gradient
    xb = (torch.from_numpy(x[:10]).cuda().permute(0, 3, 1, 2).float() / 255).contiguous()
    yb = torch.from_numpy(y[:10]).cuda()
    agent.model.train()
    if agent.params.agent == "SCR":
        loss = agent.criterion_views(agent.model.forward_views([xb, xb]), yb, 2)
    else:
        loss = agent.criterion(agent.model.forward(xb), yb)
    agent.opt.zero_grad()
    loss.backward(unit_gradient(loss))
    agent._step_scaled(0.1)


def test_er_agent_steps_are_adam_steps(cuda):
    from ocl_amd.optim import FusedAdam
    cfg = STEP_CASES["er_c10"]
    params, model, opt, agent = _build_agent(cfg, mem_size=50)
    assert type(opt) is FusedAdam
    calls = _record_steps(opt)
    x, y = _task(cfg, 30)      # 60 images: 6 iterations of 10
    agent.train_learner(x, y)
    assert len(calls) == 6 and [c.count_after for c in calls] == [1, 2, 3, 4, 5, 6] and not any(c.fresh for c in calls)
    assert opt._skip_range() == (0, 0)
    for c in calls:
        ratios = _judge(c, 1e-3, 0.0)
        print("ER   step %d  worst |err|/bound  p %.2f m %.2f v %.2f" % ((c.count_after,) + tuple(ratios)))
        assert max(ratios) <= FACTOR, ratios
        assert not np.array_equal(c.before[0], c.after[0])
    _review_step(agent, x, y)
    c = calls[-1]
    assert len(calls) == 7 and c.count_after == 7 and c.gs == 0.1
    ratios = _judge(c, 1e-3, 0.0)
    print("ER   review-trick step (grad_scale 0.1)  p %.2f m %.2f v %.2f" % tuple(ratios))
    assert max(ratios) <= FACTOR, ratios


def test_scr_agent_steps_are_adam_steps_and_the_unused_classifier_stays(cuda):
    cfg = STEP_CASES["scr_c100"]
    params, model, opt, agent = _build_agent(cfg, mem_size=200, weight_decay=1e-4)
    unused = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith("encoder.linear.")}
    assert sorted(unused) == ["encoder.linear.bias", "encoder.linear.weight"]
    calls = _record_steps(opt)
    x, y = _task(cfg, 30)      # 6 iterations; the first finds the memory empty and trains nothing (agents/scr.py:49)
    agent.train_learner(x, y)
    assert len(calls) == 5 and [c.count_after for c in calls] == [1, 2, 3, 4, 5] and not any(c.fresh for c in calls)
    b, e = opt._skip_range()
    named = dict(model.named_parameters())
    flat = model.flat_params()
    assert e - b == 160 * 100 + 100
    assert named["encoder.linear.weight"].data_ptr() == flat.data_ptr() + 4 * b
    assert named["encoder.linear.bias"].data_ptr() + 4 * 100 == flat.data_ptr() + 4 * e
    for c in calls:
        ratios = _judge(c, 1e-3, 1e-4, (b, e))
        print("SCR  step %d  worst |err|/bound  p %.2f m %.2f v %.2f" % ((c.count_after,) + tuple(ratios)))
        assert max(ratios) <= FACTOR, ratios
        assert not c.before[1][b:e].any(), "encoder.linear.* received a gradient"
    _review_step(agent, x, y)
    c = calls[-1]
    assert len(calls) == 6 and c.count_after == 6 and c.gs == 0.1
    ratios = _judge(c, 1e-3, 1e-4, (b, e))
    print("SCR  review-trick step (grad_scale 0.1)  p %.2f m %.2f v %.2f" % tuple(ratios))
    assert max(ratios) <= FACTOR, ratios
    for n, old in unused.items():
        assert torch.equal(named[n].detach(), old), "%s changed (weight decay 1e-4 must not reach a parameter without a gradient)" % n
    assert not opt.exp_avg[b:e].any() and not opt.exp_avg_sq[b:e].any()


def test_er_with_adam_learns_a_fixed_batch(cuda):
    """Sanity only: the cross-entropy of a fixed batch is lower after 30 ER iterations with Adam than before."""
    from ocl_amd import ops
    import torch.nn.functional as F
    cfg = STEP_CASES["er_c10"]
    ops.set_deterministic(True)
    try:
        params, model, opt, agent = _build_agent(cfg, mem_size=50)
        x, y = _task(cfg, 150)      # 300 images: 30 iterations
        pick = np.r_[0:10, 150:160]
        xb = (torch.from_numpy(x[pick]).cuda().permute(0, 3, 1, 2).float() / 255).contiguous()
        yb = torch.from_numpy(y[pick]).cuda()

        def ce():
            model.train()
            with torch.no_grad():
                return float(F.cross_entropy(model.forward(xb), yb))

        before = ce()
        agent.train_learner(x, y)
        after = ce()
        print("ER + Adam, fixed batch CE: %.4f -> %.4f after %d steps" % (before, after, opt.step_count))
        assert opt.step_count == 30 and np.isfinite(after) and after < before, (before, after)
    finally:
        ops.set_deterministic(False)
