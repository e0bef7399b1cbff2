"""GPU: EWC++'s three fused kernels (csrc/ewc.hip: ocl_ewc_accumulate, ocl_ewc_fisher_ema, ocl_ewc_fisher_normalize; ops.ewc_*) and the
agent built on them (agents/ewc_pp.py), against the float64 statement of the accumulate step, the float32 statements of the moving
average and the normalisation, and the restatement of the reference's loop (tests/ewc_ref.py, all pinned on the CPU by
tests/test_cpu_ewc.py).

The accumulate step is judged element by element against 2 x accumulate_bounds, the first-order fp32 round-off of its statements: the
factor covers an fma in place of a separate product and sum (the same factor, for the same reason, as test_gpu_agem.FACTOR).  The
moving average and the normalisation are judged bit for bit.  Observed values: profiles/ewc_parity.txt."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (TRICK, build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from conftest import gold
from oracle.synth import make_stream, seed_all, digest_state, digest_nbt
from test_cpu_adam import make_grads
import ewc_ref
from ewc_ref import EWC_CASE, EWC_LOOPS_CASE, ema_f32, normalize_f32

pytestmark = pytest.mark.gpu

_build_agent = functools.partial(build_agent, extra=ewc_ref.ref_params)

FACTOR = 2.0
SIZES = [1, 3, 4, 5, 1003, 4099, 1094750, 1109240]      # the last two: the parameter counts of the two Reduced-ResNet18 models


def _same_bits(t, a):
    return np.array_equal(_host(t).view(np.uint32), np.ascontiguousarray(a, dtype=np.float32).view(np.uint32))


# ---- 1. the accumulate step against ref_accumulate ------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [0.0, 2.0, 200.0])
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_vs_float64_reference(cuda, n, scale):
    from ocl_amd import ops
    c = ewc_ref.make_case(np.random.default_rng(3000 + n), n, make_grads)
    ref = ewc_ref.ref_accumulate(c.g, c.t, c.p, c.q, c.f, scale)
    g, t, p, q, f = (_dev(a, cuda) for a in (c.g, c.t, c.p, c.q, c.f))
    pen = torch.full((1,), -7.0, device=cuda)
    out = ops.ewc_accumulate(g, t, p, q, f, scale=scale, penalty_out=pen)
    assert out is g
    rg, rt = ewc_ref.worst_ratios(_host(g), _host(t), ref)
    got, want = float(_host(pen)[0]), np.float32(ref.penalty)
    print("ewc accumulate n=%-8d scale=%-4g worst |err|/bound: g %.3f tmp %.3f   penalty %.9g (float64 %.9g)" % (n, scale, rg, rt, got, ref.penalty))
    assert rg <= FACTOR and rt <= FACTOR, (rg, rt)
    # the kernel adds in another order than numpy: the two doubles differ by a few 1e-16 relative, which can cross a float rounding boundary
    assert abs(got - want) <= np.spacing(np.abs(want)), (got, want)
    if scale == 0.0:
        assert _same_bits(g, c.g), "scale 0 changed g"
    for name, dev, host in (("p", p, c.p), ("p_prev", q, c.q), ("f_hat", f, c.f)):
        assert _same_bits(dev, host), name + " was written"


# ---- 2. the accumulate-only mode and other exact properties ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_accumulate_only_leaves_g_bit_identical_with_a_nan_in_it(cuda, n):
    from ocl_amd import ops
    c = ewc_ref.make_case(np.random.default_rng(41 + n), n, make_grads, prev=False)
    gi = c.g.view(np.uint32).copy()
    gi[n // 2] = 0x7FC12345              # a NaN with a payload
    gd = torch.from_numpy(gi.view(np.int32)).to(cuda).view(torch.float32)
    t, p = _dev(c.t, cuda), _dev(c.p, cuda)
    ws = torch.full((512,), float("nan"), dtype=torch.float64, device=cuda)
    ops.ewc_accumulate(gd, t, p, workspace=ws)
    assert np.array_equal(_host(gd).view(np.uint32), gi), "g changed"
    assert bool(torch.isnan(ws).all()), "the workspace was touched without penalty_out"
    ref = ewc_ref.ref_accumulate(gi.view(np.float32), c.t)
    got = _host(t)
    assert np.isnan(got[n // 2]) and _same_bits(p, c.p)
    keep = np.arange(n) != n // 2
    ref_k = SimpleNamespace(g=ref.g[keep], t=ref.t[keep], pg=ref.pg[keep], g1=ref.g1[keep], t1=ref.t1[keep], has_prev=False)
    if keep.any():
        rg, rt = ewc_ref.worst_ratios(ref.g[keep], got[keep], ref_k)
        print("ewc accumulate-only n=%-8d worst |err|/bound tmp %.3f" % (n, rt))
        assert rt <= FACTOR, rt


@pytest.mark.parametrize("n", [5, 4099, 1094750])
def test_scale_zero_with_prev_leaves_g_bit_identical_and_still_reports_the_penalty(cuda, n):
    from ocl_amd import ops
    c = ewc_ref.make_case(np.random.default_rng(51 + n), n, make_grads)
    gi = c.g.view(np.uint32).copy()
    gi[n // 2], gi[0] = 0x7FC12345, 0x80000000      # a NaN with a payload; a negative zero (g + 0 would make it +0)
    gd = torch.from_numpy(gi.view(np.int32)).to(cuda).view(torch.float32)
    t, p, q, f = (_dev(a, cuda) for a in (c.t, c.p, c.q, c.f))
    for pen in (None, torch.zeros(1, device=cuda)):
        ops.ewc_accumulate(gd, t, p, q, f, scale=0.0, penalty_out=pen)
        assert np.array_equal(_host(gd).view(np.uint32), gi), "g changed"
    want = np.float32(ewc_ref.ref_accumulate(c.g, c.t, c.p, c.q, c.f, 0.0).penalty)
    assert abs(float(pen[0]) - want) <= np.spacing(want) and want > 0


def test_penalty_is_zero_where_p_equals_prev_and_without_prev_and_two_runs_are_bit_identical(cuda):
    from ocl_amd import ops
    n = 1109240
    c = ewc_ref.make_case(np.random.default_rng(61), n, make_grads)
    pen = torch.full((1,), -7.0, device=cuda)
    g, t, p, f = (_dev(a, cuda) for a in (c.g, c.t, c.p, c.f))
    ops.ewc_accumulate(g, t, p, p.clone(), f, scale=200.0, penalty_out=pen)
    assert float(pen[0]) == 0.0 and _same_bits(g, c.g + np.float32(0.0))
    pen.fill_(-7.0)
    ops.ewc_accumulate(g, t, p, penalty_out=pen)
    assert float(pen[0]) == 0.0
    outs = []
    for _ in range(2):
        g, t, p, q, f = (_dev(a, cuda) for a in (c.g, c.t, c.p, c.q, c.f))
        pen = torch.zeros(1, device=cuda)
        ops.ewc_accumulate(g, t, p, q, f, scale=2.0, penalty_out=pen, workspace=torch.full((512,), float("nan"), dtype=torch.float64, device=cuda))
        outs.append((g, t, pen))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs))
    assert not _same_bits(outs[0][0], c.g) and float(outs[0][2][0]) > 0


# ---- 3. the moving average ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep,gain", [(0.1, 0.45), (0.1, 0.018), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("n", SIZES)
def test_fisher_ema_is_bit_equal_to_the_float32_statement(cuda, n, keep, gain):
    from ocl_amd import ops
    rng = np.random.default_rng(71 + n)
    r = (make_grads(rng, n, 4).astype(np.float64) ** 2).astype(np.float32)
    t = (make_grads(rng, n, 4).astype(np.float64) ** 2).astype(np.float32)
    want = ema_f32(r, t, keep, gain)
    outs = []
    for _ in range(2):
        rd, td = _dev(r, cuda), _dev(t, cuda)
        assert ops.ewc_fisher_ema(rd, td, keep, gain) is rd
        assert not bool(td.any()), "tmp is not zero afterwards"
        outs.append(rd)
    assert _same_bits(outs[0], want), "max |difference| %g" % np.abs(_host(outs[0]) - want).max()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ---- 4. the normalisation ----------------------------------------------------------------------------------------------------------------

def _normalize(cuda, r):
    from ocl_amd import ops
    rd = _dev(r, cuda)
    out = torch.full_like(rd, -7.0)
    mm = torch.full((2,), -7.0, device=cuda)
    assert ops.ewc_fisher_normalize(rd, out, minmax_out=mm) is out
    assert _same_bits(rd, r), "the running Fisher was written"
    return _host(out), _host(mm)


@pytest.mark.parametrize("n", SIZES)
def test_fisher_normalize_is_bit_equal_to_the_float32_statement(cuda, n):
    rng = np.random.default_rng(81 + n)
    r = (make_grads(rng, n, 4).astype(np.float64) ** 2).astype(np.float32)
    want, mm = normalize_f32(r)
    got, got_mm = _normalize(cuda, r)
    assert np.array_equal(got_mm, mm), (got_mm, mm)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max |difference| %g" % np.abs(got - want).max()
    if r.max() > r.min():
        assert got.min() == 0.0 and got.max() == 1.0


@pytest.mark.parametrize("n", [1, 5, 4099, 1094750])
def test_fisher_normalize_of_a_zero_a_constant_and_a_nan_holding_fisher(cuda, n):
    got, mm = _normalize(cuda, np.zeros(n, np.float32))
    assert not got.any() and not mm.any() and not np.signbit(got).any()
    got, mm = _normalize(cuda, np.full(n, 0.37, np.float32))
    assert not got.any() and (mm == np.float32(0.37)).all()
    r = (make_grads(np.random.default_rng(n), n, 1).astype(np.float64) ** 2).astype(np.float32)
    for at in sorted({0, n // 2, n - 1}):
        bad = r.copy()
        bad[at] = np.nan
        got, mm = _normalize(cuda, bad)
        assert np.isnan(got).all() and np.isnan(mm).all(), at


@pytest.mark.parametrize("n", [1003, 4099, 1094750, 1109240])
def test_fisher_normalize_finds_extremes_in_the_scalar_tail_and_in_different_blocks(cuda, n):
    """The minimum and the maximum each in turn in the last element (the scalar tail where n is no multiple of 4) with the other far
    away: the first element (block 0) or, at the model sizes, an element a later block of the 512 handles (float4 group 300 * 256)."""
    rng = np.random.default_rng(91 + n)
    base = (0.5 + rng.random(n)).astype(np.float32)
    far = 4 * 300 * 256 + 1 if n > 4 * 301 * 256 else 0
    for lo_at, hi_at in ((n - 1, far), (far, n - 1), (n - 2, n - 1)):
        r = base.copy()
        r[lo_at], r[hi_at] = 0.25, 3.0
        want, mm = normalize_f32(r)
        got, got_mm = _normalize(cuda, r)
        assert got_mm.tolist() == [0.25, 3.0] == mm.tolist(), (lo_at, hi_at, got_mm)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[lo_at] == 0.0 and got[hi_at] == 1.0


# ---- 5. refused arguments ----------------------------------------------------------------------------------------------------------------

def test_misaligned_or_overlapping_pointers_are_refused_and_nothing_is_touched(cuda):
    from ocl_amd import ffi
    n = 1024
    lib = ffi.lib()
    arrs = [torch.full((n + 8,), float(k + 1), device=cuda) for k in range(5)]
    ws = torch.zeros(lib.ocl_ewc_workspace_doubles(n) + 1, dtype=torch.float64, device=cuda)
    pen = torch.zeros(2, device=cuda)
    ptrs = [a.data_ptr() for a in arrs]
    pw = ws.data_ptr()

    def accumulate(ps, w=pw, wn=ws.numel() - 1):
        rc = lib.ocl_ewc_accumulate(*(ffi.vp(x) for x in ps), n, 2.0, ffi.vp(w), wn, ffi.ptr(pen), ffi.stream())
        return rc, lib.ocl_last_error()

    for k in range(5):
        for shift, word in ((4, b"aligned"), (8, b"aligned")):
            ps = list(ptrs)
            ps[k] += shift
            rc, msg = accumulate(ps)
            assert rc == -1 and msg.startswith(b"ewc:") and word in msg, (k, shift, rc, msg)
        for j in range(5):
            if j != k:
                for at in (ptrs[j], ptrs[j] + 16):
                    ps = list(ptrs)
                    ps[k] = at
                    rc, msg = accumulate(ps)
                    assert rc == -1 and msg.startswith(b"ewc:") and b"overlap" in msg, (k, j, rc, msg)
    rc, msg = accumulate(ptrs, w=pw + 4)
    assert rc == -1 and b"aligned" in msg
    rc, msg = accumulate(ptrs, wn=0)
    assert rc == -1 and b"workspace" in msg
    rc, msg = accumulate(ptrs[:3] + [0, ptrs[4]])
    assert rc == -1 and msg.startswith(b"ewc:")
    for r_ptr, t_ptr, word in ((ptrs[0] + 4, ptrs[1], b"aligned"), (ptrs[0], ptrs[1] + 8, b"aligned"), (ptrs[0], ptrs[0], b"overlap"), (ptrs[0], ptrs[0] + 16, b"overlap")):
        rc = lib.ocl_ewc_fisher_ema(ffi.vp(r_ptr), ffi.vp(t_ptr), n, 0.1, 0.45, ffi.stream())
        msg = lib.ocl_last_error()
        assert rc == -1 and msg.startswith(b"ewc:") and word in msg, (rc, msg)
        rc = lib.ocl_ewc_fisher_normalize(ffi.vp(r_ptr), ffi.vp(t_ptr), n, ffi.vp(pw), 2 * (ws.numel() - 1), ffi.ptr(pen), ffi.stream())
        msg = lib.ocl_last_error()
        assert rc == -1 and msg.startswith(b"ewc:") and word in msg, (rc, msg)
    rc = lib.ocl_ewc_fisher_normalize(ffi.vp(ptrs[0]), ffi.vp(ptrs[1]), n, ffi.vp(pw), 1, ffi.ptr(pen), ffi.stream())
    assert rc == -1 and b"workspace" in lib.ocl_last_error()
    torch.cuda.synchronize()
    assert all(bool((a == k + 1).all()) for k, a in enumerate(arrs)) and not bool(ws.any()) and not bool(pen.any())


def test_ops_wrappers_check_their_arguments_and_reuse_their_workspace(cuda):
    from ocl_amd import ops
    a, b, c, d, e = (torch.zeros(8, device=cuda) for _ in range(5))
    pen = torch.zeros(1, device=cuda)
    for bad in ((a, b[:4], c), (a.double(), b, c), (a, b, c.cpu()), (a, b, c, d), (a, b, c, None, e), (a, b, c, d[:4], e), (a, b, c, d, e.double())):
        with pytest.raises(RuntimeError):
            ops.ewc_accumulate(*bad)
    for kw in (dict(workspace=torch.zeros(2, device=cuda)), dict(penalty_out=torch.zeros(1, dtype=torch.float64, device=cuda)),
               dict(penalty_out=pen, workspace=torch.zeros(2, device=cuda)), dict(penalty_out=pen.cpu())):
        with pytest.raises(RuntimeError):
            ops.ewc_accumulate(a, b, c, d, e, scale=2.0, **kw)
    for bad in ((a, b[:4]), (a.double(), b), (a, b.cpu())):
        with pytest.raises(RuntimeError):
            ops.ewc_fisher_ema(*bad, 0.1, 0.45)
        with pytest.raises(RuntimeError):
            ops.ewc_fisher_normalize(*bad)
    with pytest.raises(RuntimeError):
        ops.ewc_fisher_normalize(a, b, workspace=torch.zeros(2, device=cuda))
    with pytest.raises(RuntimeError):
        ops.ewc_fisher_normalize(a, b, minmax_out=torch.zeros(1, device=cuda))
    ops._ewc_workspaces.pop((cuda.index, 8), None)
    assert ops.ewc_accumulate(a, b, c, d, e, scale=2.0) is a
    assert (cuda.index, 8) not in ops._ewc_workspaces, "no workspace is needed without penalty_out"
    ops.ewc_accumulate(a, b, c, d, e, scale=2.0, penalty_out=pen)
    ws = ops._ewc_workspaces[(cuda.index, 8)]
    ops.ewc_accumulate(a, b, c, d, e, scale=2.0, penalty_out=pen)
    assert ops.ewc_fisher_normalize(a, b) is b and ops.ewc_fisher_ema(a, b, 0.1, 0.45) is a
    assert ops._ewc_workspaces[(cuda.index, 8)] is ws, "the default workspace is allocated once per (device, n)"


# ---- 6. the agent ---------------------------------------------------------------------------------------------------------------------

def _record_ops(monkeypatch):
    """Wraps the three ops: per accumulate call its inputs as they were before and its outputs; per moving average and normalisation
    the number of accumulate calls made before it."""
    from ocl_amd import ops
    acc, ema, norm = [], [], []
    inner_acc, inner_ema, inner_norm = ops.ewc_accumulate, ops.ewc_fisher_ema, ops.ewc_fisher_normalize

    def accumulate(grads_inout, tmp_fisher_inout, params, prev_params=None, fisher_hat=None, scale=0.0, workspace=None, penalty_out=None):
        rec = SimpleNamespace(g=grads_inout.clone(), t=tmp_fisher_inout.clone(), p=params.clone(), q=None if prev_params is None else prev_params.clone(),
                              f=None if fisher_hat is None else fisher_hat.clone(), scale=scale, penalty_out=penalty_out)
        out = inner_acc(grads_inout, tmp_fisher_inout, params, prev_params, fisher_hat, scale=scale, workspace=workspace, penalty_out=penalty_out)
        rec.out, rec.out_is_g, rec.t_out = out.clone(), out is grads_inout, tmp_fisher_inout.clone()
        acc.append(rec)
        return out

    def fisher_ema(running_inout, tmp_inout, keep, gain):
        ema.append(SimpleNamespace(at=len(acc), keep=keep, gain=gain, r=running_inout.clone(), t=tmp_inout.clone()))
        return inner_ema(running_inout, tmp_inout, keep, gain)

    def fisher_normalize(running, fisher_hat_out, workspace=None, minmax_out=None):
        norm.append(SimpleNamespace(at=len(acc)))
        return inner_norm(running, fisher_hat_out, workspace=workspace, minmax_out=minmax_out)

    monkeypatch.setattr(ops, "ewc_accumulate", accumulate)
    monkeypatch.setattr(ops, "ewc_fisher_ema", fisher_ema)
    monkeypatch.setattr(ops, "ewc_fisher_normalize", fisher_normalize)
    return acc, ema, norm


@pytest.mark.parametrize("kd_trick", [False, True])
def test_agent_hands_the_right_things_to_the_kernels_and_their_output_to_the_optimiser(cuda, monkeypatch, kd_trick):
    """Two train_learner calls, three batches and then two, order-independent batch sums.  Call 1 accumulates without prev / f_hat; at
    its end prev_params is the flat parameter array and normalized_fisher the float32 statement of the agent's own running Fisher.  In
    call 2 the g that enters the kernel is the CE gradient (recomputed by a plain forward and backward on a second model holding a copy
    of the state before that step), scale is float32(2 * lambda_ * w), and what opt.step() reads -- the flat array and the p.grad views --
    is the kernel's output.  The moving average runs where the reference's counter (restarted per call) says: before the second batch."""
    from ocl_amd import ops
    from ocl_amd.loss import unit_gradient
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    cfg = dict(EWC_CASE, seed=21)
    lam, alpha, fua = cfg["lambda_"], cfg["alpha"], cfg["fisher_update_after"]
    ops.set_deterministic(True)
    try:
        params, model, opt, agent = _build_agent(cfg, trick=dict(TRICK, kd_trick=kd_trick))
        acc, ema, norm = _record_ops(monkeypatch)
        steps, states, seen_x, seen_y = [], [], [], []
        inner_step, inner_forward, inner_criterion = opt.step, model.forward, agent.criterion

        def step(*a, **k):
            steps.append(SimpleNamespace(flat=model.flat_grads().clone(), views=torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone(),
                                         n_acc=len(acc)))
            out = inner_step(*a, **k)
            states.append({k_: v.clone() for k_, v in model.state_dict().items()})
            return out

        def forward(x):
            seen_x.append(x.clone())
            return inner_forward(x)

        def criterion(logits, labels):
            seen_y.append(labels.clone())
            return inner_criterion(logits, labels)

        opt.step, model.forward, agent.criterion = step, forward, criterion
        tasks, _ = make_stream(cfg)
        (x0, y0), (x1, y1) = tasks[0], tasks[1]
        pick0, pick1 = np.r_[0:15, 30:45], np.r_[0:10, 30:40]
        assert agent.prev_params is None and not bool(agent.tmp_fisher.any())
        agent.train_learner(x0[pick0], y0[pick0])
        assert agent.task_seen == 1 and len(steps) == 3 and [s.n_acc for s in steps] == [1, 2, 3]
        assert all(c.q is None and c.f is None and c.out_is_g and torch.equal(_bits(c.out), _bits(c.g)) for c in acc)
        assert [e.at for e in ema] == [1] and [e.at for e in norm] == [3]
        assert np.float32(ema[0].keep) == np.float32(1. - alpha) and np.float32(ema[0].gain) == np.float32(1. / fua * alpha)
        assert torch.equal(_bits(agent.prev_params), _bits(model.flat_params())) and agent.prev_params.data_ptr() != model.flat_params().data_ptr()
        want, _ = normalize_f32(_host(agent.running_fisher))
        assert _same_bits(agent.normalized_fisher, want) and want.max() == 1.0
        assert _same_bits(agent.running_fisher, ema_f32(_host(ema[0].r), _host(ema[0].t), 1. - alpha, 1. / fua * alpha))
        assert torch.equal(_bits(ema[0].t), _bits(acc[0].t_out)) and not bool(acc[1].t.any()), "tmp_fisher: one step's squares, then zero"

        agent.train_learner(x1[pick1], y1[pick1])
        assert len(steps) == 5 and len(acc) == 5 and [s.n_acc for s in steps[3:]] == [4, 5]
        assert [e.at for e in ema] == [1, 4] and [e.at for e in norm] == [3, 5]
        w = 1 / 2 if kd_trick else 1.0
        for k in (3, 4):
            c = acc[k]
            assert c.out_is_g and c.penalty_out is None, "the penalty's value is not fetched outside verbose / debug runs"
            assert np.float32(c.scale) == (np.float32(2 * lam / (1 + 1)) if kd_trick else np.float32(2 * lam))
            assert torch.equal(_bits(steps[k].flat), _bits(c.out)), "opt.step() did not read the kernel's output"
            assert torch.equal(_bits(steps[k].views), _bits(c.out)), "the p.grad views show other numbers"
            ref = ewc_ref.ref_accumulate(_host(c.g), _host(c.t), _host(c.p), _host(c.q), _host(c.f), np.float32(2 * lam * w))
            rg, rt = ewc_ref.worst_ratios(_host(c.out), _host(c.t_out), ref)
            assert rg <= FACTOR and rt <= FACTOR, (k, rg, rt)
        assert torch.equal(_bits(acc[3].p), _bits(acc[3].q)), "prev_params is not the parameters the first task ended with"
        assert torch.equal(_bits(acc[3].out), _bits(acc[3].g)), "p == prev on the first step of a task: no penalty gradient"
        assert not torch.equal(_bits(acc[4].out), _bits(acc[4].g)) and torch.equal(_bits(acc[4].q), _bits(acc[3].q)) and torch.equal(_bits(acc[4].f), _bits(acc[3].f))
        assert _same_bits(acc[3].f, want), "f_hat is not the normalised Fisher of the first task"
        if not kd_trick:
            # the CE gradient, recomputed on a copy of the state before each of the two steps
            model2 = setup_architecture(params).cuda()
            opt2 = setup_opt("SGD", model2, params.learning_rate, 0)
            for k in (3, 4):
                model2.load_state_dict(states[k - 1])
                model2.train()
                loss = inner_criterion(model2.forward(seen_x[k]), seen_y[k])
                opt2.zero_grad()
                loss.backward(unit_gradient(loss))
                assert torch.equal(_bits(acc[k].g), _bits(model2.flat_grads())), "g is not the CE gradient (step %d)" % k
                assert torch.equal(_bits(acc[k].p), _bits(model2.flat_params())), "params is not the flat parameter array"
    finally:
        ops.set_deterministic(False)


# ---- 7. co-simulation against EwcOracle ------------------------------------------------------------------------------------------------

def _l1_rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).sum() / np.abs(want).sum())


def test_cosim_ewc(cuda, monkeypatch):
    """The three tasks of ewc_c10 concatenated, 9 sequential slices of 20, one train_learner call (two batches, one moving average)
    per slice; before every call the HIP model and the agent's four arrays are loaded with the oracle's (teacher forcing), between the
    two steps of a call the model is loaded with the oracle's again (the per-step bounds below are bounds for one step from the same
    state: left alone, the second step would also carry what the first step's 1e-3 does to a gradient), and both sides consume the same
    host RNG streams.  Per step: RNG state equal, CE within 1e-4 (ER's bound), the penalty within 1e-4
    relative, the update within 1e-2 norm-wise (ER's co-simulation bound).  Per call: tmp_fisher and running_fisher within
    2 eps + eps^2, eps = 1e-2, relative in the L1 norm (sum |2 g e| <= 2 |g| |e| moves the gradient's bound to its squares);
    normalized_fisher bit-equal to the float32 statement of the agent's own running Fisher."""
    from ocl_amd import debug
    cfg = EWC_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = ewc_ref.EwcOracle(cfg)
    xs, ys = ewc_ref.cosim_stream(cfg)
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
    eps = 1e-2
    fisher_bound = 2 * eps + eps * eps
    worst = dict(ce=0.0, penalty=0.0, update=0.0, tmp=0.0, running=0.0)
    positive = 0
    for it in range(9):
        x, y = xs[it * 20:(it + 1) * 20], ys[it * 20:(it + 1) * 20]
        model.load_state_dict(oa.state_dict())
        for mine, which in ((agent.tmp_fisher, "tmp"), (agent.running_fisher, "running"), (agent.normalized_fisher, "normalized")):
            mine.copy_(oa.flat(which))
        if it == 0:
            assert agent.prev_params is None and oa.flat("prev") is None
        else:
            agent.prev_params.copy_(oa.flat("prev"))
        w_before = [_flat(oa.state, oa.names)]
        st = _rng_get()
        n_log = len(oa.log)
        del ostates[:]
        # the oracle, one batch at a time (to see its weights between the two steps): the same loader draws as train_learner
        inner_ewc_step = ewc_ref.ewc_step

        def spy(state, names, *a, **k):
            out = inner_ewc_step(state, names, *a, **k)
            w_before.append(_flat(state, names))
            ostates.append({k_: v.detach().clone() for k_, v in state.items()})
            return out

        monkeypatch.setattr(ewc_ref, "ewc_step", spy)
        oa.train_learner(x, y)
        monkeypatch.setattr(ewc_ref, "ewc_step", inner_ewc_step)
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
        assert len(logs) == 2 and [e["ema"] for e in logs] == [False, True] and agent.task_seen == oa.task_seen == it + 1
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged in call %d" % it
        tags = [t for t, _ in ev if t.startswith("ewc_")]
        assert tags == ["ewc_loss", "ewc_fisher_update", "ewc_loss", "ewc_task_end"], tags
        loss = _events(ev, "ewc_loss")
        assert len(steps) == 2 and len(w_before) == 3
        for k in range(2):
            ol = logs[k]
            d_ce = abs(loss[k]["loss"] - ol["ce"])
            d_pen = abs(loss[k]["penalty"] - ol["penalty"]) / ol["penalty"] if ol["penalty"] > 0 else abs(loss[k]["penalty"])
            # the update of step k from the weights both sides held before it
            dw_o = w_before[k + 1] - w_before[k]
            dw_m = steps[k] - w_before[k]
            upd = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
            print("ewc cosim call %d step %d  ce %.6f / %.6f  penalty %.6e / %.6e (rel %.2e)  lambda*penalty %.4f  update err %.2e"
                  % (it, k, loss[k]["loss"], ol["ce"], loss[k]["penalty"], ol["penalty"], d_pen, cfg["lambda_"] * ol["penalty"], upd))
            worst["ce"], worst["penalty"], worst["update"] = max(worst["ce"], d_ce), max(worst["penalty"], d_pen), max(worst["update"], upd)
            assert d_ce < 1e-4, (it, k, loss[k], ol)
            assert d_pen <= 1e-4, (it, k, loss[k], ol)
            assert upd <= 1e-2, (it, k, upd)
            assert (ol["penalty"] > 0) == (it > 0 and k == 1) and (loss[k]["penalty"] > 0) == (ol["penalty"] > 0)
        positive += logs[1]["penalty"] > 0
        e_tmp, e_run = _l1_rel(_host(agent.tmp_fisher), oa.flat("tmp").numpy()), _l1_rel(_host(agent.running_fisher), oa.flat("running").numpy())
        worst["tmp"], worst["running"] = max(worst["tmp"], e_tmp), max(worst["running"], e_run)
        print("ewc cosim call %d  tmp_fisher L1 rel %.2e  running_fisher L1 rel %.2e (allowed %.4f)" % (it, e_tmp, e_run, fisher_bound))
        assert e_tmp <= fisher_bound and e_run <= fisher_bound, (it, e_tmp, e_run)
        want, mm = normalize_f32(_host(agent.running_fisher))
        assert _same_bits(agent.normalized_fisher, want)
        end = _events(ev, "ewc_task_end")[0]
        assert [np.float32(end["min_fisher"]), np.float32(end["max_fisher"])] == mm.tolist()
        assert torch.equal(_bits(agent.prev_params), _bits(model.flat_params()))
    print("ewc cosim: %d calls with a positive penalty; worst |ce diff| %.2e, penalty rel %.2e, update err %.2e, tmp_fisher L1 %.2e, "
          "running_fisher L1 %.2e" % (positive, worst["ce"], worst["penalty"], worst["update"], worst["tmp"], worst["running"]))
    assert positive >= 7


# ---- 8. the comparator ------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-5


def test_fused_bookkeeping_against_the_reference_statements_on_the_same_state(cuda, monkeypatch):
    """`_force_torch_bookkeeping` runs the reference's per-tensor statements over the p / p.grad views.  Two agents run the first task
    (one each way), the comparator is then loaded with the fused agent's state, and both run the second task's six steps from the same
    host RNG state under order-independent batch sums.  After every step the weights, and after the task the four arrays, agree within
    1e-5 norm-wise: the CE gradients are the same function of the weights on both sides, the moving average and the normalisation are
    the same float32 statements, so the two differ by the float32 rounding of the penalty's gradient alone."""
    from ocl_amd import ops
    cfg = EWC_CASE
    ops.set_deterministic(True)
    try:
        _, model_a, opt_a, a = _build_agent(cfg)
        _, model_b, opt_b, b = _build_agent(cfg)
        b._force_torch_bookkeeping = True
        acc, ema, norm = _record_ops(monkeypatch)        # the fused agent's alone: the comparator calls none of the three ops
        tasks, _ = make_stream(cfg)
        snaps = {id(a): [], id(b): []}
        for agent, model, opt in ((a, model_a, opt_a), (b, model_b, opt_b)):
            inner = opt.step

            def step(*args, _inner=inner, _agent=agent, _model=model, **kw):
                out = _inner(*args, **kw)
                snaps[id(_agent)].append((_model.flat_params().double().cpu().numpy(), _agent.tmp_fisher.double().cpu().numpy()))
                return out

            opt.step = step

        def rel(x, y):
            return float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300))

        def arrays(agent):
            return [t.double().cpu().numpy() for t in (agent.tmp_fisher, agent.running_fisher, agent.normalized_fisher, agent.prev_params)]

        worst = 0.0
        for t in range(2):
            if t == 1:
                model_b.load_state_dict(model_a.state_dict())
                for dst, src in zip((b.tmp_fisher, b.running_fisher, b.normalized_fisher, b.prev_params),
                                    (a.tmp_fisher, a.running_fisher, a.normalized_fisher, a.prev_params)):
                    dst.copy_(src)
            st = _rng_get()
            n_before = len(acc)
            for agent in (a, b):
                _rng_set(st)
                del snaps[id(agent)][:]
                agent.train_learner(*tasks[t])
            assert len(acc) == n_before + 6 and len(snaps[id(a)]) == len(snaps[id(b)]) == 6
            for k, ((wa, ta), (wb, tb)) in enumerate(zip(snaps[id(a)], snaps[id(b)])):
                dw, dt = rel(wa, wb), rel(ta, tb)
                print("ewc comparator task %d step %d  weights %.2e  tmp_fisher %.2e" % (t, k, dw, dt))
                if t == 1:
                    worst = max(worst, dw, dt)
                    assert dw < COMPARATOR_BOUND and dt < COMPARATOR_BOUND, (k, dw, dt)
            ds = [rel(x, y) for x, y in zip(arrays(a), arrays(b))]
            print("ewc comparator task %d end  tmp %.2e  running %.2e  normalized %.2e  prev %.2e" % ((t,) + tuple(ds)))
            if t == 1:
                worst = max([worst] + ds)
                assert max(ds) < COMPARATOR_BOUND, ds
                assert any(not torch.equal(c.out, c.g) for c in acc[n_before:]), "no step of the second task carried a penalty gradient"
        print("ewc comparator: worst norm-wise difference over the second task %.2e (allowed %.0e)" % (worst, COMPARATOR_BOUND))
    finally:
        ops.set_deterministic(False)


# ---- 9. free run against the recorded reference run -----------------------------------------------------------------------------------

def test_free_run_vs_reference_golden(cuda):
    """Whole tasks, free running, against the run recorded from the REAL reference agent (tests/golden/ewc.npz): the weights and the
    Fisher arrays follow a chaotic trajectory and get the sanity band of test_gpu_agem's free run."""
    from ocl_amd.data import setup_test_loader
    g = gold("ewc")
    cfg = EWC_CASE
    params, model, opt, agent = _build_agent(cfg)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        pre = "ewc_c10_t%d_" % t
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        lo, hi = float(agent.running_fisher.min()), float(agent.running_fisher.max())
        glo, ghi = g[pre + "minmax"]
        print("ewc_c10", t, "state digest rel err", rel, "norm ratio", ratio, "running Fisher min / max", lo, hi, "recorded", glo, ghi, "acc", acc, g[pre + "acc"])
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert 0.0 <= lo < hi and 0.5 < hi / ghi < 2.0, (lo, hi, ghi)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()
        nf = agent.normalized_fisher
        assert float(nf.min()) == 0.0 and float(nf.max()) == 1.0 and torch.equal(_bits(agent.prev_params), _bits(model.flat_params()))
        pn, gn = float(agent.prev_params.double().norm()), np.sqrt((g[pre + "prev"][:, 1] ** 2).sum())
        assert 0.5 < pn / gn < 2.0, (pn, gn)


def test_free_run_two_epochs_schedule_and_forward_counts_vs_reference_golden(cuda):
    """ewc_loops (epoch 2, three batches per epoch, fisher_update_after 2), free running with the trace on, against the reference's
    recording: the task's iterations that begin with the running Fisher's moving average (1, 3, 5: the counter of ewc_pp.py:41 runs
    across the epochs, so the second epoch updates at other i than the first) and num_batches_tracked exact; the very first step
    starts from the seeded initial weights on both sides, its cross-entropy within 1e-4 (the co-simulation's bound); the weights get
    the sanity band of the free run above."""
    from ocl_amd import debug
    from ocl_amd.data import setup_test_loader
    g = gold("ewc")
    cfg = EWC_LOOPS_CASE
    params, model, opt, agent = _build_agent(cfg)
    assert agent.epoch == 2 and agent.fisher_update_after == 2
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        acc = agent.evaluate(loaders)
        pre = "ewc_loops_t%d_" % t
        tags = [tag for tag, _ in ev if tag in ("ewc_loss", "ewc_fisher_update")]
        ema_at = [tags[:k].count("ewc_loss") for k, tag in enumerate(tags) if tag == "ewc_fisher_update"]
        assert tags.count("ewc_loss") == 6 and ema_at == g[pre + "ema_at"].tolist() == [1, 3, 5], (tags, g[pre + "ema_at"])
        assert digest_nbt(model.state_dict()).tolist() == g[pre + "nbt"].tolist(), "train-mode forward count differs from the reference"
        if t == 0:
            first = _events(ev, "ewc_loss")[0]
            assert abs(first["loss"] - g["ewc_loops_ce"][0]) < 1e-4 and first["penalty"] == 0.0, (first, g["ewc_loops_ce"][0])
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        hi, ghi = float(agent.running_fisher.max()), g[pre + "minmax"][1]
        print("ewc_loops", t, "updates at", ema_at, "state digest rel err", rel, "norm ratio", ratio, "running Fisher max", hi, "recorded", ghi, "acc", acc)
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert 0.5 < hi / ghi < 2.0, (hi, ghi)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()


# ---- 10. with Adam ----------------------------------------------------------------------------------------------------------------------

def test_ewc_with_fused_adam_counts_one_step_per_iteration(cuda, monkeypatch):
    from ocl_amd.optim import FusedAdam
    cfg = dict(EWC_CASE, n_train=15)        # 30 images per task: 3 iterations
    params, model, opt, agent = _build_agent(cfg, optimizer="Adam", learning_rate=1e-3)
    assert type(opt) is FusedAdam
    acc, ema, norm = _record_ops(monkeypatch)
    tasks, _ = make_stream(cfg)
    counts = []
    inner = opt.step

    def step(*a, **k):
        out = inner(*a, **k)
        counts.append((opt.step_count, len(acc)))
        return out

    opt.step = step
    w0 = model.flat_params().clone()
    agent.train_learner(*tasks[0])
    agent.train_learner(*tasks[1])
    assert counts == [(k, k) for k in range(1, 7)], counts
    assert [c.q is None for c in acc] == [True] * 3 + [False] * 3 and [e.at for e in ema] == [1, 4] and [e.at for e in norm] == [3, 6]
    assert bool(torch.isfinite(model.flat_params()).all()) and not torch.equal(model.flat_params(), w0)
