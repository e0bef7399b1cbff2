"""GPU: the fused global-norm gradient clip (csrc/clip.hip, ocl_clip_grad_norm, ops.clip_grad_norm_), the device-resident greedy
class-balanced memory (gdumb_memory.py) and the GDumb agent built on them (agents/gdumb.py), against the float64 statement of the clip
and the restatement of the reference's agent (tests/gdumb_ref.py, both pinned on the CPU by tests/test_cpu_gdumb.py).

The kernel is judged element by element against 1 x clip_bound, the first-order fp32 round-off of the clip (one half-ulp for the
coefficient rounded to float, one for the product, plus the double accumulation).  Observed values: profiles/gdumb_parity.txt."""
import functools
import gc
import random
import weakref
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (build_agent, make_params, dev as _dev, host as _host, bits as _bits, rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from conftest import gold
from oracle.synth import make_stream, seed_all, digest_state
from test_cpu_adam import make_grads
import gdumb_ref
from gdumb_ref import ref_clip, worst_ratio, max_norm_for, GDUMB_CASE, BALANCER_CASES

pytestmark = pytest.mark.gpu

_rng_get = functools.partial(rng_get, python=True)      # the balancer draws from Python's `random`
_params = functools.partial(make_params, extra=gdumb_ref.gdumb_params)
_build_agent = functools.partial(build_agent, extra=gdumb_ref.gdumb_params)

SIZES = [1, 3, 4, 5, 1003, 4099, 1094750, 1109240]


# ---- 1. the kernel against ref_clip ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [0.5, 1.5, 100.0])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_vs_float64_reference(cuda, n, ratio):
    from ocl_amd import ops
    rng = np.random.default_rng(2000 + n)
    g = make_grads(rng, n, 1)
    max_norm = max_norm_for(g, ratio)
    ref = ref_clip(g, max_norm)
    assert ref.clipped == (ratio > 1)
    gd = _dev(g, cuda)
    info = torch.full((4,), -7.0, device=cuda)
    total = ops.clip_grad_norm_(gd, max_norm, info=info)
    err = worst_ratio(_host(gd), ref)
    got = _host(info)
    print("clip parity n=%-8d total/max_norm=%-5g clipped=%d  worst |err|/bound %.3f  coef %.9g (float64 %.9g)  total %.9g (float64 %.9g)"
          % (n, ratio, ref.clipped, err, got[1], ref.coef, got[0], ref.total))
    assert err <= 1.0, err
    # the kernel adds in another order than numpy: the double differs by a few 1e-16 relative, which can cross a float rounding boundary
    want = np.array([ref.total, ref.coef, 1.0 if ref.clipped else 0.0, ref.sumsq]).astype(np.float32)
    assert np.all(np.abs(got[[0, 1, 3]] - want[[0, 1, 3]]) <= np.spacing(np.abs(want[[0, 1, 3]]))), (got, want)      # one float ulp
    assert got[2] == want[2] and (ref.clipped or got[1] == 1.0), (got, want)                                          # the decision: exact
    assert total.shape == (1,) and total.data_ptr() == info.data_ptr() and float(total) == got[0]
    if not ref.clipped:
        assert np.array_equal(_host(gd).view(np.uint32), g.view(np.uint32))


# ---- 2. exact properties --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 1003, 4099])
def test_not_clipped_array_is_left_bit_identical(cuda, n):
    from ocl_amd import ops
    g = make_grads(np.random.default_rng(31 + n), n, 1)
    gi = g.view(np.uint32).copy()
    gi[0] = 0x80000000                       # -0.0, a denormal and a negative denormal: patterns a multiply by 1.0f could still touch
    if n > 4:                                # under a flush-to-zero mode (no NaN: it would make the norm NaN)
        gi[n // 2], gi[n - 1] = 0x00000001, 0x807FFFFF
    gd = torch.from_numpy(gi.view(np.int32)).to(cuda).view(torch.float32)
    info = torch.zeros(4, device=cuda)
    ops.clip_grad_norm_(gd, 1e6, info=info)
    assert torch.equal(_bits(gd), torch.from_numpy(gi.view(np.int32)).to(cuda))
    h = _host(info)
    assert h[1] == 1.0 and h[2] == 0.0 and np.isfinite(h[0])


def test_two_clipped_runs_are_bit_identical_with_a_nan_filled_workspace(cuda):
    from ocl_amd import ops
    n = 1109240
    g = make_grads(np.random.default_rng(11), n, 1)
    max_norm = max_norm_for(g, 3.0)
    outs = []
    for _ in range(2):
        gd, info = _dev(g, cuda), torch.zeros(4, device=cuda)
        ops.clip_grad_norm_(gd, max_norm, workspace=torch.full((512,), float("nan"), dtype=torch.float64, device=cuda), info=info)
        outs.append((gd, info))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert not torch.equal(outs[0][0], _dev(g, cuda)) and _host(outs[0][1])[2] == 1.0


@pytest.mark.parametrize("n", [5, 4099])
def test_nan_inf_and_zero_cases(cuda, n):
    from ocl_amd import ops
    g = make_grads(np.random.default_rng(9), n, 1)
    info = torch.zeros(4, device=cuda)
    bad = g.copy()
    bad[n // 2] = np.nan
    gd = _dev(bad, cuda)
    total = ops.clip_grad_norm_(gd, 1.0, info=info)
    assert bool(torch.isnan(gd).all()) and bool(torch.isnan(total).all()) and np.isnan(_host(info)[0])      # a NaN norm multiplies through
    bad = g.copy()
    bad[n // 2] = np.inf
    gd = _dev(bad, cuda)
    ops.clip_grad_norm_(gd, 1.0, info=info)
    h = _host(gd)
    assert np.isnan(h[n // 2]) and not np.delete(h, n // 2).any() and np.isinf(_host(info)[0]) and _host(info)[1] == 0.0
    gd = _dev(g, cuda)
    ops.clip_grad_norm_(gd, 0.0, info=info)                  # max_norm = 0 zeroes a finite array
    assert not bool(gd.any()) and _host(info)[1] == 0.0 and _host(info)[2] == 1.0
    zeros = torch.zeros(n, device=cuda)
    ops.clip_grad_norm_(zeros, 1.0, info=info)               # coef = max_norm / 1e-6 >= 1: untouched
    assert not bool(zeros.any()) and torch.equal(_bits(zeros), torch.zeros(n, dtype=torch.int32, device=cuda))
    assert _host(info).tolist() == [0.0, 1.0, 0.0, 0.0]
    ops.clip_grad_norm_(zeros, 0.0, info=info)
    assert not bool(zeros.any()) and _host(info)[0] == 0.0


# ---- 3. refusals on the device ---------------------------------------------------------------------------------------------------------

def test_misaligned_pointers_and_a_short_workspace_are_refused_and_nothing_is_touched(cuda):
    from ocl_amd import ffi
    n = 4096
    lib = ffi.lib()
    a = torch.ones(n + 8, device=cuda)
    need = lib.ocl_clip_workspace_doubles(n)
    ws = torch.zeros(need + 1, dtype=torch.float64, device=cuda)
    info = torch.zeros(4, device=cuda)
    pa, pw = a.data_ptr(), ws.data_ptr()
    for g_ptr, w_ptr, wn, word in ((pa + 4, pw, need, b"aligned"), (pa + 8, pw, need, b"aligned"), (pa, pw + 4, need, b"aligned"),
                                   (pa, pw, need - 1, b"workspace"), (pa, pw, 0, b"workspace")):
        rc = lib.ocl_clip_grad_norm(ffi.vp(g_ptr), n, 0.5, ffi.vp(w_ptr), wn, ffi.ptr(info), ffi.stream())
        msg = lib.ocl_last_error()
        assert rc == -1 and msg.startswith(b"clip:") and word in msg, (rc, msg)
    for max_norm in (-1.0, float("nan")):
        rc = lib.ocl_clip_grad_norm(ffi.vp(pa), n, max_norm, ffi.vp(pw), need, ffi.ptr(info), ffi.stream())
        assert rc == -1 and lib.ocl_last_error().startswith(b"clip:")
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and not bool(ws.any()) and not bool(info.any())


def test_ops_wrapper_checks_its_arguments(cuda):
    from ocl_amd import ops
    g = torch.ones(8, device=cuda)
    for bad in (g.double(), g.cpu(), torch.ones(16, device=cuda)[::2]):
        with pytest.raises(RuntimeError):
            ops.clip_grad_norm_(bad, 1.0)
    with pytest.raises(RuntimeError):
        ops.clip_grad_norm_(g, 1.0, workspace=torch.zeros(2, device=cuda))
    with pytest.raises(RuntimeError):
        ops.clip_grad_norm_(g, 1.0, info=torch.zeros(3, device=cuda))
    with pytest.raises(RuntimeError):
        ops.clip_grad_norm_(g, -1.0)
    assert bool((g == 1).all())
    total = ops.clip_grad_norm_(g, 1.0)
    assert abs(float(total) - 8 ** 0.5) < 1e-6 and abs(float(g.norm()) - 1.0) < 1e-6
    ws, info = ops._clip_workspaces[(cuda.index, 8)], ops._clip_infos[cuda.index]
    total2 = ops.clip_grad_norm_(g, 1.0)
    assert ops._clip_workspaces[(cuda.index, 8)] is ws, "the default workspace is allocated once per (device, n)"
    assert ops._clip_infos[cuda.index] is info and total2.data_ptr() == info.data_ptr(), "the default info is allocated once per device"


# ---- 4. the device-resident memory ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spare", [16, 4])
@pytest.mark.parametrize("case", BALANCER_CASES, ids=lambda c: c[0])
def test_memory_follows_the_recorded_reference_update_with_one_scatter_per_batch(cuda, monkeypatch, case, spare):
    """The golden's label sequences, image k a random 3x8x8 array: after every batch the device labels and the image row sums, read in
    order()'s order, are those of the samples the reference holds.  With room for a whole batch behind the memory (spare 16) an update
    is one scatter launch; with less (spare 4) it is cut into pieces and must give the same memory."""
    from ocl_amd import ops
    from ocl_amd.gdumb_memory import GdumbMemory
    name, mem_size, seed, batches = case
    g = gold("gdumb")
    n_all = sum(len(b) for b in batches)
    imgs = np.random.default_rng(77).random((n_all, 3, 8, 8), dtype=np.float32)
    rowsum = imgs.astype(np.float64).sum(axis=(1, 2, 3))
    calls = []
    inner = ops.scatter_rows
    monkeypatch.setattr(ops, "scatter_rows", lambda dst, idx, src: (calls.append(int(idx.numel())), inner(dst, idx, src))[1])
    random.seed(seed)
    mem = GdumbMemory(mem_size, (3, 8, 8), cuda, batch=spare)
    seen = 0
    for b, ys in enumerate(batches):
        n_before = len(calls)
        slots = mem.update(_dev(imgs[seen:seen + len(ys)], cuda), np.asarray(ys, dtype=np.int64))
        seen += len(ys)
        if spare >= len(ys):
            assert len(calls) - n_before == (1 if len(slots) else 0), "an update is one scatter launch"
        order_slots, order_labels = mem.order()
        assert np.array_equal(order_labels, g["bal_%s_b%d_labels" % (name, b)])
        idx = torch.from_numpy(order_slots).to(cuda)
        assert np.array_equal(_host(mem.label[idx]), order_labels) and np.array_equal(mem.label_host[order_slots], order_labels)
        got = _host(mem.img[idx].double().sum(dim=(1, 2, 3)))
        assert np.abs(got - rowsum[g["bal_%s_b%d_items" % (name, b)]]).max() < 1e-6, "a slot holds another image than the reference's memory"
    assert mem.img.shape[0] == mem_size and mem.img.is_contiguous()


# ---- 5. the agent -----------------------------------------------------------------------------------------------------------------------

def _record_clips(monkeypatch):
    """Wraps ops.clip_grad_norm_: per call the array it was given, its contents before and after, and the info words."""
    from ocl_amd import ops
    calls = []
    inner = ops.clip_grad_norm_

    def wrapped(grads_flat, max_norm, workspace=None, info=None):
        rec = SimpleNamespace(ptr=grads_flat.data_ptr(), numel=grads_flat.numel(), before=grads_flat.clone(), max_norm=max_norm)
        out = inner(grads_flat, max_norm, workspace=workspace, info=info)
        rec.after, rec.info = grads_flat.clone(), None if info is None else _host(info).copy()
        calls.append(rec)
        return out

    monkeypatch.setattr(ops, "clip_grad_norm_", wrapped)
    return calls


def test_agent_hands_the_flat_gradients_to_the_clip_and_its_output_to_the_optimiser(cuda, monkeypatch):
    """One task: train_mem builds a fresh network (zeroed BatchNorm counters, not the constructor's model), runs
    mem_epoch * (M // batch) steps, and on every one of them the clip sees the flat gradient array and opt.step() reads -- through the
    flat array and through the p.grad views -- the clip's output bit for bit."""
    cfg = GDUMB_CASE
    params, model, opt, agent = _build_agent(cfg)
    calls = _record_clips(monkeypatch)
    steps, fresh = [], []
    inner_fresh = agent._fresh_learner

    def fresh_learner():
        m, o = inner_fresh()
        fresh.append(SimpleNamespace(model=m, opt=o, counters=[int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")]))
        inner_step = o.step

        def step(*a, **k):
            steps.append(SimpleNamespace(flat=m.flat_grads().clone(), views=torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone(),
                                         ptr=m.flat_grads().data_ptr(), n_clips=len(calls)))
            return inner_step(*a, **k)

        o.step = step
        return m, o

    agent._fresh_learner = fresh_learner
    tasks, _ = make_stream(cfg)
    w_init = model.flat_params().clone()
    agent.train_learner(*tasks[0])
    n_steps = cfg["mem_epoch"] * (50 // cfg["batch"])
    assert len(fresh) == 1 and fresh[0].model is agent.model and agent.model is not model and fresh[0].opt is agent.mem_opt is not opt
    assert fresh[0].counters and not any(fresh[0].counters), "the fresh network's BatchNorm counters are not zero"
    assert torch.equal(model.flat_params(), w_init), "the constructor's model was trained"
    assert len(steps) == len(calls) == agent.mem_steps == n_steps == 10
    kinds = set()
    for k, (s, c) in enumerate(zip(steps, calls)):
        assert s.n_clips == k + 1 and c.ptr == s.ptr and c.numel == s.flat.numel() and c.max_norm == cfg["clip"], k
        assert torch.equal(_bits(s.flat), _bits(c.after)), "opt.step() did not read the clip's output (step %d)" % k
        assert torch.equal(_bits(s.views), _bits(c.after)), "the p.grad views show other numbers (step %d)" % k
        ref = ref_clip(_host(c.before), cfg["clip"])
        assert bool(c.info[2]) == ref.clipped and worst_ratio(_host(c.after), ref) <= 1.0, k
        kinds.add(ref.clipped)
    assert kinds == {True, False}, "this task was chosen to see both kinds of step"
    assert [int(v) for k, v in agent.model.state_dict().items() if k.endswith("num_batches_tracked")] == [n_steps] * len(fresh[0].counters)


def test_a_run_of_several_tasks_does_not_accumulate_networks(cuda):
    """Every task's fresh network replaces the last one, which must be freed by reference counting alone (the cycle collector is off
    here): its engine object, flat arrays and workspace go with it."""
    cfg = dict(GDUMB_CASE, mem_epoch=1)
    params, model, opt, agent = _build_agent(cfg)
    tasks, _ = make_stream(cfg)
    refs = []
    gc.collect()
    gc.disable()
    try:
        for x, y in tasks:
            agent.train_learner(x, y)
            refs.append((weakref.ref(agent.model), weakref.ref(agent.mem_opt)))
    finally:
        gc.enable()
    assert [r() is None for r, _ in refs] == [True, True, False] and [o() is None for _, o in refs] == [True, True, False]
    assert refs[-1][0]() is agent.model


# ---- 6. co-simulation against GdumbOracle -----------------------------------------------------------------------------------------------

def test_cosim_gdumb(cuda):
    """The three tasks of gdumb_c10, one train_learner call per task on both sides from the same host RNG state; before every memory
    step the HIP model is loaded with the oracle's state at that step (teacher forcing through _mem_step).  Per step: the same
    mini-batch, loss within 1e-4, the same clip decision, the update within 1e-2 norm-wise where nothing is clipped (the bound of ER's
    and A-GEM's co-simulations) and 2e-2 where it is (a relative error eps of the gradient moves the coefficient by at most eps as
    well).  Per task: host RNG state (torch, numpy, random) equal, memory contents exact.  tests/test_cpu_gdumb.py shows that both kinds
    of step occur and that |total / clip - 1| >= 1e-2 on every one."""
    from ocl_amd import debug
    cfg = GDUMB_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = gdumb_ref.GdumbOracle(cfg)
    tasks, _ = make_stream(cfg)
    kinds = {True: [], False: []}
    worst_loss = 0.0
    inner = agent._mem_step
    for t, (x, y) in enumerate(tasks):
        st = _rng_get()
        pre = []
        oa.on_step = lambda s, bx, by: pre.append(({k: v.clone() for k, v in s.items()}, bx.clone(), by.clone()))
        n0 = len(oa.log)
        oa.train_learner(x, y)
        logs = oa.log[n0:]
        post = [_flat(p[0], oa.names) for p in pre[1:]] + [_flat(oa.state, oa.names)]
        st_o = _rng_get()
        _rng_set(st)
        done = []

        def forced(bx, by):
            k = len(done)
            state, ox, oy = pre[k]
            assert torch.equal(bx.cpu(), ox) and torch.equal(by.cpu(), oy), "memory step %d of task %d trains on another mini-batch" % (k, t)
            agent.model.load_state_dict(state)
            w0 = _flat(state, oa.names)
            debug.LOG = []
            try:
                inner(bx, by)
                ev = list(debug.LOG)
            finally:
                debug.LOG = None
            loss, clip = _events(ev, "gdumb_loss"), _events(ev, "gdumb_clip")
            assert len(loss) == len(clip) == 1
            ol = logs[k]
            assert abs(ol["ratio"] - 1) >= 1e-2, "the oracle's norm on this machine is too close to the threshold to compare decisions: %r" % (ol,)
            assert abs(loss[0]["loss"] - ol["loss"]) < 1e-4, (t, k, loss, ol)
            assert clip[0]["clipped"] == ol["clipped"], (t, k, clip[0], ol)
            dw_o, dw_m = post[k] - w0, agent.model.flat_params().double().cpu().numpy() - w0
            upd_err = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
            done.append((abs(loss[0]["loss"] - ol["loss"]), upd_err))
            kinds[ol["clipped"]].append(upd_err)
            print("gdumb cosim task %d step %2d  clipped %d  total %.6f (oracle %.6f)  coef %.6g  loss %.6f / %.6f  update err %.2e"
                  % (t, k, ol["clipped"], clip[0]["total_norm"], ol["total_norm"], clip[0]["coef"], loss[0]["loss"], ol["loss"], upd_err))
            assert upd_err <= (2e-2 if ol["clipped"] else 1e-2), (t, k, ol["clipped"], upd_err)

        agent._mem_step = forced
        agent.train_learner(x, y)
        assert len(done) == len(logs) == len(pre) == 10 and agent.task_seen == oa.task_seen == t + 1
        worst_loss = max([worst_loss] + [d[0] for d in done])
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged in task %d" % t
        # the memory, in train_mem's order
        ox, oy = oa.memory()
        slots, labels = agent.memory.order()
        assert np.array_equal(labels, oy.numpy()) and list(agent.memory.balancer.mem_c.items()) == list(oa.mem_c.items())
        idx = torch.from_numpy(slots).to(cuda)
        assert torch.equal(agent.memory.img[idx].cpu(), ox) and np.array_equal(_host(agent.memory.label[idx]), oy.numpy())
    print("gdumb cosim: %d clipped steps, worst update err %.2e; %d not clipped, worst %.2e; worst |loss difference| %.2e"
          % (len(kinds[True]), max(kinds[True]), len(kinds[False]), max(kinds[False]), worst_loss))
    assert len(kinds[True]) >= 3 and len(kinds[False]) >= 3


# ---- 7. the comparator ------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-4


def test_fused_clip_against_torch_clip_grad_norm_on_the_same_state(cuda):
    """`_force_torch_clip` runs torch.nn.utils.clip_grad_norm_ over the p.grad views.  Two agents over two tasks from the same host RNG
    state, order-independent batch sums; before every memory step the second is loaded with the state the first had there, so both take
    the same gradient to the clip: they decide alike and their updates differ by the clip's arithmetic alone (torch forms the norm and
    the coefficient in float32: a few 1e-7 relative) -- below 1e-4 norm-wise, asserted on every step with |total / clip - 1| >= 1e-2."""
    from ocl_amd import debug, ops
    cfg = GDUMB_CASE
    ops.set_deterministic(True)
    try:
        _, _, _, a = _build_agent(cfg)
        _, _, _, b = _build_agent(cfg)
        b._force_torch_clip = True
        tasks, _ = make_stream(cfg)
        seed_all(1000 + cfg["seed"])
        inner_a, inner_b = a._mem_step, b._mem_step
        worst, flags, judged = 0.0, [], 0
        for t, (x, y) in enumerate(tasks[:2]):
            rec = []

            def step_a(bx, by):
                state = {k: v.clone() for k, v in a.model.state_dict().items()}
                w0 = a.model.flat_params().double().cpu().numpy()
                debug.LOG = []
                try:
                    inner_a(bx, by)
                    ev = list(debug.LOG)
                finally:
                    debug.LOG = None
                rec.append(SimpleNamespace(state=state, w0=w0, x=bx.clone(), y=by.clone(), clip=_events(ev, "gdumb_clip")[0],
                                           dw=a.model.flat_params().double().cpu().numpy() - w0))

            done = []

            def step_b(bx, by):
                r = rec[len(done)]
                assert torch.equal(bx, r.x) and torch.equal(by, r.y)
                b.model.load_state_dict(r.state)
                debug.LOG = []
                try:
                    inner_b(bx, by)
                    ev = list(debug.LOG)
                finally:
                    debug.LOG = None
                cb = _events(ev, "gdumb_clip")[0]
                dw = b.model.flat_params().double().cpu().numpy() - r.w0
                diff = float(np.linalg.norm(r.dw - dw) / np.linalg.norm(dw))
                margin = abs(r.clip["total_norm"] / cfg["clip"] - 1)
                done.append(diff)
                print("gdumb comparator task %d step %2d  clipped %d / %d  total %.7g / %.7g  coef %.8g / %.8g  update difference %.2e"
                      % (t, len(done) - 1, r.clip["clipped"], cb["clipped"], r.clip["total_norm"], cb["total_norm"], r.clip["coef"], cb["coef"], diff))
                if margin >= 1e-2:
                    assert r.clip["clipped"] == cb["clipped"] == (r.clip["total_norm"] > cfg["clip"]), (t, r.clip, cb)
                    assert diff < COMPARATOR_BOUND, (t, len(done) - 1, diff)
                    flags.append(r.clip["clipped"])

            a._mem_step, b._mem_step = step_a, step_b
            st = _rng_get()
            a.train_learner(x, y)
            _rng_set(st)
            b.train_learner(x, y)
            assert len(rec) == len(done) == 10
            worst, judged = max([worst] + done), judged + len(done)
        print("gdumb comparator: %d steps, %d judged, worst update difference %.2e" % (judged, len(flags), worst))
        assert len(flags) >= 15 and any(flags) and not all(flags), flags
    finally:
        ops.set_deterministic(False)


# ---- 8. free run against the recorded reference run -----------------------------------------------------------------------------------

def test_free_run_vs_reference_golden(cuda):
    """Whole tasks, free running, against the run recorded from the REAL reference agent (tests/golden/gdumb.npz): everything driven by
    the host RNGs -- the memory's labels, per-class counts and images -- is exact after every task; the weights follow a chaotic
    trajectory and get the sanity band of test_gpu_agem.test_free_run_vs_reference_golden."""
    from ocl_amd.data import setup_test_loader
    g = gold("gdumb")
    cfg = GDUMB_CASE
    params, model, opt, agent = _build_agent(cfg)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        pre = "gdumb_c10_t%d_" % t
        slots, labels = agent.memory.order()
        assert np.array_equal(labels, g[pre + "mem_label"]), "memory labels differ from the reference"
        counts = np.array([[c, n] for c, n in agent.memory.balancer.mem_c.items()], dtype=np.int64)
        assert np.array_equal(counts, g[pre + "mem_counts"]), "per-class counts (or their dict order) differ from the reference"
        idx = torch.from_numpy(slots).to(cuda)
        assert np.array_equal(_host(agent.memory.label[idx]), labels), "device labels out of step with the planner"
        rs = _host(agent.memory.img[idx].double().sum(dim=(1, 2, 3)))
        assert np.abs(rs - g[pre + "mem_rowsum"]).max() < 1e-6, "memory images differ (slots or image bytes)"
        ds, gs = digest_state(agent.model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        print("gdumb_c10", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, g[pre + "acc"])
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()


def test_single_run_trains_and_evaluates_gdumb_through_the_registry(cuda):
    """run.single_run (experiment/run.py's loop: model, optimiser and agent by name, per task train_learner + evaluate) with
    --agent GDUMB: same seed, same memory and accuracies of the right shape as the free run above."""
    from ocl_amd import run
    from ocl_amd.agents.gdumb import Gdumb
    g = gold("gdumb")
    cfg = GDUMB_CASE
    tasks, tests = make_stream(cfg)
    acc, _, n_img, agent = run.single_run(_params(cfg), tasks, tests, cfg["seed"])
    assert type(agent) is Gdumb and acc.shape == (3, 3) and (acc >= 0).all() and (acc <= 1).all() and n_img == 180
    assert np.array_equal(agent.memory.order()[1], g["gdumb_c10_t2_mem_label"]) and agent.mem_steps == 30 and agent.task_seen == 3


# ---- 9. with Adam ------------------------------------------------------------------------------------------------------------------------

def test_gdumb_with_fused_adam_counts_one_step_per_memory_step_and_restarts_per_task(cuda):
    from ocl_amd.optim import FusedAdam
    cfg = dict(GDUMB_CASE, mem_epoch=1)
    params, model, opt, agent = _build_agent(cfg, optimizer="Adam", learning_rate=1e-3)
    assert type(opt) is FusedAdam
    tasks, _ = make_stream(cfg)
    counts = []
    inner = agent._mem_step

    def step(bx, by):
        out = inner(bx, by)
        counts.append(agent.mem_opt.step_count)
        return out

    agent._mem_step = step
    seen = []
    for x, y in tasks[:2]:
        agent.train_learner(x, y)
        assert type(agent.mem_opt) is FusedAdam and agent.mem_opt is not opt and all(agent.mem_opt is not o for o in seen)
        seen.append(agent.mem_opt)
        assert bool(torch.isfinite(agent.model.flat_params()).all())
    assert counts == [1, 2, 3, 4, 5] * 2, counts
    assert opt.step_count == 0, "the constructor's optimiser took a step"
