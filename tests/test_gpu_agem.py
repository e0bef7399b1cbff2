"""GPU: A-GEM's fused gradient projection (csrc/gradproj.hip, ocl_agem_project, ops.agem_project) and the agent built on it
(agents/agem.py), against the float64 statement of the projection and the restatement of the reference's iteration (tests/agem_ref.py,
both pinned on the CPU by tests/test_cpu_agem.py).

The kernel is judged element by element against 2 x project_bound, the first-order fp32 round-off of the projection (one half-ulp for
the coefficient rounded to float, the product and the subtraction, plus the double accumulation): the factor covers an fma in place of
the separate product and subtraction, and a whole-ulp float division.  Observed values: profiles/agem_parity.txt."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (build_agent as _build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from conftest import gold
from oracle.synth import make_stream, seed_all, digest_state, digest_nbt, class_images
from test_cpu_adam import make_grads
import agem_ref
from agem_ref import ref_project, worst_ratio, with_cosine, AGEM_CASE, AGEM_LOOPS_CASE

pytestmark = pytest.mark.gpu

FACTOR = 2.0
SIZES = [1, 3, 4, 5, 1003, 4099, 1094750, 1109240]


# ---- 1. the kernel against ref_project -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cos", [-0.1, -1e-3, 0.1])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_vs_float64_reference(cuda, n, cos):
    from ocl_amd import ops
    rng = np.random.default_rng(2000 + n)
    r = make_grads(rng, n, 1)
    g = with_cosine(rng, r, cos)
    ref = ref_project(g, r)
    assert ref.projected == (cos < 0)
    gd, rd = _dev(g, cuda), _dev(r, cuda)
    info = torch.full((4,), -7.0, device=cuda)
    out = ops.agem_project(gd, rd, info=info)
    assert out is rd
    ratio = worst_ratio(_host(rd), ref)
    got = _host(info)
    print("agem parity n=%-8d cos=%-6g projected=%d  worst |err|/bound %.3f  coef %.9g (float64 %.9g)" % (n, cos, ref.projected, ratio, got[2], ref.coef))
    assert ratio <= FACTOR, ratio
    # the kernel adds in another order than numpy: the two doubles differ by a few 1e-16 relative, which can cross a float rounding boundary
    want = np.array([ref.prod, ref.prod_ref, ref.coef if ref.projected else 0.0, 1.0 if ref.projected else 0.0]).astype(np.float32)
    assert np.all(np.abs(got[:3] - want[:3]) <= np.spacing(np.abs(want[:3]))), (got, want)      # one float ulp
    assert got[3] == want[3] and (ref.projected or got[2] == 0.0), (got, want)                  # the decision and the zero field: exact
    assert np.array_equal(_host(gd), g), "g was written"


# ---- 2. exact properties --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 1003, 4099])
def test_not_projected_output_is_a_bit_copy_of_g_with_a_nan_in_it(cuda, n):
    from ocl_amd import ops
    rng = np.random.default_rng(31 + n)
    r = make_grads(rng, n, 1)
    g = with_cosine(rng, r, -0.5)        # would be projected ...
    gi = g.view(np.uint32).copy()
    gi[n // 2] = 0x7FC12345              # ... but for one NaN (with a payload): prod is NaN, and NaN < 0 is false
    gd = torch.from_numpy(gi.view(np.int32)).to(cuda).view(torch.float32)
    rd = _dev(r, cuda)
    info = torch.zeros(4, device=cuda)
    ops.agem_project(gd, rd, info=info)
    assert torch.equal(_bits(rd), torch.from_numpy(gi.view(np.int32)).to(cuda))
    h = _host(info)
    assert np.isnan(h[0]) and h[2] == 0.0 and h[3] == 0.0


def test_orthogonal_supports_and_zero_reference_give_a_copy(cuda):
    from ocl_amd import ops
    n = 4099
    rng = np.random.default_rng(8)
    g, r = make_grads(rng, n, 1), make_grads(rng, n, 1)
    g[::2], r[1::2] = 0.0, 0.0
    info = torch.full((4,), -7.0, device=cuda)
    for ref_vec in (r, np.zeros(n, np.float32)):
        gd, rd = _dev(g, cuda), _dev(ref_vec, cuda)
        ops.agem_project(gd, rd, info=info)
        assert torch.equal(_bits(rd), _bits(gd)) and bool(torch.isfinite(rd).all())
        h = _host(info)
        assert h[0] == 0.0 and h[2] == 0.0 and h[3] == 0.0 and h[1] == np.float32((ref_vec.astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("n", [5, 4099, 1109240])
def test_opposite_gradient_projects_to_exact_zero(cuda, n):
    from ocl_amd import ops
    r = make_grads(np.random.default_rng(9), n, 1)
    rd = _dev(r, cuda)
    info = torch.zeros(4, device=cuda)
    ops.agem_project(_dev(-r, cuda), rd, info=info)
    assert not bool(rd.any())
    h = _host(info)
    assert h[2] == -1.0 and h[3] == 1.0 and h[0] == -h[1]


def test_two_runs_are_bit_identical_and_g_is_never_written(cuda):
    from ocl_amd import ops
    n = 1109240
    rng = np.random.default_rng(11)
    r = make_grads(rng, n, 1)
    g = with_cosine(rng, r, -0.1)
    outs = []
    for _ in range(2):
        gd, rd, info = _dev(g, cuda), _dev(r, cuda), torch.zeros(4, device=cuda)
        ops.agem_project(gd, rd, workspace=torch.full((1024,), float("nan"), dtype=torch.float64, device=cuda), info=info)
        assert torch.equal(_bits(gd), _bits(_dev(g, cuda))), "g was written"
        outs.append((rd, info))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert not torch.equal(outs[0][0], _dev(g, cuda)) and _host(outs[0][1])[3] == 1.0


def test_misaligned_or_overlapping_pointers_are_refused_and_nothing_is_touched(cuda):
    from ocl_amd import ffi
    n = 1024
    lib = ffi.lib()
    a, b = torch.ones(n + 8, device=cuda), torch.full((n + 8,), 2.0, device=cuda)
    ws = torch.zeros(lib.ocl_agem_workspace_doubles(n) + 1, dtype=torch.float64, device=cuda)
    info = torch.zeros(4, device=cuda)
    pa, pb, pw = a.data_ptr(), b.data_ptr(), ws.data_ptr()
    for g_ptr, r_ptr, w_ptr, word in ((pa + 4, pb, pw, b"aligned"), (pa, pb + 4, pw, b"aligned"), (pa, pb + 8, pw, b"aligned"),
                                      (pa, pb, pw + 4, b"aligned"), (pa, pa, pw, b"overlap"), (pa, pa + 16, pw, b"overlap"),
                                      (pa + 16, pa, pw, b"overlap")):
        rc = lib.ocl_agem_project(ffi.vp(g_ptr), ffi.vp(r_ptr), n, ffi.vp(w_ptr), ws.numel() - 1, ffi.ptr(info), ffi.stream())
        msg = lib.ocl_last_error()
        assert rc == -1 and msg.startswith(b"agem:") and word in msg, (rc, msg)
    rc = lib.ocl_agem_project(ffi.vp(pa), ffi.vp(pb), n, ffi.vp(pw), 1, ffi.ptr(info), ffi.stream())
    assert rc == -1 and b"workspace" in lib.ocl_last_error()
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and bool((b == 2).all()) and not bool(ws.any()) and not bool(info.any())


def test_ops_wrapper_checks_its_arguments(cuda):
    from ocl_amd import ops
    g, r = torch.zeros(8, device=cuda), torch.zeros(8, device=cuda)
    for bad in ((g, r[:4]), (g.double(), r), (g, r.cpu())):
        with pytest.raises(RuntimeError):
            ops.agem_project(*bad)
    with pytest.raises(RuntimeError):
        ops.agem_project(g, r, workspace=torch.zeros(2, device=cuda))
    with pytest.raises(RuntimeError):
        ops.agem_project(g, r, info=torch.zeros(3, device=cuda))
    assert ops.agem_project(g, r) is r
    ws = ops._agem_workspaces[(cuda.index, 8)]
    ops.agem_project(g, r)
    assert ops._agem_workspaces[(cuda.index, 8)] is ws, "the default workspace is allocated once per (device, n)"


# ---- 3. the agent ---------------------------------------------------------------------------------------------------------------------

def _prefill(agent, cls, n_fill, seed):
    """n_fill images of one class in the first slots of the replay memory, as if n_fill stream items had been seen."""
    xs = class_images(cls, n_fill, (32, 32), np.random.default_rng(seed))
    b = agent.buffer
    b.buffer_img[:n_fill] = (torch.from_numpy(xs).permute(0, 3, 1, 2).float() / 255).to(b.buffer_img.device)
    b.buffer_label[:n_fill] = cls
    b.label_host[:n_fill] = cls
    b.current_index, b.n_seen_so_far = n_fill, n_fill


def _record_projections(monkeypatch):
    """Wraps ops.agem_project: per call the two inputs and the info words as they were before, and the output."""
    from ocl_amd import ops
    calls = []
    inner = ops.agem_project

    def wrapped(g, g_ref_inout, workspace=None, info=None):
        rec = SimpleNamespace(g=g.clone(), g_ref=g_ref_inout.clone())
        out = inner(g, g_ref_inout, workspace=workspace, info=info)
        rec.out, rec.out_is_ref, rec.info = out.clone(), out is g_ref_inout, None if info is None else _host(info).copy()
        calls.append(rec)
        return out

    monkeypatch.setattr(ops, "agem_project", wrapped)
    return calls


def test_agent_hands_the_batch_and_memory_gradients_to_the_kernel_and_its_output_to_the_optimiser(cuda, monkeypatch):
    """Two train_learner calls of one batch each: a batch of class 2 against a memory that is mostly class 0.  The first (task_seen == 0) must not
    project; in the second, g is the batch gradient and g_ref the memory gradient (recomputed by a plain forward and backward on a
    second model holding a copy of the state, bit for bit under order-independent batch sums), and what opt.step() reads -- the flat
    array and the p.grad views -- is the projection's output."""
    from ocl_amd import ops
    from ocl_amd.loss import unit_gradient
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    cfg = dict(AGEM_CASE, seed=21)
    ops.set_deterministic(True)
    try:
        params, model, opt, agent = _build_agent(cfg)
        _prefill(agent, 0, 40, 5)
        calls = _record_projections(monkeypatch)
        steps, seen_x, seen_y = [], [], []
        inner_step, inner_forward, inner_criterion = opt.step, model.forward, agent.criterion

        def step(*a, **k):
            steps.append(SimpleNamespace(flat=model.flat_grads().clone(), views=torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone(),
                                         n_proj=len(calls)))
            return inner_step(*a, **k)

        def forward(x):
            seen_x.append(x.clone())
            return inner_forward(x)

        def criterion(logits, labels):
            seen_y.append(labels.clone())
            return inner_criterion(logits, labels)

        opt.step, model.forward, agent.criterion = step, forward, criterion
        x = class_images(2, 20, (32, 32), np.random.default_rng(6))
        y = np.full(20, 2, dtype=np.int64)
        agent.train_learner(x[:10], y[:10])
        assert agent.task_seen == 1 and len(steps) == 1 and len(calls) == 0 and len(seen_x) == len(seen_y) == 1, "a projection while task_seen == 0"
        state = {k: v.clone() for k, v in model.state_dict().items()}
        agent.train_learner(x[10:], y[10:])
        assert len(steps) == 2 and len(calls) == 1 and steps[1].n_proj == 1 and len(seen_x) == len(seen_y) == 3
        assert seen_y[1].tolist() == [2] * 10 and seen_y[2].tolist().count(0) >= 5      # the batch; the memory rows, mostly the other class
        c = calls[0]
        assert c.out_is_ref and c.info[3] == 1.0, "this step was built to project (prod %g)" % c.info[0]
        # the two gradients, recomputed on a copy of the state
        model2 = setup_architecture(params).cuda()
        model2.load_state_dict(state)
        model2.train()
        opt2 = setup_opt("SGD", model2, 0.1, 0)
        grads = []
        for xb, yb in zip(seen_x[1:], seen_y[1:]):
            loss = inner_criterion(model2.forward(xb), yb)
            opt2.zero_grad()
            loss.backward(unit_gradient(loss))
            grads.append(model2.flat_grads().clone())
        assert seen_x[2].size(0) == 10
        assert torch.equal(c.g, grads[0]), "g is not the batch gradient"
        assert torch.equal(c.g_ref, grads[1]), "g_ref is not the memory gradient"
        assert not torch.equal(grads[0], grads[1])
        # the projection itself, and what the optimiser read
        ref = ref_project(_host(c.g), _host(c.g_ref))
        assert ref.projected and worst_ratio(_host(c.out), ref) <= FACTOR
        assert torch.equal(_bits(steps[1].flat), _bits(c.out)), "opt.step() did not read the projection's output"
        assert torch.equal(_bits(steps[1].views), _bits(c.out)), "the p.grad views show other numbers"
    finally:
        ops.set_deterministic(False)


# ---- 4. co-simulation against agem_step ------------------------------------------------------------------------------------------------

def _buffers_equal(agent, oa):
    return (np.array_equal(agent.buffer.buffer_label.cpu().numpy(), oa.buf.label.numpy()) and torch.equal(agent.buffer.buffer_img.cpu(), oa.buf.img)
            and np.array_equal(agent.buffer.label_host, oa.buf.label.numpy())
            and [agent.buffer.current_index, agent.buffer.n_seen_so_far] == [oa.buf.current_index, oa.buf.n_seen_so_far])


def test_cosim_agem(cuda):
    """The three tasks of agem_c10 concatenated, 18 sequential slices of 10, one train_learner call per slice; before every call the HIP
    model is loaded with the oracle's state (teacher forcing) and both sides consume the same host RNG streams.  Per step: RNG state,
    retrieved indices, reservoir slots and buffers exact, both losses within 1e-4, the same decision, and the update within 1e-2
    norm-wise without projection (the bound of ER's co-simulation) and 3e-2 with it (two gradients and the coefficient each carry the
    per-gradient error).  tests/test_cpu_agem.py shows that both kinds of step occur and that |cos| >= 1e-3 on every one."""
    from ocl_amd import debug
    cfg = AGEM_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = agem_ref.AgemOracle(cfg)
    xs, ys = agem_ref.cosim_stream(cfg)
    seed_all(1000 + cfg["seed"])
    kinds = {True: [], False: []}
    for it in range(18):
        x, y = xs[it * 10:(it + 1) * 10], ys[it * 10:(it + 1) * 10]
        model.load_state_dict(oa.state_dict())
        w0 = _flat(oa.state, oa.names)
        st = _rng_get()
        oa.train_learner(x, y)
        ol = oa.log[-1]
        st_o = _rng_get()
        _rng_set(st)
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        assert len(oa.log) == it + 1 and agent.task_seen == oa.task_seen == it + 1
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged at iteration %d" % it
        loss = _events(ev, "agem_loss")
        assert len(loss) == 1 and abs(loss[0]["loss"] - ol["loss"]) < 1e-4, (loss, ol["loss"])
        rr, proj, loss_mem = _events(ev, "random_retrieve"), _events(ev, "agem"), _events(ev, "agem_loss_mem")
        if it == 0:
            assert not rr and not proj and not loss_mem and ol["cos"] is None
            projected = False
        else:
            assert len(rr) == 1 and np.array_equal(rr[0]["indices"], ol["idx"])
            assert len(loss_mem) == 1 and abs(loss_mem[0]["loss"] - ol["loss_mem"]) < 1e-4, (loss_mem, ol["loss_mem"])
            assert len(proj) == 1
            projected = proj[0]["projected"]
            assert projected == ol["projected"], (it, proj[0], ol["cos"])
        assert [list(e["slots"]) for e in _events(ev, "reservoir")] == [list(ol["slots"])]
        assert _buffers_equal(agent, oa)
        dw_o, dw_m = _flat(oa.state, oa.names) - w0, model.flat_params().double().cpu().numpy() - w0
        upd_err = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
        kinds[projected].append(upd_err)
        print("agem cosim it %2d  projected %d  cos %s  coef %s (oracle %.6g)  loss %.6f / %.6f  update err %.2e"
              % (it, projected, "   -   " if ol["cos"] is None else "%+.4f" % ol["cos"], "%.6g" % proj[0]["coef"] if proj else "-", ol["coef"],
                 loss[0]["loss"], ol["loss"], upd_err))
        assert upd_err <= (3e-2 if projected else 1e-2), (it, projected, upd_err)
    print("agem cosim: %d projected steps, worst update err %.2e; %d without projection, worst %.2e"
          % (len(kinds[True]), max(kinds[True]), len(kinds[False]), max(kinds[False])))
    assert len(kinds[True]) >= 3 and len(kinds[False]) >= 3


def test_cosim_agem_inner_steps(cuda):
    """agem_loops' stream, one stream batch per call at mem_iters 2 (agents/agem.py:38): two batch passes, from the second call on two
    draws from the memory and two projections, then ONE reservoir update.  Host RNG state, both retrievals, the slots and the buffers
    exact; the first pass starts from identical state: its two losses within 1e-4 and its decision the oracle's (|cos| is printed; the
    CPU test of the case shows it is never close to zero in the free run)."""
    from ocl_amd import debug
    cfg = dict(AGEM_LOOPS_CASE, epoch=1)
    params, model, opt, agent = _build_agent(cfg)
    assert agent.mem_iters == 2
    seed_all(cfg["seed"])
    oa = agem_ref.AgemOracle(cfg)
    xs, ys = agem_ref.cosim_stream(cfg)
    seed_all(1000 + cfg["seed"])
    for it in range(6):
        x, y = xs[it * 10:(it + 1) * 10], ys[it * 10:(it + 1) * 10]
        model.load_state_dict(oa.state_dict())
        st = _rng_get()
        oa.train_learner(x, y)
        ol = oa.log[-1]
        st_o = _rng_get()
        _rng_set(st)
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged at call %d" % it
        loss = _events(ev, "agem_loss")
        assert len(loss) == 2 and abs(loss[0]["loss"] - ol["loss"][0]) < 1e-4, (loss, ol["loss"])
        rr, proj, loss_mem = _events(ev, "random_retrieve"), _events(ev, "agem"), _events(ev, "agem_loss_mem")
        if it == 0:
            assert not rr and not proj and not loss_mem and ol["cos"] == [None, None]
        else:
            assert len(rr) == 2 and all(np.array_equal(a["indices"], b) for a, b in zip(rr, ol["idx"])), "retrieval of pass j differs"
            assert len(loss_mem) == 2 and abs(loss_mem[0]["loss"] - ol["loss_mem"][0]) < 1e-4, (loss_mem, ol["loss_mem"])
            assert len(proj) == 2
            print("agem_loops call %d  cos %s  projected %s (oracle %s)" % (it, ["%+.4f" % c for c in ol["cos"]], [p["projected"] for p in proj], ol["projected"]))
            if abs(ol["cos"][0]) >= 1e-3:
                assert proj[0]["projected"] == ol["projected"][0], (it, proj[0], ol["cos"])
        assert [list(e["slots"]) for e in _events(ev, "reservoir")] == [list(ol["slots"])], "one reservoir update per stream batch"
        assert _buffers_equal(agent, oa)


# ---- 5. the comparator ------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-4
COMPARATOR_MIN_COS = 20 * 2.0 ** -24 / COMPARATOR_BOUND       # 0.0119


def test_fused_projection_against_the_reference_statements_on_the_same_state(cuda, monkeypatch):
    """`_force_torch_projection` runs agents/agem.py:60-80 as written over the p.grad views.  Two agents, the second loaded with the
    first's state before every one of 8 slices of the co-simulation's stream, host RNG restored in between, order-independent batch
    sums: both take the same gradients to the projection, so they decide alike and their updates differ by the projection's arithmetic
    alone -- below 1e-4 norm-wise.  The fp32 pairwise sums move the coefficient by about 20 * 2^-24 / |cos| relative, and the update by
    no more than that, so the bound holds where |cos| >= 20 * 2^-24 / 1e-4 = 0.012: the cosine of the two gradients the fused agent
    hands to the kernel is computed here in float64 on every step and asserted to be at least that (a decision cannot flip there either)."""
    from ocl_amd import debug, ops
    cfg = AGEM_CASE
    ops.set_deterministic(True)
    try:
        _, model_a, _, a = _build_agent(cfg)
        _, model_b, _, b = _build_agent(cfg)
        b._force_torch_projection = True
        calls = _record_projections(monkeypatch)        # the fused agent's alone: the comparator does not call ops.agem_project
        xs, ys = agem_ref.cosim_stream(cfg)
        seed_all(1000 + cfg["seed"])
        flags = []
        for it in range(8):
            x, y = xs[it * 10:(it + 1) * 10], ys[it * 10:(it + 1) * 10]
            model_b.load_state_dict(model_a.state_dict())
            w0 = model_a.flat_params().double().cpu().numpy()
            st = _rng_get()
            evs = []
            for agent in (a, b):
                _rng_set(st)
                debug.LOG = []
                try:
                    agent.train_learner(x, y)
                    evs.append(list(debug.LOG))
                finally:
                    debug.LOG = None
            pa, pb = _events(evs[0], "agem"), _events(evs[1], "agem")
            assert len(pa) == len(pb) == (0 if it == 0 else 1)
            dw_a, dw_b = model_a.flat_params().double().cpu().numpy() - w0, model_b.flat_params().double().cpu().numpy() - w0
            diff = float(np.linalg.norm(dw_a - dw_b) / np.linalg.norm(dw_b))
            assert len(calls) == it
            if pa:
                gv, rv = calls[-1].g.double(), calls[-1].g_ref.double()
                cos = float(torch.dot(gv, rv) / (gv.norm() * rv.norm()))
                print("agem comparator it %d  projected %d  cos %+.4f  prod %.6g / %.6g  coef %.8g / %.8g  update difference %.2e"
                      % (it, pa[0]["projected"], cos, pa[0]["prod"], pb[0]["prod"], pa[0]["coef"], pb[0]["coef"], diff))
                assert abs(cos) >= COMPARATOR_MIN_COS, (it, cos)
                assert pa[0]["projected"] == pb[0]["projected"] == (cos < 0), (it, pa, pb, cos)
                flags.append(pa[0]["projected"])
            assert diff < COMPARATOR_BOUND, (it, diff)
            assert torch.equal(a.buffer.buffer_label, b.buffer.buffer_label) and a.buffer.n_seen_so_far == b.buffer.n_seen_so_far
        assert any(flags) and not all(flags), flags
    finally:
        ops.set_deterministic(False)


# ---- 6. free run against the recorded reference run -----------------------------------------------------------------------------------

def test_free_run_vs_reference_golden(cuda):
    """Whole tasks, free running, against the run recorded from the REAL reference agent (tests/golden/agem.npz): everything driven by
    the host RNGs is exact; the weights follow a chaotic trajectory and get the sanity band of
    test_gpu_steps.test_free_running_cases_vs_reference_golden."""
    from ocl_amd.data import setup_test_loader
    g = gold("agem")
    cfg = AGEM_CASE
    params, model, opt, agent = _build_agent(cfg)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        pre = "agem_c10_t%d_" % t
        assert np.array_equal(agent.buffer.buffer_label.cpu().numpy(), g[pre + "buf_label"]), "buffer labels differ from the reference"
        assert np.array_equal(agent.buffer.label_host, g[pre + "buf_label"]), "host label mirror out of step"
        assert [agent.buffer.current_index, agent.buffer.n_seen_so_far] == g[pre + "counters"].tolist()
        rs = agent.buffer.buffer_img.double().sum(dim=(1, 2, 3)).cpu().numpy()
        assert np.abs(rs - g[pre + "buf_rowsum"]).max() < 1e-6, "buffer images differ (slot indices or image bytes)"
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        print("agem_c10", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, g[pre + "acc"])
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()


def test_free_run_nested_loops_vs_reference_golden(cuda):
    """agem_loops (epoch 2, mem_iters 2), free running, against the reference's recording: the replay memory, the counters and the count
    of train-mode forwards per BatchNorm (one per pass in the first task, two from the second on) exact; the weights get the sanity band."""
    from ocl_amd.data import setup_test_loader
    g = gold("agem")
    cfg = AGEM_LOOPS_CASE
    params, model, opt, agent = _build_agent(cfg)
    assert (agent.epoch, agent.mem_iters) == (2, 2)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        pre = "agem_loops_t%d_" % t
        assert np.array_equal(agent.buffer.buffer_label.cpu().numpy(), g[pre + "buf_label"]), "buffer labels differ from the reference"
        assert np.array_equal(agent.buffer.label_host, g[pre + "buf_label"]), "host label mirror out of step"
        assert [agent.buffer.current_index, agent.buffer.n_seen_so_far] == g[pre + "counters"].tolist()
        rs = agent.buffer.buffer_img.double().sum(dim=(1, 2, 3)).cpu().numpy()
        assert np.abs(rs - g[pre + "buf_rowsum"]).max() < 1e-6, "buffer images differ (slot indices or image bytes)"
        assert digest_nbt(model.state_dict()).tolist() == g[pre + "nbt"].tolist(), "train-mode forward count differs from the reference"
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        print("agem_loops", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, g[pre + "acc"])
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()


# ---- 7. with Adam ------------------------------------------------------------------------------------------------------------------------

def test_agem_with_fused_adam_counts_one_step_per_iteration(cuda, monkeypatch):
    from ocl_amd.optim import FusedAdam
    cfg = dict(AGEM_CASE, n_train=15)        # 30 images per task: 3 iterations
    params, model, opt, agent = _build_agent(cfg, optimizer="Adam", learning_rate=1e-3)
    assert type(opt) is FusedAdam
    calls = _record_projections(monkeypatch)
    tasks, _ = make_stream(cfg)
    counts = []
    inner = opt.step

    def step(*a, **k):
        out = inner(*a, **k)
        counts.append((opt.step_count, len(calls)))
        return out

    opt.step = step
    w0 = model.flat_params().clone()
    agent.train_learner(*tasks[0])
    agent.train_learner(*tasks[1])
    assert counts == [(1, 0), (2, 0), (3, 0), (4, 1), (5, 2), (6, 3)], counts
    assert bool(torch.isfinite(model.flat_params()).all()) and not torch.equal(model.flat_params(), w0)
    assert all(c.out_is_ref for c in calls)
