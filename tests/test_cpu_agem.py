"""CPU: the host side of the A-GEM agent (ocl_agem_project's argument checks, the registries) and the references the GPU tests rely on:
the float64 projection with its round-off bound, and the restatement of the reference's iteration (tests/agem_ref.py) against the
reference itself, against its recorded run (tests/golden/agem.npz) and over the co-simulation's stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from conftest import gold
from oracle import ref_import
from oracle.synth import make_stream, seed_all, case_params
from test_cpu_adam import make_grads
import agem_ref
from agem_ref import ref_project, project_bound, worst_ratio, with_cosine, AGEM_CASE, AGEM_LOOPS_CASE, GOLDEN_KEYS

OCL_ERR_ARG = -1    # include/ocl_hip.h


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # 16-byte aligned host address: never dereferenced, every case below is refused first


def _call(**over):
    a = A
    kw = dict(g=a, r=a + (1 << 24), n=16, ws=a + 128, ws_doubles=2, info=a + 160)
    kw.update(over)
    rc = ffi.lib().ocl_agem_project(ffi.vp(kw["g"]), ffi.vp(kw["r"]), kw["n"], ffi.vp(kw["ws"]), kw["ws_doubles"], ffi.vp(kw["info"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signatures_are_registered():
    res, args = ffi.SIGNATURES["ocl_agem_project"]
    assert res is C.c_int and args == [ffi.vp, ffi.vp, ffi.i64, ffi.vp, ffi.i64, ffi.vp, ffi.vp]
    assert ffi.SIGNATURES["ocl_agem_workspace_doubles"] == (ffi.i64, [ffi.i64])


@pytest.mark.parametrize("over", [
    dict(g=0), dict(r=0), dict(ws=0),
    dict(n=0), dict(n=-16),
    dict(ws_doubles=1), dict(ws_doubles=0), dict(n=4096, ws_doubles=6),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_abi_refuses_bad_arguments_without_a_device(over):
    rc, msg = _call(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("agem:"), msg


def test_abi_refuses_misaligned_and_overlapping_pointers_without_a_device():
    a = A
    for over in (dict(g=a + 4), dict(r=a + 64 + 4), dict(g=a + 8), dict(r=a + 64 + 8), dict(ws=a + 128 + 4)):
        rc, msg = _call(**over)
        assert rc == OCL_ERR_ARG and msg.startswith("agem:") and "aligned" in msg, (over, rc, msg)
    for over in (dict(r=a), dict(r=a + 48), dict(g=a + 112, r=a + 64), dict(r=a + 16, n=4096, ws_doubles=1024)):
        rc, msg = _call(**over)
        assert rc == OCL_ERR_ARG and msg.startswith("agem:") and "overlap" in msg, (over, rc, msg)


def test_workspace_size_is_small_positive_and_monotone():
    f = ffi.lib().ocl_agem_workspace_doubles
    sizes = [1, 2, 3, 4, 5, 1003, 1024, 1025, 4099, 65536, 524288, 524289, 1094750, 1109240, 1 << 24, 1 << 31, 1 << 40]
    got = [f(n) for n in sizes]
    assert all(0 < w <= 1024 and w % 2 == 0 for w in got), got
    assert got == sorted(got) and got[0] == 2 and got[-1] == 1024, got
    assert f(0) > 0 and f(-5) > 0


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_agem_is_an_extra_agent_and_the_baseline_table_is_unchanged():
    from ocl_amd import name_match
    from ocl_amd.agents.agem import AGEM
    from ocl_amd.agents.exp_replay import ExperienceReplay
    from ocl_amd.agents.scr import SupContrastReplay
    assert set(name_match.extra_agents.keys()) == {"AGEM"}
    assert name_match.get_agent("ER") is ExperienceReplay and name_match.get_agent("SCR") is SupContrastReplay
    assert name_match.get_agent("AGEM") is AGEM is name_match.extra_agents["AGEM"]
    with pytest.raises(KeyError):
        name_match.get_agent("nope")
    assert set(name_match.agents.keys()) == {"ER", "SCR"} and "AGEM" not in name_match.agents
    assert AGEM._force_torch_projection is False
    assert ExperienceReplay._kd_mix is AGEM._kd_mix      # one blend for both loops


# ---- the float64 projection and its bound ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cos", [-0.1, -1e-3, 0.1])
@pytest.mark.parametrize("n", [1, 3, 5, 1003, 100003])
def test_fp32_emulation_stays_inside_the_bound(n, cos):
    """numpy float32 in the kernel's order of roundings -- the coefficient rounded to float32, fl(g - fl(coef * r)) -- from the float64
    sums: within 1 x project_bound; exact equality where nothing is projected."""
    rng = np.random.default_rng(100 + n)
    r = make_grads(rng, n, 1)
    g = with_cosine(rng, r, cos)
    ref = ref_project(g, r)
    assert ref.projected == (cos < 0)
    if n > 100:
        got_cos = ref.prod / (np.linalg.norm(ref.g) * np.linalg.norm(ref.r))
        assert abs(got_cos - cos) < 1e-3 * abs(cos) + 1e-6, got_cos
    coef = np.float32(ref.coef)
    out = (g - coef * r) if ref.projected else g
    assert out.dtype == np.float32
    ratio = worst_ratio(out, ref)
    print("fp32 emulation n=%d cos=%g: worst |err| / bound %.3f" % (n, cos, ratio))
    assert ratio <= 1.0, ratio


def test_ref_project_exact_cases():
    rng = np.random.default_rng(8)
    r = make_grads(rng, 4099, 1)
    ref = ref_project(-r, r)
    assert ref.projected and ref.coef == -1.0 and not ref.out.any()
    g = make_grads(rng, 4099, 1)
    g[::2], r[1::2] = 0.0, 0.0                      # orthogonal supports
    ref = ref_project(g, r)
    assert ref.prod == 0.0 and not ref.projected and np.array_equal(ref.out, g.astype(np.float64)) and not project_bound(ref).any()
    ref = ref_project(g, np.zeros_like(g))
    assert not ref.projected and np.isfinite(ref.out).all() and np.array_equal(ref.out, g.astype(np.float64))


# ---- the restatement against the reference and its recorded run ------------------------------------------------------------------------

@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_agem_step_equals_the_reference_agent_over_one_task():
    """Two tasks' worth would be needed to see memory; the first task pins the loader, the batch pass, the SGD step and the reservoir,
    the golden test below (recorded from the reference, all three tasks) pins the rest."""
    torch.set_num_threads(1)
    cfg = AGEM_CASE
    ref_import.activate()
    params = ref_import.default_params(**case_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = ref_import.build_agent(params)
    tasks, _ = make_stream(cfg)
    x, y = tasks[0]
    with ref_import.quiet():
        agent.train_learner(x, y)
    seed_all(cfg["seed"])
    ag = agem_ref.AgemOracle(cfg)
    ag.train_learner(x, y)
    assert np.array_equal(agent.buffer.buffer_label.numpy(), ag.buf.label.numpy()) and torch.equal(agent.buffer.buffer_img, ag.buf.img)
    assert [agent.buffer.current_index, agent.buffer.n_seen_so_far] == [ag.buf.current_index, ag.buf.n_seen_so_far]
    sd = model.state_dict()
    assert list(sd.keys()) == list(ag.state.keys())
    for k, v in sd.items():
        assert torch.equal(v, ag.state[k].detach()), k


def test_agem_step_free_run_reproduces_the_recorded_reference_run():
    """Everything the host RNGs drive is exact on any machine.  The weights are bit-equal only on a CPU whose float32 convolution and
    matrix kernels add in the order of the recording machine's (another vector width is another order), and they follow a chaotic
    trajectory: they get the sanity band of test_gpu_steps.test_free_running_cases_vs_reference_golden, as the GPU free run does.
    Bit equality with the reference itself is asserted where both run on one machine: the test above and scripts/make_agem_golden.py."""
    g = gold("agem")
    recs, ag = agem_ref.run_oracle_case()
    assert len(recs) == int(g["agem_c10_ntasks"]) == 3
    assert set(GOLDEN_KEYS) == {"acc", "buf_label", "buf_rowsum", "counters", "state"}
    for t, rec in enumerate(recs):
        for k in ("buf_label", "buf_rowsum", "counters"):
            assert np.array_equal(rec[k], g["agem_c10_t%d_%s" % (t, k)]), (t, k)
        ds, gs, acc, gacc = rec["state"], g["agem_c10_t%d_state" % t], rec["acc"], g["agem_c10_t%d_acc" % t]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        print("agem_c10 oracle", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, gacc)
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (t, rel, ratio)
        assert acc.shape == gacc.shape and (acc >= 0).all() and (acc <= 1).all()
    seen = [e for e in ag.log if e["cos"] is not None]
    assert len(ag.log) == 18 and len(seen) == 12 and sum(e["projected"] for e in seen) == 4
    assert all(e["projected"] == (e["cos"] < 0) for e in seen)


def test_agem_step_nested_loops_reproduce_the_recorded_reference_run():
    """agem_loops (epoch 2, mem_iters 2; agents/agem.py:32-38): everything the host RNGs drive and the count of train-mode forwards
    per BatchNorm are exact against the reference's recording; one log entry per stream batch with per-j lists."""
    g = gold("agem")
    recs, ag = agem_ref.run_oracle_case(AGEM_LOOPS_CASE)
    assert len(recs) == int(g["agem_loops_ntasks"]) == 2
    for t, rec in enumerate(recs):
        for k in ("buf_label", "buf_rowsum", "counters", "nbt"):
            assert np.array_equal(rec[k], g["agem_loops_t%d_%s" % (t, k)]), (t, k)
    # 2 epochs x 3 batches x 2 passes: one forward each in the first task (12), two each in the second (24)
    assert g["agem_loops_t0_nbt"].tolist() == [12] * 20 and g["agem_loops_t1_nbt"].tolist() == [36] * 20
    assert g["agem_loops_t1_counters"].tolist() == [50, 120]
    assert len(ag.log) == 12 and all(len(e["loss"]) == 2 and len(e["idx"]) == 2 for e in ag.log)
    assert all(e["cos"] == [None, None] for e in ag.log[:6]) and all(None not in e["cos"] for e in ag.log[6:])
    assert all(p == (c < 0) for e in ag.log[6:] for p, c in zip(e["projected"], e["cos"]))


@pytest.mark.parametrize("seed", [14, 15, 16])
def test_cosim_stream_takes_both_branches_far_from_the_decision_boundary(seed):
    """What tests/test_gpu_agem.py's co-simulation relies on: over its 18 slices at least 3 steps project and at least 3 do not, and the
    two gradients are never close to orthogonal (|cos| >= 1e-3), so that a flipped decision cannot come from rounding."""
    oa = agem_ref.cosim_oracle(dict(AGEM_CASE, seed=seed))
    seen = [e for e in oa.log if e["cos"] is not None]
    proj = sum(e["projected"] for e in seen)
    cmin = min(abs(e["cos"]) for e in seen)
    print("seed %d: %d slices, %d see memory, %d project, %d do not, min |cos| %.4f" % (seed, len(oa.log), len(seen), proj, len(seen) - proj, cmin))
    assert len(oa.log) == 18 and oa.log[0]["cos"] is None and len(seen) == 17
    assert proj >= 3 and len(seen) - proj >= 3
    assert cmin >= 1e-3
    assert all(e["projected"] == (e["cos"] < 0) for e in seen)
