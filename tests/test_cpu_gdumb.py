"""CPU: the host side of the GDumb agent (ocl_clip_grad_norm's argument checks, the registries, the greedy class-balanced planner) and
the references the GPU tests rely on: the float64 clip with its round-off bound, and the restatement of the reference's agent
(tests/gdumb_ref.py) against the reference itself, against its recorded run (tests/golden/gdumb.npz) and over the co-simulation's run."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from conftest import gold
from oracle import ref_import
from oracle.synth import make_stream, seed_all, case_params
from test_cpu_adam import make_grads
import gdumb_ref
from gdumb_ref import ref_clip, clip_bound, worst_ratio, max_norm_for, GDUMB_CASE, GOLDEN_KEYS, BALANCER_CASES

OCL_ERR_ARG = -1    # include/ocl_hip.h


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # 16-byte aligned host address: never dereferenced, every case below is refused first


def _call(**over):
    kw = dict(g=A, n=16, max_norm=1.0, ws=A + 128, ws_doubles=1, info=A + 160)
    kw.update(over)
    rc = ffi.lib().ocl_clip_grad_norm(ffi.vp(kw["g"]), kw["n"], kw["max_norm"], ffi.vp(kw["ws"]), kw["ws_doubles"], ffi.vp(kw["info"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signatures_are_registered():
    res, args = ffi.SIGNATURES["ocl_clip_grad_norm"]
    assert res is C.c_int and args == [ffi.vp, ffi.i64, ffi.f32, ffi.vp, ffi.i64, ffi.vp, ffi.vp]
    assert ffi.SIGNATURES["ocl_clip_workspace_doubles"] == (ffi.i64, [ffi.i64])
    assert hasattr(ffi.lib(), "ocl_clip_grad_norm") and hasattr(ffi.lib(), "ocl_clip_workspace_doubles")


@pytest.mark.parametrize("over", [
    dict(g=0), dict(ws=0),
    dict(n=0), dict(n=-16),
    dict(ws_doubles=0), dict(ws_doubles=-1), dict(n=4096, ws_doubles=3),
    dict(max_norm=-1.0), dict(max_norm=-1e-30), dict(max_norm=float("nan")),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_abi_refuses_bad_arguments_without_a_device(over):
    rc, msg = _call(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("clip:"), msg


def test_abi_refuses_misaligned_pointers_without_a_device():
    for over in (dict(g=A + 4), dict(g=A + 8), dict(g=A + 12), dict(ws=A + 128 + 4)):
        rc, msg = _call(**over)
        assert rc == OCL_ERR_ARG and msg.startswith("clip:") and "aligned" in msg, (over, rc, msg)


def test_workspace_size_is_small_positive_and_monotone():
    f = ffi.lib().ocl_clip_workspace_doubles
    sizes = [1, 2, 3, 4, 5, 1003, 1024, 1025, 4099, 65536, 524288, 524289, 1094750, 1109240, 1 << 24, 1 << 31, 1 << 40]
    got = [f(n) for n in sizes]
    assert all(0 < w <= 512 for w in got), got
    assert got == sorted(got) and got[0] == 1 and got[-1] == 512, got
    assert f(0) > 0 and f(-5) > 0


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_gdumb_is_an_offline_agent_and_the_other_tables_are_unchanged():
    from ocl_amd import name_match
    from ocl_amd.agents.gdumb import Gdumb
    assert set(name_match.offline_agents.keys()) == {"GDUMB"}
    assert name_match.get_agent("GDUMB") is Gdumb is name_match.offline_agents["GDUMB"]
    assert set(name_match.agents.keys()) == {"ER", "SCR"}
    assert set(name_match.extra_agents.keys()) == {"AGEM"}
    assert set(name_match.regularization_agents.keys()) == {"EWC"}
    with pytest.raises(KeyError):
        name_match.get_agent("nope")
    assert Gdumb._force_torch_clip is False


# ---- the greedy class-balanced planner ---------------------------------------------------------------------------------------------------

def _assert_same(got, want, where):
    assert len(got) == len(want), where
    for b, (g, w) in enumerate(zip(got, want)):
        for k in ("counts", "items", "labels"):        # counts: [class, count] rows in dict order; items: per-class contents in that order
            assert np.array_equal(g[k], w[k]), (where, b, k, g[k], w[k])


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
@pytest.mark.parametrize("case", BALANCER_CASES, ids=lambda c: c[0])
def test_balancer_equals_the_reference_update_after_every_batch(case):
    from ocl_amd.gdumb_memory import GreedyBalancer
    name, mem_size, seed, batches = case
    want = gdumb_ref.run_reference_balancer(mem_size, seed, batches)
    got, _ = gdumb_ref.run_balancer_case(GreedyBalancer, mem_size, seed, batches)
    _assert_same(got, want, name)


@pytest.mark.parametrize("case", BALANCER_CASES, ids=lambda c: c[0])
def test_balancer_equals_the_recorded_reference_update(case):
    from ocl_amd.gdumb_memory import GreedyBalancer
    name, mem_size, seed, batches = case
    g = gold("gdumb")
    want = [{k: g["bal_%s_b%d_%s" % (name, b, k)] for k in ("counts", "items", "labels")} for b in range(len(batches))]
    got, _ = gdumb_ref.run_balancer_case(GreedyBalancer, mem_size, seed, batches)
    _assert_same(got, want, name)


def test_balancer_cases_cover_what_they_are_named_for():
    """The sequences see an eviction at a full memory, k_c of 1 and of 0, and a slot written twice within one batch."""
    from ocl_amd.gdumb_memory import GreedyBalancer
    by_name = {c[0]: c for c in BALANCER_CASES}
    out, bal = gdumb_ref.run_balancer_case(GreedyBalancer, *by_name["fill"][1:])
    assert sum(bal.mem_c.values()) < bal.mem_size and len(bal.free) == bal.mem_size - sum(bal.mem_c.values())
    out, bal = gdumb_ref.run_balancer_case(GreedyBalancer, *by_name["new_class_at_full"][1:])
    assert sum(bal.mem_c.values()) == bal.mem_size and list(bal.mem_c.keys()) == [0, 1, 2, 3] and min(bal.mem_c.values()) >= 1
    out, bal = gdumb_ref.run_balancer_case(GreedyBalancer, *by_name["many_classes"][1:])
    assert len(bal.mem_c) == 12 and bal.mem_size // len(bal.mem_c) == 1
    name, mem_size, seed, batches = by_name["fill_then_evict_in_one_batch"]

    class Counting(GreedyBalancer):
        accepted = 0

        def _update(self, y, row, writes):
            before = dict(writes)
            super()._update(y, row, writes)
            self.accepted += writes != before

    out, bal = gdumb_ref.run_balancer_case(Counting, mem_size, seed, batches)
    assert bal.accepted > sum(len(o["rows"]) for o in out), "no row was accepted and dropped again within its batch"
    assert all(len(o["rows"]) <= mem_size for o in out)
    out, bal = gdumb_ref.run_balancer_case(GreedyBalancer, *by_name["fewer_slots_than_classes"][1:])
    assert len(bal.mem_c) > bal.mem_size and bal.mem_size // len(bal.mem_c) == 0 and sum(bal.mem_c.values()) == bal.mem_size


@pytest.mark.parametrize("mem_size,n_cls,seed", [(1, 3, 0), (7, 3, 1), (10, 10, 2), (16, 40, 3), (50, 6, 4)])
def test_balancer_properties_on_random_label_streams(mem_size, n_cls, seed):
    """A plan never names a slot (or a row) twice; the slots in use and the free slots partition range(mem_size); order() has
    sum(mem_c) entries; the host view of what each slot holds agrees with a sample-by-sample replay."""
    from ocl_amd.gdumb_memory import GreedyBalancer
    rng = np.random.default_rng(seed)
    random.seed(seed)
    bal = GreedyBalancer(mem_size)
    slot_label = np.full(mem_size, -1, dtype=np.int64)
    for it in range(30):
        ys = rng.integers(0, n_cls, int(rng.integers(1, 14)))
        rows, slots = bal.plan(ys)
        assert len(set(slots.tolist())) == len(slots) and len(set(rows.tolist())) == len(rows)
        assert ((slots >= 0) & (slots < mem_size)).all() and ((rows >= 0) & (rows < len(ys))).all()
        slot_label[slots] = ys[rows]
        used = [s for c in bal.mem_slots for s in bal.mem_slots[c]]
        assert sorted(used + bal.free) == list(range(mem_size))
        assert all(len(bal.mem_slots[c]) == bal.mem_c[c] for c in bal.mem_c) and list(bal.mem_slots.keys()) == list(bal.mem_c.keys())
        order_slots, order_labels = bal.order()
        assert len(order_slots) == len(order_labels) == sum(bal.mem_c.values()) <= mem_size
        assert np.array_equal(slot_label[order_slots], order_labels), "a slot holds another class than the planner believes"


# ---- the float64 clip and its bound -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [0.5, 1.5, 100.0])
@pytest.mark.parametrize("n", [1, 3, 5, 1003, 100003])
def test_fp32_emulation_stays_inside_the_bound(n, ratio):
    """numpy in the kernel's order of roundings -- the sum of squares, the square root and the quotient in float64, the coefficient
    rounded to float32, fl(g * coef) -- within 1 x clip_bound; exact equality where nothing is clipped."""
    rng = np.random.default_rng(100 + n)
    g = make_grads(rng, n, 1)
    max_norm = max_norm_for(g, ratio)
    ref = ref_clip(g, max_norm)
    assert ref.clipped == (ratio > 1) and abs(ref.total / max_norm - ratio) < 1e-6 * ratio
    g64 = g.astype(np.float64)
    coef_d = np.float64(max_norm) / (np.sqrt((g64 * g64).sum()) + 1e-6)
    coef = np.float32(coef_d)
    clipped = not (coef_d >= 1.0) and not (coef == np.float32(1.0))
    out = g * coef if clipped else g
    assert out.dtype == np.float32 and clipped == ref.clipped
    ratio_err = worst_ratio(out, ref)
    print("fp32 emulation n=%d total/max_norm=%g: worst |err| / bound %.3f" % (n, ratio, ratio_err))
    assert ratio_err <= 1.0, ratio_err
    if not ref.clipped:
        assert np.array_equal(out, g) and not clip_bound(ref).any()


def test_ref_clip_exact_cases():
    g = make_grads(np.random.default_rng(8), 4099, 1)
    ref = ref_clip(g, 0.0)
    assert ref.clipped and ref.coef == 0.0 and not ref.out.any()
    ref = ref_clip(np.zeros(5, np.float32), 1.0)
    assert not ref.clipped and ref.coef == 1.0 and ref.total == 0.0 and not ref.out.any()
    ref = ref_clip(np.zeros(5, np.float32), 0.0)          # 0 / 1e-6 = 0: "clipped" by a coefficient of 0, and still all zero
    assert ref.clipped and not ref.out.any()
    ref = ref_clip(g, 1e9)
    assert not ref.clipped and np.array_equal(ref.out, g.astype(np.float64))


# ---- the restatement against the reference and its recorded run ------------------------------------------------------------------------

@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
def test_gdumb_oracle_equals_the_reference_agent_over_one_task():
    """One task pins the loader, the greedy memory, the fresh network, the composed permutations, the clip and the SGD step bit for bit;
    the golden test below (recorded from the reference, all three tasks) pins the evictions of the later tasks."""
    torch.set_num_threads(1)
    cfg = GDUMB_CASE
    ref_import.activate()
    params = ref_import.default_params(**case_params(cfg), **gdumb_ref.gdumb_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = ref_import.build_agent(params)
    tasks, _ = make_stream(cfg)
    x, y = tasks[0]
    with ref_import.quiet():
        agent.train_learner(x, y)
    seed_all(cfg["seed"])
    ag = gdumb_ref.GdumbOracle(cfg)
    ag.train_learner(x, y)
    assert list(agent.mem_c.items()) == list(ag.mem_c.items()) and list(agent.mem_img.keys()) == list(ag.mem_img.keys())
    for c in agent.mem_img:
        assert len(agent.mem_img[c]) == len(ag.mem_img[c]) and all(torch.equal(a, b) for a, b in zip(agent.mem_img[c], ag.mem_img[c])), c
    sd = agent.model.state_dict()
    assert agent.model is not model, "train_mem builds a fresh network"
    assert list(sd.keys()) == list(ag.state.keys())
    for k, v in sd.items():
        assert torch.equal(v, ag.state[k].detach()), k
    assert len(ag.log) == 10 and any(e["clipped"] for e in ag.log) and not all(e["clipped"] for e in ag.log)


def test_gdumb_oracle_free_run_reproduces_the_recorded_reference_run():
    """Everything the host RNGs drive is exact on any machine.  The weights are bit-equal only on a CPU whose float32 convolution and
    matrix kernels add in the order of the recording machine's, and they follow a chaotic trajectory: they get the sanity band of
    test_cpu_agem.test_agem_step_free_run_reproduces_the_recorded_reference_run, as the GPU free run does."""
    g = gold("gdumb")
    recs, ag = gdumb_ref.run_oracle_case()
    assert len(recs) == int(g["gdumb_c10_ntasks"]) == 3
    assert set(GOLDEN_KEYS) == {"acc", "mem_label", "mem_rowsum", "mem_counts", "state"}
    for t, rec in enumerate(recs):
        for k in ("mem_label", "mem_rowsum", "mem_counts"):
            assert np.array_equal(rec[k], g["gdumb_c10_t%d_%s" % (t, k)]), (t, k)
        ds, gs, acc, gacc = rec["state"], g["gdumb_c10_t%d_state" % t], rec["acc"], g["gdumb_c10_t%d_acc" % t]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())
        print("gdumb_c10 oracle", t, "state digest rel err", rel, "norm ratio", ratio, "acc", acc, gacc)
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (t, rel, ratio)
        assert acc.shape == gacc.shape and (acc >= 0).all() and (acc <= 1).all()
    assert len(ag.log) == len(g["gdumb_c10_total_norm"]) == 30
    assert [len(r["mem_label"]) for r in recs] == [50, 50, 50] and [len(r["mem_counts"]) for r in recs] == [2, 4, 6]


def test_cosim_run_takes_both_branches_far_from_the_threshold():
    """What tests/test_gpu_gdumb.py's co-simulation relies on (the case's three tasks without evaluate() in between): at least 3 memory
    steps clip and at least 3 do not, and |total / clip - 1| >= 1e-2 on every one, so that a decision cannot flip by rounding."""
    recs, ag = gdumb_ref.run_oracle_case(evaluate=False)
    ratios = np.array([e["ratio"] for e in ag.log])
    n_clip = sum(e["clipped"] for e in ag.log)
    print("%d memory steps, %d clip, %d do not, min |total/clip - 1| %.4f" % (len(ag.log), n_clip, len(ag.log) - n_clip, np.abs(ratios - 1).min()))
    assert len(ag.log) == GDUMB_CASE["mem_epoch"] * (50 // GDUMB_CASE["batch"]) * 3 == 30
    assert n_clip >= 3 and len(ag.log) - n_clip >= 3
    assert np.abs(ratios - 1).min() >= 1e-2
    assert all(e["clipped"] == (e["ratio"] > 1) for e in ag.log)
