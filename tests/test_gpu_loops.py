"""GPU: the outer control flow of the agents' loops -- epoch > 1, mem_iters > 1, batch != eps_mem_batch, drop_last.

 * co-simulation against the oracle, one stream batch per call at mem_iters = 2: host RNG state, the retrieval of BOTH inner passes,
   the ONE buffer update after them, the first pass's loss (identical state: 1e-4), the two chained SGD steps against the oracle's
   own +-1-ulp sensitivity for the same call;
 * the schedule-only comparisons of tests/test_gpu_steps.py at epoch 2 / mem_iters 2, and ER at batch 8 / eps_mem_batch 12 with
   the data-stream overlap on and off;
 * ER + ASER free running through the pipelined loop: forward counts and counters against the oracle agent.
(The free-running runs against the reference's recording, new cases included: test_gpu_steps.py::test_free_running_cases_vs_reference_golden.)
"""
import numpy as np
import pytest
import torch

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, digest_nbt
import test_gpu_steps as S
from test_gpu_steps import build_agent, cosim, _buffers_equal

pytestmark = pytest.mark.gpu


def _bound(self_dist):
    """Two chained SGD steps per call: the one-step bound 1e-2 does not transfer.  The engine may be as far from the oracle as 5x
    (the factor of test_gpu_parity2.test_free_running_trajectory_inside_the_oracles_own_spread) the oracle is from itself when its
    weights move by one unit in the last place -- measured on the CPU for the same call, never from the engine's error."""
    return max(1e-2, 5 * self_dist)


def _cosim_cfg(name, mem_size):
    """One stream batch per call: one epoch of one batch; a small memory so that the reservoir overwrites within the calls."""
    return dict(STEP_CASES[name], epoch=1, mem_size=mem_size)


@pytest.mark.parametrize("name,n_calls", [("er_loops", 6), ("er_uneven", 7)])
def test_cosim_er_inner_steps(cuda, name, n_calls):
    """ER random / random at mem_iters 2.  er_loops (batch 10 = eps_mem_batch): the merged two-group pass, twice per call.  er_uneven
    (batch 8, eps_mem_batch 12, weight decay 1e-4, lr 0.05): the second call retrieves min(12, 8) = 8 and merges, every later one
    retrieves 12 and takes the two-pass step."""
    cfg = _cosim_cfg(name, 30)
    batch = cfg.get("batch", 10)
    n_two_pass = 0
    for it, ev, ol, chk in cosim(cfg, n_calls, cuda, batch=batch, self_distance=True):
        assert chk["rng_equal"], "host RNG streams diverged at call %d" % it
        rr = [e["indices"] for t, e in ev if t == "random_retrieve"]
        assert len(rr) == 2 == len(ol["idx"]) and all(np.array_equal(a, b) for a, b in zip(rr, ol["idx"])), "retrieval of pass j differs"
        res = [list(e["slots"]) for t, e in ev if t == "reservoir"]
        assert res == [list(ol["slots"])], "one reservoir update per stream batch, after the inner passes"
        assert _buffers_equal(chk["agent"], chk["oa"])
        losses = [e["loss"] for t, e in ev if t == "er_loss"]
        assert len(losses) == 2 and abs(losses[0] - ol["loss"][0]) < 1e-4, (losses, ol["loss"])
        mem_losses = [e["loss"] for t, e in ev if t == "er_loss_mem"]
        o_mem = ol.get("loss_mem", [None, None])          # (no entry at all while the memory is empty)
        assert len(mem_losses) == sum(l is not None for l in o_mem)
        if mem_losses:
            assert abs(mem_losses[0] - o_mem[0]) < 1e-4
        n_two_pass += bool(len(rr[0])) and len(rr[0]) != batch
        print("%s call %d: oracle self-distance %.3e, bound %.3e, engine update error %.3e; j=1 loss %.6f (oracle %.6f)"
              % (name, it, chk["self_dist"], _bound(chk["self_dist"]), chk["upd_err"], losses[1], ol["loss"][1]))
        assert chk["upd_err"] <= _bound(chk["self_dist"]), (it, chk["upd_err"], chk["self_dist"])
        if cfg.get("weight_decay"):
            # Weight decay is below the update bound (lr * wd * |w| against lr * |g|), so it gets a statement of its own.  An optimiser
            # that dropped it would leave lr * wd * w behind per step, mem_iters * lr * wd * w0 per call to first order: the coefficient of
            # (engine update - oracle update) along w0 would be 2 * lr * wd = 1e-5.  The rest of the difference (ReLU sign flips, round-off)
            # has no reason to point along w0 -- a BatchNorm-fed convolution's gradient is orthogonal to its weights -- so a quarter of
            # that coefficient separates the two.
            coef = float(chk["dw_err"] @ chk["w0"] / (chk["w0"] @ chk["w0"]))
            full = cfg["mem_iters"] * cfg["learning_rate"] * cfg["weight_decay"]
            print("%s call %d: update difference along w0 %.3e (a dropped weight decay: %.3e)" % (name, it, coef, full))
            assert abs(coef) < full / 4, (it, coef, full)
        opt_group = chk["agent"].opt.param_groups[0]
        assert (opt_group["lr"], opt_group["weight_decay"]) == (cfg.get("learning_rate", 0.1), cfg.get("weight_decay", 0))
    assert n_two_pass == (n_calls - 2 if name == "er_uneven" else 0)


def test_cosim_scr_inner_steps(cuda):
    """SCR at mem_iters 2: retrieve + two views + SupCon + SGD twice, then ONE reservoir update."""
    cfg = _cosim_cfg("scr_loops", 30)
    for it, ev, ol, chk in cosim(cfg, 4, cuda, self_distance=True):
        assert chk["rng_equal"], "host RNG streams diverged at call %d" % it
        rr = [e["indices"] for t, e in ev if t == "random_retrieve"]
        assert len(rr) == 2 == len(ol[1]) and all(np.array_equal(a, b) for a, b in zip(rr, ol[1]))
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"] == [list(ol[2])]
        assert _buffers_equal(chk["agent"], chk["oa"])
        losses = [e["loss"] for t, e in ev if t == "scr_loss"]
        if ol[0][0] is None:
            assert not losses and ol[0][1] is None
            continue
        assert len(losses) == 2 and abs(losses[0] - ol[0][0]) < 1e-4, (losses, ol[0])
        print("scr_loops call %d: oracle self-distance %.3e, bound %.3e, engine update error %.3e; j=1 loss %.6f (oracle %.6f)"
              % (it, chk["self_dist"], _bound(chk["self_dist"]), chk["upd_err"], losses[1], ol[0][1]))
        assert chk["upd_err"] <= _bound(chk["self_dist"]), (it, chk["upd_err"], chk["self_dist"])


def test_cosim_mir_inner_steps(cuda, monkeypatch):
    """MIR at mem_iters 2: the candidate subsample of both passes is exact (numpy RNG); the first pass's virtual step gets the oracle's
    gradient (test_gpu_steps._force_mir_gradient's reason) and its scores are the oracle's to 1e-4, its retrieval a valid top-k under
    them; the second pass reads the engine's own gradient of the batch pass of ITS j -- from the stepped weights."""
    import ocl_amd.plugins.mir_retrieve as mr
    real, holder = mr.get_grad_vector, {}

    def first_call_forced(model):
        holder["n"] += 1
        return holder["g"] if holder["n"] == 1 else real(model)
    monkeypatch.setattr(mr, "get_grad_vector", first_call_forced)

    def before_hip(olog):
        holder["g"], holder["n"] = olog["grad"][0].to(cuda).contiguous(), 0
    cfg = _cosim_cfg("mir_loops", 30)
    for it, ev, ol, chk in cosim(cfg, 5, cuda, before_hip=before_hip, self_distance=True):
        assert chk["rng_equal"], "host RNG streams diverged at call %d" % it
        assert holder["n"] == 2, "one virtual step per inner pass"
        rr = [e["indices"] for t, e in ev if t == "random_retrieve"]
        assert len(rr) == 2 and all(np.array_equal(a, b) for a, b in zip(rr, ol["sub"])), "candidate subsample of pass j differs"
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"] == [list(ol["slots"])]
        assert _buffers_equal(chk["agent"], chk["oa"])
        losses = [e["loss"] for t, e in ev if t == "er_loss"]
        assert len(losses) == 2 and abs(losses[0] - ol["loss"][0]) < 1e-4, (losses, ol["loss"])
        mir_ev = [e for t, e in ev if t == "mir"]
        if "scores" not in ol:          # empty memory: nothing to score
            assert not mir_ev
            continue
        assert len(mir_ev) == 2
        sc, osc = mir_ev[0]["scores"], ol["scores"][0]
        assert np.abs(sc - osc).max() < 1e-4 * (1 + np.abs(osc).max()), (it, np.abs(sc - osc).max())
        k = len(mir_ev[0]["big_ind"])
        thr = np.sort(osc)[::-1][k - 1]
        assert osc[mir_ev[0]["big_ind"]].min() >= thr - 1e-4 * (1 + abs(thr))
        same = set(mir_ev[0]["big_ind"].tolist()) == set(np.argsort(-osc, kind="stable")[:k].tolist())
        print("mir_loops call %d: oracle self-distance %.3e, bound %.3e, engine update error %.3e (same j=0 retrieval: %s)"
              % (it, chk["self_dist"], _bound(chk["self_dist"]), chk["upd_err"], same))
        if same:     # (a near-tie of the oracle's own scores may legitimately retrieve another sample: then the updates are not comparable)
            assert chk["upd_err"] <= _bound(chk["self_dist"]), (it, chk["upd_err"], chk["self_dist"])


# ---------------------------------------------------------------------------------------------------------------------
# schedule-only at epoch 2 / mem_iters 2 (a third of the samples: as many steps as the epoch 1 / mem_iters 1 legs)
# ---------------------------------------------------------------------------------------------------------------------

def test_scr_data_stream_overlap_is_schedule_only_in_nested_loops(cuda, monkeypatch):
    S.scr_data_stream_overlap_legs(cuda, monkeypatch, 2, 2, 200)


def test_er_data_stream_overlap_is_schedule_only_in_nested_loops(cuda, monkeypatch):
    S.er_data_stream_overlap_legs(cuda, monkeypatch, 2, 2, 200)


def test_er_merged_step_direct_backward_is_schedule_only_in_nested_loops(cuda):
    S.er_merged_step_direct_backward_legs(cuda, 2, 2, 200)


def test_aser_pipelined_loop_is_schedule_only_in_nested_loops(cuda, monkeypatch):
    S.aser_pipelined_loop_legs(cuda, monkeypatch, 2, 2, 130)


def test_aser_passes_without_readers_are_schedule_only_in_nested_loops(cuda):
    S.aser_passes_without_readers_legs(cuda, 2, 2, 130)


def test_er_uneven_batches_data_stream_overlap_is_schedule_only(cuda, monkeypatch):
    """batch 8 against eps_mem_batch 12: from the third step on every pass is the two-pass step with a retrieval fetched on the data
    stream; 204 samples = 25 batches, 4 samples dropped.  Overlap on against off, bit for bit in the deterministic mode."""
    S.er_data_stream_overlap_legs(cuda, monkeypatch, 1, 2, 204, batch=8, eps_mem_batch=12, mem_size=100, weight_decay=1e-4,
                                  learning_rate=0.05)


# ---------------------------------------------------------------------------------------------------------------------
# ER + ASER: forward counts of the pipelined loop
# ---------------------------------------------------------------------------------------------------------------------

def test_aser_pipelined_loop_forward_counts_vs_oracle(cuda):
    """aser_loops free running with the pipeline on (no trace): the batch-pass forward issued ahead of update_finish, the
    forward_stats_only passes and the combined pass must add up to the oracle agent's count of train-mode forwards per BatchNorm, and
    the memory counters to its counters -- none of which depends on how a Shapley tie is ordered.  The class table describes the memory."""
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CB
    cfg = STEP_CASES["aser_loops"]
    params, model, agent = build_agent(cfg)
    assert (agent.epoch, agent.mem_iters) == (2, 2)
    tasks, _ = make_stream(cfg)
    x, y = tasks[0]
    agent.train_learner(x, y)
    torch.cuda.synchronize()
    seed_all(cfg["seed"])
    oa = O.OracleAgent(cfg)
    oa.train_learner(x, y)
    assert digest_nbt(model.state_dict()).tolist() == digest_nbt(oa.state_dict()).tolist()
    assert [agent.buffer.current_index, agent.buffer.n_seen_so_far] == [oa.buf.current_index, oa.buf.n_seen_so_far] == [40, 120]
    lab = agent.buffer.buffer_label.cpu().numpy()
    assert np.array_equal(lab, agent.buffer.label_host)
    for c, members in CB.class_index_cache.items():
        assert all(lab[i] == c for i in members)
    assert sum(len(m) for m in CB.class_index_cache.values()) == cfg["mem_size"] == int(CB.class_num_cache.sum())
