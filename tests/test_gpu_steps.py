"""GPU: whole replay steps of the HIP path (agents + plugins + engine) against
 (a) the runs recorded from the REAL reference (tests/golden/steps.npz): buffer labels / counters bit-exact, accuracies
     exact, weights / BN buffers within 1e-3 relative after ~10 free-running SGD steps,
 (b) the CPU oracle on identical state for single teacher-forced steps (ASER: tie-aware, see oracle/synth.py),
 (c) size-independent properties at BASELINE.json's full sizes (mem 5000 / 10000, eps_mem_batch 100, 84x84).
"""
import copy

import numpy as np
import pytest
import torch

import agent_harness as H
from agent_harness import TRICK, make_params, rng_get as _rng_get, rng_set as _rng_set, rng_equal as _rng_equal, flat as _flat  # noqa: F401  (other test files import them from here)
from conftest import gold
from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, digest_state, digest_nbt, digest_rng, class_images

pytestmark = pytest.mark.gpu


def build_agent(cfg, **over):
    """(params, model, agent): the shape this file, test_gpu_loops, test_gpu_parity2, test_gpu_f4 and test_gpu_datasets unpack."""
    params, model, _, agent = H.build_agent(cfg, **over)
    return params, model, agent


# er_gss is left out here: its multinomial draws are weighted by gradient similarities of the free-running weights, so the slots
# are not a function of the host RNG alone; test_gpu_parity2.test_cosim_gss compares it step by step from identical state
@pytest.mark.parametrize("name", [n for n, c in STEP_CASES.items() if c.get("golden", True) and c.get("free_run_gpu", True)])
def test_free_running_cases_vs_reference_golden(cuda, name):
    """Whole tasks, free running, against the run recorded from the REAL reference.  Everything driven by the host RNGs
    (which slots are written, with which samples, in which order; counters) must be bit-exact.  The weights themselves
    follow a chaotic trajectory (lr 0.1: the reference's own 1-thread vs 8-thread runs differ by |dw| ~ 0.2-0.4, SURVEY
    headline fact 4), so they are only sanity-checked here; per-step numerical parity is `test_cosim_*` below."""
    from ocl_amd.data import setup_test_loader
    g = gold("steps")
    cfg = STEP_CASES[name]
    params, model, agent = build_agent(cfg)
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        pre = "%s_t%d_" % (name, t)
        assert np.array_equal(agent.buffer.buffer_label.cpu().numpy(), g[pre + "buf_label"]), "buffer labels differ from the reference"
        assert np.array_equal(agent.buffer.label_host, g[pre + "buf_label"]), "host label mirror out of step"
        assert [agent.buffer.current_index, agent.buffer.n_seen_so_far] == g[pre + "counters"].tolist()
        # integer invariants of the loop: the count of train-mode forwards per BatchNorm, and where the host generators stand after
        # evaluate() (every permutation, retrieval and reservoir draw of the task taken, none twice)
        assert digest_nbt(model.state_dict()).tolist() == g[pre + "nbt"].tolist(), "train-mode forward count differs from the reference"
        assert digest_rng().tolist() == g[pre + "rng"].tolist(), "host RNG streams are not where the reference leaves them"
        rs = agent.buffer.buffer_img.double().sum(dim=(1, 2, 3)).cpu().numpy()
        assert np.abs(rs - g[pre + "buf_rowsum"]).max() < 1e-6, "buffer images differ (slot indices or image bytes)"
        ds, gs = digest_state(model.state_dict()), g[pre + "state"]
        rel = np.abs(ds - gs).max() / (1e-12 + np.abs(gs).max())
        print(name, t, "state digest rel err", rel, "acc", acc, g[pre + "acc"])
        # sanity only (the trajectory is chaotic: a different summation order in one kernel moves `rel` between 0.3 and 1.0+ from
        # build to build, as the reference's own thread counts do): everything finite, the state of the same magnitude as the reference's;
        # quantitative trajectory statistics: test_gpu_parity2.test_free_running_trajectory_inside_the_oracles_own_spread
        ratio = np.sqrt((ds[:, 1] ** 2).sum() / (gs[:, 1] ** 2).sum())      # all tensors together: L2 norm against the reference's
        assert np.isfinite(ds).all() and 0.5 < ratio < 2.0 and rel < 3.0, (rel, ratio)
        assert acc.shape == g[pre + "acc"].shape and (acc >= 0).all() and (acc <= 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# co-simulation: HIP agent and CPU oracle agent stepped one iteration at a time from IDENTICAL state
# ---------------------------------------------------------------------------------------------------------------------

def _oracle_self_distance(oa, x, y, st, w0, dw_o):
    """The oracle's own sensitivity for one call: the same call from a copy of the oracle whose weights are moved by one unit in the
    last place (up / down; test_gpu_parity2._oracle_run's perturbation), same memory, same host RNG state.  -> the larger norm-wise
    difference of the two updates from the unperturbed oracle's, relative to the latter."""
    out = 0.0
    for ulp in (1, -1):
        ob = copy.deepcopy(oa)
        with torch.no_grad():
            for k in ob.names:
                ob.state[k].copy_(torch.nextafter(ob.state[k].detach(), torch.full_like(ob.state[k], float("inf") * ulp)))
        wp0 = _flat(ob.state, ob.names)
        _rng_set(st)
        ob.train_learner(x, y)
        out = max(out, float(np.linalg.norm((_flat(ob.state, ob.names) - wp0) - dw_o) / (1e-30 + np.linalg.norm(dw_o))))
    return out


def cosim(cfg, n_iters, cuda, prefill=None, x_stream=None, before_hip=None, sync_extra=None, batch=10, self_distance=False):
    """Yields per iteration (events of the HIP agent, oracle log entry, dict of checks already made).  Before every
    iteration the HIP model is loaded with the oracle's weights and BatchNorm buffers (teacher forcing); both sides then
    consume the SAME host RNG streams (state saved / restored), and must leave them in the same state.  `batch` samples are fed per
    call; self_distance=True adds the oracle's own +-1-ulp sensitivity for the same call (`self_dist`)."""
    from ocl_amd import debug
    params, model, agent = build_agent(cfg)
    seed_all(cfg["seed"])
    oa = O.OracleAgent(cfg)
    if prefill is not None:
        prefill(agent, oa)
    if x_stream is None:
        tasks, _ = make_stream(cfg)
        x_stream = tasks[0]
    xs, ys = x_stream
    assert len(ys) >= n_iters * batch
    seed_all(1000 + cfg["seed"])
    for it in range(n_iters):
        x, y = xs[it * batch:(it + 1) * batch], ys[it * batch:(it + 1) * batch]
        model.load_state_dict(oa.state_dict())
        if sync_extra is not None:
            sync_extra(agent, oa)          # plugin state beyond weights / memory (e.g. GSS slot scores)
        state_before = {k: v.clone() for k, v in oa.state_dict().items()}
        buf_before = (oa.buf.img, oa.buf.label.clone())   # images of a slot change only when it is overwritten: callers index rows the step did not touch
        w0 = _flat(oa.state, oa.names)
        st = _rng_get()
        n_log = len(oa.log)
        probe = copy.deepcopy(oa) if self_distance else None
        oa.train_learner(x, y)
        st_o = _rng_get()
        self_dist = _oracle_self_distance(probe, x, y, st, w0, _flat(oa.state, oa.names) - w0) if self_distance else None
        _rng_set(st)
        if before_hip is not None:
            before_hip(oa.log[-1])
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        st_m = _rng_get()
        assert len(oa.log) == n_log + 1
        w1_o = _flat(oa.state, oa.names)
        w1_m = model.flat_params().double().cpu().numpy()
        dw_o, dw_m = w1_o - w0, w1_m - w0
        upd_err = float(np.linalg.norm(dw_m - dw_o) / (1e-30 + np.linalg.norm(dw_o))) if np.linalg.norm(dw_o) > 0 else float(np.linalg.norm(dw_m))
        yield it, ev, oa.log[-1], dict(rng_equal=_rng_equal(st_o, st_m), upd_err=upd_err, agent=agent, oa=oa, model=model,
                                       state_before=state_before, buf_before=buf_before, self_dist=self_dist, w0=w0, dw_err=dw_m - dw_o)


def _buffers_equal(agent, oa):
    return (np.array_equal(agent.buffer.buffer_label.cpu().numpy(), oa.buf.label.numpy()) and torch.equal(agent.buffer.buffer_img.cpu(), oa.buf.img)
            and [agent.buffer.current_index, agent.buffer.n_seen_so_far] == [oa.buf.current_index, oa.buf.n_seen_so_far])


def test_cosim_er_random(cuda):
    """BASELINE config 1 shape (ER random/random): per step, both CE losses within 1e-4 (north_star tolerance; observed
    ~1e-6), retrieved indices / reservoir slots / RNG state exact, SGD update within 1e-2 norm-wise (observed <= 4e-3: a handful
    of ReLU sign flips at ~0 per step perturb single channels; with the activation pattern teacher-forced the gradient agrees to
    2e-4, test_gpu_net and test_gpu_parity2.test_er_step_gradient_with_forced_relu_pattern_at_early_iterations)."""
    cfg = dict(STEP_CASES["er_c10"], mem_size=30)
    worst = 0.0
    for it, ev, ol, chk in cosim(cfg, 6, cuda):
        assert chk["rng_equal"], "host RNG streams diverged at iteration %d" % it
        assert abs([e["loss"] for t, e in ev if t == "er_loss"][0] - ol["loss"]) < 1e-4
        rr = [e["indices"] for t, e in ev if t == "random_retrieve"]
        assert np.array_equal(rr[0], ol["idx"])
        if "loss_mem" in ol:
            assert abs([e["loss"] for t, e in ev if t == "er_loss_mem"][0] - ol["loss_mem"]) < 1e-4
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"][0] == list(ol["slots"])
        assert _buffers_equal(chk["agent"], chk["oa"])
        worst = max(worst, chk["upd_err"])
        print("er it", it, "update err", chk["upd_err"])
    assert worst < 1e-2


def test_cosim_scr(cuda):
    """BASELINE config 2 shape at small size (SCR, two views, SupCon, identity augmentation on both sides)."""
    cfg = STEP_CASES["scr_c100"]
    worst = 0.0
    for it, ev, ol, chk in cosim(cfg, 5, cuda):
        assert chk["rng_equal"]
        losses = [e["loss"] for t, e in ev if t == "scr_loss"]
        if ol[0] is None:
            assert not losses
        else:
            assert abs(losses[0] - ol[0]) < 1e-4, (losses, ol[0])
        assert np.array_equal([e["indices"] for t, e in ev if t == "random_retrieve"][0], ol[1])
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"][0] == list(ol[2])
        assert _buffers_equal(chk["agent"], chk["oa"])
        worst = max(worst, chk["upd_err"])
        print("scr it", it, "update err", chk["upd_err"])
    assert worst < 1e-2


def _force_mir_gradient(monkeypatch, cuda):
    """MIR evaluates the model at theta - lr*grad: a single ReLU sign flip in the preceding backward (1 element in ~10^6,
    see test_gpu_net) moves every interference score by ~1e-3 relative.  To check the scoring path itself to 1e-4 the
    oracle's gradient vector is handed to the HIP plugin (get_grad_vector is its only input besides the weights)."""
    import ocl_amd.plugins.mir_retrieve as mr
    holder = {}
    monkeypatch.setattr(mr, "get_grad_vector", lambda model: holder["g"])

    def before_hip(olog):
        holder["g"] = olog["grad"].to(cuda).contiguous()
    return before_hip


def test_cosim_mir(cuda, monkeypatch):
    """MIR: identical candidate subsample (numpy RNG), interference scores within 1e-4 (relative to the score scale) of the
    oracle's for the same virtual step, the retrieved set a valid top-k under the ORACLE's scores."""
    hook = _force_mir_gradient(monkeypatch, cuda)
    for name, n_it in (("mir_c10", 5), ("mir_mini", 3)):
        cfg = STEP_CASES[name]
        for it, ev, ol, chk in cosim(cfg, n_it, cuda, before_hip=hook):
            assert chk["rng_equal"]
            assert abs([e["loss"] for t, e in ev if t == "er_loss"][0] - ol["loss"]) < 1e-4 * (1 + abs(ol["loss"]))
            assert np.array_equal([e["indices"] for t, e in ev if t == "random_retrieve"][0], ol["sub"])
            mir_ev = [e for t, e in ev if t == "mir"]
            if "scores" in ol:
                sc, osc = mir_ev[0]["scores"], ol["scores"]
                print(name, "it", it, "score err", np.abs(sc - osc).max(), "scale", np.abs(osc).max())
                assert np.abs(sc - osc).max() < 1e-4 * (1 + np.abs(osc).max()), (name, it, np.abs(sc - osc).max())
                k = len(mir_ev[0]["big_ind"])
                thr = np.sort(osc)[::-1][k - 1]
                assert osc[mir_ev[0]["big_ind"]].min() >= thr - 1e-4 * (1 + abs(thr))
                if set(mir_ev[0]["big_ind"].tolist()) == set(np.argsort(-osc, kind="stable")[:k].tolist()):
                    assert abs([e["loss"] for t, e in ev if t == "er_loss_mem"][0] - ol["loss_mem"]) < 1e-3 * (1 + abs(ol["loss_mem"]))
            else:
                assert not mir_ev
            assert _buffers_equal(chk["agent"], chk["oa"])


def test_mir_free_gradient_scores_close(cuda):
    """Same without forcing the gradient: scores within 1e-2 relative (ReLU-flip sensitivity of the virtual step)."""
    cfg = STEP_CASES["mir_c10"]
    for it, ev, ol, chk in cosim(cfg, 4, cuda):
        mir_ev = [e for t, e in ev if t == "mir"]
        if "scores" in ol:
            assert np.abs(mir_ev[0]["scores"] - ol["scores"]).max() < 1e-2 * (1 + np.abs(ol["scores"]).max())


def _sv_given_order(aux, order, k, feat_tol=1e-4):
    """Near-tie-aware kNN-SV check: the HIP kernel's per-row candidate order must be a valid ascending order of the ORACLE's squared
    distances up to what the feature tolerance allows, and given that order the Shapley values are the oracle's closed form.
    Eval-mode features agree with the oracle's to `feat_tol` of the largest feature (asserted at 1e-4 by
    test_eval_forward_features_vs_oracle, observed ~1e-5), i.e. each feature vector is off by at most e = feat_tol * max|f| * sqrt(D)
    in norm; a squared distance d = |u - v|^2 then moves by at most 4 e sqrt(d) + 4 e^2, so two candidates whose oracle distances
    are closer than the sum of their bounds may legitimately swap (which moves their SVs by a discrete 1/j-sized step -- hence SVs
    are compared under the kernel's own order).  A fixed RELATIVE tolerance would be wrong for near-duplicate pairs (d -> 0)."""
    f_e, y_e, f_c, y_c = aux
    d = O.sq_dist_matrix(f_e, f_c)
    ds = np.take_along_axis(d, order, axis=1).astype(np.float64)
    e = feat_tol * max(np.abs(f_e).max(), np.abs(f_c).max()) * np.sqrt(f_e.shape[1])
    bound = 4 * e * np.sqrt(np.maximum(ds, 0)) + 4 * e * e
    slack = (ds[:, :-1] - ds[:, 1:]) - (bound[:, :-1] + bound[:, 1:])
    worst = np.unravel_index(np.argmax(slack), slack.shape)
    assert slack.max() <= 0, ("kNN order is not an ascending order of the oracle distances within the feature tolerance: d[%d,%d] = %.6g before %.6g "
                              "(allowed %.3g)" % (worst[0], worst[1], ds[worst], ds[worst[0], worst[1] + 1], bound[worst] + bound[worst[0], worst[1] + 1]))
    sv, _ = O.knn_sv(f_e, y_e, f_c, y_c, k, order=order)
    return sv


def test_cosim_aser_tie_aware(cuda):
    """ER + ASER retrieve + ASER update from identical state each step: the class-balanced candidate / evaluation index sets
    are identical (torch RNG, class cache, CPython set order), score vectors within 1e-5, and the HIP selections are valid
    top-N choices under the ORACLE's scores.  Exact SV ties are ubiquitous and torch's argsort is unstable, so once a tie
    is ordered differently the two buffers legitimately differ: the comparison stops there (oracle/synth.py)."""
    cfg = STEP_CASES["aser_c100"]
    eps = 1e-5
    n_ret = n_upd = 0
    for it, ev, ol, chk in cosim(cfg, 16, cuda):
        assert chk["rng_equal"], "host RNG streams diverged at iteration %d" % it
        ret_ev = [e for t, e in ev if t == "aser_retrieve"]
        upd_ev = [e for t, e in ev if t == "aser_update"]
        if ol.get("cand") is not None:
            r = ret_ev[0]
            assert np.array_equal(r["cand_ind"], ol["cand"]), "ASER retrieve: candidate set differs at iteration %d" % it
            sv_adv = _sv_given_order(ol["ret_aux"]["adv"], r["order_adv"], cfg["k"])
            sv_coop = _sv_given_order(ol["ret_aux"]["coop"], r["order_coop"], cfg["k"])
            sv_exp = O.aser_score(sv_adv, sv_coop, cfg.get("aser_type", "asvm"))
            assert np.abs(r["sv"] - sv_exp).max() < eps, np.abs(r["sv"] - sv_exp).max()
            k = len(r["ret"])
            thr = np.sort(sv_exp)[::-1][k - 1]
            pos = {c: j for j, c in enumerate(ol["cand"].tolist())}
            assert min(sv_exp[pos[c]] for c in r["ret"].tolist()) >= thr - eps, "ASER retrieve: not a valid top-%d" % k
            n_ret += 1
        else:
            assert not ret_ev and np.array_equal([e["indices"] for t, e in ev if t == "random_retrieve"][0], ol["ret_idx"])
        assert abs([e["loss"] for t, e in ev if t == "er_loss_combined"][0] - ol["loss"]) < 1e-3 * (1 + abs(ol["loss"])) or ol.get("cand") is not None
        if ol.get("upd") is not None:
            u, ou = upd_ev[0], ol["upd"]
            assert np.array_equal(u["eval_indices"], ou["eval_indices"]) and np.array_equal(u["cand_ind"], ou["cand_ind"])
            assert u["n_minority"] == ou["n_minority"]
            sv_exp = _sv_given_order(ou["aux"], u["knn_order"], cfg["k"]).sum(0)
            assert np.abs(u["sv"] - sv_exp).max() < eps, np.abs(u["sv"] - sv_exp).max()
            n_buf = len(u["cand_ind"])
            thr = np.sort(sv_exp)[::-1][n_buf - 1]
            large, small = u["order"][:n_buf], u["order"][n_buf:]
            assert sv_exp[large].min() >= thr - eps and (len(small) == 0 or sv_exp[small].max() <= thr + eps), "invalid SV partition"
            n_upd += 1
        else:
            assert not upd_ev
        if not _buffers_equal(chk["agent"], chk["oa"]):
            print("legitimate tie divergence at iteration", it)
            break
    print("ASER steps compared: %d retrievals, %d updates" % (n_ret, n_upd))
    assert n_ret >= 1 and n_upd >= 2
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CB
    lab = chk["agent"].buffer.buffer_label.cpu().numpy()
    assert np.array_equal(lab, chk["agent"].buffer.label_host)
    for c, members in CB.class_index_cache.items():
        assert all(lab[i] == c for i in members)
    assert sum(len(m) for m in CB.class_index_cache.values()) == cfg["mem_size"] == int(CB.class_num_cache.sum())


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE.json full sizes
# ---------------------------------------------------------------------------------------------------------------------

def _prefill_fn(n_fill, n_seen, classes, hw, seed):
    def fn(agent, oa):
        rng = np.random.default_rng(seed)
        ys = np.array(classes, dtype=np.int64)[rng.integers(0, len(classes), n_fill)]
        protos = {c: np.random.default_rng(500 + c).random((3, hw, hw)).astype(np.float32) for c in classes}
        xs = 0.5 * rng.random((n_fill, 3, hw, hw), dtype=np.float32)
        for i in range(n_fill):
            xs[i] += 0.5 * protos[int(ys[i])]
        b = agent.buffer
        b.buffer_img[:n_fill] = torch.from_numpy(xs).to(b.buffer_img.device)
        b.buffer_label[:n_fill] = torch.from_numpy(ys).to(b.buffer_label.device)
        b.label_host[:n_fill] = ys
        b.current_index, b.n_seen_so_far = n_fill, n_seen
        oa.buf.img[:n_fill] = torch.from_numpy(xs)
        oa.buf.label[:n_fill] = torch.from_numpy(ys)
        oa.buf.current_index, oa.buf.n_seen_so_far = n_fill, n_seen
    return fn


def test_scr_step_at_baseline_size_vs_oracle(cuda):
    """BASELINE config 2: SCR, mem_size 5000 (full), eps_mem_batch 100, temp 0.07, 110+110 views.  Retrieved indices and
    reservoir slots bit-exact, SupCon loss within 1e-4 (north_star tolerance), buffers bit-identical."""
    cfg = dict(agent="SCR", retrieve="random", update="random", data="cifar100", mem_size=5000, eps_mem_batch=100, seed=21,
               tasks=[list(range(10))], n_train=2, n_test=1, temp=0.07, head="mlp")
    for it, ev, ol, chk in cosim(cfg, 2, cuda, prefill=_prefill_fn(5000, 12345, list(range(10, 40)), 32, 77)):
        assert chk["rng_equal"]
        losses = [e["loss"] for t, e in ev if t == "scr_loss"]
        print("scr full-size losses", losses, ol[0], "update err", chk["upd_err"])
        assert abs(losses[0] - ol[0]) < 1e-4
        rr = [e["indices"] for t, e in ev if t == "random_retrieve"][0]
        assert len(rr) == 100 and np.array_equal(rr, ol[1])
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"][0] == list(ol[2])
        assert _buffers_equal(chk["agent"], chk["oa"])
        assert chk["upd_err"] < 1e-2


def test_aser_knn_path_at_baseline_size_properties(cuda):
    """BASELINE config 3 shapes (mem 5000, 100 classes in the buffer, k=3, n_smp_cls 1.5): full ASER iterations on
    the GPU; checks size-independent properties (class-balanced candidates, permutation, counters, cache consistency)."""
    from ocl_amd import debug
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CB
    cfg = dict(agent="ER", retrieve="ASER", update="ASER", data="cifar100", mem_size=5000, eps_mem_batch=10, seed=31,
               tasks=[list(range(10))], n_train=2, n_test=1, k=3, n_smp_cls=1.5, aser_type="asvm")
    params, model, agent = build_agent(cfg)
    rng = np.random.default_rng(5)
    protos = np.random.default_rng(6).random((100, 3, 32, 32)).astype(np.float32)
    for s in range(0, 5000, 500):
        ys = rng.integers(0, 100, 500)
        xs = (0.5 * protos[ys] + 0.5 * rng.random((500, 3, 32, 32), dtype=np.float32)).astype(np.float32)
        agent.buffer.update(torch.from_numpy(xs).to(cuda), torch.from_numpy(ys).to(cuda), y_host=ys)
    assert agent.buffer.current_index == 5000 and agent.buffer.n_seen_so_far == 5000
    tasks, _ = make_stream(cfg)
    x, y = tasks[0]
    debug.LOG = []
    try:
        agent.train_learner(x, y)       # 2 iterations: update #1 makes n_seen > mem, so iteration 2 retrieves with ASER
        ev = list(debug.LOG)
    finally:
        debug.LOG = None
    ups = [e for t, e in ev if t == "aser_update"]
    rets = [e for t, e in ev if t == "aser_retrieve"]
    assert len(ups) == 2 and len(rets) == 1
    lab = agent.buffer.buffer_label.cpu().numpy()
    assert np.array_equal(lab, agent.buffer.label_host)
    r = rets[0]
    assert len(r["cand_ind"]) == 100 == len(set(r["cand_ind"].tolist()))        # 1 candidate per class, 100 classes
    assert len(r["ret"]) == 10 and set(r["ret"].tolist()) <= set(r["cand_ind"].tolist())
    for u in ups:
        assert len(u["eval_indices"]) == 100 and len(u["cand_ind"]) == 150 and len(u["sv"]) == 160
        assert sorted(u["order"].tolist()) == list(range(160))                  # argsort is a permutation
        assert (np.diff(u["sv"][u["order"]]) <= 0).all()                        # ... in descending score order
        assert len(u["ind_buffer"]) == len(u["ind_cur"]) <= 10
        assert not (set(u["cand_ind"].tolist()) & set(u["eval_indices"].tolist()))
    assert agent.buffer.n_seen_so_far == 5020 and agent.buffer.current_index == 5000
    assert sum(len(m) for m in CB.class_index_cache.values()) == 5000 and int(CB.class_num_cache.sum()) == 5000
    for c, members in CB.class_index_cache.items():
        assert all(lab[i] == c for i in members)


def test_mir_step_at_baseline_size(cuda, monkeypatch):
    """BASELINE config 4: ER + MIR, Mini-ImageNet 84x84, mem_size 10000, subsample 50 -> 10: one iteration vs the oracle."""
    cfg = dict(agent="ER", retrieve="MIR", update="random", data="mini_imagenet", mem_size=10000, eps_mem_batch=10, seed=41,
               tasks=[[3, 4]], n_train=5, n_test=1, subsample=50)
    n_fill = 600                                    # part-filled 10000-slot buffer (the full one is 847 MB on both sides)
    hook = _force_mir_gradient(monkeypatch, cuda)
    for it, ev, ol, chk in cosim(cfg, 1, cuda, prefill=_prefill_fn(n_fill, n_fill, list(range(20, 30)), 84, 78), before_hip=hook):
        assert chk["rng_equal"]
        mir_ev = [e for t, e in ev if t == "mir"][0]
        assert len(mir_ev["scores"]) == 50 and len(mir_ev["big_ind"]) == 10
        assert np.abs(mir_ev["scores"] - ol["scores"]).max() < 1e-4 * (1 + np.abs(ol["scores"]).max())
        thr = np.sort(ol["scores"])[::-1][9]
        assert ol["scores"][mir_ev["big_ind"]].min() >= thr - 1e-4 * (1 + abs(thr))
        assert abs([e["loss"] for t, e in ev if t == "er_loss"][0] - ol["loss"]) < 1e-4 * (1 + abs(ol["loss"]))
        a, o = chk["agent"], chk["oa"]
        assert np.array_equal(a.buffer.buffer_label.cpu().numpy()[:n_fill + 10], o.buf.label.numpy()[:n_fill + 10])
        assert [a.buffer.current_index, a.buffer.n_seen_so_far] == [o.buf.current_index, o.buf.n_seen_so_far]


def test_reference_style_agent_code_runs_on_the_engine(cuda):
    """Drop-in check of the plugin surface: the loop body of the reference's SCR agent, written against nothing but
    model.forward / criterion / opt / buffer.retrieve / buffer.update (two separate forward calls per step, torch's own
    optimizer and zero_grad(set_to_none)), gives the same loss as the batched fast path."""
    cfg = STEP_CASES["scr_c100"]
    params, model, agent = build_agent(cfg)
    tasks, _ = make_stream(cfg)
    x, y = tasks[0]
    agent.train_learner(x[:30], y[:30])          # put something in the buffer
    sd = copy.deepcopy({k: v.clone() for k, v in model.state_dict().items()})
    bx = torch.from_numpy(x[30:40].transpose(0, 3, 1, 2).astype(np.float32) / 255).to(cuda)
    by = torch.from_numpy(y[30:40]).to(cuda)
    np.random.seed(3)
    mem_x, mem_y = agent.buffer.retrieve(x=bx, y=by)
    cx, cy = torch.cat((mem_x, bx)), torch.cat((mem_y, by))
    model.train()
    # fast path
    l_fast = agent.criterion_views(model.forward_views([cx, cx]), cy, 2)
    # reference-style path (agents/scr.py:55-60) with torch.optim.SGD
    model.load_state_dict(sd)
    topt = torch.optim.SGD(model.parameters(), lr=0.1)
    feats = torch.cat([model.forward(cx).unsqueeze(1), model.forward(cx).unsqueeze(1)], dim=1)
    l_ref = agent.criterion(feats, cy)
    assert abs(float(l_fast) - float(l_ref)) < 1e-5
    topt.zero_grad()
    l_ref.backward()
    g = model.flat_grads().clone()
    before = model.flat_params().clone()
    topt.step()
    assert torch.allclose(model.flat_params(), before - 0.1 * g, atol=1e-7)


def _bn_state(model):
    """BatchNorm running statistics and num_batches_tracked (the exact count of train-mode forwards, per layer)."""
    return {k: v.cpu().numpy().copy() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def _assert_bn_state(r1, r0, rel=None):
    """num_batches_tracked exact always; the running statistics exact (rel None) or within `rel` of the tensor's largest element."""
    assert any("num_batches" in k for k in r0)
    for k in r0:
        if rel is None or "num_batches" in k:
            assert np.array_equal(r1[k], r0[k]), k
        else:
            assert np.abs(r1[k] - r0[k]).max() < rel * max(1.0, np.abs(r0[k]).max()), k


# The five schedule-only comparisons below take the loop shape as arguments: the tests of this file run them at epoch 1 / mem_iters 1,
# tests/test_gpu_loops.py at epoch 2 / mem_iters 2 on a third of the samples (as many steps).  n_seen counts every epoch's samples.

def test_scr_data_stream_overlap_is_schedule_only(cuda, monkeypatch):
    """agents/scr.py issues the data path (loader gather, random retrieve, concat, augmentation, reservoir scatter) on its own
    stream so that it runs next to the previous step's backward.  Same statements, same RNG draws: 60 free-running SCR steps
    (real augmentation kernel, buffer filling up and being overwritten) with and without the overlap must end in the same
    replay buffer bit for bit and the same weights up to the order of the fp64 statistic atomics."""
    scr_data_stream_overlap_legs(cuda, monkeypatch, 1, 1, 600)


def scr_data_stream_overlap_legs(cuda, monkeypatch, epoch, mem_iters, n):
    cfg = dict(STEP_CASES["scr_c100"], mem_size=200, epoch=epoch, mem_iters=mem_iters)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 10, n).astype(np.int64)
    finals = []
    for flag in ("1", "0"):
        monkeypatch.setenv("OCL_DATA_STREAM", flag)
        params, model, agent = build_agent(cfg)
        assert (agent.epoch, agent.mem_iters) == (epoch, mem_iters)
        from ocl_amd.agents.scr import ScrAugment
        agent.transform = ScrAugment(size=(32, 32), scale=(0.2, 1.))
        agent.train_learner(torch.from_numpy(x).to(cuda), y)
        torch.cuda.synchronize()
        finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                       agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far, _bn_state(model)))
    (w1, b1, l1, n1, r1), (w0, b0, l0, n0, r0) = finals
    assert n1 == n0 == epoch * n and np.array_equal(l1, l0) and np.array_equal(b1, b0)
    assert np.abs(w1 - w0).max() < 1e-4 * max(1.0, np.abs(w0).max())
    _assert_bn_state({k: v for k, v in r1.items() if "num_batches" in k}, {k: v for k, v in r0.items() if "num_batches" in k})


def test_er_data_stream_overlap_is_schedule_only(cuda, monkeypatch):
    """agents/exp_replay.py (random retrieve / reservoir update, merged two-group pass) issues its data path on the data stream as
    agents/scr.py does.  Same statements, same RNG draws, and the batch sums are order-independent: 60 free-running ER steps (memory
    filling up and being overwritten) with and without the overlap end in the same replay memory AND the same weights, bit for bit."""
    er_data_stream_overlap_legs(cuda, monkeypatch, 1, 1, 600)


def er_data_stream_overlap_legs(cuda, monkeypatch, epoch, mem_iters, n, **over):
    """`over`: further keys of the case (tests/test_gpu_loops.py: batch 8 against eps_mem_batch 12, the non-merged pass with a
    retrieval fetched on the data stream)."""
    from ocl_amd import ops
    ops.set_deterministic(True)   # (bit-identical weights need the order-independent batch sums; restored below)
    cfg = dict(STEP_CASES["er_c10"], mem_size=200, epoch=epoch, mem_iters=mem_iters)
    cfg.update(over)
    batch = cfg.get("batch", 10)
    rng = np.random.default_rng(79)
    x = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 10, n).astype(np.int64)
    finals = []
    try:
        for flag in ("1", "0"):
            monkeypatch.setenv("OCL_DATA_STREAM", flag)
            params, model, agent = build_agent(cfg)
            assert (agent.epoch, agent.mem_iters, agent.batch) == (epoch, mem_iters, batch)
            agent.train_learner(torch.from_numpy(x).to(cuda), y)
            torch.cuda.synchronize()
            finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                           agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far, _bn_state(model)))
    finally:
        ops.set_deterministic(False)   # (also when a step raised: the rest of the session must not run in the integer-sum mode)
    (w1, b1, l1, n1, r1), (w0, b0, l0, n0, r0) = finals
    assert n1 == n0 == epoch * (n // batch) * batch and np.array_equal(l1, l0) and np.array_equal(b1, b0)
    assert np.array_equal(w1, w0)
    _assert_bn_state(r1, r0)


def test_er_merged_step_direct_backward_is_schedule_only(cuda):
    """agents/exp_replay.py::_merged_step hands the engine's backward ONE dL/dlogits buffer whose two row blocks the two cross-entropy
    launches wrote, instead of letting autograd assemble it (two slice-backward fills, two copies, an add, the loss add).  Same numbers
    into the same backward: with order-independent batch sums 60 free-running ER steps end in bit-identical weights, running
    statistics and replay memory on both paths (`_force_autograd` = the autograd path)."""
    er_merged_step_direct_backward_legs(cuda, 1, 1, 600)


def er_merged_step_direct_backward_legs(cuda, epoch, mem_iters, n):
    from ocl_amd import ops
    cfg = dict(STEP_CASES["er_c10"], mem_size=200, epoch=epoch, mem_iters=mem_iters)
    rng = np.random.default_rng(81)
    x = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 10, n).astype(np.int64)
    finals = []
    ops.set_deterministic(True)
    try:
        for force in (False, True):
            params, model, agent = build_agent(cfg)
            assert (agent.epoch, agent.mem_iters) == (epoch, mem_iters)
            agent._force_autograd = force
            agent.train_learner(torch.from_numpy(x).to(cuda), y)
            torch.cuda.synchronize()
            finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                           agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far, _bn_state(model)))
    finally:
        ops.set_deterministic(False)
    (w1, b1, l1, n1, r1), (w0, b0, l0, n0, r0) = finals
    assert n1 == n0 == epoch * n and np.array_equal(l1, l0) and np.array_equal(b1, b0)
    assert np.array_equal(w1, w0)
    _assert_bn_state(r1, r0)


def test_aser_combined_pass_direct_backward_is_schedule_only(cuda):
    """The ASER iteration's combined pass (exp_replay.py:76-84) hands the loss kernel's dL/dlogits straight to the engine's backward instead of
    going through autograd's engine: same numbers into the same backward.  With order-independent batch sums 40 free-running ER + ASER steps
    (memory filling up, then Shapley-ranked retrieval and replacement) end in bit-identical weights, running statistics, replay memory and
    class table on both paths (`_force_autograd` = the autograd path)."""
    from ocl_amd import ops
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CBRS
    cfg = dict(STEP_CASES["aser_c100"])
    rng = np.random.default_rng(79)
    x = rng.integers(0, 256, (400, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 8, 400).astype(np.int64)
    finals = []
    ops.set_deterministic(True)
    try:
        for force in (False, True):
            params, model, agent = build_agent(cfg)
            agent._force_autograd = force
            agent.train_learner(torch.from_numpy(x).to(cuda), y)
            torch.cuda.synchronize()
            finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                           agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far,
                           {k: v.cpu().numpy().copy() for k, v in model.state_dict().items() if "running" in k},
                           {int(k): sorted(v) for k, v in CBRS.class_index_cache.items()}))
    finally:
        ops.set_deterministic(False)
    (w1, b1, l1, n1, r1, c1), (w0, b0, l0, n0, r0, c0) = finals
    assert n1 == n0 == 400 and np.array_equal(l1, l0) and np.array_equal(b1, b0) and c1 == c0
    assert np.array_equal(w1, w0)
    for k in r0:
        assert np.array_equal(r1[k], r0[k]), k


def test_aser_retrieval_feature_pass_split_keeps_the_retrieval(cuda, monkeypatch):
    """plugins/aser_retrieve.py issues the eval-mode feature pass over batch + candidates BEFORE the host draws the cooperative samples
    (OCL_ASER_SPLIT=0: one pass over all three pieces after both draws).  Eval-mode features are per sample and the host draws are the same
    draws in the same order, so the replay memory, the class table and the counters of 40 free-running ER + ASER steps are exactly those of
    the one-pass schedule; the weights agree to rounding (the two schedules run their passes at other batch sizes, i.e. under other plans)."""
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CBRS
    cfg = dict(STEP_CASES["aser_c100"])
    rng = np.random.default_rng(80)
    x = rng.integers(0, 256, (400, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 8, 400).astype(np.int64)
    finals = []
    for flag in ("1", "0"):
        monkeypatch.setenv("OCL_ASER_SPLIT", flag)
        params, model, agent = build_agent(cfg)
        agent.train_learner(torch.from_numpy(x).to(cuda), y)
        torch.cuda.synchronize()
        finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                       agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far,
                       {int(k): sorted(v) for k, v in CBRS.class_index_cache.items()}))
    (w1, b1, l1, n1, c1), (w0, b0, l0, n0, c0) = finals
    assert n1 == n0 == 400 and np.array_equal(l1, l0) and np.array_equal(b1, b0) and c1 == c0
    assert np.abs(w1 - w0).max() <= 1e-3 * max(1.0, np.abs(w0).max())


def test_aser_pipelined_loop_is_schedule_only(cuda, monkeypatch):
    """agents/exp_replay.py issues the batch-pass forward of iteration i+1 before the host half of iteration i's ASER update (wait
    for the ranking, class table, row moves).  Same kernels on the same data, same RNG draws: 40 free-running ER + ASER steps
    (memory filling up, then Shapley-ranked replacement and retrieval) with and without the pipelining must end in the same replay
    memory, class table and counters exactly, and the same weights up to the order of the fp64 statistic atomics."""
    aser_pipelined_loop_legs(cuda, monkeypatch, 1, 1, 400)


def aser_pipelined_loop_legs(cuda, monkeypatch, epoch, mem_iters, n):
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CBRS
    cfg = dict(STEP_CASES["aser_c100"], epoch=epoch, mem_iters=mem_iters)
    rng = np.random.default_rng(78)
    x = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 8, n).astype(np.int64)
    finals = []
    for flag in ("1", "0"):
        monkeypatch.setenv("OCL_ASER_PIPELINE", flag)
        params, model, agent = build_agent(cfg)
        assert (agent.epoch, agent.mem_iters) == (epoch, mem_iters)
        agent.train_learner(torch.from_numpy(x).to(cuda), y)
        torch.cuda.synchronize()
        table = {int(k): sorted(v) for k, v in CBRS.class_index_cache.items()}
        finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                       agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far, table, _bn_state(model)))
    (w1, b1, l1, n1, t1, r1), (w0, b0, l0, n0, t0, r0) = finals
    assert n1 == n0 == epoch * n and np.array_equal(l1, l0) and np.array_equal(b1, b0) and t1 == t0
    assert np.abs(w1 - w0).max() < 1e-4 * max(1.0, np.abs(w0).max())
    _assert_bn_state(r1, r0, rel=1e-4)


def test_aser_passes_without_readers_are_schedule_only(cuda):
    """ER + ASER: the batch pass and the memory pass of an iteration only leave their BatchNorm running-statistic updates behind (the
    reference throws their gradients away, agents/exp_replay.py:76).  Without a reader of their logits / losses the loop runs them as
    model.forward_stats_only (no head, no loss kernels, no tape), the retrieval's two Shapley matrices come out of ONE kNN launch, and
    the engine packs the weights once per optimiser step (OCL_FWD_SAME_WEIGHTS).  Against the readers' path (`_force_losses`: full
    forwards under autograd + both losses, as the co-simulations run it), with order-independent batch sums: 40 free-running steps
    (memory filling up, then Shapley-ranked replacement and retrieval) end in the same weights, running statistics, replay memory,
    class table and counters BIT FOR BIT."""
    aser_passes_without_readers_legs(cuda, 1, 1, 400)


def aser_passes_without_readers_legs(cuda, epoch, mem_iters, n):
    from ocl_amd import ops
    from ocl_amd.plugins.buffer_utils import ClassBalancedRandomSampling as CBRS
    cfg = dict(STEP_CASES["aser_c100"], epoch=epoch, mem_iters=mem_iters)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 8, n).astype(np.int64)
    finals = []
    ops.set_deterministic(True)
    try:
        for force in (False, True):
            params, model, agent = build_agent(cfg)
            assert (agent.epoch, agent.mem_iters) == (epoch, mem_iters)
            agent._force_losses = force
            agent.train_learner(torch.from_numpy(x).to(cuda), y)
            torch.cuda.synchronize()
            table = {int(k): sorted(v) for k, v in CBRS.class_index_cache.items()}
            finals.append((model.flat_params().cpu().numpy().copy(), agent.buffer.buffer_img.cpu().numpy().copy(),
                           agent.buffer.buffer_label.cpu().numpy().copy(), agent.buffer.n_seen_so_far, table, _bn_state(model)))
    finally:
        ops.set_deterministic(False)
    (w1, b1, l1, n1, t1, r1), (w0, b0, l0, n0, t0, r0) = finals
    assert n1 == n0 == epoch * n and np.array_equal(l1, l0) and np.array_equal(b1, b0) and t1 == t0
    assert np.array_equal(w1, w0)
    _assert_bn_state(r1, r0)


def test_kd_trick_teacher_and_combined_loss_vs_oracle(cuda):
    """KD trick (agents/exp_replay.py:42-44,64-66, utils/kd_manager.py): after the first task the teacher is the end-of-task
    model; its train-mode forward (batch statistics, no effect on the student's running statistics) and the combined loss
    1/(t+1) * CE + (1 - 1/(t+1)) * KD and its gradient w.r.t. the student logits against the oracle (torch-CPU autograd);
    then one more task runs through the KD branches of the ER loop."""
    cfg = STEP_CASES["er_c10"]
    trick = dict(TRICK, kd_trick=True)
    params, model, agent = build_agent(cfg, trick=trick)
    tasks, _ = make_stream(cfg)
    x0, y0 = tasks[0]
    assert agent.kd_manager.teacher_model is None
    agent.train_learner(x0[:40], y0[:40])
    teacher = agent.kd_manager.teacher_model
    assert teacher is not None and agent.task_seen == 1 and torch.equal(teacher, model.flat_params())
    sd_teacher = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    # move the student away from the teacher
    with torch.no_grad():
        model.flat_params().mul_(1.01)
    running_before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
    x1, y1 = tasks[1]
    bx = torch.from_numpy(x1[:10].transpose(0, 3, 1, 2).astype(np.float32) / 255)
    by = torch.from_numpy(y1[:10])
    model.train()
    with torch.no_grad():
        t_logits = model.forward_with_params(bx.to(cuda), teacher)
    t_ref = O.OracleNet(O.clone_state(sd_teacher, requires_grad=False), head=None, training=True)
    with torch.no_grad():
        t_logits_ref = t_ref.forward(bx)
    assert np.abs(t_logits.cpu().numpy() - t_logits_ref.numpy()).max() < 1e-4 * max(1.0, float(t_logits_ref.abs().max()))
    for k, v in running_before.items():
        assert torch.equal(model.state_dict()[k], v), "teacher forward touched the student's %s" % k
    # combined loss on leaf logits: kernels + autograd glue
    rng = np.random.default_rng(3)
    lg = (2.0 * rng.standard_normal((10, 10))).astype(np.float32)
    a = 1 / (agent.task_seen + 1)
    lt = torch.from_numpy(lg).to(cuda).requires_grad_(True)
    loss = a * agent.criterion(lt, by.to(cuda)) + (1 - a) * agent.kd_manager.get_kd_loss(lt, bx.to(cuda))
    loss.backward()
    lr = torch.from_numpy(lg).requires_grad_(True)
    loss_ref = a * O.ce_mean(lr, by) + (1 - a) * O.loss_fn_kd(lr, t_logits_ref)
    loss_ref.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-4
    assert np.abs(lt.grad.cpu().numpy() - lr.grad.numpy()).max() < 1e-4
    # the ER loop with the KD branches (batch and memory passes), second task
    agent.train_learner(x1[:40], y1[:40])
    assert agent.task_seen == 2 and torch.isfinite(model.flat_params()).all()
    assert not torch.equal(agent.kd_manager.teacher_model, teacher)
