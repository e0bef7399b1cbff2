"""Helper of tests/test_cpu_agem.py, tests/test_gpu_agem.py and scripts/make_agem_golden.py (no tests here): the float64 statement of
A-GEM's projection with its fp32 round-off bound, and one iteration of the reference's agents/agem.py:38-83 restated over the
functions of oracle/ocl_oracle.py."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all

U = 2.0 ** -24      # half an fp32 ulp, relative

# the free-running case of tests/golden/agem.npz: ER's er_c10 with a third task (two tasks see memory) and the A-GEM agent
AGEM_CASE = dict(STEP_CASES["er_c10"], agent="AGEM", seed=14, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20, mem_size=50,
                 eps_mem_batch=10)
GOLDEN_KEYS = ("acc", "buf_label", "buf_rowsum", "counters", "state")
# the nested loops of agents/agem.py:32-38: two epochs of three batches, two memory iterations per batch (each with a draw from the
# memory and a projection of its own from the second task on), ONE reservoir update after them; recorded as `agem_loops`
AGEM_LOOPS_CASE = dict(AGEM_CASE, seed=15, tasks=[[0, 1], [2, 3]], n_train=15, epoch=2, mem_iters=2)
LOOPS_KEYS = GOLDEN_KEYS + ("nbt",)          # + num_batches_tracked of every BatchNorm: the count of train-mode forwards


# ---- the projection in float64 ---------------------------------------------------------------------------------------------------------

def ref_project(g, r):
    """agents/agem.py:72-80 in float64: prod = sum g*r, prod_ref = sum r*r, out = g - prod / prod_ref * r where prod < 0, else g.
    S_abs = sum |g*r| (what the rounding of the sum is relative to)."""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    gr = g * r
    prod, prod_ref, s_abs = float(gr.sum()), float((r * r).sum()), float(np.abs(gr).sum())
    projected = bool(prod < 0)
    coef = prod / prod_ref if projected else 0.0
    out = g - coef * r if projected else g.copy()
    return SimpleNamespace(g=g, r=r, prod=prod, prod_ref=prod_ref, projected=projected, coef=coef, out=out, S_abs=s_abs)


def project_bound(ref):
    """Per-element bound on |out_fp32 - out|: one half-ulp (U = 2^-24) each for the coefficient rounded to float, the product coef*r and
    the subtraction (at most U * (|g| + |coef*r|)), and the double accumulation of prod (2^-40 relative to S_abs, and to prod_ref) moved
    through coef.  Zero where nothing is projected: the output is g itself."""
    if not ref.projected:
        return np.zeros_like(ref.out)
    cr = np.abs(ref.coef * ref.r)
    return U * (np.abs(ref.g) + 3.0 * cr) + cr * 2.0 ** -40 * (ref.S_abs / abs(ref.prod) + 1.0)


def worst_ratio(got, ref):
    """max |got - ref.out| / bound (0 where both are zero, inf where a zero bound is exceeded)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref.out)
    e = project_bound(ref)
    return float(np.divide(d, e, out=np.where(d > 0, np.inf, 0.0), where=e > 0).max())


def with_cosine(rng, r, cos):
    """A float32 vector whose cosine against r (float32, magnitudes as make_grads) is `cos` up to the rounding to float32: r's
    direction times cos plus a random direction orthogonal to r times sqrt(1 - cos^2), at r's norm."""
    r64 = np.asarray(r, dtype=np.float64)
    nr = np.linalg.norm(r64)
    z = rng.standard_normal(r64.shape[0]) * np.abs(r64)
    if r64.shape[0] > 1:
        z -= (z @ r64) / (nr * nr) * r64
        z /= np.linalg.norm(z)
    else:
        z[:] = 0.0
    return (nr * (cos * r64 / nr + np.sqrt(max(0.0, 1.0 - cos * cos)) * z)).astype(np.float32)


# ---- one iteration of the reference agent ------------------------------------------------------------------------------------------------

def agem_step(state, names, buf, bx, by, eps, lr, task_seen, kd=None, update=True):
    """agents/agem.py:38-83 for ONE stream batch (mem_iters 1; update=False: one pass of the mem_iters loop, :39-81, slots None): batch pass; from the second task on a uniform draw from the memory,
    the memory pass and the reference's own fp32 projection statements (per-tensor torch.sum, the builtin sum, g - prod / prod_ref * g_r);
    SGD step; reservoir update.  kd(loss, logits, x) -> loss: the KD tricks' blend (:41-46)."""
    net = O.OracleNet(state, head=None, training=True)
    logits = net.forward(bx)
    loss = O.ce_mean(logits, by)
    if kd is not None:
        loss = kd(loss, logits, bx)
    O.zero_grad(state, names)
    loss.backward()
    info = dict(loss=float(loss.detach()), loss_mem=None, idx=np.zeros(0, dtype=np.int64), projected=False, coef=0.0, cos=None)
    if task_seen > 0:
        idx = O.random_retrieve_indices(buf, eps)
        info["idx"] = idx
        if idx.shape[0] > 0:
            params = [state[n] for n in names]
            grad = [p.grad.clone() for p in params]
            g64 = O.flat_grad(state, names).double()
            mem_logits = net.forward(buf.img[idx])
            loss_mem = O.ce_mean(mem_logits, buf.label[idx])
            O.zero_grad(state, names)
            loss_mem.backward()
            grad_ref = [p.grad.clone() for p in params]
            r64 = O.flat_grad(state, names).double()
            prod = sum([torch.sum(g * g_r) for g, g_r in zip(grad, grad_ref)])
            if prod < 0:
                prod_ref = sum([torch.sum(g_r ** 2) for g_r in grad_ref])
                grad = [g - prod / prod_ref * g_r for g, g_r in zip(grad, grad_ref)]
                info["projected"], info["coef"] = True, float(prod / prod_ref)
            for g, p in zip(grad, params):
                p.grad.data.copy_(g)
            info["loss_mem"] = float(loss_mem.detach())
            info["cos"] = float((g64 @ r64) / (g64.norm() * r64.norm()))
    O.sgd_step(state, names, lr)
    info["slots"] = O.reservoir_update(buf, bx, by) if update else None
    return info


class AgemOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, loader, evaluate) with agem_step as its iteration."""

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        kd = self._kd_mix if (self.trick.get("kd_trick") or self.trick.get("kd_trick_star")) else None
        for ep in range(self.epoch):                     # agem.py:32: a fresh permutation per epoch
            for idx in loader:
                parts = [agem_step(self.state, self.names, self.buf, xs[idx], ys[idx], self.p["eps_mem_batch"], self.p["lr"],
                                   self.task_seen, kd=kd, update=False) for j in range(self.mem_iters)]      # :38
                slots = O.reservoir_update(self.buf, xs[idx], ys[idx])                                       # :83, once per batch
                if self.mem_iters == 1:
                    self.log.append(dict(parts[0], slots=slots))
                else:                                    # per-j lists
                    self.log.append(dict({k: [p[k] for p in parts] for k in parts[0] if k != "slots"}, slots=slots))
        self.after_train(new)


def record(acc, buf_label, buf_img, current_index, n_seen_so_far, state_dict):
    """What the golden file keeps per task (the arrays of oracle/make_golden.py's step cases)."""
    from oracle.synth import digest_state, digest_nbt
    return dict(acc=np.asarray(acc, dtype=np.float64), buf_label=np.asarray(buf_label).copy(),
                buf_rowsum=buf_img.double().sum(dim=(1, 2, 3)).cpu().numpy(),
                counters=np.array([current_index, n_seen_so_far], dtype=np.int64), state=digest_state(state_dict),
                nbt=digest_nbt(state_dict))


def run_oracle_case(cfg=None):
    """The free run of agem_step over the case's tasks: per-task records, and the agent (its .log holds every iteration)."""
    cfg = AGEM_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    ag = AgemOracle(cfg)
    tasks, tests = make_stream(cfg)
    recs = []
    for x, y in tasks:
        ag.train_learner(x, y)
        acc = ag.evaluate(tests)
        recs.append(record(acc, ag.buf.label.numpy(), ag.buf.img, ag.buf.current_index, ag.buf.n_seen_so_far, ag.state_dict()))
    return recs, ag


def cosim_stream(cfg=None):
    """The co-simulation's stream: the case's tasks concatenated, to be cut into sequential slices of 10."""
    cfg = AGEM_CASE if cfg is None else cfg
    tasks, _ = make_stream(cfg)
    return np.concatenate([x for x, _ in tasks], 0), np.concatenate([y for _, y in tasks], 0)


def cosim_oracle(cfg=None, n_iters=18):
    """The oracle side of the co-simulation on its own: one train_learner-shaped call per slice of 10, seed_all(1000 + seed) before
    the first.  Returns the agent (its .log: one entry per slice)."""
    cfg = AGEM_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    oa = AgemOracle(cfg)
    xs, ys = cosim_stream(cfg)
    seed_all(1000 + cfg["seed"])
    for it in range(n_iters):
        oa.train_learner(xs[it * 10:(it + 1) * 10], ys[it * 10:(it + 1) * 10])
    return oa
