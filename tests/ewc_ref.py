"""Helper of tests/test_cpu_ewc.py, tests/test_gpu_ewc.py and scripts/make_ewc_golden.py (no tests here): the float64 statements of the
three EWC++ kernels (csrc/ewc.hip) with their fp32 round-off bounds, the float32 statements two of them must reproduce bit for bit, and
one iteration of the reference's agents/ewc_pp.py:33-63 restated over the functions of oracle/ocl_oracle.py."""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, case_params, digest_state, digest_nbt

U = 2.0 ** -24      # half an fp32 ulp, relative
TINY = 2.0 ** -149  # the smallest fp32 denormal: what a result that underflows can be off by

# the free-running case of tests/golden/ewc.npz: ER's er_c10 with a third task (two tasks carry a penalty) and the EWC++ agent.  At
# learning_rate 0.1 and lambda_ 100 the reference itself diverges in its second task; at 0.01 the weights stay at |w| ~ 44.8.
EWC_CASE = dict(STEP_CASES["er_c10"], agent="EWC", seed=14, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20, lambda_=100, alpha=0.9,
                fisher_update_after=2, learning_rate=0.01, lr=0.01)
EWC_KEYS = ("lambda_", "alpha", "fisher_update_after", "learning_rate")
FISHER_KEYS = ("running", "tmp", "normalized", "prev")
GOLDEN_KEYS = ("acc", "state", "minmax") + FISHER_KEYS
# two epochs of three batches with the running Fisher updated after every second iteration, counted ACROSS the epochs
# (ewc_pp.py:41: (ep * len(train_loader) + i + 1) % fisher_update_after): iterations 1 | 3 and 5 of a task, i.e. i = 1 in the first epoch
# and i = 0, 2 in the second; recorded as `ewc_loops`
EWC_LOOPS_CASE = dict(EWC_CASE, seed=15, tasks=[[0, 1], [2, 3]], n_train=15, epoch=2)
LOOPS_KEYS = GOLDEN_KEYS + ("nbt", "ema_at")      # + num_batches_tracked per BatchNorm, + the task's iterations (0-based) that began with the update


def ref_params(cfg):
    """The keyword arguments of oracle.ref_import.default_params / of the agent's params for the case."""
    return dict(case_params(cfg), **{k: cfg[k] for k in EWC_KEYS})


# ---- the accumulate step in float64 ----------------------------------------------------------------------------------------------------

def ref_accumulate(g, t, p=None, q=None, f=None, scale=0.0):
    """ewc_pp.py:83-92 differentiated, and :104-106, in float64: d = p - q, pg = scale * f * d, g1 = g + pg, t1 = t + g1 * g1,
    penalty = sum f * d * d.  With p, q, f None (first task): pg = 0, penalty = 0."""
    g, t = np.asarray(g, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if q is None:
        pg, penalty = np.zeros_like(g), 0.0
    else:
        p, q, f = (np.asarray(a, dtype=np.float64) for a in (p, q, f))
        d = p - q
        pg = float(scale) * f * d
        penalty = float((f * d * d).sum())
    g1 = g + pg
    return SimpleNamespace(g=g, t=t, pg=pg, g1=g1, t1=t + g1 * g1, penalty=penalty, has_prev=q is not None and float(scale) != 0.0)


def accumulate_bounds(ref):
    """Per-element bounds (eg, et) on |g1_fp32 - g1| and |t1_fp32 - t1|, first order in U = 2^-24.
    g1: d = fl(p - q), scale * f and their product are rounded once each, 3 U |pg| together; the sum g + pg is rounded once, at most
    U (|g| + |pg|).  eg = U (|g| + 4 |pg|); zero where no penalty is added (g is not rewritten).
    t1: g1's error moves the square by 2 |g1| eg; the square is rounded once (U g1^2) and so is the sum (U (|t| + g1^2)).
    et = 2 |g1| eg + U (|t| + 2 g1^2).  Both carry one denormal for a product that underflows."""
    eg = U * (np.abs(ref.g) + 4.0 * np.abs(ref.pg)) + TINY if ref.has_prev else np.zeros_like(ref.g)
    et = 2.0 * np.abs(ref.g1) * eg + U * (np.abs(ref.t) + 2.0 * ref.g1 * ref.g1) + TINY
    return eg, et


def worst_ratios(g_got, t_got, ref):
    """(max |g_got - g1| / eg, max |t_got - t1| / et): 0 where both are zero, inf where a zero bound is exceeded."""
    out = []
    for got, want, e in zip((g_got, t_got), (ref.g1, ref.t1), accumulate_bounds(ref)):
        d = np.abs(np.asarray(got, dtype=np.float64) - want)
        out.append(float(np.divide(d, e, out=np.where(d > 0, np.inf, 0.0), where=e > 0).max()))
    return tuple(out)


def make_case(rng, n, make_grads, prev=True):
    """Inputs of one accumulate call: g and p with make_grads' magnitudes, t = a square of such, q = p moved by 1e-3 |p|, f in [0, 1]
    with exact zeros and exact ones present (where n allows)."""
    g, p = make_grads(rng, n, 1), make_grads(rng, n, 1)
    t = (make_grads(rng, n, 1).astype(np.float64) ** 2).astype(np.float32)
    if not prev:
        return SimpleNamespace(g=g, t=t, p=p, q=None, f=None)
    q = (p.astype(np.float64) * (1.0 + 1e-3 * rng.standard_normal(n))).astype(np.float32)
    f = rng.random(n).astype(np.float32)
    f[rng.random(n) < 0.1] = 0.0
    f[rng.random(n) < 0.05] = 1.0
    if n >= 3:
        f[0], f[n - 1] = 0.0, 1.0
    return SimpleNamespace(g=g, t=t, p=p, q=q, f=f)


# ---- the moving average and the normalisation ----------------------------------------------------------------------------------------

def ema_f32(r, t, keep, gain):
    """ewc_pp.py:99-100 as float32 arithmetic: both scalars rounded to float32, two products and one sum, each rounded."""
    r, t = np.asarray(r, dtype=np.float32), np.asarray(t, dtype=np.float32)
    out = np.float32(keep) * r + np.float32(gain) * t
    assert out.dtype == np.float32
    return out


def ref_ema(r, t, keep, gain):
    """The same in float64 (from the float32 scalars) and its bound: U on each product and U on the sum."""
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    a, b = float(np.float32(keep)) * r, float(np.float32(gain)) * t
    return a + b, U * (2.0 * (np.abs(a) + np.abs(b))) + TINY


def normalize_f32(r):
    """ewc_pp.py:77-80 as float32 arithmetic over the whole array: (r - min) / (max - min + 1e-32); numpy's min and max keep a NaN."""
    r = np.asarray(r, dtype=np.float32)
    lo, hi = r.min(), r.max()
    with np.errstate(invalid="ignore"):
        out = (r - lo) / (hi - lo + np.float32(1e-32))
    assert out.dtype == np.float32
    return out, np.array([lo, hi], dtype=np.float32)


def ref_normalize(r):
    """The same in float64 and its bound: numerator and denominator are each rounded once (the 1e-32 vanishes unless max == min),
    the quotient once: 3 U |out|, plus the numerator's cancellation U |r - min| / den, which the first term covers."""
    r = np.asarray(r, dtype=np.float64)
    lo, hi = r.min(), r.max()
    out = (r - lo) / (hi - lo + float(np.float32(1e-32)))
    return out, 3.0 * U * np.abs(out) + TINY


# ---- one iteration of the reference agent ------------------------------------------------------------------------------------------------

def init_fisher(state, names):
    """ewc_pp.py:94-95."""
    return OrderedDict((n, state[n].clone().detach().fill_(0)) for n in names)


def ewc_step(state, names, ewc, bx, by, lr, lambda_, kd=None):
    """agents/ewc_pp.py:44-63 for ONE stream batch: forward, total_loss (:83-92: CE, plus lambda_ * sum f_hat * (p - prev)^2 once a task
    has ended), the KD tricks' blend of the whole loss, backward, tmp_fisher += grad^2, SGD step.  ewc: namespace of the four
    dictionaries (prev, running, tmp, normalized).  kd(loss, logits, x) -> loss."""
    net = O.OracleNet(state, head=None, training=True)
    logits = net.forward(bx)
    loss = O.ce_mean(logits, by)
    ce = float(loss.detach())
    penalty = 0.0
    if len(ewc.prev) > 0:
        reg_loss = 0
        for n in names:
            reg_loss += (ewc.normalized[n] * (state[n] - ewc.prev[n]) ** 2).sum()
        loss = loss + lambda_ * reg_loss
        penalty = float(reg_loss.detach())
    if kd is not None:
        loss = kd(loss, logits, bx)
    O.zero_grad(state, names)
    loss.backward()
    with torch.no_grad():
        for n in names:
            ewc.tmp[n] += state[n].grad ** 2
    O.sgd_step(state, names, lr)
    return dict(ce=ce, penalty=penalty, loss=float(loss.detach()))


class EwcOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, evaluate) with ewc_pp.py:20-81 as its train_learner."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.p["lr"] = cfg["learning_rate"]
        self.lambda_, self.alpha, self.fisher_update_after = cfg["lambda_"], cfg["alpha"], cfg["fisher_update_after"]
        self.ewc = SimpleNamespace(prev=OrderedDict(), running=init_fisher(self.state, self.names), tmp=init_fisher(self.state, self.names),
                                   normalized=init_fisher(self.state, self.names))
        self.minmax = []
        self.ema_at = []            # per train_learner call: the iterations (0-based, counted over the epochs) that began with the moving average

    def update_running_fisher(self):
        e = self.ewc
        for n in self.names:
            e.running[n] = (1. - self.alpha) * e.running[n] + 1. / self.fisher_update_after * self.alpha * e.tmp[n]
        e.tmp = init_fisher(self.state, self.names)

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        kd = self._kd_mix if (self.trick.get("kd_trick") or self.trick.get("kd_trick_star")) else None
        e = self.ewc
        self.ema_at.append([])
        for ep in range(self.epoch):                               # ewc_pp.py:33: a fresh permutation per epoch
            for i, idx in enumerate(loader):
                ema = (ep * len(loader) + i + 1) % self.fisher_update_after == 0          # :41
                if ema:
                    self.update_running_fisher()
                    self.ema_at[-1].append(ep * len(loader) + i)
                self.log.append(dict(ewc_step(self.state, self.names, e, xs[idx], ys[idx], self.p["lr"], self.lambda_, kd=kd), ema=ema))
        for n in self.names:
            e.prev[n] = self.state[n].clone().detach()
        max_fisher = max([torch.max(m) for m in e.running.values()])
        min_fisher = min([torch.min(m) for m in e.running.values()])
        for n in self.names:
            e.normalized[n] = (e.running[n] - min_fisher) / (max_fisher - min_fisher + 1e-32)
        self.minmax.append([float(min_fisher), float(max_fisher)])
        self.after_train(new)

    def flat(self, which):
        """One of the four dictionaries as a float32 vector in parameter order (prev: None before the first task ends)."""
        d = getattr(self.ewc, which)
        return None if len(d) == 0 else torch.cat([d[n].detach().reshape(-1) for n in self.names])


def record(acc, state_dict, running, tmp, normalized, prev, ema_at=()):
    """What the golden file keeps per task: the accuracies, the digest_state rows of the model and of the four dictionaries, and the
    running Fisher's [min, max]; for ewc_loops also num_batches_tracked and the iterations that began with the moving average."""
    return dict(acc=np.asarray(acc, dtype=np.float64), state=digest_state(state_dict), nbt=digest_nbt(state_dict),
                ema_at=np.asarray(list(ema_at), dtype=np.int64),
                minmax=np.array([min(float(v.min()) for v in running.values()), max(float(v.max()) for v in running.values())]),
                running=digest_state(running), tmp=digest_state(tmp), normalized=digest_state(normalized), prev=digest_state(prev))


def run_oracle_case(cfg=None, tasks_only=None):
    """The free run of EwcOracle over the case's tasks: per-task records, and the agent (its .log holds every iteration)."""
    cfg = EWC_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    ag = EwcOracle(cfg)
    tasks, tests = make_stream(cfg)
    recs = []
    for x, y in tasks[:tasks_only]:
        ag.train_learner(x, y)
        acc = ag.evaluate(tests)
        recs.append(record(acc, ag.state_dict(), ag.ewc.running, ag.ewc.tmp, ag.ewc.normalized, ag.ewc.prev, ema_at=ag.ema_at[-1]))
    return recs, ag


def cosim_stream(cfg=None):
    """The co-simulation's stream: the case's tasks concatenated, to be cut into sequential slices of 20 (two batches per call)."""
    cfg = EWC_CASE if cfg is None else cfg
    tasks, _ = make_stream(cfg)
    return np.concatenate([x for x, _ in tasks], 0), np.concatenate([y for _, y in tasks], 0)
