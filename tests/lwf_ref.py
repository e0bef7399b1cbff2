"""Helper of tests/test_cpu_lwf.py, tests/test_gpu_lwf.py and scripts/make_lwf_golden.py (no tests here): the float64 statement of the
blended cross-entropy + distillation kernel (csrc/distill.hip, ocl_ce_kd_blend_fwd_bwd), the same formula in plain torch-CPU float32 (the
e_ref of parity_bounds.check_vs_torch32), and one iteration of the reference's agents/lwf.py:36-48 restated over the functions of
oracle/ocl_oracle.py."""
import numpy as np
import torch

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, case_params, digest_state

# the free-running case of tests/golden/lwf.npz: ER's er_c10 with a third task (two tasks carry a teacher) and the LwF agent
LWF_CASE = dict(STEP_CASES["er_c10"], agent="LWF", seed=17, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20)
GOLDEN_KEYS = ("acc", "state")
RECORDED_STEPS = 2          # the golden keeps loss_new / loss_old of the first two steps of each task


def ref_params(cfg):
    """The keyword arguments of oracle.ref_import.default_params / of the agent's params for the case."""
    return case_params(cfg)


# ---- the kernel's statement in float64 ----------------------------------------------------------------------------------------------------

def _log_softmax64(x):
    m = x.max(axis=1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))


def ref_blend(logits, y, teacher, T, w_new, w_old):
    """(loss3, dlogits) in float64 from the float32 inputs and the float32 roundings of T and of the two weights (what the entry point
    receives):  ce = mean_r(lse(s_r) - s_r[y_r]);  kd = mean_r(-sum_j softmax(t_r / T)_j * log_softmax(s_r / T)_j) * T^2;
    loss3 = [w_new * ce + w_old * kd, ce, kd];
    dlogits = w_new * (softmax(s) - onehot(y)) / n + w_old * (softmax(s / T) - softmax(t / T)) * T / n.  teacher None: kd = 0."""
    s = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    T, w_new, w_old = (float(np.float32(v)) for v in (T, w_new, w_old))
    n = s.shape[0]
    rows = np.arange(n)
    ls = _log_softmax64(s)
    ce = float(-ls[rows, y].mean())
    onehot = np.zeros_like(s)
    onehot[rows, y] = 1.0
    dl = w_new * (np.exp(ls) - onehot) / n
    kd = 0.0
    if teacher is not None:
        t = np.asarray(teacher, dtype=np.float64)
        lsT, pt = _log_softmax64(s / T), np.exp(_log_softmax64(t / T))
        kd = float((-pt * lsT).sum(axis=1).mean() * T * T)
        dl = dl + w_old * (np.exp(lsT) - pt) * T / n
    return np.array([w_new * ce + w_old * kd, ce, kd]), dl


def torch32_blend(logits, y, teacher, T, w_new, w_old):
    """The same formula as plain torch-CPU float32 statements (the reference's own: F.cross_entropy, loss_fn_kd, the blend of
    agents/lwf.py:39) with autograd's gradient: (loss3, dlogits) as float32 numpy."""
    s = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).requires_grad_(True)
    yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64))
    w_new, w_old = float(np.float32(w_new)), float(np.float32(w_old))
    ce = O.ce_mean(s, yt)
    if teacher is None:
        kd = torch.zeros(())
        loss = w_new * ce
    else:
        kd = O.loss_fn_kd(s, torch.from_numpy(np.ascontiguousarray(teacher, dtype=np.float32)), float(np.float32(T)))
        loss = w_new * ce + w_old * kd
    loss.backward()
    return np.array([float(loss.detach()), float(ce.detach()), float(kd.detach())], dtype=np.float32), s.grad.numpy()


def logits_for(rng, n, c, scale):
    """Random logits times `scale`; the second-to-last row has one dominant logit, the last row equal logits (where n allows): the rows of
    the CE family's cases (tests/test_gpu_small_ops.py)."""
    x = (rng.standard_normal((n, c)) * scale).astype(np.float32)
    if n >= 3:
        x[n - 2, rng.integers(0, c)] += np.float32(60.0 * scale)
        x[n - 1, :] = np.float32(0.5 * scale)
    return x


# ---- one iteration of the reference agent ------------------------------------------------------------------------------------------------

def lwf_step(state, names, teacher, task_seen, bx, by, lr):
    """agents/lwf.py:36-48 for ONE stream batch: forward, the distillation loss against the teacher (a cloned state forwarded in train
    mode under no_grad, kd_manager.py:21-28; 0 without one), CE, the blend, backward, SGD step."""
    net = O.OracleNet(state, head=None, training=True)
    logits = net.forward(bx)
    if teacher is not None:
        with torch.no_grad():
            t_logits = O.OracleNet(teacher, head=None, training=True).forward(bx)
        loss_old = O.loss_fn_kd(logits, t_logits)
    else:
        loss_old = 0
    loss_new = O.ce_mean(logits, by)
    loss = 1 / (task_seen + 1) * loss_new + (1 - 1 / (task_seen + 1)) * loss_old
    O.zero_grad(state, names)
    loss.backward()
    O.sgd_step(state, names, lr)
    return dict(loss=float(loss.detach()), loss_new=float(loss_new.detach()), loss_old=float(loss_old.detach()) if torch.is_tensor(loss_old) else 0.0,
                teacher=teacher is not None)


class LwfOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, evaluate) with agents/lwf.py:14-56 as its train_learner; after every task the teacher is a
    clone of the state (base.py:90-91 with params.agent == 'LWF'), whatever the KD tricks say."""

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        for idx in loader:
            self.log.append(lwf_step(self.state, self.names, self.teacher, self.task_seen, xs[idx], ys[idx], self.p["lr"]))
        self.after_train(new)
        self.teacher = O.clone_state(self.state, requires_grad=False)


def record(acc, state_dict):
    """What the golden file keeps per task: the accuracies and the digest_state rows of the model."""
    return dict(acc=np.asarray(acc, dtype=np.float64), state=digest_state(state_dict))


def run_oracle_case(cfg=None, tasks_only=None):
    """The free run of LwfOracle over the case's tasks: per-task records, and the agent (its .log holds every iteration)."""
    cfg = LWF_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    ag = LwfOracle(cfg)
    tasks, tests = make_stream(cfg)
    recs = []
    for x, y in tasks[:tasks_only]:
        ag.train_learner(x, y)
        recs.append(record(ag.evaluate(tests), ag.state_dict()))
    return recs, ag


def recorded_losses(log, steps_per_task):
    """[n_tasks, RECORDED_STEPS, 2]: (loss_new, loss_old) of the first RECORDED_STEPS iterations of every task."""
    rows = [[[log[t * steps_per_task + k]["loss_new"], log[t * steps_per_task + k]["loss_old"]] for k in range(RECORDED_STEPS)]
            for t in range(len(log) // steps_per_task)]
    return np.array(rows, dtype=np.float64)


def cosim_stream(cfg=None):
    """The co-simulation's stream: the case's tasks concatenated, to be cut into sequential slices of 20 (two batches per call)."""
    cfg = LWF_CASE if cfg is None else cfg
    tasks, _ = make_stream(cfg)
    return np.concatenate([x for x, _ in tasks], 0), np.concatenate([y for _, y in tasks], 0)
