"""Helper of tests/test_cpu_icarl.py, tests/test_gpu_icarl.py and scripts/make_icarl_golden.py (no tests here): the float64 statement of
the BCE-distillation kernel (csrc/icarl.hip, ocl_bce_distill_fwd_bwd), the same loss in plain torch-CPU float32 (the e_ref of
parity_bounds.check_vs_torch32), and one iteration of the reference's agents/icarl.py:38-65 restated over the functions of
oracle/ocl_oracle.py."""
import numpy as np
import torch
from torch.nn import functional as F

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, case_params, digest_state

# the free-running case of tests/golden/icarl.npz: ER's er_c10 with a third task (two tasks carry a teacher and a retrieval) and iCaRL
ICARL_CASE = dict(STEP_CASES["er_c10"], agent="ICARL", seed=17, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20, mem_size=50)
GOLDEN_KEYS = ("acc", "state")
RECORDED_STEPS = 2          # the golden keeps the loss of the first two steps of each task


def ref_params(cfg):
    """The keyword arguments of oracle.ref_import.default_params / of the agent's params for the case."""
    return case_params(cfg)


# ---- the kernel's statement in float64 ----------------------------------------------------------------------------------------------------

def _sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def targets64(teacher, pos, n, n_stream, n_cls, n_old):
    """z [n, n_cls] in float64: sigmoid(teacher) on the columns below n_old (every row); on the others 1 at (r, pos[r]) for the stream
    rows r < n_stream with n_old <= pos[r] < n_cls, else 0.  Teacher columns from n_old on are not looked at."""
    z = np.zeros((n, n_cls), dtype=np.float64)
    for r in range(n_stream):
        p = int(pos[r])
        if 0 <= p < n_cls:
            z[r, p] = 1.0
    if n_old:
        z[:, :n_old] = _sigmoid64(np.asarray(teacher, dtype=np.float64)[:, :n_old])
    return z


def ref_bce_distill(logits, teacher, pos, n_stream, n_cls, n_old):
    """(loss3, dlogits) in float64 from the float32 inputs:  l = max(s, 0) - s * z + log1p(exp(-|s|));  old / new = the column sums of l
    below / from n_old, averaged over the n rows;  loss3 = [old + new, old, new];  dlogits = (sigmoid(s) - z) / n on the columns below
    n_cls and 0 from there on.  Columns from n_cls on (and teacher columns from n_old on) are not looked at.  teacher None: n_old = 0."""
    n, c = np.asarray(logits).shape
    assert 1 <= n_stream <= n and 0 <= n_old <= n_cls <= c and (teacher is not None or n_old == 0)
    s = np.asarray(logits, dtype=np.float64)[:, :n_cls]
    z = targets64(teacher, np.asarray(pos, dtype=np.int64), n, n_stream, n_cls, n_old)
    el = np.maximum(s, 0.0) - s * z + np.log1p(np.exp(-np.abs(s)))
    old, new = float(el[:, :n_old].sum() / n), float(el[:, n_old:].sum() / n)
    dl = np.zeros((n, c), dtype=np.float64)
    dl[:, :n_cls] = (_sigmoid64(s) - z) / n
    return np.array([old + new, old, new]), dl


def torch32_bce_distill(logits, teacher, pos, n_stream, n_cls, n_old):
    """The same loss as plain torch-CPU float32 statements (the reference's own: the sigmoid of the teacher's logits, the target, torch's
    F.binary_cross_entropy_with_logits, .sum(1).mean()) with autograd's gradient: (loss3, dlogits) as float32 numpy."""
    s = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).requires_grad_(True)
    n, c = s.shape
    target = torch.zeros((n, n_cls), dtype=torch.float32)
    for r in range(n_stream):
        if 0 <= int(pos[r]) < n_cls:
            target[r, int(pos[r])] = 1.0
    if n_old:
        q = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(teacher, dtype=np.float32))[:, :n_old])
        target[:, :n_old] = q
    el = F.binary_cross_entropy_with_logits(s[:, :n_cls], target, reduction='none')
    loss = el.sum(dim=1).mean()
    loss.backward()
    old, new = el[:, :n_old].sum(dim=1).mean() if n_old else torch.zeros(()), el[:, n_old:].sum(dim=1).mean() if n_cls > n_old else torch.zeros(())
    return np.array([float(loss.detach()), float(old.detach()), float(new.detach())], dtype=np.float32), s.grad.numpy()


def logits_for(rng, n, c, scale):
    """Random logits times `scale`; the second-to-last row has one dominant logit, the last row equal logits (where n allows): the rows of
    the CE family's cases (tests/test_gpu_small_ops.py)."""
    x = (rng.standard_normal((n, c)) * scale).astype(np.float32)
    if n >= 3:
        x[n - 2, rng.integers(0, c)] += np.float32(60.0 * scale)
        x[n - 1, :] = np.float32(0.5 * scale)
    return x


# ---- one iteration of the reference agent ------------------------------------------------------------------------------------------------

def icarl_step(state, names, teacher, buf, old_labels, new_labels, bx, by, batch, updated_idx, lr):
    """agents/icarl.py:38-65 for ONE stream batch: the labels as column positions, the one-hot target, (with a teacher) `batch` memory
    rows outside `updated_idx` with all-zero targets, forward, the old columns' targets from the teacher (a cloned state forwarded in
    train mode under no_grad), BCE with logits summed over the columns and averaged over the rows, backward, SGD step, reservoir update
    (its written slots are appended to `updated_idx`)."""
    pos = by.clone()
    for k, y in enumerate(pos):
        pos[k] = len(old_labels) + new_labels.index(y)
    n_cls = len(new_labels) + len(old_labels)
    target = torch.zeros((pos.size(0), n_cls), dtype=torch.long).scatter_(1, pos.reshape((pos.size(0), 1)), 1).float()
    idx = None
    if teacher is not None:
        idx = O.random_retrieve_indices(buf, batch, updated_idx)
        batch_x = torch.cat([bx, buf.img[torch.from_numpy(idx)]])
        target = torch.cat([target, torch.zeros_like(target)])
    else:
        batch_x = bx
    logits = O.OracleNet(state, head=None, training=True).forward(batch_x)
    O.zero_grad(state, names)
    if teacher is not None:
        with torch.no_grad():
            q = torch.sigmoid(O.OracleNet(teacher, head=None, training=True).forward(batch_x))
        for k, y in enumerate(old_labels):
            target[:, k] = q[:, k]
    loss = F.binary_cross_entropy_with_logits(logits[:, :n_cls], target, reduction='none').sum(dim=1).mean()
    loss.backward()
    O.sgd_step(state, names, lr)
    excl = list(updated_idx) if teacher is not None else None     # what the retrieval excluded
    updated_idx += O.reservoir_update(buf, bx, by)
    return dict(loss=float(loss.detach()), teacher=teacher is not None, indices=idx, excl=excl, rows=int(batch_x.size(0)), n_cls=n_cls)


class IcarlOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, the NCM evaluate of base.py:121) with agents/icarl.py:23-65 as its train_learner; the teacher
    is a clone of the state taken after the task's last step and before after_train (:31-32)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.trick = dict(self.trick, ncm_trick=True)     # base.py:121: params.agent == 'ICARL' classifies by the nearest class mean

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        updated_idx = []
        for idx in loader:
            self.log.append(icarl_step(self.state, self.names, self.teacher, self.buf, self.old_labels, new, xs[idx], ys[idx], self.batch,
                                       updated_idx, self.p["lr"]))
        self.teacher = O.clone_state(self.state, requires_grad=False)
        self.after_train(new)


def record(acc, state_dict):
    """What the golden file keeps per task: the accuracies and the digest_state rows of the model."""
    return dict(acc=np.asarray(acc, dtype=np.float64), state=digest_state(state_dict))


def run_oracle_case(cfg=None, tasks_only=None):
    """The free run of IcarlOracle over the case's tasks: per-task records, and the agent (its .log holds every iteration)."""
    cfg = ICARL_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    ag = IcarlOracle(cfg)
    tasks, tests = make_stream(cfg)
    recs = []
    for x, y in tasks[:tasks_only]:
        ag.train_learner(x, y)
        recs.append(record(ag.evaluate(tests), ag.state_dict()))
    return recs, ag


def recorded_losses(losses, steps_per_task):
    """[n_tasks, RECORDED_STEPS]: the loss of the first RECORDED_STEPS iterations of every task."""
    return np.array([[losses[t * steps_per_task + k] for k in range(RECORDED_STEPS)] for t in range(len(losses) // steps_per_task)],
                    dtype=np.float64)


def retrieval_table(indices, batch):
    """[n_retrievals, batch] int64 from the list of per-retrieval index arrays (every retrieval of the case returns `batch` rows)."""
    return np.array([np.asarray(i, dtype=np.int64) for i in indices], dtype=np.int64).reshape(-1, batch)


def cosim_stream(cfg=None):
    """The co-simulation's stream: the case's tasks, each to be cut into sequential slices of 20 (two batches per call)."""
    cfg = ICARL_CASE if cfg is None else cfg
    tasks, _ = make_stream(cfg)
    return tasks
