"""Helper of tests/test_cpu_der.py and tests/test_gpu_der.py (no tests here): the float64 statement of the Dark Experience Replay loss
kernel (csrc/der.hip, ocl_der_fwd_bwd), the same formula in plain torch-CPU float32 (the e_ref of parity_bounds.check_vs_torch32), and one
iteration of the DER / DER++ agent (agents/der.py) stated over the functions of oracle/ocl_oracle.py, with a reservoir statement of its
own that keeps the slot-to-item map and stores the logits.  The method is not among the reference's agents: nothing here is recorded
from it."""
import numpy as np
import torch
from torch.nn import functional as F

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, case_params

# ER's er_c10 with a third task and a memory that is full after the third batch: every step but the first carries all three terms
DER_CASE = dict(STEP_CASES["er_c10"], agent="DER", seed=19, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20, mem_size=30)
ALPHA, BETA = 0.1, 0.5      # the agent's defaults


def ref_params(cfg):
    """The keyword arguments of the agent's params for the case."""
    return dict(case_params(cfg), der_alpha=cfg.get("der_alpha", ALPHA), der_beta=cfg.get("der_beta", BETA))


# ---- the kernel's statement in float64 ----------------------------------------------------------------------------------------------------

def _log_softmax64(x):
    m = x.max(axis=1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))


def _ce64(rows, y):
    """(mean cross-entropy, its gradient with respect to the rows) of float64 rows."""
    n = rows.shape[0]
    ls = _log_softmax64(rows)
    at = np.arange(n)
    onehot = np.zeros_like(rows)
    onehot[at, y] = 1.0
    return float(-ls[at, y].mean()), (np.exp(ls) - onehot) / n


def ref_der(logits, y0, y2, stored, slots, n0, n1, n2, alpha, beta):
    """(loss4, dlogits) in float64 from the float32 inputs and the float32 roundings of alpha and beta (what the entry point receives):
    ce = mean CE of rows [0, n0) against y0;  mse = sum (s - stored[slots])^2 / (n1 * c) over rows [n0, n0 + n1);  ce_m = mean CE of the
    last n2 rows against y2;  loss4 = [ce + alpha * mse + beta * ce_m, ce, mse, ce_m];  dlogits per block: (softmax - onehot) / n0,
    alpha * 2 * (s - z) / (n1 * c), beta * (softmax - onehot) / n2.  slots None: rows 0 .. n1 - 1 of stored.  An empty block adds 0."""
    s = np.asarray(logits, dtype=np.float64)
    assert s.shape[0] == n0 + n1 + n2 and n0 >= 1
    c = s.shape[1]
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    dl = np.zeros_like(s)
    ce, dl[:n0] = _ce64(s[:n0], np.asarray(y0, dtype=np.int64))
    mse = ce_m = 0.0
    if n1:
        at = np.arange(n1) if slots is None else np.asarray(slots, dtype=np.int64)
        d = s[n0:n0 + n1] - np.asarray(stored, dtype=np.float64)[at]
        mse = float((d * d).sum() / (n1 * c))
        dl[n0:n0 + n1] = alpha * 2.0 * d / (n1 * c)
    if n2:
        ce_m, g = _ce64(s[n0 + n1:], np.asarray(y2, dtype=np.int64))
        dl[n0 + n1:] = beta * g
    return np.array([ce + alpha * mse + beta * ce_m, ce, mse, ce_m]), dl


def torch32_der(logits, y0, y2, stored, slots, n0, n1, n2, alpha, beta):
    """The same formula as plain torch-CPU float32 statements (F.cross_entropy, F.mse_loss on a gather of the stored rows, two scalar
    multiplies and two adds) with autograd's gradient: (loss4, dlogits) as float32 numpy."""
    s = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).requires_grad_(True)
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    ce = O.ce_mean(s[:n0], torch.from_numpy(np.ascontiguousarray(y0, dtype=np.int64)))
    mse = ce_m = torch.zeros(())
    loss = ce
    if n1:
        at = torch.arange(n1) if slots is None else torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64))
        mse = F.mse_loss(s[n0:n0 + n1], torch.from_numpy(np.ascontiguousarray(stored, dtype=np.float32))[at])
        loss = loss + alpha * mse
    if n2:
        ce_m = O.ce_mean(s[n0 + n1:], torch.from_numpy(np.ascontiguousarray(y2, dtype=np.int64)))
        loss = loss + beta * ce_m
    loss.backward()
    return np.array([float(loss.detach()), float(ce.detach()), float(mse.detach()), float(ce_m.detach())], dtype=np.float32), s.grad.numpy()


def kernel_case(n0, n1, n2, c, scale, seed=0):
    """Inputs of one kernel case: logits from lwf_ref.logits_for, labels, a table of m = n1 + 5 stored rows near today's logits (the
    replayed rows moved on by a few steps), and permuted slots."""
    from lwf_ref import logits_for
    rng = np.random.default_rng(9100 + 1009 * n0 + 101 * n1 + 11 * n2 + c + seed)
    n = n0 + n1 + n2
    s = logits_for(rng, n, c, scale)
    m = n1 + 5
    stored = logits_for(rng, m, c, scale)
    slots = rng.permutation(m)[:n1].astype(np.int64)
    if n1:      # stored rows that lie near today's rows: the squared error has the cancellation of the workload's
        stored[slots] = s[n0:n0 + n1] + (rng.standard_normal((n1, c)) * 0.1 * scale).astype(np.float32)
    y0, y2 = rng.integers(0, c, n0).astype(np.int64), rng.integers(0, c, n2).astype(np.int64)
    return s, y0, y2, stored, slots, m


# ---- the memory with its logit field --------------------------------------------------------------------------------------------------------

def der_buffer(mem_size, shape, n_cls):
    buf = O.OracleBuffer(mem_size, shape)
    buf.logits = torch.zeros(mem_size, n_cls, dtype=torch.float32)
    return buf


def der_reservoir(buf, x, y, rows):
    """Reservoir sampling (utils/buffer/reservoir_update.py:8-61 of the reference) stated by the slot-to-item map: free slots are filled in
    order; every remaining item draws a slot in [0, n_seen_so_far) with one uniform_ call on the torch CPU generator and is kept when the
    slot exists, the last item drawing a slot wins.  Every (slot, item) pair writes the item's image, label and logit row.  Returns the
    pairs in the order they were written."""
    n = x.shape[0]
    take = min(max(0, buf.mem_size - buf.current_index), n)
    pairs = [(buf.current_index + i, i) for i in range(take)]
    buf.current_index += take
    buf.n_seen_so_far += take
    if take < n:
        draw = torch.FloatTensor(n - take).uniform_(0, buf.n_seen_so_far).long().tolist()
        buf.n_seen_so_far += n - take
        winner = {}
        for i, slot in enumerate(draw):
            if slot < buf.mem_size:
                winner[slot] = take + i
        pairs += list(winner.items())
    for slot, item in pairs:
        buf.img[slot], buf.label[slot], buf.logits[slot] = x[item], y[item], rows[item]
    return pairs


# ---- one iteration of the agent -------------------------------------------------------------------------------------------------------------

def der_step(state, names, buf, bx, by, lr, eps_mem_batch, alpha, beta):
    """agents/der.py for ONE iteration: the two uniform draws (the second only for beta != 0; none from an empty memory), one train-mode
    forward per batch in the order stream, logit replay, label replay, the three-term loss, backward, SGD step."""
    idx1 = idx2 = None
    if buf.current_index > 0:
        idx1 = O.random_retrieve_indices(buf, eps_mem_batch)
        if beta != 0:
            idx2 = O.random_retrieve_indices(buf, eps_mem_batch)
    net = O.OracleNet(state, head=None, training=True)
    logits = net.forward(bx)
    ce = O.ce_mean(logits, by)
    loss = ce
    mse = ce_mem = None
    if idx1 is not None:
        mse = F.mse_loss(net.forward(buf.img[idx1]), buf.logits[idx1])
        loss = loss + alpha * mse
    if idx2 is not None:
        ce_mem = O.ce_mean(net.forward(buf.img[idx2]), buf.label[idx2])
        loss = loss + beta * ce_mem
    O.zero_grad(state, names)
    loss.backward()
    O.sgd_step(state, names, lr)
    val = lambda t: 0.0 if t is None else float(t.detach())     # noqa: E731
    return dict(loss=float(loss.detach()), ce=float(ce.detach()), mse=val(mse), ce_mem=val(ce_mem), idx1=idx1, idx2=idx2,
                logits=logits.detach().clone())


class DerOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, evaluate) with agents/der.py's loop as its train_learner."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.alpha, self.beta = cfg.get("der_alpha", ALPHA), cfg.get("der_beta", BETA)
        self.buf = der_buffer(cfg["mem_size"], tuple(self.buf.img.shape[1:]), self.n_classes)

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        for ep in range(self.epoch):
            for idx in loader:
                bx, by = xs[idx], ys[idx]
                for j in range(self.mem_iters):
                    rec = der_step(self.state, self.names, self.buf, bx, by, self.p["lr"], self.p["eps_mem_batch"], self.alpha, self.beta)
                rec["written"] = der_reservoir(self.buf, bx, by, rec["logits"])
                self.log.append(rec)
        self.after_train(new)


def cosim_stream(cfg=None):
    """The co-simulation's stream: the case's tasks concatenated, to be cut into sequential slices of 20 (two batches per call)."""
    cfg = DER_CASE if cfg is None else cfg
    tasks, _ = make_stream(cfg)
    return np.concatenate([x for x, _ in tasks], 0), np.concatenate([y for _, y in tasks], 0)
