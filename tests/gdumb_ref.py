"""Helper of tests/test_cpu_gdumb.py, tests/test_gpu_gdumb.py and scripts/make_gdumb_golden.py (no tests here): the float64 statement of
the global-norm gradient clip with its fp32 round-off bound, and the reference's agents/gdumb.py:19-83 restated over the functions of
oracle/ocl_oracle.py."""
import random
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ocl_oracle as O
from oracle.synth import STEP_CASES, make_stream, seed_all, digest_state

U = 2.0 ** -24      # half an fp32 ulp, relative

# The free-running case of tests/golden/gdumb.npz: ER's er_c10 shape with a third task and the GDumb agent.  Seed 17; clip 10 (the
# value of the reference's README line) was kept after looking, on the CPU, at the norms GdumbOracle logs for this seed: 30 memory
# steps with total norms between 0.23 and 17.8.  Run without evaluate() between the tasks, as the GPU co-simulation runs it, 18 steps
# clip and 12 do not, the closest to the threshold being 9.88 (1.2 % away); with evaluate() (whose loaders draw from the torch
# generator), as the golden file's run, 16 clip and the closest is 2.7 % away (tests/test_cpu_gdumb.py asserts the former).
GDUMB_CASE = dict(STEP_CASES["er_c10"], agent="GDUMB", seed=17, tasks=[[0, 1], [2, 3], [4, 5]], n_train=30, n_test=20, mem_size=50,
                  batch=10, mem_epoch=2, clip=10.0)
GOLDEN_KEYS = ("acc", "mem_label", "mem_rowsum", "mem_counts", "state")

# Label sequences for GreedyBalancer, one list of batches per case: (name, mem_size, random.seed, batches).
BALANCER_CASES = (
    ("fill", 12, 1, [[0, 1, 0, 1, 0], [1, 1, 0, 0, 1]]),                                                    # filling only
    ("new_class_at_full", 8, 2, [[0, 0, 0, 0, 1, 1, 1, 1], [2, 2, 0, 1, 2], [3, 2, 3, 3]]),                  # a new class arrives at a full memory
    ("many_classes", 12, 3, [[0] * 6 + [1] * 6, [2, 3, 4, 5, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [0, 1, 6, 6, 7, 11, 11, 11]]),   # k_c shrinks to 1
    ("fill_then_evict_in_one_batch", 4, 4, [[0, 0, 0, 0], [1, 1, 2, 2, 3, 1, 2], [4, 4, 4, 0, 5, 5]]),       # rows of one batch fill, then are evicted
    ("fewer_slots_than_classes", 3, 5, [[0, 1, 2, 3, 4, 5], [6, 0, 7, 7, 1], [8, 9, 9, 2]]),                 # k_c reaches 0
)


# ---- the clip in float64 -----------------------------------------------------------------------------------------------------------------

def ref_clip(g, max_norm):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2) in float64: total = sqrt(sum g*g), coef = max_norm / (total + 1e-6),
    out = g * coef where coef < 1, else g."""
    g = np.asarray(g, dtype=np.float64)
    total = float(np.sqrt((g * g).sum()))
    coef = float(max_norm) / (total + 1e-6)
    clipped = not coef >= 1.0
    if not clipped:
        coef = 1.0
    out = g * coef if clipped else g.copy()
    return SimpleNamespace(g=g, total=total, coef=coef, clipped=clipped, out=out, sumsq=float((g * g).sum()))


def clip_bound(ref):
    """Per-element bound on |out_fp32 - out|: |g * coef| * (2 * 2^-24 + 2^-40) -- one half-ulp for the coefficient rounded to float, one
    half-ulp for the product, and the double accumulation / sqrt / divide.  Zero where nothing is clipped: the output is g itself."""
    if not ref.clipped:
        return np.zeros_like(ref.out)
    return np.abs(ref.g * ref.coef) * (2.0 * U + 2.0 ** -40)


def worst_ratio(got, ref):
    """max |got - ref.out| / bound (0 where both are zero, inf where a zero bound is exceeded)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref.out)
    e = clip_bound(ref)
    return float(np.divide(d, e, out=np.where(d > 0, np.inf, 0.0), where=e > 0).max())


def max_norm_for(g, ratio):
    """A float32 max_norm such that total / max_norm is `ratio` (up to the rounding to float32)."""
    return float(np.float32(np.linalg.norm(np.asarray(g, dtype=np.float64)) / ratio))


# ---- the reference agent restated ------------------------------------------------------------------------------------------------------

class GdumbOracle(O.OracleAgent):
    """O.OracleAgent (label bookkeeping, loader, evaluate) with agents/gdumb.py:19-83 as its task: the greedy class-balanced memory
    while the stream passes, then a fresh network trained on the memory alone.  .log: one entry per memory step (loss, total_norm,
    clipped, ratio = total_norm / clip); on_step(pre_state, x, y), if set, is called before every memory step."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.mem_img, self.mem_c = {}, {}
        self.mem_epoch, self.clip = cfg["mem_epoch"], cfg["clip"]
        self.on_step = None

    def greedy_balancing_update(self, x, y):
        mem_size = self.p["mem_size"]
        k_c = mem_size // max(1, len(self.mem_img))
        if y not in self.mem_img or self.mem_c[y] < k_c:
            if sum(self.mem_c.values()) >= mem_size:
                cls_max = max(self.mem_c.items(), key=lambda k: k[1])[0]
                self.mem_img[cls_max].pop(random.randrange(self.mem_c[cls_max]))
                self.mem_c[cls_max] -= 1
            if y not in self.mem_img:
                self.mem_img[y], self.mem_c[y] = [], 0
            self.mem_img[y].append(x)
            self.mem_c[y] += 1

    def memory(self):
        """(images, labels) in train_mem's order (:55-60)."""
        mem_x, mem_y = [], []
        for c in self.mem_img.keys():
            mem_x += self.mem_img[c]
            mem_y += [c] * self.mem_c[c]
        return torch.stack(mem_x), torch.LongTensor(mem_y)

    def mem_step(self, x, y):
        """:78-83 for one mini-batch: forward, CE, backward, clip_grad_norm_ over the parameters, SGD step."""
        if self.on_step is not None:
            self.on_step(self.state_dict(), x, y)
        net = O.OracleNet(self.state, head=None, training=True)
        loss = O.ce_mean(net.forward(x), y)
        O.zero_grad(self.state, self.names)
        loss.backward()
        total = torch.nn.utils.clip_grad_norm_([self.state[n] for n in self.names], self.clip)
        clipped = bool(self.clip / (total + 1e-6) < 1.0)
        O.sgd_step(self.state, self.names, self.p["lr"])
        return dict(loss=float(loss.detach()), total_norm=float(total), clipped=clipped, ratio=float(total) / self.clip)

    def train_mem(self):
        mem_x, mem_y = self.memory()
        self.state = O.init_state(self.agent, self.data)           # setup_architecture: a fresh network (:61)
        self.names = [k for k in self.state if self.state[k].requires_grad]
        for ep in range(self.mem_epoch):
            idx = np.random.permutation(len(mem_x)).tolist()
            mem_x, mem_y = mem_x[idx], mem_y[idx]
            for j in range(len(mem_y) // self.batch):
                self.log.append(self.mem_step(mem_x[self.batch * j:self.batch * (j + 1)], mem_y[self.batch * j:self.batch * (j + 1)]))

    def train_learner(self, x_u8, y):
        new = list(set(y.tolist()))
        xs = O.to_tensor(x_u8)
        ys = torch.from_numpy(np.asarray(y)).long()
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        for idx in loader:
            bx, by = xs[idx], ys[idx]
            for j in range(len(bx)):
                self.greedy_balancing_update(bx[j], by[j].item())
        self.train_mem()
        self.after_train(new)


def gdumb_params(cfg):
    """What oracle.synth.case_params does not forward (`batch` it does)."""
    return dict(mem_epoch=cfg["mem_epoch"], clip=cfg["clip"], minlr=0.0005)


def record(acc, mem_label, mem_img, mem_c, state_dict):
    """What the golden file keeps per task: the memory in train_mem's order (labels, image row sums), the per-class counts in dict
    order as [class, count] rows, the model's digest and the accuracies."""
    return dict(acc=np.asarray(acc, dtype=np.float64), mem_label=np.asarray(mem_label, dtype=np.int64).copy(),
                mem_rowsum=mem_img.double().sum(dim=(1, 2, 3)).cpu().numpy(),
                mem_counts=np.array([[c, n] for c, n in mem_c.items()], dtype=np.int64).reshape(-1, 2), state=digest_state(state_dict))


def run_oracle_case(cfg=None, evaluate=True):
    """The free run of GdumbOracle over the case's tasks: per-task records, and the agent (its .log holds every memory step)."""
    cfg = GDUMB_CASE if cfg is None else cfg
    torch.set_num_threads(1)
    seed_all(cfg["seed"])
    ag = GdumbOracle(cfg)
    tasks, tests = make_stream(cfg)
    recs = []
    for x, y in tasks:
        ag.train_learner(x, y)
        acc = ag.evaluate(tests) if evaluate else np.zeros(len(tests))
        mem_x, mem_y = ag.memory()
        recs.append(record(acc, mem_y.numpy(), mem_x, ag.mem_c, ag.state_dict()))
    return recs, ag


# ---- the balancer's label sequences --------------------------------------------------------------------------------------------------------

def run_balancer_case(balancer_cls, mem_size, seed, batches):
    """The label batches through a GreedyBalancer under random.seed(seed), sample number k (counted over the whole sequence) standing
    for the k-th image.  Per batch: [class, count] rows in dict order, and the per-class contents as sample numbers in order()'s order."""
    random.seed(seed)
    bal = balancer_cls(mem_size)
    held = np.full(mem_size, -1, dtype=np.int64)
    seen, out = 0, []
    for ys in batches:
        rows, slots = bal.plan(np.asarray(ys, dtype=np.int64))
        held[slots] = seen + rows
        seen += len(ys)
        order_slots, order_labels = bal.order()
        out.append(dict(counts=np.array([[c, n] for c, n in bal.mem_c.items()], dtype=np.int64).reshape(-1, 2),
                        items=held[order_slots].copy(), labels=order_labels.copy(), rows=rows, slots=slots))
    return out, bal


def run_reference_balancer(mem_size, seed, batches):
    """The same through the reference's own greedy_balancing_update, called on a bare instance of its agent (reference tree needed)."""
    from oracle import ref_import
    ref_import.activate()
    from agents.gdumb import Gdumb
    agent = object.__new__(Gdumb)
    agent.__dict__.update(mem_img={}, mem_c={}, params=SimpleNamespace(mem_size=mem_size))
    random.seed(seed)
    seen, out = 0, []
    for ys in batches:
        for y in ys:
            agent.greedy_balancing_update(seen, y)
            seen += 1
        items, labels = [], []
        for c in agent.mem_img.keys():
            items += agent.mem_img[c]
            labels += [c] * agent.mem_c[c]
        out.append(dict(counts=np.array([[c, n] for c, n in agent.mem_c.items()], dtype=np.int64).reshape(-1, 2),
                        items=np.asarray(items, dtype=np.int64), labels=np.asarray(labels, dtype=np.int64)))
    return out
