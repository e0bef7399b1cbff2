"""GDumb on the engine (reference: agents/gdumb.py:12-83).

While the stream passes, the reference keeps a greedily class-balanced memory (:19-31) and trains nothing; at every task's end it
builds a fresh network and trains it on that memory alone (:52-83): mem_epoch epochs of plain forward / backward / global-norm
gradient clip / optimiser step over mem_size // batch mini-batches.  Here the sampler's decisions are taken on the host from the
loader's label mirror (gdumb_memory.GreedyBalancer, one device scatter per stream batch), the epoch's permutation is composed on the
host and applied by one gather, and the clip is `ops.clip_grad_norm_` on the flat gradient array (two launches, no
synchronisation) in place of the per-tensor norm, stack, norm, clamp and per-tensor multiply of torch.nn.utils.clip_grad_norm_.

The reference's cosine-annealing scheduler and early stopping are commented out there (:17, :48, :64, :66, :73-76); they are not built.
`params.minlr` is accepted and unused for that reason."""
import numpy as np
import torch

from .. import debug
from .. import ops
from ..gdumb_memory import GdumbMemory
from ..loss import unit_gradient
from ..setup_elements import setup_architecture, setup_opt, input_size_match
from ..utils import maybe_cuda
from .base import ContinualLearner


class Gdumb(ContinualLearner):
    _same_weights = False       # train_mem() replaces self.model: the context of the network it lets go must not wrap the call
    _force_torch_clip = False   # the A/B's and one test's comparator: torch.nn.utils.clip_grad_norm_ over the p.grad views (:82 as written)

    def __init__(self, model, opt, params):
        super(Gdumb, self).__init__(model, opt, params)
        self.mem_epoch = params.mem_epoch
        self.clip = params.clip
        self.minlr = getattr(params, "minlr", None)   # the commented-out scheduler's floor: unused
        self.memory = None                            # built at the first batch, on the batch's device
        self.mem_opt = None                           # the optimiser of the network train_mem() built last
        self.mem_steps = 0
        self._info = None

    # ---- one memory-training step (:78-83) -------------------------------------------------------------------------------
    def _mem_step(self, x, y):
        opt = self.mem_opt
        opt.zero_grad()
        logits = self.model.forward(x)
        loss = self.criterion(logits, y)
        loss.backward(unit_gradient(loss))
        if self._force_torch_clip:
            total = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)
        else:
            grads = self.model.flat_grads()
            if self._info is None or self._info.device != grads.device:
                self._info = torch.zeros(4, dtype=torch.float32, device=grads.device)
            total = ops.clip_grad_norm_(grads, self.clip, info=self._info)
        opt.step()
        self.mem_steps += 1
        self._emit("gdumb_loss", loss)
        if debug.on():
            if self._force_torch_clip:
                total = float(total)
                coef = min(self.clip / (total + 1e-6), 1.0)
                debug.emit("gdumb_clip", total_norm=total, coef=coef, clipped=not coef >= 1.0)
            else:
                total, coef, clipped, _ = self._info.cpu().tolist()
                debug.emit("gdumb_clip", total_norm=total, coef=coef, clipped=bool(clipped))
        return loss

    # ---- a fresh network and its optimiser (:61-63) ----------------------------------------------------------------------
    def _fresh_learner(self):
        """`self.model = setup_architecture(params)`: the same torch-RNG draws as the reference, so the same fresh weights for a
        given seed.  The network it replaces is let go first: its engine object and device arrays are freed by reference counting
        (resnet._EngineMixin.__del__) as soon as nothing else holds it, not at some later cycle collection."""
        old, self.model, self.mem_opt = self.model, None, None
        if old is not None:
            old.__dict__.pop("_all_modules_cache", None)     # the one reference cycle of an engine-backed module (its train() cache)
        del old
        self.model = maybe_cuda(setup_architecture(self.params), self.cuda)
        self.mem_opt = setup_opt(self.params.optimizer, self.model, self.params.learning_rate, self.params.weight_decay)
        return self.model, self.mem_opt

    def train_mem(self):
        slots = self.memory.order()[0] if self.memory is not None else np.zeros(0, dtype=np.int64)
        n_mem = int(slots.shape[0])
        if n_mem == 0:
            raise RuntimeError("GDumb: the memory is empty (the reference's torch.stack of an empty list)")
        self._fresh_learner()
        bs = self.params.batch
        order = slots
        meter = []
        for ep in range(self.mem_epoch):
            # the reference reassigns mem_x = mem_x[idx] every epoch (:68-70): the permutations compose
            order = order[np.asarray(np.random.permutation(n_mem).tolist(), dtype=np.int64)]
            mem_x, mem_y = ops.gather_pair(self.memory.img, self.memory.label, torch.from_numpy(order))
            self.model = self.model.train()
            for j in range(n_mem // bs):
                loss = self._mem_step(mem_x[bs * j:bs * (j + 1)], mem_y[bs * j:bs * (j + 1)])
                if self.verbose:
                    meter.append(loss.detach())
            if self.verbose and meter:       # (one host fetch per epoch; the reference prints nothing here)
                print('==>>> mem epoch: {}, avg. loss: {:.6f}'.format(ep, float(torch.stack(meter).mean())))
                meter = []

    # ---- the loop (:33-50) -----------------------------------------------------------------------------------------------
    def _train_learner(self, x_train, y_train):
        # one pass over the stream, which only feeds the memory: the network on hand is not trained, and not put in train mode
        for batches in self._epochs(x_train, y_train, epochs=1, train=False):
            for i, batch_x, batch_y, batch_y_host in batches:
                if self.memory is None:
                    self.memory = GdumbMemory(self.params.mem_size, input_size_match[self.data], batch_x.device, batch=self.batch)
                self.memory.update(batch_x, batch_y_host)
        self.train_mem()
        self.after_train()
