"""Averaged GEM on the engine (reference: agents/agem.py:10-91).

Per stream batch the reference does: batch pass (forward, CE, backward) -> [from the second task on: buffer.retrieve(), keep the
batch gradient, memory pass (forward, CE, zero_grad, backward), project the batch gradient off the memory gradient where the two
point apart] -> opt.step -> buffer.update.  The reference keeps the two gradients as 62 cloned tensors each, forms the inner products
with one small reduction per tensor and asks the host `if prod < 0`.  Here both gradients are flat arrays: the batch gradient is
moved aside with one device copy, the memory pass overwrites the flat gradient array, and `ops.agem_project` (two launches, no
synchronisation) leaves what opt.step() reads next in that array."""
import torch

from .. import debug
from .. import ops
from ..buffer import Buffer
from ..utils import maybe_cuda, AverageMeter
from ..loss import unit_gradient
from .base import ContinualLearner


class AGEM(ContinualLearner):
    _force_torch_projection = False   # the A/B's and one test's comparator: agents/agem.py:60-80 as written, over the p.grad views

    def __init__(self, model, opt, params):
        super(AGEM, self).__init__(model, opt, params)
        self.buffer = Buffer(model, params)
        self.mem_size = params.mem_size
        self.eps_mem_batch = params.eps_mem_batch
        self.mem_iters = params.mem_iters
        self._g_batch = self._info = None   # the batch gradient beside the flat gradient array; what the projection decided

    # ---- pieces of a step ----------------------------------------------------------------------------------------------
    def _memory_pass(self, mem_x, mem_y):
        mem_logits = self.model.forward(mem_x)
        loss_mem = self.criterion(mem_logits, mem_y)
        self._emit("agem_loss_mem", loss_mem)
        self.opt.zero_grad()
        loss_mem.backward(unit_gradient(loss_mem))

    def _project_fused(self, mem_x, mem_y):
        grads = self.model.flat_grads()
        if self._g_batch is None or self._g_batch.shape != grads.shape or self._g_batch.device != grads.device:
            self._g_batch = torch.empty_like(grads)
            self._info = torch.zeros(4, dtype=torch.float32, device=grads.device)
        self._g_batch.copy_(grads)            # gradient computed using current batch (:62)
        self._memory_pass(mem_x, mem_y)       # the flat gradient array now holds the memory gradient (:65-70)
        ops.agem_project(self._g_batch, grads, info=self._info)
        if debug.on():
            prod, prod_ref, coef, projected = self._info.cpu().tolist()
            debug.emit("agem", prod=prod, prod_ref=prod_ref, coef=coef, projected=bool(projected))

    def _project_torch(self, mem_x, mem_y):
        params = [p for p in self.model.parameters() if p.requires_grad]
        grad = [p.grad.clone() for p in params]
        self._memory_pass(mem_x, mem_y)
        grad_ref = [p.grad.clone() for p in params]
        prod = sum([torch.sum(g * g_r) for g, g_r in zip(grad, grad_ref)])
        projected = bool(prod < 0)
        prod_ref = coef = 0.0
        if projected:
            prod_ref = sum([torch.sum(g_r ** 2) for g_r in grad_ref])
            grad = [g - prod / prod_ref * g_r for g, g_r in zip(grad, grad_ref)]
        for g, p in zip(grad, params):
            p.grad.data.copy_(g)
        if debug.on():
            if projected:
                coef = float(prod / prod_ref)
            debug.emit("agem", prod=float(prod), prod_ref=float(prod_ref), coef=coef, projected=projected)

    def _step(self, batch_x, batch_y, meters):
        logits = self.model.forward(batch_x)
        loss = self._kd_mix(self.criterion(logits, batch_y), logits, batch_x)
        self._track(meters, logits, batch_y, loss)
        self._emit("agem_loss", loss)
        self.opt.zero_grad()
        loss.backward(unit_gradient(loss))

        if self.task_seen > 0:
            # sample from memory of previous tasks
            mem_x, mem_y = self.buffer.retrieve()
            if mem_x.size(0) > 0:
                mem_x, mem_y = maybe_cuda(mem_x, self.cuda), maybe_cuda(mem_y, self.cuda)
                if self._force_torch_projection:
                    self._project_torch(mem_x, mem_y)
                else:
                    self._project_fused(mem_x, mem_y)
        self.opt.step()

    # ---- the loop ------------------------------------------------------------------------------------------------------
    def _train_learner(self, x_train, y_train):
        meters = (AverageMeter(), AverageMeter())
        for batches in self._epochs(x_train, y_train):
            for i, batch_x, batch_y, batch_y_host in batches:
                for j in range(self.mem_iters):
                    self._step(batch_x, batch_y, meters)
                self.buffer.update(batch_x, batch_y, y_host=batch_y_host)
                self._print_running(i, meters)
        self.after_train()
