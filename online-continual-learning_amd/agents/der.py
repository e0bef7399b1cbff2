"""Dark Experience Replay on the engine: DER and DER++ (Buzzega et al., "Dark Experience for General Continual Learning", NeurIPS 2020).
The method is not among the reference's agents; it is written over the reference's own parts (its Buffer surface, reservoir update and
uniform retrieval) in the shape of its replay agents (agents/exp_replay.py).

The memory keeps, beside every image and label, the logits the model gave that image when it entered the memory (`buffer_logits`, a
float32 [mem_size, n_classes] buffer registered on this agent's Buffer instance).  Per stream batch, for each of `mem_iters` iterations:
a batch of memory rows is drawn uniformly and, for DER++ (`der_beta` != 0), a second, independent one; the loss is
    CE(stream batch)  +  der_alpha * MSE(today's logits of the first draw, their stored logits)  +  der_beta * CE(second draw)
followed by one optimiser step.  After the iterations the reservoir update writes the batch's images, labels and the logits of the last
iteration's forward into the same slots.  `der_beta` == 0 is plain DER.  Both weights are read from params with getattr (defaults 0.1
and 0.5, untuned).

Random retrieval reads neither the model nor its gradients, so drawing before the forward leaves every RNG stream in order (the argument
of exp_replay.py's merged step).  The fused path runs the batches as ONE taped pass with one BatchNorm group per batch and gets the four
losses and dL/dlogits from ONE launch (`ops.der_loss`, which reads the stored rows in place by their slots), and the engine's backward
takes that gradient as it is.  The same statements over model.forward per batch, criterion, F.mse_loss, a gather of the stored rows and
autograd run when the batches differ in size (while the memory holds fewer rows than a batch), with the labels trick or the separated
softmax (`_taped_ce_ok`), and under `_force_autograd` (the A/B's and the tests' comparator).  The KD tricks change nothing in this
agent's loss; `ncm_trick` and `review_trick` take base.py's paths (the agent has a `buffer`)."""
import torch
from torch.nn import functional as F

from .. import ops
from ..buffer import Buffer
from ..loss import unit_gradient
from ..plugins.buffer_utils import random_retrieve
from ..setup_elements import n_classes
from ..utils import AverageMeter
from .base import ContinualLearner


class Der(ContinualLearner):
    def __init__(self, model, opt, params):
        super(Der, self).__init__(model, opt, params)
        if params.update != 'random' or params.retrieve != 'random':
            raise ValueError("DER keeps a logit field beside every memory slot: it runs with --update random --retrieve random (got update=%s, "
                             "retrieve=%s); the other update methods do not carry the logit field" % (params.update, params.retrieve))
        self.buffer = Buffer(model, params)
        self.mem_size = params.mem_size
        self.eps_mem_batch = params.eps_mem_batch
        self.mem_iters = params.mem_iters
        self.alpha = float(getattr(params, 'der_alpha', 0.1))
        self.beta = float(getattr(params, 'der_beta', 0.5))
        images = self.buffer.buffer_img
        self.buffer.register_buffer('buffer_logits', torch.zeros((images.size(0), n_classes[params.data]), dtype=torch.float32,
                                                                 device=images.device))

    def _draw(self):
        """-> (mem_x1, slots1 on the device, mem_x2, mem_y2): the logit-replay rows and, for DER++, the label-replay rows (None where a
        term is absent: an empty memory, beta == 0)."""
        if self.buffer.current_index == 0:
            return None, None, None, None
        mem_x1, _, idx1 = random_retrieve(self.buffer, self.eps_mem_batch, return_indices=True)
        slots1 = ops.upload(idx1, mem_x1.device)
        if self.beta == 0:
            return mem_x1, slots1, None, None
        mem_x2, mem_y2, _ = random_retrieve(self.buffer, self.eps_mem_batch, return_indices=True)
        return mem_x1, slots1, mem_x2, mem_y2

    def _step(self, batch_x, batch_y, meters):
        """One iteration; returns the stream rows' logits (detached)."""
        mem_x1, slots1, mem_x2, mem_y2 = self._draw()
        views = [v for v in (batch_x, mem_x1, mem_x2) if v is not None]
        n0 = batch_x.size(0)
        n1 = mem_x1.size(0) if mem_x1 is not None else 0
        n2 = mem_x2.size(0) if mem_x2 is not None else 0
        if self._taped_ce_ok() and len({v.size(0) for v in views}) == 1:
            out, tape = self.model.forward_views_taped(views)
            loss4, dl = ops.der_loss(out, batch_y, mem_y2, self.buffer.buffer_logits if n1 else None, slots1, n0, n1, n2, self.alpha, self.beta)
            logits = out[:n0]
            self._track(meters, logits, batch_y, loss4[0])
            self._emit("der_loss", loss4[0], ce=loss4[1], mse=loss4[2], ce_mem=loss4[3])
            self.opt.zero_grad()
            self.model.backward_taped(tape, dl)
            self.opt.step()
            return logits.detach()
        # the same statements over autograd, one pass per batch; each term's backward follows its forward into the same gradients (what
        # one backward of the sum adds up to), so one activation tape is alive at a time
        self.opt.zero_grad()
        logits = self.model.forward(batch_x)
        ce = self.criterion(logits, batch_y)
        ce.backward(unit_gradient(ce))
        loss = ce.detach()
        mse = ce_mem = 0.0
        if n1:
            stored = ops.gather_rows(self.buffer.buffer_logits, slots1)
            mse = F.mse_loss(self.model.forward(mem_x1), stored)
            term = self.alpha * mse
            term.backward(unit_gradient(term))
            loss = loss + term.detach()
        if n2:
            ce_mem = self.criterion(self.model.forward(mem_x2), mem_y2)
            term = self.beta * ce_mem
            term.backward(unit_gradient(term))
            loss = loss + term.detach()
        self._track(meters, logits, batch_y, loss)
        self._emit("der_loss", loss, ce=ce, mse=mse, ce_mem=ce_mem)
        self.opt.step()
        return logits.detach()

    def _train_learner(self, x_train, y_train):
        meters = (AverageMeter(), AverageMeter())
        for batches in self._epochs(x_train, y_train):
            for i, batch_x, batch_y, batch_y_host in batches:
                for j in range(self.mem_iters):
                    logits = self._step(batch_x, batch_y, meters)
                self.buffer.update(batch_x, batch_y, y_host=batch_y_host, extra=((self.buffer.buffer_logits, logits),))
                self._print_running(i, meters)
        self.after_train()
