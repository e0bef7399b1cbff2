"""Learning without Forgetting on the engine (reference: agents/lwf.py:14-56).

Per stream batch the reference does: forward -> loss_old = distillation against last task's model (0 during the first task) ->
loss_new = CE -> loss = 1 / (t + 1) * loss_new + (1 - 1 / (t + 1)) * loss_old, t the number of tasks seen -> backward -> opt.step.
There is no replay memory; the teacher is KdManager's snapshot of the flat parameter array, refreshed by after_train() (base.py:90-91).

Built from the CE and KD kernels that is two loss launches, two scalar multiplies and an add, autograd's walk back through two
Functions and an add of two gradient tensors, all on the step's dependent chain.  The fused path forwards the student on a tape,
forwards the teacher, and gets the three losses and dL/dlogits from ONE launch (`ops.ce_kd_blend`), which the engine's backward takes as
it is.  The reference's Lwf never calls the KD tricks' blend (exp_replay.py:42-47): `kd_trick` / `kd_trick_star` change nothing in its
loss, and nothing here.  The review trick needs a buffer (base.py:62) and stays skipped."""
import contextlib

import torch

from .. import debug
from .. import ops
from ..data import DeviceLoader
from ..utils import AverageMeter
from ..loss import unit_gradient
from .base import ContinualLearner


class Lwf(ContinualLearner):
    _force_autograd = False   # the A/B's and one test's comparator: the reference's statements over criterion, get_kd_loss and autograd
    T = 2.0                   # loss_fn_kd's default, which the reference's get_kd_loss never overrides (kd_manager.py:6, :25)

    def __init__(self, model, opt, params):
        super(Lwf, self).__init__(model, opt, params)

    def _fused(self):
        trick = self.params.trick
        return (hasattr(self.model, "forward_views_taped") and not trick['labels_trick'] and not trick['separated_softmax']
                and not self._force_autograd)

    def _step(self, batch_x, batch_y, meters):
        # the weights as the reference's expression forms them, in Python doubles (:39); each is rounded to float once, at the launch
        w_new = 1 / (self.task_seen + 1)
        w_old = 1 - 1 / (self.task_seen + 1)
        if self._fused():
            logits, tape = self.model.forward_views_taped([batch_x])
            loss3, dl = ops.ce_kd_blend(logits, batch_y, self.kd_manager.teacher_logits(batch_x), self.T, w_new, w_old)
            loss, loss_new, loss_old = loss3[0], loss3[1], loss3[2]
        else:
            logits = self.forward(batch_x)
            loss_old = self.kd_manager.get_kd_loss(logits, batch_x)
            loss_new = self.criterion(logits, batch_y)
            loss = w_new * loss_new + w_old * loss_old
        if self.verbose:      # (the reference's per-iteration .item() would stall the stream)
            loss_meter, acc_meter = meters
            hits = (torch.max(logits, 1)[1] == batch_y).sum()
            acc_meter.update(hits / batch_y.size(0), batch_y.size(0))
            loss_meter.update(loss.detach(), batch_y.size(0))
        if debug.on():
            debug.emit("lwf_loss", loss=float(loss.detach()), loss_new=float(loss_new.detach()), loss_old=float(loss_old.detach()) if torch.is_tensor(loss_old) else float(loss_old))
        self.opt.zero_grad()
        if self._fused():
            self.model.backward_taped(tape, dl)
        else:
            loss.backward(unit_gradient(loss))
        self.opt.step()

    def train_learner(self, x_train, y_train):
        same = self.model.same_weights() if hasattr(self.model, "same_weights") else contextlib.nullcontext()
        with self.launch_stream(), same:
            self._train_learner(x_train, y_train)

    def _train_learner(self, x_train, y_train):
        self.before_train(x_train, y_train)
        # device-resident task behind the reference's DataLoader (same sampler, same RNG draws)
        train_loader = DeviceLoader(x_train, y_train, self.batch, shuffle=True, drop_last=True)
        self.model = self.model.train()
        meters = (AverageMeter(), AverageMeter())
        for ep in range(self.epoch):
            for i, (batch_x, batch_y) in enumerate(train_loader):
                self._step(batch_x, batch_y, meters)
                if i % 100 == 1 and self.verbose:
                    print('==>>> it: {}, avg. loss: {:.6f}, running train acc: {:.3f}'.format(i, meters[0].avg(), meters[1].avg()))
        self.after_train()
