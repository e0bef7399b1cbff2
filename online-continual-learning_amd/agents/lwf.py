"""Learning without Forgetting on the engine (reference: agents/lwf.py:14-56).

Per stream batch the reference does: forward -> loss_old = distillation against last task's model (0 during the first task) ->
loss_new = CE -> loss = 1 / (t + 1) * loss_new + (1 - 1 / (t + 1)) * loss_old, t the number of tasks seen -> backward -> opt.step.
There is no replay memory; the teacher is KdManager's snapshot of the flat parameter array, refreshed by after_train() (base.py:90-91).

Built from the CE and KD kernels that is two loss launches, two scalar multiplies and an add, autograd's walk back through two
Functions and an add of two gradient tensors, all on the step's dependent chain.  The fused path forwards the student on a tape,
forwards the teacher, and gets the three losses and dL/dlogits from ONE launch (`ops.ce_kd_blend`), which the engine's backward takes as
it is.  The reference's Lwf never calls the KD tricks' blend (exp_replay.py:42-47): `kd_trick` / `kd_trick_star` change nothing in its
loss, and nothing here.  The review trick needs a buffer (base.py:62) and stays skipped."""
from .. import ops
from ..utils import AverageMeter
from ..loss import unit_gradient
from .base import ContinualLearner


class Lwf(ContinualLearner):
    T = 2.0   # loss_fn_kd's default, which the reference's get_kd_loss never overrides (kd_manager.py:6, :25)

    def __init__(self, model, opt, params):
        super(Lwf, self).__init__(model, opt, params)

    def _fused(self):
        return self._taped_ce_ok()

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
        self._track(meters, logits, batch_y, loss.detach())
        self._emit("lwf_loss", loss, loss_new=loss_new, loss_old=loss_old)
        self.opt.zero_grad()
        if self._fused():
            self.model.backward_taped(tape, dl)
        else:
            loss.backward(unit_gradient(loss))
        self.opt.step()

    def _train_learner(self, x_train, y_train):
        meters = (AverageMeter(), AverageMeter())
        for batches in self._epochs(x_train, y_train):
            for i, batch_x, batch_y, _ in batches:
                self._step(batch_x, batch_y, meters)
                self._print_running(i, meters)
        self.after_train()
