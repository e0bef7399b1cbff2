"""EWC++ on the engine (reference: agents/ewc_pp.py:8-106).

Per stream batch the reference does: [every fisher_update_after iterations: running Fisher <- exponential moving average with the
temporary Fisher, temporary Fisher <- 0] -> forward -> CE + lambda * sum f_hat * (p - p_prev)^2 (from the second task on) -> backward
-> temporary Fisher += grad^2 -> opt.step; at the task's end it keeps a copy of the parameters and normalises the running Fisher by
its global min and max.  The reference holds all of that as four dictionaries of 62 tensors and lets autograd differentiate the
penalty.  Here the four are flat arrays beside model.flat_params(): the penalty's gradient 2 * lambda * w * f_hat * (p - p_prev) and
the Fisher accumulation are one launch on the flat gradient array (`ops.ewc_accumulate`), the moving average one launch
(`ops.ewc_fisher_ema`), the normalisation two (`ops.ewc_fisher_normalize`).  There is no replay memory."""
import torch

from .. import debug
from .. import ops
from ..utils import AverageMeter
from ..loss import unit_gradient
from .base import ContinualLearner


class EWC_pp(ContinualLearner):
    _force_torch_bookkeeping = False   # the A/B's and one test's comparator: the reference's per-tensor statements over the p / p.grad views

    def __init__(self, model, opt, params):
        super(EWC_pp, self).__init__(model, opt, params)
        self.lambda_ = params.lambda_
        self.alpha = params.alpha
        self.fisher_update_after = params.fisher_update_after
        self.prev_params = None            # None until the first task ends (the reference's `len(self.prev_params) == 0`)
        self.running_fisher = self.tmp_fisher = self.normalized_fisher = None
        self._penalty = self._minmax = None
        if next(model.parameters()).is_cuda:
            self._ensure_state()

    def _ensure_state(self):
        """The flat arrays of init_fisher() (:94-95), allocated once the model is on its device."""
        flat = self.model.flat_params()
        if self.tmp_fisher is None or self.tmp_fisher.shape != flat.shape or self.tmp_fisher.device != flat.device:
            self.running_fisher, self.tmp_fisher, self.normalized_fisher = (torch.zeros_like(flat) for _ in range(3))
            self._penalty = torch.zeros(1, dtype=torch.float32, device=flat.device)
            self._minmax = torch.zeros(2, dtype=torch.float32, device=flat.device)
        return flat

    # ---- the reference's statements, tensor by tensor (the comparator) ---------------------------------------------------------
    def _per_tensor(self, flat_array):
        """The array cut as model.parameters() cuts the flat parameter array: one view per parameter tensor."""
        base = self.model.flat_params()
        return [flat_array[(p.data_ptr() - base.data_ptr()) // 4:][:p.numel()].view(p.shape) for p in self.model.parameters() if p.requires_grad]

    def _update_running_fisher_torch(self):
        for r, t in zip(self._per_tensor(self.running_fisher), self._per_tensor(self.tmp_fisher)):
            r.copy_((1. - self.alpha) * r + 1. / self.fisher_update_after * self.alpha * t)      # :99-100
            t.fill_(0)                                                                           # :102

    def _accumulate_torch(self, w):
        params = [p for p in self.model.parameters() if p.requires_grad]
        penalty = None
        if self.prev_params is not None:
            reg_loss = 0
            for f, p, q in zip(self._per_tensor(self.normalized_fisher), params, self._per_tensor(self.prev_params)):
                reg_loss += (f * (p - q) ** 2).sum()                                             # :89-90
            penalty = reg_loss.detach()
            for p, g in zip(params, torch.autograd.grad(w * (self.lambda_ * reg_loss), params)):  # :91 and the blend's weight, :59
                p.grad += g
        for t, p in zip(self._per_tensor(self.tmp_fisher), params):
            t += p.grad ** 2                                                                     # :105-106
        return penalty

    def _task_end_torch(self):
        params = [p for p in self.model.parameters() if p.requires_grad]
        if self.prev_params is None:
            self.prev_params = torch.empty_like(self.model.flat_params())
        for q, p in zip(self._per_tensor(self.prev_params), params):
            q.copy_(p.detach())                                                                  # :73-74
        running = self._per_tensor(self.running_fisher)
        max_fisher = max([torch.max(m) for m in running])                                        # :77
        min_fisher = min([torch.min(m) for m in running])                                        # :78
        for f, r in zip(self._per_tensor(self.normalized_fisher), running):
            f.copy_((r - min_fisher) / (max_fisher - min_fisher + 1e-32))                        # :80
        self._minmax.copy_(torch.stack([min_fisher, max_fisher]))

    # ---- pieces of a step ----------------------------------------------------------------------------------------------------------
    def _update_running_fisher(self):
        if self._force_torch_bookkeeping:
            self._update_running_fisher_torch()
        else:
            # keep and gain as the reference's expression forms them in double (:99-100); the kernel rounds each to float32, as torch does
            ops.ewc_fisher_ema(self.running_fisher, self.tmp_fisher, keep=1. - self.alpha, gain=1. / self.fisher_update_after * self.alpha)
        if debug.on():
            debug.emit("ewc_fisher_update")

    def _step(self, batch_x, batch_y, meters):
        logits = self.model.forward(batch_x)
        w = self._kd_weight()
        loss = self._kd_mix(self.criterion(logits, batch_y), logits, batch_x)
        self.opt.zero_grad()
        loss.backward(unit_gradient(loss))

        # the penalty's gradient and the Fisher of the current batch (:62); the penalty's value only where somebody reads it
        want = self.verbose or debug.on()
        penalty = None
        if self._force_torch_bookkeeping:
            penalty = self._accumulate_torch(w)
        else:
            seen = self.prev_params is not None
            ops.ewc_accumulate(self.model.flat_grads(), self.tmp_fisher, self.model.flat_params(), self.prev_params,
                               self.normalized_fisher if seen else None, scale=2 * self.lambda_ * w,
                               penalty_out=self._penalty if (want and seen) else None)
            if want and seen:
                penalty = self._penalty[0]
        if self.verbose:
            self._track(meters, logits, batch_y, loss.detach() if penalty is None else loss.detach() + (w * self.lambda_) * penalty)
        self._emit("ewc_loss", loss, penalty=0.0 if penalty is None else penalty)
        self.opt.step()

    def _task_end(self):
        if self._force_torch_bookkeeping:
            self._task_end_torch()
        else:
            flat = self.model.flat_params()
            if self.prev_params is None:
                self.prev_params = torch.empty_like(flat)
            self.prev_params.copy_(flat)                                                         # save params for current task (:73-74)
            ops.ewc_fisher_normalize(self.running_fisher, self.normalized_fisher, minmax_out=self._minmax if debug.on() else None)
        if debug.on():
            lo, hi = self._minmax.cpu().tolist()
            debug.emit("ewc_task_end", min_fisher=lo, max_fisher=hi)

    # ---- the loop ------------------------------------------------------------------------------------------------------------------
    def before_train(self, x_train, y_train):
        """The flat arrays exist before the task is moved to the device (a model moved after the constructor: allocated here)."""
        super(EWC_pp, self).before_train(x_train, y_train)
        self._ensure_state()

    def _train_learner(self, x_train, y_train):
        meters = (AverageMeter(), AverageMeter())
        it = 0
        for batches in self._epochs(x_train, y_train):
            for i, batch_x, batch_y, _ in batches:
                # update the running fisher (:41-42, (ep * len(train_loader) + i + 1) % fisher_update_after): the count of the call's
                # iterations restarts with every call, the temporary Fisher does not
                it += 1
                if it % self.fisher_update_after == 0:
                    self._update_running_fisher()
                self._step(batch_x, batch_y, meters)
                self._print_running(i, meters)
        self._task_end()
        self.after_train()
