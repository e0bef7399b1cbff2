"""iCaRL on the engine (reference: agents/icarl.py:15-65).

Per stream batch the reference does: relabel the batch to column positions (old classes first, then the task's new classes in their
list order) -> one-hot target -> from the second task on: `batch` memory rows drawn uniformly from the slots this call has not written
yet, appended to the batch with all-zero targets -> forward -> the old classes' target columns replaced by the sigmoid of last task's
model -> binary cross-entropy with logits over the seen columns, summed over the columns and averaged over the rows -> backward ->
opt.step -> reservoir update, whose written slots join the exclusion list.  At the task's end the model is copied (the teacher), then
after_train() runs (the review trick's steps do not reach the teacher).  Evaluation is the nearest-class-mean classifier of base.py.

The reference builds the target with a Python loop over the batch's labels on device scalars (one host synchronisation per image), a
scatter, two cats, a sigmoid and one strided copy per old class, and lets autograd walk back through the loss.  The fused path relabels
on the host from the loader's label mirror, forwards the student over (stream batch, memory rows) as one BatchNorm group of two pieces
on a tape, forwards the teacher's parameter snapshot over the same two pieces, and gets the three losses and dL/dlogits from ONE launch
(`ops.bce_distill`), which the engine's backward takes as it is.  The label tricks and the KD tricks do not enter iCaRL's loss in the
reference, and not here; `review_trick` and `ncm_trick` take base.py's paths."""
import torch
from torch.nn import functional as F

from .. import debug
from .. import ops
from ..buffer import Buffer
from ..kd_manager import KdManager
from ..plugins.buffer_utils import random_retrieve
from .base import ContinualLearner


class Icarl(ContinualLearner):
    def __init__(self, model, opt, params):
        super(Icarl, self).__init__(model, opt, params)
        self.mem_size = params.mem_size
        self.buffer = Buffer(model, params)
        self.prev = KdManager()   # the reference's prev_model (:31): a snapshot of its own, apart from the KD tricks' kd_manager

    def _fused(self):
        # (not _taped_ce_ok(): its other two terms are the label tricks, which do not enter iCaRL's loss)
        return not self._force_autograd

    def _positions(self, y_host):
        """The batch's labels as target columns (:43-44): len(old_labels) + new_labels.index(y); ValueError for a label that is not
        among the task's new labels, as list.index raises."""
        n_old = len(self.old_labels)
        return [n_old + self.new_labels.index(y) for y in y_host.tolist()]

    def _loss_autograd(self, logits, teacher_logits, pos, n_cls):
        """:46-62 as written: ohe_label, the cat with zeros_like, the sigmoid, one column copy per old class, torch's BCE."""
        b = pos.size(0)
        target = torch.zeros((b, n_cls), device=pos.device, dtype=torch.long).scatter_(1, pos.reshape((b, 1)), 1).float()
        if teacher_logits is not None:
            target = torch.cat([target, torch.zeros_like(target)])
            q = torch.sigmoid(teacher_logits)
            for k, y in enumerate(self.old_labels):
                target[:, k] = q[:, k]
        per_element = F.binary_cross_entropy_with_logits(logits[:, :n_cls], target, reduction='none')
        return per_element.sum(dim=1).mean(), per_element

    def _step(self, train_x, train_y, y_host, updated_idx):
        pos = self._positions(y_host)
        n_old, n_cls = len(self.old_labels), len(self.new_labels) + len(self.old_labels)
        b = train_x.size(0)
        have_teacher = self.prev.teacher_model is not None
        if have_teacher:
            # the reference pairs the memory rows with zeros_like(target_labels), `batch` rows: a shorter retrieval makes its BCE raise
            # ValueError (input and target sizes differ).  Same error here, before anything is drawn or launched.
            filled = self.buffer.current_index
            valid = filled - len(updated_idx)     # a lower bound (a slot may be listed twice); counted exactly only where it matters
            if valid < self.batch:
                valid = filled - len({i for i in updated_idx if 0 <= i < filled})
            if min(self.batch, valid) != b:
                raise ValueError("iCaRL pairs %d stream rows with as many memory rows, but the memory can give %d (%d filled slots, %d "
                                 "of them written during this task)" % (b, min(self.batch, valid), filled, filled - valid))
            mem_x, _ = random_retrieve(self.buffer, self.batch, excl_indices=updated_idx)
            pieces = (train_x, mem_x)
        else:
            pieces = train_x
        pos_dev = ops.upload(torch.tensor(pos, dtype=torch.long), train_x.device)
        if self._fused():
            logits, tape = self.model.forward_views_taped([pieces])
            teacher = self.prev.teacher_logits(pieces)
            loss3, dl = ops.bce_distill(logits, teacher, pos_dev, b, n_cls, n_old if have_teacher else 0)
            if debug.on():
                debug.emit("icarl_loss", loss=float(loss3[0]), old=float(loss3[1]), new=float(loss3[2]))
            self.opt.zero_grad()
            self.model.backward_taped(tape, dl)
        else:
            logits = self.model.forward(pieces)
            self.opt.zero_grad()
            loss, per_element = self._loss_autograd(logits, self.prev.teacher_logits(pieces), pos_dev, n_cls)
            if debug.on():
                k = n_old if have_teacher else 0
                debug.emit("icarl_loss", loss=float(loss.detach()), old=float(per_element[:, :k].sum(dim=1).mean().detach()),
                           new=float(per_element[:, k:].sum(dim=1).mean().detach()))
            loss.backward()
        self.opt.step()

    def _train_learner(self, x_train, y_train):
        self.update_representation(self._epochs(x_train, y_train))
        self.prev.update_teacher(self.model)      # prev_model = copy.deepcopy(model) (:31), before after_train's review steps
        self.after_train()

    def update_representation(self, train_loader):
        """`train_loader`: the epochs of ContinualLearner._epochs."""
        updated_idx = []
        for batches in train_loader:
            for i, train_x, train_y, y_host in batches:
                self._step(train_x, train_y, y_host, updated_idx)
                updated_idx += self.buffer.update(train_x, train_y, y_host=y_host)
