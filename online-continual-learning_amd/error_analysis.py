"""agents/base.py:144-153, :182-205, :209-226 -- the error analysis of evaluate(): where the wrong predictions land (old classes or the
newest task's), the mean logit of the old and of the new class columns, the mean weight and bias of the old and the new rows of the last
layer, and the task-level confusion lists.

The reference reads every one of these through the host as it goes: one .item() per predicted label, one (wrong == i).sum().item() per
class of the comparison set, a column gather with mean().item() -- 140 to 230 device synchronisations per test batch.  Here a batch is ONE
launch (ops.row_argmax_groupsum: the arg-max of every row and the sum of the row's logits over the comparison set's columns) that writes
into a loader-long device table, a loader is ONE device-to-host copy of that table, and everything else is numpy on the copy.

ErrorAnalysis is driven by ContinualLearner.evaluate() and can be driven with logits of one's own:

    ea.begin(old_labels, new_labels_zombie, class_task_map, task_seen, n_cols, device)
    for task, loader: ea.begin_loader(task, n_rows); pred = ea.batch(logits, y_host) ...; counts = ea.end_loader()
    norms = ea.end(model.linear)

TorchErrorAnalysis has the same interface and does the same bookkeeping with per-tensor torch operations and one host read per value:
the comparator of scripts/error_analysis_ab.py and of the equivalence test (ContinualLearner._force_torch_error_analysis)."""
import numpy as np
import torch

from . import ops
from .utils import AverageMeter


def to_host(t):
    """The device-to-host copy (it waits for the stream): the one synchronisation of a loader."""
    return t.cpu().numpy()


def item(t):
    """One value read through the host (TorchErrorAnalysis): a synchronisation each."""
    return t.item()


def group_table(old_labels, new_labels_zombie, n_cols):
    """int32 [n_cols]: 1 for the newest task's classes, 0 for set(old_labels) - set(new_labels_zombie), -1 for every other column."""
    g = np.full(n_cols, -1, dtype=np.int32)
    new = sorted(set(new_labels_zombie))
    old = sorted(set(old_labels) - set(new_labels_zombie))
    g[np.asarray(old, dtype=np.int64)] = 0
    g[np.asarray(new, dtype=np.int64)] = 1
    return g, old, new


def _mean_or_nan(total, count):
    return float(total) / count if count else float("nan")   # (the mean of an empty selection: what the reference's first evaluate prints)


class _Bookkeeping(object):
    """What both legs share: the class sets, the counters (zero at every begin), the two score meters and the confusion lists."""

    def begin(self, old_labels, new_labels_zombie, class_task_map, task_seen, n_cols, device):
        self.group_host, self.old_cols, self.new_cols = group_table(old_labels, new_labels_zombie, n_cols)
        self.class_task_map = class_task_map
        self.task_seen = task_seen
        self.n_cols = n_cols
        self.device = device
        self.no = self.nn = self.oo = self.on = 0
        self.new_class_score = AverageMeter()
        self.old_class_score = AverageMeter()
        self.correct_lb = []
        self.predict_lb = []
        self._begin_device()

    def _kind(self, task):
        """0: a test set of an old task, 1: the newest task's, None: a task not trained yet (accuracy only)."""
        return 0 if task < self.task_seen - 1 else (1 if task == self.task_seen - 1 else None)

    def error_tuple(self):
        return (int(self.no), int(self.nn), int(self.oo), int(self.on))

    def _norms(self, w_row_sums, n_in, bias):
        """The four means of end(): over the new / old rows of the last layer's weight (from the rows' sums) and of its bias."""
        new, old = np.asarray(self.new_cols, dtype=np.int64), np.asarray(self.old_cols, dtype=np.int64)
        return dict(fc_norm_new=_mean_or_nan(w_row_sums[new].sum(), len(new) * n_in), fc_norm_old=_mean_or_nan(w_row_sums[old].sum(), len(old) * n_in),
                    bias_norm_new=_mean_or_nan(bias[new].sum(), len(new)), bias_norm_old=_mean_or_nan(bias[old].sum(), len(old)))


class ErrorAnalysis(_Bookkeeping):
    """One ops.row_argmax_groupsum launch per batch and one per evaluate; one to_host per loader and one at the end."""

    def _begin_device(self):
        self.group = ops.upload(torch.from_numpy(self.group_host), self.device)    # once per evaluate

    def begin_loader(self, task, n_rows):
        self.task = task
        self.sel = self._kind(task)
        self.n_rows = n_rows
        self.at = 0
        self.bounds = []
        self.labels = []
        # one table, one copy: the predictions (int64) and, behind them, the rows' sums (the bits of doubles)
        self.table = torch.empty(n_rows * (2 if self.sel is not None else 1), dtype=torch.int64, device=self.device)
        self.pred = self.table[:n_rows]
        self.sums = self.table[n_rows:].view(torch.float64) if self.sel is not None else None

    def batch(self, logits, y_host):
        n, a = logits.shape[0], self.at
        if a + n > self.n_rows:
            raise RuntimeError("error analysis: the loader of task %d yields more than the %d rows announced" % (self.task, self.n_rows))
        ops.row_argmax_groupsum(logits, self.group if self.sel is not None else None, self.sel or 0, want_sum=self.sel is not None,
                                argmax_out=self.pred[a:a + n], sum_out=None if self.sel is None else self.sums[a:a + n])
        self.bounds.append((a, a + n))
        self.labels.append(np.asarray(y_host, dtype=np.int64))
        self.at = a + n
        return self.pred[a:a + n]

    def end_loader(self):
        """[(correct, n)] per batch, for the loader's accuracy meter.  The loader's one synchronisation."""
        if not self.bounds:
            return []
        table = to_host(self.table[:self.at] if self.sel is None else self.table)
        pred = table[:self.n_rows]
        sums = table[self.n_rows:].view(np.float64) if self.sel is not None else None
        k = len(self.old_cols) if self.sel == 0 else len(self.new_cols)
        score = self.old_class_score if self.sel == 0 else self.new_class_score
        counts = []
        for (a, b), y in zip(self.bounds, self.labels):
            p = pred[a:b]
            self.correct_lb += [self.task] * (b - a)
            for lbl in p.tolist():
                self.predict_lb.append(self.class_task_map[lbl])        # KeyError(label) for a class no task has introduced
            wrong = p[p != y]
            counts.append((int((p == y).sum()), b - a))
            if self.sel == 0:
                on = int((self.group_host[wrong] == 1).sum())
                self.on += on
                self.oo += len(wrong) - on
            elif self.sel == 1:
                no = int((self.group_host[wrong] == 0).sum())
                self.no += no
                self.nn += len(wrong) - no
            if self.sel is not None:
                score.update(_mean_or_nan(sums[a:b].sum(), (b - a) * k), b - a)
        return counts

    def end(self, linear):
        weight, bias = linear.weight.detach(), linear.bias.detach()
        c, n_in = weight.shape
        table = torch.empty(2 * c, dtype=torch.float64, device=weight.device)
        ops.row_argmax_groupsum(weight, None, 0, want_argmax=False, sum_out=table[:c])
        table[c:].copy_(bias)                   # (float32 -> float64 is exact; rides along in the one copy)
        host = to_host(table)
        return self._norms(host[:c], n_in, host[c:])


class TorchErrorAnalysis(_Bookkeeping):
    """The same results from per-tensor torch operations on the logits, each value read through the host as it is produced."""

    def _begin_device(self):
        self.old_idx = torch.tensor(self.old_cols, dtype=torch.int64, device=self.device)
        self.new_idx = torch.tensor(self.new_cols, dtype=torch.int64, device=self.device)

    def begin_loader(self, task, n_rows):
        self.task = task
        self.sel = self._kind(task)
        self.counts = []

    def batch(self, logits, y_host):
        n = logits.shape[0]
        y = torch.from_numpy(np.asarray(y_host, dtype=np.int64)).to(logits.device)
        _, pred = torch.max(logits, 1)
        self.counts.append((item((pred == y).sum()), n))
        self.correct_lb += [self.task] * n
        for p in pred:
            self.predict_lb.append(self.class_task_map[item(p)])
        if self.sel is None:
            return pred
        miss = pred != y
        total = item(miss.sum())
        wrong = pred[miss]
        if self.sel == 0:
            on = sum(item((wrong == c).sum()) for c in self.new_cols)
            self.on += on
            self.oo += total - on
            self.old_class_score.update(item(logits[:, self.old_idx].mean()), n)
        else:
            no = sum(item((wrong == c).sum()) for c in self.old_cols)
            self.no += no
            self.nn += total - no
            self.new_class_score.update(item(logits[:, self.new_idx].mean()), n)
        return pred

    def end_loader(self):
        return self.counts

    def end(self, linear):
        weight, bias = linear.weight.detach(), linear.bias.detach()
        return dict(fc_norm_new=item(weight[self.new_idx].mean()), fc_norm_old=item(weight[self.old_idx].mean()),
                    bias_norm_new=item(bias[self.new_idx].mean()), bias_norm_old=item(bias[self.old_idx].mean()))
