"""agents/base.py:14-227 — ContinualLearner: label bookkeeping, criterion (CE / SupCon), review trick, and
evaluate() with the nearest-class-mean classifier (NCM) or argmax, on the MI355X.

The labels trick and the separated softmax share one segmented cross-entropy kernel; the KD tricks use ocl_kd_fwd_bwd with a
parameter-snapshot teacher (kd_manager.py).

It also owns what the agents' loops share ("The agents' loop skeleton"): train_learner, the prologue and batch iteration
(_epochs), the verbose meters (_track, _print_running), the loss trace (_emit) and the predicate _taped_ce_ok."""
import abc
import contextlib
import copy
import pickle

import numpy as np
import torch

from .. import ops
from .. import debug
from ..data import DeviceLoader
from ..loss import SupConLoss, cross_entropy_mean, cross_entropy_segmented_mean, unit_gradient
from ..kd_manager import KdManager
from ..error_analysis import ErrorAnalysis, TorchErrorAnalysis
from ..utils import maybe_cuda, AverageMeter


class ContinualLearner(torch.nn.Module, metaclass=abc.ABCMeta):
    '''
    Abstract module which is inherited by each and every continual learning algorithm.
    '''

    def __init__(self, model, opt, params):
        super(ContinualLearner, self).__init__()
        self.params = params
        self.model = model
        self.opt = opt
        self.data = params.data
        self.cuda = params.cuda
        self.epoch = params.epoch
        self.batch = params.batch
        self.verbose = params.verbose
        self.old_labels = []
        self.new_labels = []
        self.task_seen = 0
        self.lbl_inv_map = {}
        self.class_task_map = {}
        self.kd_manager = KdManager()
        # agents/base.py:33-39: what evaluate() appends to with params.error_analysis (error_analysis.py)
        self.error_list = []
        self.new_class_score = []
        self.old_class_score = []
        self.fc_norm_new = []
        self.fc_norm_old = []
        self.bias_norm_new = []
        self.bias_norm_old = []
        if getattr(params, 'error_analysis', False) and self._predicts_by_ncm():
            raise NotImplementedError(
                "error_analysis with nearest-class-mean prediction (ncm_trick, or agent ICARL, SCR or SCP) is not defined: the reference's "
                "branch reads the `logits` its NCM path never computes, and compares indices into old_labels with class labels")

    _gc_frozen = False
    _same_weights = True                   # train_learner runs the loop inside model.same_weights() (False: SCR, one forward per step; GDumb, whose loop replaces self.model)
    _force_torch_error_analysis = False    # the error analysis by per-tensor torch operations and host reads (the comparator of the fused path)
    _force_autograd = False                # the A/Bs' and the tests' comparator: the loss through criterion / torch ops and autograd instead of the taped backward
    _force_losses = False                  # ER, ASER mode: run the losses of passes 1 and 2 although nobody reads them (_passes_12_have_readers)

    def _predicts_by_ncm(self):
        return self.params.trick['ncm_trick'] or self.params.agent in ['ICARL', 'SCR', 'SCP']

    @classmethod
    def _freeze_long_lived_objects(cls):
        """Once per process, at the first training call: gc.freeze() moves everything alive (the imported packages' ~10^6 containers, the
        model, the replay memory's bookkeeping) to the collector's permanent generation.  Without it CPython's full (generation 2)
        collection walks all of them whenever its counters say so -- 105 - 133 ms in the middle of a training loop whose step is 3 ms
        (profiles/r6_aser_stall_probe.txt: the deterministic '+0.8 ms per step' of every fifth repeat of the ASER bench leg, at the same
        step of a fixed-seed run, was exactly one such collection).  Reference counting is untouched: frozen objects are still freed when
        their last reference goes, only cycle detection skips them; collections keep running over everything created afterwards.
        OCL_GC_FREEZE=0 turns it off."""
        if cls._gc_frozen:
            return
        cls._gc_frozen = True
        import gc
        import os
        if os.environ.get("OCL_GC_FREEZE", "1") != "0":
            gc.collect()
            gc.freeze()
        # (the young generations' collections do not show in the step: collector off / threshold 100000 change nothing, profiles/r6_gc_threshold_ab.txt)

    def before_train(self, x_train, y_train):
        """agents/base.py:43-50."""
        self._freeze_long_lived_objects()
        new_labels = list(set(y_train.tolist()))
        self.new_labels += new_labels
        for i, lbl in enumerate(new_labels):
            self.lbl_inv_map[lbl] = len(self.old_labels) + i

        for i in new_labels:
            self.class_task_map[i] = self.task_seen

    # ---- what every agent's loop shares --------------------------------------------------------------------------------------------
    def train_learner(self, x_train, y_train):
        """One task: the agent's `_train_learner` inside launch_stream() and, where `_same_weights` says so, model.same_weights():
        between two optimiser steps every forward of the loop reads the same weights (ASER mode: five of them per iteration), and
        inside that block the engine packs them once per step (resnet.py; writes by anybody else are detected, not assumed away)."""
        with self.launch_stream(), (self.model.same_weights() if self._same_weights else contextlib.nullcontext()):
            self._train_learner(x_train, y_train)

    def _train_learner(self, x_train, y_train):
        raise NotImplementedError

    def _epochs(self, x_train, y_train, epochs=None, train=True, data=None):
        """The loop's prologue -- before_train, the device-resident task behind the reference's DataLoader (same sampler, same RNG
        draws), the model in train mode -- done at the call; returns an iterable with one iterable of (i, batch_x, batch_y, batch_y_host)
        per epoch.  `data` (agents/_streams.py) is opened behind the prologue, and the loader's gathers are issued on its stream."""
        self.before_train(x_train, y_train)
        train_loader = DeviceLoader(x_train, y_train, self.batch, shuffle=True, drop_last=True)
        if train:
            self.model = self.model.train()
        on_data = contextlib.nullcontext
        if data is not None:
            data.open()
            on_data = data.on_data

        def batches():
            loader_it = iter(train_loader)
            i = 0
            while True:
                with on_data():
                    batch_data = next(loader_it, None)
                if batch_data is None:
                    return
                yield i, batch_data[0], batch_data[1], train_loader.last_y_host
                i += 1

        return (batches() for ep in range(self.epoch if epochs is None else epochs))

    def _track(self, meters, logits, labels, value):
        """Running loss / accuracy (only when printing: the reference's per-iteration .item() would stall the stream).  `meters` is
        (loss meter, accuracy meter); logits=None records the loss alone."""
        if not self.verbose:
            return
        loss_meter, acc_meter = meters
        if logits is not None:
            hits = (torch.max(logits, 1)[1] == labels).sum()
            acc_meter.update(hits / labels.size(0), labels.size(0))
        loss_meter.update(value, labels.size(0))

    _running_format = '==>>> it: {}, {}avg. loss: {:.6f}, running {}acc: {:.3f}'

    def _print_running(self, i, meters, tag=""):
        if i % 100 == 1 and self.verbose:
            print(self._running_format.format(i, tag, meters[0].avg(), tag or "train ", meters[1].avg()))

    @staticmethod
    def _emit(tag, loss, **more):
        """A debug event of a step's loss (and further scalars): each value is fetched -- a host synchronisation -- only when tracing."""
        if debug.on():
            debug.emit(tag, loss=float(loss.detach()), **{k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in more.items()})

    def _taped_ce_ok(self):
        """Plain cross-entropy (agents/base.py:113) on the engine's taped backward: the loss kernel's dL/dlogits may go straight into
        model.backward_taped, without autograd between the two."""
        trick = self.params.trick
        return not trick['labels_trick'] and not trick['separated_softmax'] and not self._force_autograd

    def launch_stream(self):
        """Context for the training loop.  With launch-sequence replay requested (OCL_GRAPH=1, csrc/net.hip run_replayed) the loop runs
        on a stream of its own, ordered after and before the caller's stream: hipStreamBeginCapture is refused on the default stream,
        and the replay is what keeps a host-bound loop (ER + ASER: one synchronisation per step) from waiting on launch calls."""
        import os

        @contextlib.contextmanager
        def ctx():
            # (the loop on a HIGH-priority stream of its own against the lowest-priority weight-gradient stream: no gain on SCR, ER + 0.02 ms --
            # profiles/r6_loop_prio_ab.txt; the switch is gone)
            if not (self.cuda and os.environ.get("OCL_GRAPH") == "1") or debug.on():
                yield
                return
            cur = torch.cuda.current_stream()
            if cur != torch.cuda.default_stream():
                yield
                return
            own = self.__dict__.get("_ocl_stream")
            if own is None:
                own = self.__dict__["_ocl_stream"] = torch.cuda.Stream()
            own.wait_stream(cur)
            with torch.cuda.stream(own):
                yield
            cur.wait_stream(own)
        return ctx()

    def after_train(self):
        """agents/base.py:56-91 (review trick branch :62-88)."""
        self.old_labels += self.new_labels
        self.new_labels_zombie = copy.deepcopy(self.new_labels)
        self.new_labels.clear()
        self.task_seen += 1
        if self.params.trick['review_trick'] and hasattr(self, 'buffer'):
            self.model.train()
            filled = self.buffer.current_index
            if filled > 0:
                from torch.utils.data import DataLoader
                from ..data import _IndexDataset
                bs = self.params.eps_mem_batch
                rv_loader = DataLoader(_IndexDataset(filled), batch_size=bs, shuffle=True, num_workers=0, drop_last=True)
                dev = self.buffer.buffer_img.device
                for ep in range(1):
                    for i, idx in enumerate(rv_loader):
                        idx = idx.to(dev)
                        batch_x = ops.gather_rows(self.buffer.buffer_img, idx)
                        batch_y = ops.gather_rows(self.buffer.buffer_label, idx)
                        if self.params.agent == 'SCR':
                            # the reference also runs one extra plain forward whose only effect is a BatchNorm
                            # running-stat update (base.py:77) before the two-view forwards (:78-80)
                            with torch.no_grad():
                                self.model.forward(batch_x)
                            feats = self.model.forward_views([batch_x, self.transform(batch_x)])
                            loss = self.criterion_views(feats, batch_y, 2)
                        else:
                            logits = self.model.forward(batch_x)
                            loss = self.criterion(logits, batch_y)
                        if debug.on():
                            debug.emit("review", indices=idx.cpu().numpy().copy(), loss=float(loss.detach()))
                        self.opt.zero_grad()
                        loss.backward(unit_gradient(loss))
                        self._step_scaled(0.1)   # grads / 10 (base.py:84-87)
        if self.params.trick['kd_trick'] or self.params.agent == 'LWF':   # base.py:90-91 (kd_trick_star alone never gets a teacher)
            self.kd_manager.update_teacher(self.model)

    def _step_scaled(self, scale):
        if hasattr(self.opt, "model"):
            self.opt.step(grad_scale=scale)
        else:   # a stock torch optimiser: setup_opt never returns one, scripts/adam_step_ab.py builds its comparator around one

            for p in self.model.parameters():
                if p.requires_grad and p.grad is not None:
                    p.grad.data.mul_(scale)
            self.opt.step()

    def _kd_mix(self, loss, logits, x):
        """CE blended with the distillation loss against last task's model (exp_replay.py:42-47 / :64-69, agem.py:41-46)."""
        trick = self.params.trick
        if trick['kd_trick']:
            w = 1 / (self.task_seen + 1)
            loss = w * loss + (1 - w) * self.kd_manager.get_kd_loss(logits, x)
        if trick['kd_trick_star']:
            w = 1 / ((self.task_seen + 1) ** 0.5)
            loss = w * loss + (1 - w) * self.kd_manager.get_kd_loss(logits, x)
        return loss

    def _kd_weight(self):
        """The factor _kd_mix puts on the loss it is given (1 without the KD tricks): what a term of that loss whose gradient is formed
        outside autograd has to carry (ewc_pp.py:45-51 blend the whole total_loss, penalty included)."""
        trick = self.params.trick
        w = 1.0
        if trick['kd_trick']:
            w *= 1 / (self.task_seen + 1)
        if trick['kd_trick_star']:
            w *= 1 / ((self.task_seen + 1) ** 0.5)
        return w

    def _host_labels(self, labels):
        h = getattr(labels, 'host', None)
        return np.asarray(h).astype(np.int64) if h is not None else labels.detach().cpu().numpy().astype(np.int64)

    def criterion(self, logits, labels):
        """agents/base.py:93-113.  The labels trick (:96-101) and the separated softmax (:102-108) are one kernel: a softmax
        over the logit columns of the row's label segment (ocl_ce_segmented_fwd_bwd); the segment table is built on the host
        from the labels' numpy mirror, as the reference builds `unq_lbls` / `lbl_inv_map`."""
        if self.params.trick['labels_trick']:
            y_host = self._host_labels(labels)
            seg = np.full(logits.shape[1], -1, dtype=np.int32)
            seg[np.unique(y_host)] = 0          # labels.unique().sort()[0]: the heads that appear in the batch
            return cross_entropy_segmented_mean(logits, labels, ops.upload(torch.from_numpy(seg), logits.device))
        elif self.params.trick['separated_softmax']:
            y_host = self._host_labels(labels)
            for lbl in y_host.tolist():
                self.lbl_inv_map[lbl]           # KeyError for a label outside old_labels + new_labels, as in the reference (:106)
            seg = np.full(logits.shape[1], -1, dtype=np.int32)
            seg[np.asarray(self.old_labels, dtype=np.int64)] = 0
            seg[np.asarray(self.new_labels, dtype=np.int64)] = 1
            return cross_entropy_segmented_mean(logits, labels, ops.upload(torch.from_numpy(seg), logits.device))
        # (the reference clones the labels first, agents/base.py:94, because its label tricks relabel in place; nothing here writes to them: no copy launch)
        if self.params.agent in ['SCR', 'SCP']:
            SC = SupConLoss(temperature=self.params.temp)
            return SC(logits, labels)
        else:
            return cross_entropy_mean(logits, labels)

    def criterion_views(self, feat_view_major, labels, n_views):
        """SupConLoss on the engine's native view-major [n_views*bsz, dim] layout (no permute / cat)."""
        SC = SupConLoss(temperature=self.params.temp)
        return SC.forward_view_major(feat_view_major, labels, n_views)

    def forward(self, x):
        return self.model.forward(x)

    def evaluate(self, test_loaders):
        """agents/base.py:118-227.  The reference extracts exemplar features one image at a time (:130-134);
        eval-mode BatchNorm makes the batched extraction below numerically equivalent per sample."""
        self.model.eval()
        acc_array = np.zeros(len(test_loaders))
        use_ncm = self._predicts_by_ncm()
        if use_ncm:
            buffer_filled = self.buffer.current_index
            dev = self.buffer.buffer_img.device
            labels = self.buffer.buffer_label[:buffer_filled].contiguous()
            # every buffered label must be a seen class (the reference would raise KeyError, base.py:126)
            host_labels = set(self.buffer.label_host[:buffer_filled].tolist())
            missing = host_labels - set(self.old_labels)
            if missing:
                raise KeyError(sorted(missing)[0])
            class_ids = torch.tensor(self.old_labels, dtype=torch.long, device=dev)
            with torch.no_grad():
                if buffer_filled > 0:
                    feats = self.model.features_batched(self.buffer.buffer_img[:buffer_filled])
                else:
                    feats = torch.zeros((0, self.model.feature_dim), device=dev)
                means, counts = ops.ncm_class_means(feats, labels, class_ids)
                counts_h = counts.cpu().numpy()
                for ci in range(len(self.old_labels)):   # dict order of cls_exemplar = old_labels order
                    if counts_h[ci] == 0:
                        # no exemplar: random mean (base.py:135-137), drawn on the CPU generator
                        mu_y = torch.normal(0, 1, size=(1, feats.shape[1])).squeeze()
                        mu_y = mu_y / mu_y.norm()
                        means[ci] = mu_y.to(dev)
        ea = None
        if getattr(self.params, 'error_analysis', False):
            # agents/base.py:144-153: counters, score meters and confusion lists start afresh in every call
            ea = TorchErrorAnalysis() if self._force_torch_error_analysis else ErrorAnalysis()
            ea.begin(self.old_labels, self.new_labels_zombie, self.class_task_map, self.task_seen, self.model.linear.out_features,
                     self.model.linear.weight.device)
        with torch.no_grad():
            for task, test_loader in enumerate(test_loaders):
                acc = AverageMeter()
                correct = []
                sizes = []
                seen_idx, seen_pred = [], []
                if ea is not None:
                    ea.begin_loader(task, self._loader_rows(test_loader))
                for i, (batch_x, batch_y) in enumerate(test_loader):
                    batch_x = maybe_cuda(batch_x, self.cuda)
                    batch_y = maybe_cuda(batch_y, self.cuda)
                    if ea is not None:
                        # the softmax branch through error_analysis.py: one launch for the batch, read with the loader's one copy below
                        logits = self.model.forward(batch_x)
                        pred_label = ea.batch(logits, self._host_labels(batch_y))
                        if debug.on():
                            seen_idx.append(np.asarray(test_loader.last_index_host).copy())
                            seen_pred.append(pred_label.cpu().numpy())
                        continue
                    if use_ncm:
                        feature = self.model.features_batched(batch_x)  # (batch_size, feature_size)
                        pred = ops.ncm_predict(feature, means)
                        pred_label = ops.gather_rows(class_ids, pred)
                    else:
                        logits = self.model.forward(batch_x)
                        _, pred_label = torch.max(logits, 1)
                    correct.append((pred_label == batch_y).sum())
                    sizes.append(batch_y.size(0))
                    if debug.on():
                        seen_idx.append(np.asarray(test_loader.last_index_host).copy())
                        seen_pred.append(pred_label.cpu().numpy())
                if debug.on():
                    debug.emit("evaluate", task=task, index=np.concatenate(seen_idx) if seen_idx else np.zeros(0, dtype=np.int64),
                               pred=np.concatenate(seen_pred) if seen_pred else np.zeros(0, dtype=np.int64))
                if ea is not None:
                    for c, n in ea.end_loader():                      # one sync per task loader
                        acc.update(c / n, n)
                elif correct:
                    correct_h = torch.stack(correct).cpu().tolist()   # one sync per task loader
                    for c, n in zip(correct_h, sizes):
                        acc.update(c / n, n)
                acc_array[task] = acc.avg()
        print(acc_array)
        if ea is not None:
            self._report_error_analysis(ea)
        return acc_array

    @staticmethod
    def _loader_rows(test_loader):
        """The number of rows a test loader will yield (the length of the error analysis' device tables)."""
        y_host = getattr(test_loader, 'y_host', None)
        return len(y_host) if y_host is not None else len(test_loader.dataset)

    def _report_error_analysis(self, ea):
        """agents/base.py:209-226: the appends, the prints and the `confusion` file of the reference, in its order."""
        no, nn, oo, on = ea.error_tuple()
        self.error_list.append((no, nn, oo, on))
        self.new_class_score.append(ea.new_class_score.avg())
        self.old_class_score.append(ea.old_class_score.avg())
        print("no ratio: {}\non ratio: {}".format(no / (no + nn + 0.1), on / (oo + on + 0.1)))
        print(self.error_list)
        print(self.new_class_score)
        print(self.old_class_score)
        norms = ea.end(self.model.linear)
        self.fc_norm_new.append(norms['fc_norm_new'])
        self.fc_norm_old.append(norms['fc_norm_old'])
        self.bias_norm_new.append(norms['bias_norm_new'])
        self.bias_norm_old.append(norms['bias_norm_old'])
        print(self.fc_norm_old)
        print(self.fc_norm_new)
        print(self.bias_norm_old)
        print(self.bias_norm_new)
        self.confusion = [ea.correct_lb, ea.predict_lb]
        with open('confusion', 'wb') as fp:
            pickle.dump(self.confusion, fp)
