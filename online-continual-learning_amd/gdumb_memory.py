"""GDumb's greedy class-balanced sampler (reference: agents/gdumb.py:19-31) as a host-side planner over slot numbers and a
device-resident memory that applies a whole batch's plan with one scatter.

The reference keeps a Python list of image tensors per class, appends and pops one sample at a time and asks the device for every
label (`.item()`).  Here the decisions -- which depend on the labels and on Python's `random` alone -- are taken on the host from the
loader's label mirror, and the images never leave the device."""
import random

import numpy as np
import torch

from . import ops


class GreedyBalancer(object):
    """The reference's `mem_c` (class -> count) and `mem_img` (class -> list, here of memory slots instead of tensors), in the same
    dict insertion order and list order, plus the list of free slots.  No torch device is involved."""

    def __init__(self, mem_size):
        self.mem_size = int(mem_size)
        self.mem_c = {}
        self.mem_slots = {}
        self.free = list(range(self.mem_size - 1, -1, -1))   # a stack: slot 0 goes first, a slot just evicted is the next one filled

    def _update(self, y, row, writes):
        """agents/gdumb.py:19-31 for one sample; `writes[slot] = row` stands for `mem_img[y].append(x)`."""
        k_c = self.mem_size // max(1, len(self.mem_slots))
        if y not in self.mem_slots or self.mem_c[y] < k_c:
            if sum(self.mem_c.values()) >= self.mem_size:
                cls_max = max(self.mem_c.items(), key=lambda k: k[1])[0]      # the first maximum in dict order
                idx = random.randrange(self.mem_c[cls_max])
                self.free.append(self.mem_slots[cls_max].pop(idx))
                self.mem_c[cls_max] -= 1
            if y not in self.mem_slots:
                self.mem_slots[y] = []
                self.mem_c[y] = 0
            slot = self.free.pop()
            self.mem_slots[y].append(slot)
            self.mem_c[y] += 1
            writes[slot] = row

    def plan(self, y_host):
        """The greedy update for the labels of one batch, in order.  Returns (rows, slots): row rows[i] of the batch is to be written
        to slot slots[i].  A slot filled, evicted and refilled within the batch appears once, with its last writer (an evicted slot is
        always the next one filled, so none is left holding a row that was dropped again)."""
        writes = {}
        for row, y in enumerate(np.asarray(y_host).tolist()):
            self._update(y, row, writes)
        slots = np.fromiter(writes.keys(), dtype=np.int64, count=len(writes))
        rows = np.fromiter(writes.values(), dtype=np.int64, count=len(writes))
        return rows, slots

    def order(self):
        """(slots, labels) in the order train_mem concatenates the per-class lists (agents/gdumb.py:55-57)."""
        slots, labels = [], []
        for c in self.mem_slots.keys():
            slots += self.mem_slots[c]
            labels += [c] * self.mem_c[c]
        return np.asarray(slots, dtype=np.int64), np.asarray(labels, dtype=np.int64)


class GdumbMemory(object):
    """img [mem_size, C, H, W] float32 and label [mem_size] int64 on the device, filled by GreedyBalancer's plans.

    update() is one scatter launch: the whole batch is scattered, the rows the plan keeps to their slots and every other row j to spare
    row mem_size + j behind the memory (distinct targets: no duplicate index).  The labels are decided on the host; their device copy
    is refreshed by one upload when it is next read."""

    def __init__(self, mem_size, shape, device, batch=10):
        self.mem_size = int(mem_size)
        self.balancer = GreedyBalancer(mem_size)
        self._spare = max(1, int(batch))
        self._store = torch.zeros((self.mem_size + self._spare,) + tuple(shape), dtype=torch.float32, device=device)
        self.img = self._store[:self.mem_size]
        self.label_host = np.zeros(self.mem_size, dtype=np.int64)
        self._label = torch.zeros(self.mem_size, dtype=torch.int64, device=device)
        self._label_stale = False

    @property
    def label(self):
        if self._label_stale:
            self._label = ops.upload(torch.from_numpy(self.label_host.copy()), self._store.device)
            self._label_stale = False
        return self._label

    def update(self, batch_x, y_host):
        y_host = np.asarray(y_host, dtype=np.int64)
        if batch_x.shape[0] != y_host.shape[0]:
            raise RuntimeError("GdumbMemory.update: %d images, %d labels" % (batch_x.shape[0], y_host.shape[0]))
        rows, slots = self.balancer.plan(y_host)
        if rows.shape[0] == 0:
            return slots
        self.label_host[slots] = y_host[rows]
        self._label_stale = True
        batch_x = batch_x.contiguous()
        for lo in range(0, batch_x.shape[0], self._spare):     # one pass for a batch of at most `batch` rows
            hi = min(lo + self._spare, batch_x.shape[0])
            target = self.mem_size + np.arange(hi - lo, dtype=np.int64)
            sel = (rows >= lo) & (rows < hi)
            if not sel.any():
                continue
            target[rows[sel] - lo] = slots[sel]
            ops.scatter_rows(self._store, ops.upload(torch.from_numpy(target), self._store.device), batch_x[lo:hi])
        return slots

    def order(self):
        return self.balancer.order()
