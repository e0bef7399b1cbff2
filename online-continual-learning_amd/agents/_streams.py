"""The data path of a replay loop on a stream of its own (agents/exp_replay.py, agents/scr.py).

Loader gather, retrieve gather, concatenation / augmentation and reservoir scatter never touch the model: ~20 tiny launches per step,
~0.15 ms back to back, 5 % of a 1 ms step.  Issued on a second stream, those of step i+1 run next to step i's backward instead of in
front of step i+1's forward.  The statements, their order and the RNG draws are those of the loop without it; only the stream they are
issued on differs.  Each agent decides with a predicate of its own when that is safe; OCL_DATA_STREAM=0 turns it off for all of them
(everything on the main stream)."""
import contextlib
import os

import torch

from .. import ops


class DataStream(object):
    """`with data.on_data():` around the data statements, `data.hand_over(...)` before the main stream consumes what they made,
    `data.join()` after the loop.  `on` is the agent's predicate; where it (or the switch) says no, all of them do nothing.
    ContinualLearner._epochs opens it, once the task is on the device."""

    def __init__(self, on, x_train):
        self.on = on and os.environ.get("OCL_DATA_STREAM", "1") != "0"
        self.x_train = x_train
        self.main = self.ds = None

    def open(self):
        if self.on:
            x_train = self.x_train
            self.main = torch.cuda.current_stream()
            self.ds = ops.data_stream(x_train.device if torch.is_tensor(x_train) and x_train.is_cuda else torch.cuda.current_device())
            self.ds.wait_stream(self.main)

    def on_data(self):
        return torch.cuda.stream(self.ds) if self.on else contextlib.nullcontext()

    def hand_over(self, *tensors):
        if self.on:
            self.main.wait_stream(self.ds)
            for t in tensors:
                t.record_stream(self.main)   # allocated on the data stream, consumed on the main one

    def join(self):
        if self.on:
            self.main.wait_stream(self.ds)
