"""Device tensors with sentinel regions around them, shared by the GPU parity tests (test_gpu_layers.py, test_gpu_small_ops.py).

dev() / assert_slack_untouched(): a tensor with SLACK elements of FILL behind it (the layer tests: plans may READ a padded channel split past a
tensor's end, so the slack is finite, and visible if it is accumulated).
Guarded: every tensor handed to a small-op entry point -- inputs, outputs, workspaces, index vectors -- is a view into a larger buffer with GUARD
elements of a sentinel before and after it, at a chosen offset from 16-byte alignment; after the call both regions of every tensor must be unchanged
and every input bit-identical to what was uploaded."""
import numpy as np
import torch

SLACK = 1 << 16          # elements of slack behind every dev() tensor
FILL = 4096              # what the slack holds: finite (a padded read times a zero weight still cancels), but visible if it is accumulated
GUARD = 4096             # elements of sentinel on each side of a Guarded tensor (a multiple of 16 bytes for every element size)


def dev(t):
    """A cuda copy of t (float32 / int64) with SLACK elements of FILL behind it."""
    t = t.contiguous()
    buf = torch.full((t.numel() + SLACK,), FILL, dtype=t.dtype, device="cuda")
    buf[: t.numel()].copy_(t.reshape(-1))
    return buf[: t.numel()].view(t.shape)


def assert_slack_untouched(t, what):
    """The slack behind a dev() tensor still holds FILL: nothing wrote past the tensor's end."""
    tail = t._base[t.numel():]
    assert bool((tail == FILL).all()), "%s: %d elements written past the end" % (what, int((tail != FILL).sum()))


def _fill_of(dtype):
    return 77 if dtype == torch.uint8 else FILL


class Guarded(object):
    """The tensors of one library call."""
    POISON = -7777           # what an output holds before the call (NaN-free, visible if it survives or is summed)

    def __init__(self):
        self.items = []      # (view, buffer, front, numel, name, host copy or None)

    def _place(self, shape, dtype, off, name, host):
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        front = GUARD + off
        buf = torch.full((front + n + GUARD,), _fill_of(dtype), dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[front: front + n]
        if host is not None:
            v.copy_(host.reshape(-1))
        else:
            v.fill_(77 if dtype == torch.uint8 else self.POISON)
        v = v.view(shape)
        self.items.append((v, buf, front, n, name, host))
        return v

    def inp(self, t, off=0, name="input"):
        """Upload t (a CPU tensor or numpy array) `off` elements past 16-byte alignment; check() verifies it is left unchanged."""
        t = torch.as_tensor(t).contiguous()
        return self._place(tuple(t.shape), t.dtype, off, name, t.clone())

    def out(self, shape, dtype=torch.float32, off=0, name="output", init=None):
        """An output / workspace of POISON (or a copy of init: an accumulated-onto or partly written destination)."""
        if init is not None:
            init = torch.as_tensor(init).contiguous()
            v = self._place(tuple(init.shape), init.dtype, off, name, init)
            self.items[-1] = self.items[-1][:5] + (None,)
            return v
        return self._place(tuple(shape), dtype, off, name, None)

    def check(self, what):
        torch.cuda.synchronize()
        for v, buf, front, n, name, host in self.items:
            fill = _fill_of(buf.dtype)
            lo, hi = buf[:front], buf[front + n:]
            assert bool((lo == fill).all()), "%s: %s: %d elements written before its start" % (what, name, int((lo != fill).sum()))
            assert bool((hi == fill).all()), "%s: %s: %d elements written past its end" % (what, name, int((hi != fill).sum()))
            if host is not None:
                assert v.cpu().numpy().tobytes() == host.numpy().tobytes(), "%s: input %s was modified" % (what, name)
