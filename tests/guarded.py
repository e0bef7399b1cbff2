"""Device tensors with sentinel regions around them, shared by the GPU parity tests (test_gpu_layers.py, test_gpu_small_ops.py).

dev() / assert_slack_untouched(): a tensor with SLACK elements of FILL behind it (the layer tests: plans may READ a padded channel split past a
tensor's end, so the slack is finite, and visible if it is accumulated).
Guarded: every tensor handed to a small-op entry point -- inputs, outputs, workspaces, index vectors -- is a view into a larger buffer with GUARD
elements of a sentinel before and after it, at a chosen offset from 16-byte alignment; after the call both regions of every tensor must be unchanged
and every input bit-identical to what was uploaded.

The NaN leg (nan_leg(); run_both_legs()): the same call with every output, workspace and guard region of a floating tensor holding all-ones bits
(0xFFFFFFFF: a NaN) and those of an integer tensor the type's minimum, instead of the finite POISON / FILL.  A kernel that reads a cell it has not
written -- an output it accumulates onto, a workspace it assumes zero, an element past a tensor's end that it multiplies by zero -- gives another
result there; what the call leaves in every output must equal the finite leg's bit for bit (cells neither leg wrote hold each leg's own poison).
Outputs created with init= are accumulated onto by contract and keep their contents in both legs.  check() compares bit patterns in both legs."""
import contextlib

import numpy as np
import torch

SLACK = 1 << 16          # elements of slack behind every dev() tensor
FILL = 4096              # what the slack holds: finite (a padded read times a zero weight still cancels), but visible if it is accumulated
GUARD = 4096             # elements of sentinel on each side of a Guarded tensor (a multiple of 16 bytes for every element size)

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NP_VIEW = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


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


def _bits(t):
    """A torch tensor's elements as integers of the same size (bit patterns)."""
    return t.view(_INT_VIEW[t.element_size()])


class Guarded(object):
    """The tensors of one library call."""
    POISON = -7777           # what an output holds before the call in the finite leg (NaN-free, visible if it survives or is summed)
    LEG = "finite"           # "nan" inside nan_leg()
    RECORD = None            # inside run_both_legs(): what check() found in every output, call by call

    def __init__(self):
        self.items = []      # (view, buffer, front, numel, name, host copy or None)
        self.leg = Guarded.LEG

    # ---- what unwritten memory holds in this leg ---------------------------------------------------------------------------------------
    @classmethod
    def _value(cls, dtype, guard, leg=None):
        """A one-element CPU tensor of dtype: the guard regions' sentinel (guard) or an output's pre-fill."""
        leg = leg or cls.LEG
        t = torch.empty(1, dtype=dtype)
        if leg == "nan":
            if dtype.is_floating_point:
                t.view(torch.uint8).fill_(255)
            else:
                t.fill_(torch.iinfo(dtype).min)
        else:
            t.fill_(_fill_of(dtype) if guard else (77 if dtype == torch.uint8 else cls.POISON))
        return t

    @classmethod
    def is_poison(cls, a):
        """Elementwise: a (numpy array or torch tensor, an output's dtype) still holds the current leg's output pre-fill, by bit pattern."""
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        want = cls._value(torch.from_numpy(np.empty(0, a.dtype)).dtype, False).numpy()
        view = _NP_VIEW[a.dtype.itemsize]
        return np.ascontiguousarray(a).view(view) == want.view(view)[0]

    @classmethod
    def poison_array(cls, n, dtype):
        """A host array of n elements of the current leg's output pre-fill (what a partly written output is expected to keep)."""
        want = cls._value(torch.from_numpy(np.empty(0, dtype)).dtype, False).numpy()
        view = _NP_VIEW[want.dtype.itemsize]
        out = np.empty(n, want.dtype)
        out.view(view)[:] = want.view(view)[0]
        return out

    def _place(self, shape, dtype, off, name, host):
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        front = GUARD + off
        buf = torch.empty((front + n + GUARD,), dtype=dtype, device="cuda")
        _bits(buf).fill_(_bits(self._value(dtype, True, self.leg)).item())
        assert buf.data_ptr() % 16 == 0
        v = buf[front: front + n]
        if host is not None:
            v.copy_(host.reshape(-1))
        else:
            _bits(v).fill_(_bits(self._value(dtype, False, self.leg)).item())
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
        outputs = []
        for v, buf, front, n, name, host in self.items:
            fill = _bits(self._value(buf.dtype, True, self.leg)).item()
            lo, hi = _bits(buf[:front]), _bits(buf[front + n:])
            assert bool((lo == fill).all()), "%s: %s: %d elements written before its start" % (what, name, int((lo != fill).sum()))
            assert bool((hi == fill).all()), "%s: %s: %d elements written past its end" % (what, name, int((hi != fill).sum()))
            if host is not None:
                assert v.cpu().numpy().tobytes() == host.numpy().tobytes(), "%s: input %s was modified" % (what, name)
            elif Guarded.RECORD is not None:
                got = _bits(buf[front: front + n]).cpu().numpy()
                outputs.append((name, got, got == _bits(self._value(buf.dtype, False, self.leg)).item()))
        if Guarded.RECORD is not None:
            Guarded.RECORD.append((what, outputs))


@contextlib.contextmanager
def nan_leg():
    prev, Guarded.LEG = Guarded.LEG, "nan"
    try:
        yield
    finally:
        Guarded.LEG = prev


def _recorded(fn, nan):
    prev, Guarded.RECORD = Guarded.RECORD, []
    try:
        with (nan_leg() if nan else contextlib.nullcontext()):
            fn()
        return Guarded.RECORD
    finally:
        Guarded.RECORD = prev


def run_both_legs(fn, what):
    """fn() -- a test body: it builds its Guarded tensors, calls the library, check()s and asserts -- once in the finite leg and once in the
    NaN leg (its own assertions hold in both).  Every output of every call must be the same in both legs, bit for bit; a cell that still
    holds the finite leg's pre-fill must still hold the NaN leg's."""
    finite, nan = _recorded(fn, False), _recorded(fn, True)
    assert len(finite) == len(nan) and len(finite) > 0, "%s: %d calls in the finite leg, %d in the NaN leg" % (what, len(finite), len(nan))
    compared = 0
    for (wf, outs_f), (wn, outs_n) in zip(finite, nan):
        assert wf == wn and [o[0] for o in outs_f] == [o[0] for o in outs_n], (what, wf, wn)
        for (name, bf, pf), (_, bn, pn) in zip(outs_f, outs_n):
            same = (bf == bn) | (pf & pn)
            assert bf.shape == bn.shape and bool(same.all()), "%s: %s: output %s differs between the legs in %d of %d elements (%d unwritten in one leg only)" % (
                what, wf, name, int((~same).sum()), same.size, int((pf != pn).sum()))
            compared += 1
    assert compared > 0, "%s: no output was compared" % what
