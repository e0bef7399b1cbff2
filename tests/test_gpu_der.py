"""GPU: the Dark Experience Replay loss kernel (csrc/der.hip: ocl_der_fwd_bwd; ops.der_loss), the reservoir update's `extra` fields and
the DER agent built on them (agents/der.py), against the float64 statement of the loss, the plain float32 statement, and the statement of
the agent's loop over the oracle's functions (tests/der_ref.py, all pinned on the CPU by tests/test_cpu_der.py).

The kernel is judged by parity_bounds.check_vs_torch32, the project's rule for transcendental kernels: its error against float64 is at
most max(4 x the error of torch's own float32 statements on the same inputs, 4 ulp of the largest reference element), for each of the
four losses and for the gradient.  Observed values: profiles/der_parity.txt (written by this module's report when PARITY_REPORT_DIR
names a directory)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agent_harness import (TRICK, build_agent, dev as _dev, host as _host, bits as _bits, rng_get as _rng_get, rng_set as _rng_set,
                           rng_equal as _rng_equal, flat as _flat, events as _events)
from guarded import Guarded
from oracle.synth import make_stream, seed_all
import parity_bounds
import der_ref
from der_ref import DER_CASE, ALPHA, BETA, ref_der, torch32_der, kernel_case

pytestmark = pytest.mark.gpu

_build_agent = functools.partial(build_agent, extra=der_ref.ref_params)

REPORT = []
# (n0, n1, n2): both sides of four waves per workgroup, empty blocks, unequal blocks
SHAPES = [(1, 0, 0), (1, 1, 1), (3, 3, 3), (4, 4, 4), (5, 5, 5), (10, 10, 10), (10, 10, 0), (10, 0, 10), (10, 7, 3), (5, 37, 3)]
# both sides of 64 lanes per row and of the row length at which the kernel stops holding the row in registers (256)
COLUMNS = [5, 10, 63, 64, 65, 100, 192, 193, 256, 257, 321, 1000]
SCALES = [1, 30, 300]
FEW_COLUMNS = [10, 65, 256, 257]      # a register row, a two-register row, the last register row, the first strided row


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    """After the module's tests: the rows parity_bounds recorded, as a table, into $PARITY_REPORT_DIR/der_parity.txt."""
    yield
    out = os.environ.get("PARITY_REPORT_DIR")
    if out and REPORT:
        with open(os.path.join(out, "der_parity.txt"), "w") as f:
            f.write("%-52s %-8s %-12s %-12s %-12s %s\n" % ("case", "tensor", "kernel err", "torch32 err", "bound", "err/bound"))
            for case, tensor, err, e_ref, bound, ratio in REPORT:
                f.write("%-52s %-8s %-12.4g %-12s %-12.4g %.3f\n" % (case, tensor, err, e_ref, bound, ratio))
            f.write("worst err/bound %.3f over %d rows\n" % (max(r[5] for r in REPORT), len(REPORT)))


def _abi(g, s, y0, y2, stored, slots, n0, n1, n2, m, alpha, beta, want_grad=True):
    """One call through the C-ABI with every tensor in a Guarded buffer: (rc, loss4 on the device, dlogits on the device or None)."""
    from ocl_amd import ffi
    lib = ffi.lib()
    c = s.shape[1]
    d_s, d_y0 = g.inp(s, 0, "logits"), g.inp(y0, 0, "y0")
    d_y2 = g.inp(y2, 0, "y2") if n2 else None
    d_st = g.inp(stored, 0, "stored") if n1 else None
    d_sl = g.inp(slots, 0, "slots") if n1 and slots is not None else None
    d_l = g.out((4,), torch.float32, 0, "loss_out")
    d_dl = g.out((n0 + n1 + n2, c), torch.float32, 0, "dlogits") if want_grad else None
    rc = lib.ocl_der_fwd_bwd(ffi.ptr(d_s), ffi.ptr(d_y0), ffi.ptr(d_y2), ffi.ptr(d_st), ffi.ptr(d_sl), n0, n1, n2, c, m, alpha, beta, ffi.ptr(d_l),
                             ffi.ptr(d_dl), ffi.stream())
    assert rc == 0, lib.ocl_last_error()
    g.check("der_loss")
    return d_l, d_dl


# ---- 1. the kernel against the float64 statement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", COLUMNS)
@pytest.mark.parametrize("n0,n1,n2", SHAPES)
def test_der_loss_vs_float64_reference(cuda, n0, n1, n2, c):
    for scale in SCALES:
        s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, scale)
        l64, g64 = ref_der(s, y0, y2, stored, slots, n0, n1, n2, ALPHA, BETA)
        l32, g32 = torch32_der(s, y0, y2, stored, slots, n0, n1, n2, ALPHA, BETA)
        d_l, d_dl = _abi(Guarded(), s, y0, y2, stored, slots, n0, n1, n2, m, ALPHA, BETA)
        got_l, got_g = _host(d_l), _host(d_dl)
        assert np.isfinite(got_l).all() and np.isfinite(got_g).all()
        name = "der n=(%d, %d, %d) c=%d scale=%g" % (n0, n1, n2, c, scale)
        for k, which in enumerate(("loss", "ce", "mse", "ce_m")):
            parity_bounds.check_vs_torch32(REPORT, name, which, got_l[k:k + 1], l64[k:k + 1], l32[k:k + 1])
        parity_bounds.check_vs_torch32(REPORT, name, "dlogits", got_g, g64, g32)


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------

def _on_device(cuda, n0, n1, n2, c, scale=1):
    s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, scale)
    return SimpleNamespace(s=_dev(s, cuda), y0=_dev(y0, cuda, np.int64), y2=_dev(y2, cuda, np.int64) if n2 else None,
                           stored=_dev(stored, cuda) if n1 else None, slots=_dev(slots, cuda, np.int64) if n1 else None, n=(n0, n1, n2), m=m)


def _run(k, alpha=ALPHA, beta=BETA, **over):
    from ocl_amd import ops
    a = dict(logits=k.s, y0=k.y0, y2=k.y2, stored=k.stored, slots=k.slots)
    kw = {key: over.pop(key) for key in ("want_grad", "dl_out") if key in over}
    a.update(over)
    return ops.der_loss(a["logits"], a["y0"], a["y2"], a["stored"], a["slots"], k.n[0], k.n[1], k.n[2], alpha, beta, **kw)


@pytest.mark.parametrize("c", COLUMNS)
def test_without_replay_blocks_the_loss_is_the_cross_entropy_kernel_bit_for_bit(cuda, c):
    from ocl_amd import ops
    for n0 in (1, 3, 4, 5, 10, 37):
        for scale in SCALES:
            k = _on_device(cuda, n0, 0, 0, c, scale)
            want_l, want_dl = ops.cross_entropy(k.s, k.y0, "mean")
            for alpha, beta in ((ALPHA, BETA), (0.0, 0.0), (3.0, 7.0)):      # without the blocks the weights multiply nothing
                loss4, dl = _run(k, alpha, beta)
                assert torch.equal(_bits(loss4[0]), _bits(want_l)) and torch.equal(_bits(loss4[1]), _bits(want_l))
                assert float(loss4[2]) == 0.0 and float(loss4[3]) == 0.0
                assert torch.equal(_bits(dl), _bits(want_dl))


@pytest.mark.parametrize("c", COLUMNS)
def test_stored_rows_equal_to_todays_rows_give_exactly_zero(cuda, c):
    for n0, n1, n2 in SHAPES:
        if n1 == 0:
            continue
        k = _on_device(cuda, n0, n1, n2, c, 30)
        k.stored[k.slots] = k.s[n0:n0 + n1]
        clean = _run(k, 0.0, BETA)
        for alpha in (ALPHA, 1.0, 1e6, -3.0):
            loss4, dl = _run(k, alpha, BETA)
            assert float(loss4[2]) == 0.0 and bool((dl[n0:n0 + n1] == 0).all())
            assert torch.equal(_bits(loss4), _bits(clean[0])), "alpha times an exact zero changed the total"


@pytest.mark.parametrize("c", FEW_COLUMNS)
def test_alpha_zero_writes_zeros_to_block_one(cuda, c):
    for n0, n1, n2 in SHAPES:
        if n1 == 0:
            continue
        k = _on_device(cuda, n0, n1, n2, c)
        dl = torch.full((n0 + n1 + n2, c), -7777.0, device=cuda)
        loss4, out = _run(k, 0.0, BETA, dl_out=dl)
        want4, want = _run(k, ALPHA, BETA)
        assert out is dl and bool((dl[n0:n0 + n1] == 0).all()) and not bool((dl == -7777.0).any())
        assert torch.equal(_bits(dl[:n0]), _bits(want[:n0])) and torch.equal(_bits(dl[n0 + n1:]), _bits(want[n0 + n1:]))
        assert torch.equal(_bits(loss4[1:]), _bits(want4[1:])) and float(loss4[2]) > 0.0


@pytest.mark.parametrize("c", FEW_COLUMNS)
def test_no_slots_means_the_first_rows_of_the_table(cuda, c):
    for n0, n1, n2 in SHAPES:
        if n1 == 0:
            continue
        k = _on_device(cuda, n0, n1, n2, c, 30)
        a4, a = _run(k, slots=None)
        b4, b = _run(k, slots=torch.arange(n1, device=cuda))
        assert torch.equal(_bits(a4), _bits(b4)) and torch.equal(_bits(a), _bits(b))
        if not torch.equal(k.slots, torch.arange(n1, device=cuda)):
            p4, p = _run(k)
            assert not torch.equal(_bits(p4[2]), _bits(a4[2])), "the permuted slots address the same rows as no slots"


@pytest.mark.parametrize("c", COLUMNS)
def test_two_runs_are_bit_identical_and_the_losses_do_not_depend_on_want_grad(cuda, c):
    for n0, n1, n2 in SHAPES:
        k = _on_device(cuda, n0, n1, n2, c, 30)
        l_a, dl_a = _run(k)
        l_b, dl_b = _run(k)
        l_c, dl_c = _run(k, want_grad=False)
        assert dl_c is None and dl_a is not dl_b
        assert torch.equal(_bits(l_a), _bits(l_b)) and torch.equal(_bits(dl_a), _bits(dl_b)) and torch.equal(_bits(l_a), _bits(l_c))


def test_dl_out_writes_into_a_row_block_of_a_larger_buffer_and_leaves_the_rest(cuda):
    n0, n1, n2, c = 10, 7, 3, 100
    n = n0 + n1 + n2
    k = _on_device(cuda, n0, n1, n2, c)
    big = torch.full((3 * n, c), -7777.0, device=cuda)
    loss4, dl = _run(k, dl_out=big[n:2 * n])
    want_l, want_dl = _run(k)
    assert dl.data_ptr() == big[n:2 * n].data_ptr() and torch.equal(_bits(dl), _bits(want_dl)) and torch.equal(_bits(loss4), _bits(want_l))
    assert bool((big[:n] == -7777.0).all()) and bool((big[2 * n:] == -7777.0).all())
    for bad in (big[:, :c // 2], big[:n].double(), big[:n + 1], big[:n].cpu()):
        with pytest.raises(RuntimeError):
            _run(k, dl_out=bad)
    with pytest.raises(RuntimeError):
        _run(k, stored=k.stored[:, :50])
    with pytest.raises(RuntimeError):
        _run(k, y0=k.y0.cpu())
    with pytest.raises(RuntimeError, match="overlaps"):
        _run(k, dl_out=k.s)


# ---- 3. addresses ------------------------------------------------------------------------------------------------------------------------

def _bits_np(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("c", FEW_COLUMNS)
@pytest.mark.parametrize("block", [0, 2])
def test_a_label_outside_the_row_is_no_address(cuda, c, block):
    """-1, c and 2^62 in block 0 (block 2): ce (ce_m) and the total are NaN, the other losses and every other row's gradient keep the
    bits of the clean run; the row itself gets its softmax without a one-hot; nothing outside the tensors is touched (Guarded)."""
    n0, n1, n2 = 5, 6, 7
    s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, 1)
    clean_l, clean_g = (_host(t) for t in _abi(Guarded(), s, y0, y2, stored, slots, n0, n1, n2, m, ALPHA, BETA))
    nan_at, keep = ((1, 0), (2, 3)) if block == 0 else ((3, 0), (1, 2))
    for row, label in ((0, -1), (2, c), (4, 1 << 62)):
        ya, yb = y0.copy(), y2.copy()
        (ya if block == 0 else yb)[row] = label
        g = Guarded()
        d_l, d_dl = _abi(g, s, ya, yb, stored, slots, n0, n1, n2, m, ALPHA, BETA)
        got_l, got_g = _host(d_l), _host(d_dl)
        assert all(np.isnan(got_l[i]) for i in nan_at), (label, got_l)
        assert np.array_equal(_bits_np(got_l[list(keep)]), _bits_np(clean_l[list(keep)])), (label, got_l, clean_l)
        at = row if block == 0 else n0 + n1 + row
        others = np.ones(n0 + n1 + n2, dtype=bool)
        others[at] = False
        assert np.array_equal(_bits_np(got_g[others]), _bits_np(clean_g[others])), label
        scale = (1.0 / n0) if block == 0 else float(np.float32(BETA)) / n2
        p = np.exp(der_ref._log_softmax64(s[at:at + 1].astype(np.float64)))[0] * scale
        assert np.isfinite(got_g[at]).all() and np.abs(got_g[at] - p).max() <= 1e-6 * scale, "the row's softmax without a one-hot"


@pytest.mark.parametrize("c", FEW_COLUMNS)
def test_a_slot_outside_the_table_is_no_address(cuda, c):
    """-1, m and 2^62: mse and the total are NaN, that row's gradient is NaN, ce, ce_m and every other row's gradient keep the bits of
    the clean run; nothing outside the tensors is touched (Guarded)."""
    n0, n1, n2 = 5, 6, 7
    s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, 1)
    clean_l, clean_g = (_host(t) for t in _abi(Guarded(), s, y0, y2, stored, slots, n0, n1, n2, m, ALPHA, BETA))
    for row, slot in ((0, -1), (3, m), (5, 1 << 62)):
        sl = slots.copy()
        sl[row] = slot
        d_l, d_dl = _abi(Guarded(), s, y0, y2, stored, sl, n0, n1, n2, m, ALPHA, BETA)
        got_l, got_g = _host(d_l), _host(d_dl)
        assert np.isnan(got_l[0]) and np.isnan(got_l[2]), (slot, got_l)
        assert np.array_equal(_bits_np(got_l[[1, 3]]), _bits_np(clean_l[[1, 3]]))
        others = np.ones(n0 + n1 + n2, dtype=bool)
        others[n0 + row] = False
        assert np.array_equal(_bits_np(got_g[others]), _bits_np(clean_g[others])), slot
        assert np.isnan(got_g[n0 + row]).all()


def test_block_one_reads_no_label_and_an_empty_block_reads_nothing(cuda):
    """y0 has n0 entries and y2 n2 entries, each with sentinels behind it: a kernel that indexed the labels by the row of the whole block
    would read a sentinel (4096: outside the row) and return NaN.  With n1 = 0 (n2 = 0) the table and the slots (y2) are null."""
    for n0, n1, n2 in ((5, 37, 3), (10, 0, 10), (10, 10, 0)):
        s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, 100, 1)
        d_l, d_dl = _abi(Guarded(), s, y0, y2, stored, slots, n0, n1, n2, m, ALPHA, BETA)
        assert np.isfinite(_host(d_l)).all() and np.isfinite(_host(d_dl)).all()


def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from ocl_amd import ffi
    lib = ffi.lib()
    n0, n1, n2, c, m = 4, 3, 2, 8, 6
    n = n0 + n1 + n2
    s, st = torch.full((n, c), 1.0, device=cuda), torch.full((m, c), 2.0, device=cuda)
    y0, y2, sl = (torch.zeros(k, dtype=torch.int64, device=cuda) for k in (n0, n2, n1))
    loss, dl = torch.full((4,), -7777.0, device=cuda), torch.full((n, c), -7777.0, device=cuda)
    nan, inf = float("nan"), float("inf")

    def call(**over):
        kw = dict(s=s.data_ptr(), y0=y0.data_ptr(), y2=y2.data_ptr(), st=st.data_ptr(), sl=sl.data_ptr(), n0=n0, n1=n1, n2=n2, c=c, m=m,
                  alpha=0.1, beta=0.5, loss=loss.data_ptr(), dl=dl.data_ptr())
        kw.update(over)
        rc = lib.ocl_der_fwd_bwd(ffi.vp(kw["s"]), ffi.vp(kw["y0"]), ffi.vp(kw["y2"]), ffi.vp(kw["st"]), ffi.vp(kw["sl"]), kw["n0"], kw["n1"],
                                 kw["n2"], kw["c"], kw["m"], kw["alpha"], kw["beta"], ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.stream())
        return rc, lib.ocl_last_error()

    for over in (dict(n0=0), dict(n0=-1), dict(n1=-1), dict(n2=-2), dict(c=0), dict(c=-5), dict(m=0), dict(alpha=nan), dict(alpha=inf),
                 dict(beta=nan), dict(beta=-inf), dict(s=0), dict(y0=0), dict(y2=0), dict(st=0), dict(loss=0),
                 dict(dl=s.data_ptr()), dict(dl=s.data_ptr() + 4 * (n * c - 1)), dict(dl=st.data_ptr()), dict(dl=st.data_ptr() + 64)):
        rc, msg = call(**over)
        assert rc == -1 and msg.startswith(b"der_loss:"), (over, rc, msg)
        if "dl" in over:
            assert b"overlap" in msg, (over, msg)
    torch.cuda.synchronize()
    assert bool((loss == -7777.0).all()) and bool((dl == -7777.0).all()) and bool((s == 1.0).all()) and bool((st == 2.0).all())
    rc, msg = call()
    assert rc == 0, msg
    rc, msg = call(sl=0, dl=0)                       # both optional pointers null: the losses alone, rows 0 .. n1 - 1 of the table
    assert rc == 0, msg
    rc, msg = call(n1=0, n2=0, y2=0, st=0, sl=0, m=0)    # the stream rows alone
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool((dl[:n0] == -7777.0).any()) and float(loss[2]) == 0.0 and float(loss[3]) == 0.0


# ---- 4. the reservoir update's extra fields ----------------------------------------------------------------------------------------------

def _memory(cuda, mem_size=30):
    from ocl_amd.buffer import Buffer
    params = SimpleNamespace(data="cifar10", cuda=True, mem_size=mem_size, update="random", retrieve="random", eps_mem_batch=10, buffer_tracker=False)
    b = Buffer(None, params)
    b.register_buffer("buffer_logits", torch.full((mem_size, 10), -7777.0, device=cuda))
    return b


def test_reservoir_update_carries_extra_fields_to_the_slots_of_the_images(cuda):
    """mem_size 30, batches of 10, 70, 10 and 10 items: a fill, a batch that straddles the end of the fill (20 fill, 50 draw), overwrites.
    With and without `extra` from one RNG state: images, labels, label mirror, counters, returned slots and the generator's state
    afterwards are bit-equal.  With it every filled slot's row is the row that came with the image now in that slot (both encode the
    item's running index), and an unfilled slot's row is untouched."""
    sizes = (10, 70, 10, 10)
    a, b = _memory(cuda), _memory(cuda)
    torch.manual_seed(11)
    seen = 0
    for n in sizes:
        ids = torch.arange(seen, seen + n, dtype=torch.float32, device=cuda)
        x = ids.reshape(n, 1, 1, 1).expand(n, 3, 32, 32).contiguous()
        y = (torch.arange(seen, seen + n, device=cuda) % 7).long()
        rows = (ids.reshape(n, 1) + torch.arange(10, device=cuda).reshape(1, 10) / 16).contiguous()
        seen += n
        st = _rng_get()
        slots_a = a.update(x, y)
        after = _rng_get()
        _rng_set(st)
        slots_b = b.update(x, y, extra=((b.buffer_logits, rows),))
        assert _rng_equal(after, _rng_get()) and slots_a == slots_b
        assert torch.equal(_bits(a.buffer_img), _bits(b.buffer_img)) and torch.equal(a.buffer_label, b.buffer_label)
        assert np.array_equal(a.label_host, b.label_host) and np.array_equal(a.label_host, _host(a.buffer_label))
        assert (a.current_index, a.n_seen_so_far) == (b.current_index, b.n_seen_so_far)
        k = b.current_index
        want = b.buffer_img[:k, 0, 0, 0].reshape(k, 1) + torch.arange(10, device=cuda).reshape(1, 10) / 16
        assert torch.equal(_bits(b.buffer_logits[:k]), _bits(want)), "a slot's row is not the row of the image in that slot"
        assert bool((b.buffer_logits[k:] == -7777.0).all()) and bool((a.buffer_logits == -7777.0).all())
    assert b.current_index == 30 and b.n_seen_so_far == sum(sizes)
    assert len(torch.unique(b.buffer_img[:, 0, 0, 0])) == 30 and float(b.buffer_img[:, 0, 0, 0].max()) >= 30, "no overwrite took place"
    with pytest.raises(ValueError, match="extra field"):
        b.update(x, y, extra=((b.buffer_logits, rows[:5]),))


# ---- 5. the agent ------------------------------------------------------------------------------------------------------------------------

def _spy_der(monkeypatch):
    from ocl_amd import ops
    calls = []
    inner = ops.der_loss

    def der_loss(logits, y0, y2, stored, slots, n0, n1, n2, alpha, beta, want_grad=True, dl_out=None):
        loss4, dl = inner(logits, y0, y2, stored, slots, n0, n1, n2, alpha, beta, want_grad=want_grad, dl_out=dl_out)
        calls.append(SimpleNamespace(logits=logits, logits_bits=logits.clone(), y0=y0.clone(), y2=None if y2 is None else y2.clone(), stored=stored,
                                     slots=None if slots is None else slots.clone(), n=(n0, n1, n2), alpha=alpha, beta=beta, dl=dl, dl_bits=dl.clone(),
                                     loss4=loss4.clone(), table=None if stored is None else stored.clone()))
        return loss4, dl

    monkeypatch.setattr(ops, "der_loss", der_loss)
    return calls


def _spy_retrieve(monkeypatch):
    from ocl_amd.agents import der as der_module
    draws = []
    inner = der_module.random_retrieve

    def random_retrieve(buffer, num_retrieve, excl_indices=None, return_indices=False):
        out = inner(buffer, num_retrieve, excl_indices=excl_indices, return_indices=return_indices)
        draws.append(SimpleNamespace(x=out[0], y=out[1], indices=out[2].clone()))
        return out

    monkeypatch.setattr(der_module, "random_retrieve", random_retrieve)
    return draws


def _bn_stats(state):
    return {k: v for k, v in state.items() if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


def _key(image):
    return image.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("beta", [BETA, 0.0], ids=["der++", "der"])
def test_agent_hands_the_right_things_to_the_kernel_and_its_gradient_to_the_backward(cuda, monkeypatch, beta):
    """Two train_learner calls of two batches each, mem_size 30.  Step 1 finds the memory empty: one group, n1 = n2 = 0, no draw.  Later
    steps: three groups of 10 and two draws (beta = 0: two groups, one draw); `slots` is the first draw's indices and `stored` the
    memory's table itself; the kernel's dl is the very tensor backward_taped receives, unchanged.  Every stream image is forwarded as a
    stream row once: after the run every filled slot's buffer_logits row is the bits of the logits the agent computed for that slot's
    image."""
    cfg = dict(DER_CASE, seed=23)
    params, model, opt, agent = _build_agent(cfg, der_beta=beta)
    assert agent.alpha == ALPHA and agent.beta == beta and tuple(agent.buffer.buffer_logits.shape) == (30, 10)
    calls, draws = _spy_der(monkeypatch), _spy_retrieve(monkeypatch)
    taped, backs, steps, updates, seen = [], [], [], [], {}
    inner_taped, inner_back, inner_step, inner_update = model.forward_views_taped, model.backward_taped, opt.step, agent.buffer.update

    def forward_views_taped(views):
        out, tape = inner_taped(views)
        taped.append(SimpleNamespace(views=views, out=out, tape=tape, n_draws=len(draws)))
        for i in range(views[0].size(0)):
            assert _key(views[0][i]) not in seen, "a stream image was forwarded twice at epoch 1"
            seen[_key(views[0][i])] = out[i].clone()
        return out, tape

    def backward_taped(tape, dout):
        backs.append(SimpleNamespace(tape=tape, dout=dout, bits=dout.clone(), n_calls=len(calls)))
        return inner_back(tape, dout)

    def step(*a, **k):
        steps.append(len(backs))
        return inner_step(*a, **k)

    def update(x, y, **kw):
        updates.append(SimpleNamespace(x=x, rows=kw["extra"][0][1], table=kw["extra"][0][0], n_steps=len(steps), keys=sorted(kw)))
        return inner_update(x, y, **kw)

    model.forward_views_taped, model.backward_taped, opt.step, agent.buffer.update = forward_views_taped, backward_taped, step, update
    tasks, _ = make_stream(cfg)
    pick = np.r_[0:10, 30:40]
    for t in range(2):
        agent.train_learner(tasks[t][0][pick], tasks[t][1][pick])
        assert agent.task_seen == t + 1 and len(calls) == len(taped) == len(backs) == len(steps) == len(updates) == 2 * (t + 1)
    groups = 3 if beta else 2
    per_step = groups - 1
    assert len(draws) == 3 * per_step, "the draws per step"
    for k, c in enumerate(calls):
        tp = taped[k]
        assert c.alpha == ALPHA and c.beta == beta
        assert c.logits is tp.out and backs[k].dout is c.dl and backs[k].tape is tp.tape and backs[k].n_calls == k + 1 and steps[k] == k + 1
        assert torch.equal(_bits(backs[k].bits), _bits(c.dl_bits)), "dl was changed between the kernel and the backward"
        assert updates[k].n_steps == k + 1 and updates[k].table is agent.buffer.buffer_logits and updates[k].keys == ["extra", "y_host"]
        assert updates[k].x is tp.views[0] and torch.equal(_bits(updates[k].rows), _bits(c.logits_bits[:10]))
        if k == 0:
            assert len(tp.views) == 1 and c.n == (10, 0, 0) and c.stored is None and c.slots is None and c.y2 is None and tp.n_draws == 0
            assert float(c.loss4[2]) == 0.0 and float(c.loss4[3]) == 0.0 and torch.equal(_bits(c.loss4[0]), _bits(c.loss4[1]))
            continue
        first = draws[(k - 1) * per_step]
        assert len(tp.views) == groups and c.n == (10, 10, 10 if beta else 0) and tp.n_draws == k * per_step, "drawn before the forward"
        assert c.stored is agent.buffer.buffer_logits and tp.views[1] is first.x
        assert torch.equal(c.slots.cpu(), first.indices) and c.slots.is_cuda
        if beta:
            second = draws[(k - 1) * per_step + 1]
            assert tp.views[2] is second.x and torch.equal(c.y2, second.y)
        else:
            assert c.y2 is None and float(c.loss4[3]) == 0.0
        want_l, want_dl = ref_der(_host(c.logits_bits), _host(c.y0), None if c.y2 is None else _host(c.y2), _host(c.table), _host(c.slots),
                                  c.n[0], c.n[1], c.n[2], ALPHA, beta)
        assert np.abs(_host(c.loss4) - want_l).max() <= 1e-5 * max(1.0, np.abs(want_l).max())
        assert np.abs(_host(c.dl_bits) - want_dl).max() <= 1e-5 * np.abs(want_dl).max()
        assert float(c.loss4[2]) > 0.0
    b = agent.buffer
    assert b.current_index == 30 and b.n_seen_so_far == 40 and len(seen) == 40
    for slot in range(30):
        assert torch.equal(_bits(b.buffer_logits[slot]), _bits(seen[_key(b.buffer_img[slot])])), "slot %d holds another image's logits" % slot
    assert set(agent.state_dict()) >= {"buffer.buffer_img", "buffer.buffer_label", "buffer.buffer_logits"}


# ---- 6. co-simulation against DerOracle ------------------------------------------------------------------------------------------------

def _snapshot(buf):
    return SimpleNamespace(img=buf.img.clone(), label=buf.label.clone(), logits=buf.logits.clone(), current_index=buf.current_index,
                           n_seen_so_far=buf.n_seen_so_far)


def _load_memory(agent, snap):
    b = agent.buffer
    b.buffer_img.copy_(snap.img)
    b.buffer_label.copy_(snap.label)
    b.buffer_logits.copy_(snap.logits)
    b.label_host = snap.label.numpy().copy()
    b.current_index, b.n_seen_so_far = snap.current_index, snap.n_seen_so_far


def test_cosim_der(cuda, monkeypatch):
    """The three tasks of DER_CASE concatenated, 9 sequential slices of 20, one train_learner call (two batches) per slice.  Before every
    call the HIP model is loaded with the oracle's state and the memory with the oracle's images, labels, logit table and counters;
    between the two steps of a call both are loaded with the oracle's again (the per-step bounds are bounds for one step from the same
    state; the images and labels the agent's own update left must already be the oracle's, bit for bit); both sides consume the same
    host RNG streams.  Per call: RNG state equal.  Per step: ce, ce_mem and the total within 1e-4 * max(1, |.|), mse within 1e-4 * max(1,
    |mse|), the update within 1e-2 norm-wise (ER's co-simulation bounds)."""
    from ocl_amd import debug
    cfg = DER_CASE
    params, model, opt, agent = _build_agent(cfg)
    seed_all(cfg["seed"])
    oa = der_ref.DerOracle(cfg)
    xs, ys = der_ref.cosim_stream(cfg)
    assert xs.shape[0] == 180
    seed_all(1000 + cfg["seed"])
    steps, ostates, omems = [], [], []
    inner_step, inner_update = opt.step, agent.buffer.update

    def step(*a, **k):
        out = inner_step(*a, **k)
        steps.append(model.flat_params().double().cpu().numpy())
        return out

    def update(x, y, **kw):
        out = inner_update(x, y, **kw)
        k = len(steps) - 1
        b = agent.buffer
        assert torch.equal(b.buffer_img.cpu(), omems[k].img) and torch.equal(b.buffer_label.cpu(), omems[k].label), "the memory's images diverged"
        assert (b.current_index, b.n_seen_so_far) == (omems[k].current_index, omems[k].n_seen_so_far)
        filled = b.current_index
        # (a sanity band, not a parity bound: the rows written in this step come from two float32 forwards of the same state; which row
        # goes to which slot is pinned bit for bit by the wiring test above)
        assert float((b.buffer_logits[:filled].cpu() - omems[k].logits[:filled]).abs().max()) <= 1e-3, "the stored logits are not those of the forward"
        if len(steps) < len(ostates):           # not after the call's last step: the task's end keeps the agent's own weights
            model.load_state_dict(ostates[k])
            _load_memory(agent, omems[k])
        return out

    opt.step, agent.buffer.update = step, update
    worst = dict(ce=0.0, mse=0.0, ce_mem=0.0, loss=0.0, update=0.0)
    three_terms = 0
    for it in range(9):
        x, y = xs[it * 20:(it + 1) * 20], ys[it * 20:(it + 1) * 20]
        model.load_state_dict(oa.state_dict())
        _load_memory(agent, _snapshot(oa.buf))
        w_before = [_flat(oa.state, oa.names)]
        st = _rng_get()
        n_log = len(oa.log)
        del ostates[:], omems[:]
        inner_der_step, inner_reservoir = der_ref.der_step, der_ref.der_reservoir

        def spy_step(state, names, *a, **k):
            out = inner_der_step(state, names, *a, **k)
            w_before.append(_flat(state, names))
            ostates.append({k_: v.detach().clone() for k_, v in state.items()})
            return out

        def spy_reservoir(buf, *a, **k):
            out = inner_reservoir(buf, *a, **k)
            omems.append(_snapshot(buf))
            return out

        monkeypatch.setattr(der_ref, "der_step", spy_step)
        monkeypatch.setattr(der_ref, "der_reservoir", spy_reservoir)
        oa.train_learner(x, y)
        monkeypatch.setattr(der_ref, "der_step", inner_der_step)
        monkeypatch.setattr(der_ref, "der_reservoir", inner_reservoir)
        logs = oa.log[n_log:]
        st_o = _rng_get()
        _rng_set(st)
        del steps[:]
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        assert len(logs) == 2 and agent.task_seen == oa.task_seen == it + 1
        assert _rng_equal(st_o, _rng_get()), "host RNG streams diverged in call %d" % it
        loss = _events(ev, "der_loss")
        drawn = [e["indices"] for e in _events(ev, "random_retrieve")]
        assert len(loss) == 2 and len(steps) == 2 and len(w_before) == 3 and len(omems) == 2
        for k in range(2):
            ol = logs[k]
            want_draws = [i for i in (ol["idx1"], ol["idx2"]) if i is not None]
            got_draws, drawn = drawn[:len(want_draws)], drawn[len(want_draws):]
            assert len(got_draws) == len(want_draws) and all(np.array_equal(a, b) for a, b in zip(got_draws, want_draws)), "the replayed slots"
            d = {key: abs(loss[k][key] - ol[key]) / max(1.0, abs(ol[key])) for key in ("ce", "mse", "ce_mem", "loss")}
            dw_o = w_before[k + 1] - w_before[k]
            dw_m = steps[k] - w_before[k]
            d["update"] = float(np.linalg.norm(dw_m - dw_o) / np.linalg.norm(dw_o))
            print("der cosim call %d step %d  ce %.6f / %.6f  mse %.6f / %.6f  ce_mem %.6f / %.6f  loss %.6f / %.6f  update err %.2e"
                  % (it, k, loss[k]["ce"], ol["ce"], loss[k]["mse"], ol["mse"], loss[k]["ce_mem"], ol["ce_mem"], loss[k]["loss"], ol["loss"], d["update"]))
            for key in worst:
                worst[key] = max(worst[key], d[key])
            assert d["ce"] <= 1e-4 and d["ce_mem"] <= 1e-4 and d["loss"] <= 1e-4, (it, k, loss[k], ol)
            assert d["mse"] <= 1e-4, (it, k, loss[k], ol)
            assert d["update"] <= 1e-2, (it, k, d["update"])
            full = ol["idx1"] is not None and ol["idx2"] is not None
            assert full == (loss[k]["mse"] > 0 and loss[k]["ce_mem"] > 0) and full == (it > 0 or k > 0)
            three_terms += full
        assert not drawn
    print("der cosim: %d steps with all three terms; worst relative differences (absolute below 1) %s" % (three_terms, worst))
    assert three_terms >= 16


# ---- 7. the comparator -------------------------------------------------------------------------------------------------------------------

COMPARATOR_BOUND = 1e-5     # test_gpu_ewc.COMPARATOR_BOUND


def _copy_memory(dst, src):
    d, s = dst.buffer, src
    d.buffer_img.copy_(s.img)
    d.buffer_label.copy_(s.label)
    d.buffer_logits.copy_(s.logits)
    d.label_host = s.label_host.copy()
    d.current_index, d.n_seen_so_far = s.current_index, s.n_seen_so_far


def _device_snapshot(agent):
    b = agent.buffer
    return SimpleNamespace(img=b.buffer_img.clone(), label=b.buffer_label.clone(), logits=b.buffer_logits.clone(), label_host=b.label_host.copy(),
                           current_index=b.current_index, n_seen_so_far=b.n_seen_so_far)


def test_fused_step_against_the_autograd_statements_on_the_same_state(cuda, monkeypatch):
    """`_force_autograd` runs the same statements over model.forward per batch, criterion, F.mse_loss, a gather of the stored rows and
    autograd.  Two agents from one seed run the first task (one each way, from the same host RNG state); then, for the six steps of the
    second task, the comparator starts every step from the fused agent's weights, running statistics and memory, under
    order-independent batch sums.  One step's updates agree within 1e-5 norm-wise and the running statistics bit for bit.  The comparator
    calls ops.der_loss never."""
    from ocl_amd import ops
    cfg = DER_CASE
    ops.set_deterministic(True)
    try:
        _, model_a, opt_a, a = _build_agent(cfg)
        _, model_b, opt_b, b = _build_agent(cfg)
        b._force_autograd = True
        calls = _spy_der(monkeypatch)
        tasks, _ = make_stream(cfg)
        st = _rng_get()
        a.train_learner(*tasks[0])
        assert len(calls) == 6
        _rng_set(st)
        b.train_learner(*tasks[0])
        assert len(calls) == 6, "the comparator called the fused kernel"
        assert torch.equal(a.buffer.buffer_img, b.buffer.buffer_img) and torch.equal(a.buffer.buffer_label, b.buffer.buffer_label)
        model_b.load_state_dict(model_a.state_dict())
        _copy_memory(b, _device_snapshot(a))
        pre, post, got, mems = [], [], [], []
        inner_a, inner_b, update_a, update_b = opt_a.step, opt_b.step, a.buffer.update, b.buffer.update

        def step_a(*args, **kw):
            w0 = model_a.flat_params().double().cpu().numpy()
            out = inner_a(*args, **kw)
            pre.append(w0)
            post.append({k: v.clone() for k, v in model_a.state_dict().items()})
            return out

        def upd_a(x, y, **kw):
            out = update_a(x, y, **kw)
            mems.append(_device_snapshot(a))
            return out

        def step_b(*args, **kw):
            out = inner_b(*args, **kw)
            got.append({k: v.clone() for k, v in model_b.state_dict().items()})
            return out

        def upd_b(x, y, **kw):
            out = update_b(x, y, **kw)
            k = len(got) - 1
            assert torch.equal(b.buffer.buffer_img, mems[k].img) and torch.equal(b.buffer.buffer_label, mems[k].label)
            model_b.load_state_dict(post[k])
            _copy_memory(b, mems[k])
            return out

        opt_a.step, opt_b.step, a.buffer.update, b.buffer.update = step_a, step_b, upd_a, upd_b
        st = _rng_get()
        a.train_learner(*tasks[1])
        _rng_set(st)
        b.train_learner(*tasks[1])
        assert len(calls) == 12 and len(pre) == len(post) == len(got) == len(mems) == 6 and all(c.n == (10, 10, 10) for c in calls[6:])
        names = [n for n, _ in model_a.named_parameters()]
        worst = 0.0
        for k in range(6):
            wa, wb = _flat(post[k], names), _flat(got[k], names)
            diff = float(np.linalg.norm((wb - pre[k]) - (wa - pre[k])) / np.linalg.norm(wa - pre[k]))
            worst = max(worst, diff)
            print("der comparator step %d  update difference %.2e (allowed %.0e)" % (k, diff, COMPARATOR_BOUND))
            assert diff <= COMPARATOR_BOUND, (k, diff)
            sa, sb = _bn_stats(post[k]), _bn_stats(got[k])
            assert sa.keys() == sb.keys() and all(torch.equal(sa[n], sb[n]) for n in sa), "running statistics differ at step %d" % k
        print("der comparator: worst norm-wise update difference over the second task %.2e" % worst)
    finally:
        ops.set_deterministic(False)


# ---- 8. the label tricks --------------------------------------------------------------------------------------------------------------------

def test_label_tricks_take_the_autograd_path(cuda, monkeypatch):
    """With the labels trick or the separated softmax the criterion is the segmented cross-entropy: the agent takes the statements over
    autograd.  No der_loss call; over two tasks every loss is finite, the replay terms are present from the second step on, and the
    memory's logit field is filled."""
    from ocl_amd import debug
    cfg = DER_CASE
    for trick in (dict(labels_trick=True), dict(separated_softmax=True)):
        params, model, opt, agent = _build_agent(cfg, trick=dict(TRICK, **trick))
        calls = _spy_der(monkeypatch)
        tasks, _ = make_stream(cfg)
        debug.LOG = []
        try:
            agent.train_learner(*tasks[0])
            agent.train_learner(*tasks[1])
            ev = _events(list(debug.LOG), "der_loss")
        finally:
            debug.LOG = None
        assert not calls and len(ev) == 12
        print("der %s: (ce, mse, ce_mem) %s" % (trick, [(round(e["ce"], 3), round(e["mse"], 4), round(e["ce_mem"], 3)) for e in ev]))
        assert all(np.isfinite([e["loss"], e["ce"], e["mse"], e["ce_mem"]]).all() for e in ev)
        assert ev[0]["mse"] == 0.0 and ev[0]["ce_mem"] == 0.0 and all(e["mse"] > 0.0 and e["ce_mem"] > 0.0 for e in ev[1:])
        assert bool(torch.isfinite(model.flat_params()).all()) and agent.buffer.current_index == 30
        assert bool((agent.buffer.buffer_logits.abs().sum(dim=1) > 0).all())


# ---- 9. a free run ------------------------------------------------------------------------------------------------------------------------

def test_free_run_of_three_tasks_with_evaluate(cuda, monkeypatch):
    """Whole tasks, free running: counters and label bookkeeping are exact, the weights finite, one kernel call per optimiser step, each
    task's cross-entropy ends below where it began (two separable classes per task), accuracies in [0, 1]."""
    from ocl_amd.data import setup_test_loader
    cfg = DER_CASE
    params, model, opt, agent = _build_agent(cfg)
    calls = _spy_der(monkeypatch)
    n_steps = []
    inner = opt.step

    def step(*a, **k):
        n_steps.append(len(calls))
        return inner(*a, **k)

    opt.step = step
    tasks, tests = make_stream(cfg)
    loaders = setup_test_loader(tests, params)
    seen = []
    for t, (x, y) in enumerate(tasks):
        agent.train_learner(x, y)
        acc = agent.evaluate(loaders)
        seen += cfg["tasks"][t]
        assert agent.task_seen == t + 1 and sorted(agent.old_labels) == seen and agent.new_labels == []
        assert {k: v for k, v in agent.class_task_map.items()} == {c: i for i, cs in enumerate(cfg["tasks"][:t + 1]) for c in cs}
        assert n_steps == list(range(1, 6 * (t + 1) + 1)), "one kernel call per optimiser step"
        b = agent.buffer
        assert b.current_index == 30 and b.n_seen_so_far == 60 * (t + 1)
        assert np.array_equal(b.label_host, _host(b.buffer_label)) and set(b.label_host.tolist()) <= set(seen)
        assert [c.n for c in calls[6 * t:]] == ([(10, 0, 0)] if t == 0 else [(10, 10, 10)]) + [(10, 10, 10)] * 5
        ce = [float(c.loss4[1]) for c in calls[6 * t:]]
        print("der free run task %d: ce %s  acc %s" % (t, np.round(ce, 4).tolist(), acc))
        assert np.isfinite([_host(c.loss4) for c in calls[6 * t:]]).all() and ce[0] > ce[-1]
        assert bool(torch.isfinite(model.flat_params()).all()) and bool(torch.isfinite(b.buffer_logits).all())
        assert acc.shape == (3,) and (acc >= 0).all() and (acc <= 1).all()
