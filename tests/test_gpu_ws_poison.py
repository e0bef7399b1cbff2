"""GPU: no stored result of an engine pass depends on a byte that neither this pass nor bind-time initialisation wrote.

resnet.py::_ensure_bound takes the engine's workspace from torch.empty: whatever an earlier tensor of the process left there (freed uint8
images of 255s read back as 0xFFFFFFFF, a NaN; a diverged run's activations).  Here every engine gets its workspace filled, through a
32-bit view, after the bind and before its first pass -- with one of ws_poison_cases.PATTERNS for the engine under test, with zeros for
the reference -- and every case of tests/ws_poison_cases.py is held to the zero-filled result bit for bit (deterministic mode), or to the
bounds of test_pass_order_default_mode (deterministic mode off).  The recovery leg needs no access to the workspace: one engine runs
all-NaN passes at max_batch, gets its running statistics back from a copy (the checkpoint reload) and must then compute every case as a
fresh engine does.  The run-time forms behind environment switches go through the C ABI: tests/test_gpu_netcheck.py, NETCHECK_WS_FILL.
What the laws catch on an engine broken on purpose: profiles/ws_poison_mutations.txt.

Audit of the workspace (csrc/net.hip, layout code of ocl_net_create, regions in workspace order).  ocl_net_bind writes NO workspace byte;
upload_descs runs in front of the first forward of a binding (descs_uploaded is reset by the bind), so a fill between _ensure_bound() and the
first pass destroys nothing.

  region                               first writer on every path to its first reader
  -----------------------------------  ------------------------------------------------------------------------------------------------
  off_g[0..3]  eval activations; the   eval forward: conv_eval writes bufs[k] in full for the PLANNED batch before the next layer reads
               backward's gA, gD       it.  Rows N..Nplan-1 of a bucketed plan (Nplan = N rounded up to 4 / 16) are computed from rows
                                       N..Nplan-1 of x4 / of the buffer in front, which this pass did not write: the eval padding
                                       images.  Nothing reads their outputs (avgpool_fwd and the head run over N rows).
                                       backward: avgpool_bwd writes gA = gbuf(0) in full, conv2's data gradient writes gD = gbuf(3)
  off_g[4]     gE                      conv1's data gradient of the block (plain store); only then the projection shortcut's data
                                       gradient adds onto it (EPI_ACCUM)
  off_dy[0..5] dL/dy ring              bn_bwd / bn_apply_e write the whole [N, Ho, Wo, C] tensor before the weight and data gradients
                                       of the layer read it (the ring: OCL_DY_KEEP=0, two streams)
  off_dykeep   24 per-layer dL/dy      as the ring; buffer k by the k-th BatchNorm backward of the pass (take_dy)
  off_partial  weight-gradient slabs   conv_wgrad_kernel / conv_wgrad_multi_kernel store every slab that the plan's reduction reads
                                       (stores, no accumulation onto a slab); wgrad_reduce_* read exactly the plan's slabs; the stem's
                                       region (16 / 48 MB in) and the side-by-side regions of the batched reduction likewise
  off_stats    forward statistics      cleared by the last grid row of pack_weights_kernel in every forward that packs, by the
               arena, kStatReps        same_weights memset (one clear from the first cell of one arena to the last of the other) in a
               replicas                train forward that does not.  Eval passes do not read it
  off_bsums    backward statistics     the same two clears; a second backward since the last forward clears it itself (bsums_clean).
               arena, the one-pass     ARRIVAL COUNTERS: a.barrier = 9 unsigned behind each BatchNorm's 8 x 2 x 2 x C accumulator
               kernel's accumulators   cells, inside bsums_doubles and so inside every one of these clears.  Every backward needs a
               and ARRIVAL COUNTERS    valid tape; the bind invalidates every tape and resets pack_src, so the first forward of a
                                       binding can never be a same_weights pass and always runs the pack launch (both arenas cleared,
                                       bsums_clean = true); afterwards each forward either clears (pack launch; train same_weights
                                       memset) or is an eval same_weights pass, which touches neither the arena nor bsums_clean; each
                                       backward leaves bsums_clean = false, so the next one clears.  No path reads a counter that was
                                       not cleared since the bind.  (The spin on the counter is bounded at 2^22 polls, and a counter
                                       of 0xFFFFFFFF ends the wait at once: wrong sums, not a hang, would be the symptom.)
  off_bsums    backward reduce +       bn_bwd_reduce_kernel ACCUMULATES (fx_add) into [set][G][2][C] cells at barena_off, the front part of
  (barena_off) apply sums, two sets    the arena (2 * kGmax * 2 * C cells per BatchNorm), bn_bwd_apply_kernel reads them: inside
               of up to 8 groups       bsums_doubles and so inside the clears of the row above.  In the default mode only frozen tapes and
                                       passes of three or more groups take this pair (the other kernels hold two groups): the
                                       -views-taped-g3 / -g4 cases, netcheck's (9, 3, 32, 1) in every run-time mode
  off_pack     weight packs            upload_descs zeroes the whole arena once (hipMemsetAsync); pack_weights_kernel rewrites the
                                       layouts of pack_mask in every forward that packs and in a backward whose packs were displaced
                                       (repack); padding rows / columns of a pack are never written again and stay zero
  off_fold     folded BatchNorm        launch_bn_fold in every eval forward, in front of the first convolution
  off_descs    pack / fold descriptors upload_descs (two hipMemcpyAsync), in front of the first pack launch
  off_head     dh2, dh1, dfeat,        head_backward writes dh2, dh1, dfeat in this order, each in full before its reader; the staged
               staged dout             dout is copied in front of a replayed sequence (OCL_GRAPH=1)
  slot: x4                             nchw3_to_nhwc4 writes all four lanes of images 0..N-1 (the fourth as 0.f: the stem's pack holds a
                                       zero row for it, but 0 * NaN is NaN)
  slot: y (one per convolution)        the convolution of the train forward, all of [N, Ho, Wo, Cout]
  slot: zstem, a1, z (per block)       bn_fwd_kernel in full; a1 is neither written nor read on a fused tape (slot_fused: conv2 and
                                       the backward recompute relu(bn1(y1)) from y1)
  slot: save mean / invstd             bn_fwd_kernel, or conv2's staging on a fused tape: G x C entries each, the backward reads G x C
  slot: feat, h1, h2, norms, out       avgpool_fwd, the head's gemm_small / l2norm launches: N rows, the backward reads N rows

Reads beyond what the pass wrote, as the kernels state them: weights past a pack's row go through a buffer descriptor whose out-of-range
area reads as zeros (conv_t_kernel.h) or land on the arena's zeroed padding; the padding groups of a K loop (Qpad) multiply staged patch
rows by those zero weights, and the patch rows are inside the operand; tiles of images past the batch's end read a stale patch region and
store nothing (convw.hip); the eval plans' padding images are whole images whose outputs nobody reads.  All of these are harmless only
if the zero is the WEIGHT and the operand is finite, or if nothing is stored: a layout in which an operand's padded channel split ran
into the next, unwritten region would pass every finite-slack layer test (tests/guarded.py: 4096.0) and fail here, where the next
region holds NaN or +inf.  On the tree this module was written for, no such read exists: every case is green under all three fills."""
import numpy as np
import pytest
import torch

import test_gpu_net as TN
import test_gpu_pass_order as PO
import ws_poison_cases as WC

pytestmark = pytest.mark.gpu

_ZISO = {}       # results of zero-filled engines: the keys of test_gpu_pass_order._ISO, and ("direct", case id)
_DATA = {}


@pytest.fixture(autouse=True)
def _deterministic(cuda):
    PO._set_det(True)
    yield
    PO._set_det(False)


def _word(pattern):
    return int(np.array(pattern, dtype=np.uint32).view(np.int32))


def fill_workspace(m, pattern):
    """Every 32-bit word of the bound workspace := pattern.  Bind wrote nothing there and the descriptors are uploaded by the first forward."""
    assert m._net is not None and m._ws.numel() % 4 == 0 and m._ws.data_ptr() % 4 == 0
    m._ws.view(torch.int32).fill_(_word(pattern))
    return m


def engine(model, n_slots=2, pattern=0):
    """test_gpu_pass_order._engine for the models of ws_poison_cases (a superset), with its workspace filled before the first pass."""
    agent, data, head, _, max_batch = WC.MODELS[model]
    m, _ = TN.build(agent, data, head or "mlp", max_batch=max_batch)
    m.n_slots = n_slots
    m._ensure_bound()
    m.train()
    return fill_workspace(m, pattern)


@pytest.fixture(autouse=True)
def _zero_filled_references(monkeypatch):
    """Every isolated result test_gpu_pass_order computes while this module runs comes from a zero-filled engine and is kept apart from the
    results of that module's own (torch.empty) engines."""
    monkeypatch.setattr(PO, "_ISO", _ZISO)
    monkeypatch.setattr(PO, "_engine", engine)


def _x(model, kind, n):
    key = (model, kind, n)
    if key not in _DATA:
        hw = WC.MODELS[model][3]
        rng = np.random.default_rng(9000 + 131 * sum(map(ord, kind)) + n)
        _DATA[key] = torch.from_numpy(rng.random((n, 3, hw, hw)).astype(np.float32)).to(PO._dev())
    return _DATA[key]


def _weights_like(out):
    key = ("w", tuple(out.shape))
    if key not in _DATA:
        _DATA[key] = torch.linspace(-1, 1, out.numel()).view(out.shape).to(PO._dev()) / out.shape[0]
    return _DATA[key]


def run_direct(m, case):
    """One direct case on the engine (its gradient is fresh); returns name -> host array of everything the pass stores."""
    model, kind, n = case["model"], case["kind"], case["n"]
    x = _x(model, kind, n)
    res = {}
    if kind == "features":
        m.eval()
        with torch.no_grad():
            res["feat"] = m.features_batched(x)
        m.train()
    elif kind == "with_params":
        shadow = (m.flat_params() * 1.05).contiguous()
        if not case["train"]:
            m.eval()
        with torch.no_grad():
            res["out"] = m.forward_with_params(x, shadow)
        m.train()
    elif kind == "stats_only":
        m.forward_stats_only(x)
    elif kind == "no_grad":
        with torch.no_grad():
            res["out"] = m.forward(x)
    elif kind == "train":
        g = case["groups"]
        per = n // g
        out = m.forward(x) if g == 1 else m.forward_views([x[i * per:(i + 1) * per] for i in range(g)])
        (out * _weights_like(out)).sum().backward()
        res["out"], res["grad"] = out, m.flat_grads().clone()
    elif kind == "taped":
        g = case["groups"]
        per = n // g
        out, tape = m.forward_views_taped([x[i * per:(i + 1) * per] for i in range(g)])
        m.backward_taped(tape, _weights_like(out).contiguous())
        res["out"], res["grad"] = out, m.flat_grads().clone()
    elif kind == "same_weights":
        with m.same_weights():
            m.eval()
            with torch.no_grad():
                res["feat0"] = m.features_batched(x)          # packs
                res["feat1"] = m.features_batched(x[:5])      # the flag: no launch in front of the convolutions
            m.train()
            out = m.forward(x)                                # the flag in train mode: one memset over both statistics arenas
            (out * _weights_like(out)).sum().backward()
            res["out"], res["grad"] = out, m.flat_grads().clone()
    else:
        raise AssertionError(kind)
    res["running"], res["nbt"] = m._running.clone(), m._nbt.clone()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def zero_filled(case):
    key = ("direct", case["id"])
    if key not in _ZISO:
        _ZISO[key] = run_direct(engine(case["model"], case["n_slots"], 0), case)
    return _ZISO[key]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_direct(m, case, exact=True):
    want = zero_filled(case)
    PO._set_det(exact)
    got = run_direct(m, case)
    PO._set_det(True)
    assert got.keys() == want.keys()
    table = PO._tensor_table(m)
    for k in sorted(want):
        g, w = got[k], want[k]
        assert np.isfinite(w).all(), "%s: the zero-filled %s is not finite" % (case["id"], k)
        if exact:
            assert _same_bits(g, w), "%s: %s differs from the zero-filled engine's in %d of %d elements (%d not finite)" % (
                case["id"], k, int((g != w).sum()), g.size, int((~np.isfinite(g)).sum()))
            continue
        # deterministic mode off: finite, and the bounds of test_pass_order_default_mode (outputs 1e-4 absolute, every gradient tensor 2e-4 of
        # its largest entry); nothing else is bounded there, so nothing else is bounded here
        assert np.isfinite(g).all(), "%s: %s is not finite" % (case["id"], k)
        if k == "grad":
            bad = [(name, e) for name, e in ((name, float(np.abs(g[o:o + nel] - w[o:o + nel]).max() / (1e-12 + np.abs(w[o:o + nel]).max())))
                                             for name, o, nel in table) if not e < 2e-4]
            assert not bad, (case["id"], bad[:4])
        elif k in ("out", "feat", "feat0", "feat1"):
            err = float(np.abs(g - w).max())
            print("%s: %s err %.3e" % (case["id"], k, err))
            assert err < 1e-4, (case["id"], k)


def check_seq(m, case, exact=True):
    model, seq = case["model"], case["seq"]
    assert model in PO.PC.MODELS
    for op in seq:       # references first: no other engine inside the sequence
        if op[0] == "F":
            PO.isolated(model, op[2])
    PO._set_det(exact)
    rec = PO.execute(m, model, seq)
    torch.cuda.synchronize()
    PO._set_det(True)
    assert rec["backward"]
    PO.verify(m, model, rec, exact)
    if not exact:
        for b in rec["backward"]:
            assert bool(torch.isfinite(b["out"]).all()) and bool(torch.isfinite(b["got"]).all()), case["id"]
        assert bool(torch.isfinite(m._running).all()), case["id"]


def check(m, case, exact=True):
    (check_seq if case["kind"] == "seq" else check_direct)(m, case, exact)


@pytest.mark.parametrize("cid", WC.IDS)
@pytest.mark.parametrize("pattern", sorted(WC.PATTERNS))
def test_first_passes_over_a_filled_workspace(cuda, pattern, cid):
    """The case as the first passes of an engine whose workspace holds the pattern in every word: output, flat gradient, running
    statistics and num_batches_tracked equal the zero-filled engine's bit for bit."""
    case = WC.find(cid)
    check(engine(case["model"], case["n_slots"], WC.PATTERNS[pattern]), case)


@pytest.mark.parametrize("cid", WC.IDS)
def test_first_passes_over_a_nan_workspace_default_mode(cuda, cid):
    """Deterministic mode off (atomic batch sums), 0xFFFFFFFF fill: every result finite and within the bounds of
    test_pass_order_default_mode against the deterministic zero-filled result."""
    case = WC.find(cid)
    check(engine(case["model"], case["n_slots"], WC.PATTERNS["nan"]), case, exact=False)


_DIVERGED = {}   # model -> (the one engine that ran the NaN passes, copies of its initial running statistics and num_batches_tracked)


def _diverged(model):
    if model not in _DIVERGED:
        _, _, _, hw, max_batch = WC.MODELS[model]
        m = engine(model, max(c["n_slots"] for c in WC.CASES if c["model"] == model), 0)
        running, nbt = m._running.clone(), m._nbt.clone()
        nan = torch.full((max_batch, 3, hw, hw), float("nan"), device=PO._dev())
        half = max_batch // 2
        m.forward_views([nan[:half], nan[half:]]).sum().backward()
        m.eval()
        with torch.no_grad():
            m.features_batched(nan)
        m.train()
        assert not bool(torch.isfinite(m.flat_grads()).all()) and not bool(torch.isfinite(m._running).all()), "the NaN passes left no trace"
        _DIVERGED[model] = (m, running, nbt)
    return _DIVERGED[model]


@pytest.mark.parametrize("cid", WC.IDS)
def test_recovery_after_non_finite_passes(cuda, cid):
    """The checkpoint reload, on ONE engine per model and without any access to its workspace: a max_batch train forward + backward on
    all-NaN input with two BatchNorm groups and an all-NaN eval pass leave NaN in every region a pass of that size writes.  With the
    running statistics and num_batches_tracked restored from a copy and zero_grad, the case equals the zero-filled fresh engine's result
    bit for bit."""
    case = WC.find(cid)
    m, running, nbt = _diverged(case["model"])
    m._running.copy_(running)
    m._nbt.copy_(nbt)
    m.zero_grad()
    check(m, case)
