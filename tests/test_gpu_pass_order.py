"""GPU: the host state that csrc/net.hip carries from one pass to the next -- who owns the weight-pack arena and which layouts it holds
(pack_src, pack_have, pack_stream, pack_need_fwd / pack_need_bwd), whether the backward's statistics arena is clean (bsums_clean), the
per-slot tape records beside arenas that are NOT per slot (the pack arena, both statistics arenas, gbuf(0..4), the dL/dy buffers, the
weight-gradient slabs, the head scratch), the weight-gradient tables and the side stream's events, the replay keys of OCL_GRAPH=1.

With ops.set_deterministic(True) every pass is bit-reproducible, so two laws need no tolerance:

* isolation: a taped pass's output, parameter gradient and running-statistics update equal, bit for bit, those of the same pass run alone
  on a fresh engine with the same weights (forward, backward at once into a fresh gradient) -- whatever sat between its forward and its
  backward, whatever the engine ran before;
* accumulation: with accumulate = 1 every gradient element equals np.float32(existing) + np.float32(fresh), bit for bit, `fresh` being
  the isolated overwrite result (wgrad_reduce_few / wgrad_reduce_body, colsum_kernel, gemm_small_kernel and the a.accumulate branches of
  bn.hip all add the freshly computed fp32 value to the stored one); encoder.linear of a SupConResNet has a zero fresh gradient, so its
  `existing` comes back unchanged.

Every probe pass is a row of test_gpu_net.CASES (asserted, not restated), which test_train_forward_backward_vs_oracle holds to the oracle
in isolation: bit-equality carries that pin over to every ordering of tests/pass_order_cases.py.

What each law catches when the engine is broken on purpose (never re-pack in the backward, no clear of the statistics arena by a second
backward, `accumulate` ignored in wgrad_reduce_few) is recorded in profiles/pass_order_mutations.txt -- with the reason why intruder I2p
(the C ABI's OCL_FWD_PACK_ALL on another parameter array) stands beside I2 and I3.

Out of scope: writing the weights between a taped forward and its backward (the engine backpropagates through the current array; the
reference never does this)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pass_order_cases as PC
import test_gpu_net as TN
from agent_harness import host as _host
from conftest import ROOT

pytestmark = pytest.mark.gpu

_ISO = {}        # (model, probe) or (model, "fz", n, digest of the running statistics) -> isolated result
_DATA = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _set_det(on):
    from ocl_amd import ops
    ops.set_deterministic(on)


@pytest.fixture(autouse=True)
def _deterministic(cuda):
    _set_det(True)
    yield
    _set_det(False)


def _engine(model, n_slots=2):
    agent, data, head, _, max_batch = PC.MODELS[model]
    m, _ = TN.build(agent, data, head or "mlp", max_batch=max_batch)
    m.n_slots = n_slots
    m._ensure_bound()
    m.train()
    return m


def _probe_data(model, probe):
    """Inputs and labels of the probe as test_gpu_net draws them (default_rng(n))."""
    key = (model, probe)
    if key not in _DATA:
        assert PC.case_probe(model, probe) in TN.CASES, "probe %s of %s is not a case of test_gpu_net" % (probe, model)
        n, groups, _, _ = PC.PROBES[model][probe]
        hw = PC.MODELS[model][3]
        rng = np.random.default_rng(n)
        x = rng.random((n, 3, hw, hw)).astype(np.float32)
        y = rng.integers(0, 10, n).astype(np.int64)
        _DATA[key] = (torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev()), groups)
    return _DATA[key]


def _other_data(model, kind, n):
    key = (model, kind, n)
    if key not in _DATA:
        hw = PC.MODELS[model][3]
        rng = np.random.default_rng(5000 + 97 * sum(map(ord, kind)) + n)
        x = rng.random((n, 3, hw, hw)).astype(np.float32)
        y = rng.integers(0, 10, n).astype(np.int64)
        _DATA[key] = (torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev()))
    return _DATA[key]


def _loss(model, out, y):
    """As test_gpu_net: cross-entropy for the models without a head, (out * linspace).sum() for SCR."""
    if PC.MODELS[model][2] is None:
        from ocl_amd.loss import cross_entropy_mean
        return cross_entropy_mean(out, y)
    key = ("w", tuple(out.shape))
    if key not in _DATA:
        _DATA[key] = torch.linspace(-1, 1, out.numel()).view(out.shape).to(_dev())
    return (out * _DATA[key]).sum()


def _forward_probe(m, model, probe):
    x, y, groups = _probe_data(model, probe)
    per = x.shape[0] // groups
    out = m.forward(x) if groups == 1 else m.forward_views([x[g * per:(g + 1) * per] for g in range(groups)])
    return out, y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def isolated(model, probe):
    """The probe alone on a fresh engine: forward, backward at once into a fresh gradient (deterministic mode)."""
    key = (model, probe)
    if key not in _ISO:
        m = _engine(model)
        out, y = _forward_probe(m, model, probe)
        _loss(model, out, y).backward()
        _ISO[key] = dict(out=_host(out), grad=_host(m.flat_grads()).copy(), running=_host(m._running).copy(), nbt=_host(m._nbt).copy())
    return _ISO[key]


def isolated_frozen(model, n, running, nbt):
    """A frozen-BatchNorm tape alone on a fresh engine that holds the given running statistics."""
    key = (model, "fz", n, hashlib.sha1(running.tobytes()).hexdigest())
    if key not in _ISO:
        m = _engine(model)
        m._running.copy_(torch.from_numpy(running).to(_dev()))
        m._nbt.copy_(torch.from_numpy(nbt).to(_dev()))
        x, y = _other_data(model, "FZ", n)
        m.eval()
        out = m.forward(x)
        m.train()
        _loss(model, out, y).backward()
        assert np.array_equal(_host(m._running), running), "a frozen tape touched the running statistics"
        _ISO[key] = dict(out=_host(out), grad=_host(m.flat_grads()).copy())
    return _ISO[key]


def execute(m, model, seq):
    """Issues the sequence on the engine without a synchronisation in between; returns the records (device tensors)."""
    flat = m.flat_grads()
    shadow = (m.flat_params() * 1.05).contiguous()
    tapes, fresh = {}, True
    rec = dict(backward=[], running=[], errors=[])

    def stat_point(op):
        rec["running"].append((op, m._running.clone(), m._nbt.clone()))

    for op in seq:
        kind = op[0]
        if kind == "F":
            out, y = _forward_probe(m, model, op[2])
            tapes[op[1]] = dict(kind="F", probe=op[2], out=out, loss=_loss(model, out, y))
            stat_point(op)
        elif kind == "FZ":
            x, y = _other_data(model, "FZ", op[2])
            running, nbt = m._running.clone(), m._nbt.clone()
            m.eval()
            out = m.forward(x)
            m.train()
            tapes[op[1]] = dict(kind="FZ", n=op[2], out=out, loss=_loss(model, out, y), running=running, nbt=nbt)
        elif kind in ("B", "BZ"):
            t = tapes[op[1]]
            existing = None if fresh else flat.clone()
            t["loss"].backward(retain_graph=(len(op) > 2 and op[2] == "retain"))
            rec["backward"].append(dict(t, tape=op[1], existing=existing, got=flat.clone(), running_after=m._running.clone()))
            fresh = False
        elif kind == "B!":
            before = flat.clone()
            with pytest.raises(RuntimeError, match="tape"):
                tapes[op[1]]["loss"].backward()
            rec["errors"].append((op[1], before, flat.clone()))
        elif kind == "DROP":
            tapes[op[1]]["loss"] = None
        elif kind == "Z":
            m.zero_grad()
            fresh = True
        elif kind == "G0":
            assert not fresh, "G0 follows a backward (the gradient views are attached, the next backward accumulates)"
            g0 = np.random.default_rng(77).standard_normal(flat.numel()).astype(np.float32)
            flat.copy_(torch.from_numpy(g0).to(flat.device))
        elif kind == "I1":
            m.eval()
            with torch.no_grad():
                m.features_batched(_other_data(model, "I1", op[1])[0])
            m.train()
        elif kind in ("I2", "I3"):
            if kind == "I3":
                m.eval()
            with torch.no_grad():
                m.forward_with_params(_other_data(model, "I2", op[1])[0], shadow)
            m.train()
        elif kind == "I2p":
            # (resnet.py never sends OCL_FWD_PACK_ALL with another parameter array; the C ABI takes it: see pass_order_cases.py)
            from ocl_amd import ffi
            parts, n, ptrs, sizes = m._segments(_other_data(model, "I2", op[1])[0])
            scratch_out = torch.empty((n, m.out_dim), dtype=torch.float32, device=flat.device)
            ffi.check(ffi.lib().ocl_net_forward_segments(m._net, ptrs, sizes, len(parts), 1, ffi.FWD_TRAIN | ffi.FWD_PACK_ALL, ffi.ptr(shadow), None,
                                                         ffi.ptr(scratch_out), m._n_tapes, ffi.stream()), "net_forward(pack all, other array)")
        elif kind == "I4":
            m.forward_stats_only(_other_data(model, "I4", op[1])[0])
            stat_point(op)
        elif kind == "I5":
            with torch.no_grad():
                m.forward(_other_data(model, "I5", op[1])[0])
            stat_point(op)
        else:
            raise AssertionError(op)
    return rec


def _tensor_table(m):
    base = m.flat_params().data_ptr()
    return [(k, (p.data.data_ptr() - base) // 4, p.numel()) for k, p in m.named_parameters()]


def _stat_replica(model, points):
    """A fresh engine that runs only the statistic-updating passes, in the same order, each without a tape (scratch slot)."""
    m = _engine(model)
    snaps = []
    for op, _, _ in points:
        if op[0] == "F":
            with torch.no_grad():
                _forward_probe(m, model, op[2])
        elif op[0] == "I4":
            m.forward_stats_only(_other_data(model, "I4", op[1])[0])
        else:
            with torch.no_grad():
                m.forward(_other_data(model, "I5", op[1])[0])
        snaps.append((_host(m._running).copy(), _host(m._nbt).copy()))
    return snaps


def verify(m, model, rec, exact=True):
    """exact: the two laws, bit for bit.  Otherwise (deterministic mode off) the bounds test_gpu_net holds the isolated pass to: outputs
    1e-4 absolute, every gradient tensor 2e-4 of its largest entry."""
    torch.cuda.synchronize()
    table = _tensor_table(m)
    for b in rec["backward"]:
        if b["kind"] == "F":
            iso = isolated(model, b["probe"])
            what = "tape %s (probe %s)" % (b["tape"], b["probe"])
        else:
            iso = isolated_frozen(model, b["n"], _host(b["running"]), _host(b["nbt"]))
            what = "frozen tape %s (n=%d)" % (b["tape"], b["n"])
        out, got = _host(b["out"]), _host(b["got"])
        accumulate = b["existing"] is not None
        want = iso["grad"] if not accumulate else np.float32(_host(b["existing"])) + np.float32(iso["grad"])
        if exact:
            assert np.array_equal(_bits(out), _bits(iso["out"])), "%s: output differs from the isolated pass" % what
        else:
            err = float(np.abs(out - iso["out"]).max())
            print("%s: output err %.3e" % (what, err))
            assert err < 1e-4, what
        bad = []
        for name, off, nel in table:
            g, w = got[off:off + nel], want[off:off + nel]
            if exact:
                if not np.array_equal(_bits(g), _bits(w)):
                    bad.append((name, int((_bits(g) != _bits(w)).sum()), float(np.abs(g - w).max())))
            else:
                e = float(np.abs(g - w).max() / (1e-12 + np.abs(w).max()))
                if not e < 2e-4:
                    bad.append((name, e))
        assert not bad, "%s: %s law broken for %d tensors, e.g. %s" % (what, "accumulation" if accumulate else "isolation", len(bad), bad[:4])
        if b["kind"] == "FZ":
            assert np.array_equal(_host(b["running_after"]), _host(b["running"])), "%s touched the running statistics" % what
    for tape, before, after in rec["errors"]:
        assert np.array_equal(_bits(_host(before)), _bits(_host(after))), "the refused backward of %s changed the gradient" % tape
    if exact and rec["running"]:
        snaps = _stat_replica(model, rec["running"])
        for (op, run, nbt), (run_ref, nbt_ref) in zip(rec["running"], snaps):
            assert np.array_equal(_bits(_host(run)), _bits(run_ref)), "running statistics after %s" % (op,)
            assert np.array_equal(_host(nbt), nbt_ref), "num_batches_tracked after %s" % (op,)
        # ... and nothing after the last of them wrote the statistics
        assert np.array_equal(_bits(_host(m._running)), _bits(snaps[-1][0])) and np.array_equal(_host(m._nbt), snaps[-1][1])


def run_case(case, exact=True):
    model, seq = case["model"], case["seq"]
    for op in seq:       # isolated results first: no other engine, no synchronisation inside the sequence
        if op[0] == "F":
            isolated(model, op[2])
    m = _engine(model, case["n_slots"])
    _set_det(exact)
    rec = execute(m, model, seq)
    torch.cuda.synchronize()
    _set_det(True)
    assert rec["backward"], "a sequence without a backward checks nothing"
    verify(m, model, rec, exact)
    return m, rec


@pytest.mark.parametrize("cid", [c["id"] for c in PC.CASES])
def test_pass_order(cuda, cid):
    """One sequence of tests/pass_order_cases.py in deterministic mode: every backward against the isolation law (overwrite) or the
    accumulation law (accumulate), the output of every consumed tape, the running statistics after every pass that updates them against
    an engine that ran only those passes."""
    run_case(PC.find(cid))


@pytest.mark.parametrize("cid", PC.DEFAULT_MODE)
def test_pass_order_default_mode(cuda, cid):
    """Deterministic mode off (atomic batch sums): the same sequences against the deterministic isolated result, within the bounds
    test_gpu_net holds the isolated pass to."""
    run_case(PC.find(cid), exact=False)


# ---- launch-sequence replay (OCL_GRAPH=1, csrc/net.hip run_replayed) ---------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_pass_order as T
T.replay_child(sys.argv[1])
"""


def _replay_arrays(m, rec):
    out = {}
    for i, b in enumerate(rec["backward"]):
        out["out%02d" % i] = _host(b["out"])
        out["grad%02d" % i] = _host(b["got"])
    out["running"] = _host(m._running)
    out["nbt"] = _host(m._nbt)
    return out


def replay_child(path):
    """Runs in the child process: the replay sequence on a stream of its own (capture is refused on the default stream)."""
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi
    ffi.init()
    _set_det(True)
    with torch.cuda.stream(torch.cuda.Stream()):
        m = _engine(PC.REPLAY_MODEL, PC.REPLAY_SLOTS)
        rec = execute(m, PC.REPLAY_MODEL, PC.replay_sequence())
        torch.cuda.synchronize()
        np.savez(path, **_replay_arrays(m, rec))


def test_pass_order_under_launch_sequence_replay(cuda, tmp_path):
    """OCL_GRAPH=1 in a fresh child process: ordering 1 with I2 (the backward's `repack` key) and two live tapes (its `bsums_dirty` key)
    on the single-stream probes, three rounds on one engine -- first sight, capture, replay.  Every round's outputs and gradients and the
    final running statistics equal, bit for bit, what this process computes without replay (and holds to the two laws)."""
    seq = PC.replay_sequence()
    PC.check_sequence(seq, PC.REPLAY_SLOTS, PC.PROBES[PC.REPLAY_MODEL])
    m, rec = run_case(dict(model=PC.REPLAY_MODEL, seq=seq, n_slots=PC.REPLAY_SLOTS))
    want = _replay_arrays(m, rec)
    np.savez(str(tmp_path / "parent.npz"), **want)
    env = dict(os.environ, OCL_GRAPH="1", OCL_GRAPH_VERBOSE="1", PYTHONDONTWRITEBYTECODE="1")
    f = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}, f], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    want, got = dict(np.load(str(tmp_path / "parent.npz"))), dict(np.load(f))
    assert want.keys() == got.keys() and len(want) == 2 * 9 + 2
    for k in want:
        assert np.array_equal(want[k].view(np.uint32 if want[k].dtype == np.float32 else want[k].dtype),
                              got[k].view(np.uint32 if got[k].dtype == np.float32 else got[k].dtype)), "%s differs under OCL_GRAPH=1" % k
    captured = [l for l in r.stderr.splitlines() if l.startswith("ocl graph: captured kind 1")]
    failed = [l for l in r.stderr.splitlines() if l.startswith("ocl graph:") and "failed" in l]
    print("\n".join(l for l in r.stderr.splitlines() if l.startswith("ocl graph:")))
    assert captured and not failed, (captured[:4], failed[:4])
