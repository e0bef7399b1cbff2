"""CPU: the host side of the DER agent (the argument checks of csrc/der.hip's entry point and of ops.der_loss, the registries, the
kernel's use of scratch) and the references the GPU tests rely on (tests/der_ref.py): the float64 statement of the loss against torch's
float64 autograd, the plain float32 statement against torch's own functions, and the reservoir statement with its logit field against
oracle.ocl_oracle.reservoir_update."""
import ctypes as C
import math
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from conftest import ROOT
from oracle import ocl_oracle as O
import der_ref
from der_ref import ref_der, torch32_der, kernel_case

OCL_ERR_ARG = -1    # include/ocl_hip.h
HIPCC = "/opt/rocm/bin/hipcc"

SHAPES = [(1, 0, 0), (1, 1, 1), (3, 3, 3), (10, 10, 10), (10, 10, 0), (10, 0, 10), (10, 7, 3), (5, 37, 3)]


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16      # a host address: never dereferenced, every case below is refused first
MB = 1 << 24
N0, N1, N2, CC, M = 4, 3, 2, 8, 6
BYTES = (N0 + N1 + N2) * CC * 4
TABLE = M * CC * 4


def _der(**over):
    kw = dict(logits=A, y0=A + MB, y2=A + 2 * MB, stored=A + 3 * MB, slots=A + 4 * MB, n0=N0, n1=N1, n2=N2, c=CC, m=M, alpha=0.1, beta=0.5,
              loss=A + 5 * MB, dl=A + 6 * MB)
    kw.update(over)
    if "dl_at" in kw:                      # dlogits placed relative to another array (an id must not carry a process address)
        kw["dl"] = kw[kw["dl_at"][0]] + kw["dl_at"][1]
    rc = ffi.lib().ocl_der_fwd_bwd(ffi.vp(kw["logits"]), ffi.vp(kw["y0"]), ffi.vp(kw["y2"]), ffi.vp(kw["stored"]), ffi.vp(kw["slots"]), kw["n0"],
                                   kw["n1"], kw["n2"], kw["c"], kw["m"], kw["alpha"], kw["beta"], ffi.vp(kw["loss"]), ffi.vp(kw["dl"]), ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signature_is_registered_and_declared():
    vp, f32, i = ffi.vp, C.c_float, C.c_int
    assert ffi.SIGNATURES["ocl_der_fwd_bwd"] == (C.c_int, [vp, vp, vp, vp, vp, i, i, i, i, i, f32, f32, vp, vp, vp])
    header = open(ROOT + "/include/ocl_hip.h").read()
    assert hasattr(ffi.lib(), "ocl_der_fwd_bwd") and re.search(r"\bocl_der_fwd_bwd\(", header)
    assert "der.hip" in open(ROOT + "/online-continual-learning_amd/csrc/Makefile").read()
    assert "K6e" in open(ROOT + "/online-continual-learning_amd/csrc/row_dev.h").read()


@pytest.mark.parametrize("over", [
    dict(logits=0), dict(y0=0), dict(loss=0), dict(stored=0), dict(y2=0),
    dict(n0=0), dict(n0=-2), dict(n1=-1), dict(n2=-1), dict(c=0), dict(c=-1), dict(m=0), dict(m=-4),
    dict(alpha=math.nan), dict(alpha=math.inf), dict(beta=math.nan), dict(beta=-math.inf),
    dict(dl_at=("logits", 0)), dict(dl_at=("logits", BYTES - 4)), dict(dl_at=("logits", 4 - BYTES)),     # on, ending inside, starting inside
    dict(dl_at=("stored", 0)), dict(dl_at=("stored", TABLE - 4)), dict(dl_at=("stored", 4 - BYTES)),
], ids=lambda o: ",".join("%s=%s" % (k, "%s%+d" % v if isinstance(v, tuple) else v) for k, v in o.items()))
def test_entry_point_refuses_bad_arguments_without_a_device(over):
    rc, msg = _der(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("der_loss:"), msg
    if "dl_at" in over:
        assert "overlaps " + over["dl_at"][0] in msg, msg


def test_ops_wrapper_refuses_wrong_dtype_shape_layout_and_device_without_a_device():
    """Every check of ops.der_loss comes before the library is initialised: CPU tensors are enough to reach each of them (a well-formed
    set of CPU tensors is refused for its device)."""
    from ocl_amd import ops
    s, y0, y2 = torch.zeros(9, 8), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    st, sl = torch.zeros(6, 8), torch.zeros(3, dtype=torch.int64)
    wide = torch.zeros(9, 16)
    good = dict(logits=s, y0=y0, y2=y2, stored=st, slots=sl)
    bad = [
        ("logits dtype", dict(logits=s.double())), ("logits rank", dict(logits=s.reshape(-1))), ("logits layout", dict(logits=wide[:, :8])),
        ("logits rows", dict(logits=torch.zeros(10, 8))),
        ("y0 dtype", dict(y0=y0.int())), ("y0 shape", dict(y0=y0[:3])), ("y0 layout", dict(y0=torch.zeros(8, dtype=torch.int64)[::2])),
        ("y2 dtype", dict(y2=y2.int())), ("y2 shape", dict(y2=torch.zeros(3, dtype=torch.int64))), ("y2 missing", dict(y2=None)),
        ("stored dtype", dict(stored=st.double())), ("stored columns", dict(stored=torch.zeros(6, 7))), ("stored layout", dict(stored=torch.zeros(6, 16)[:, :8])),
        ("stored missing", dict(stored=None)), ("stored rank", dict(stored=torch.zeros(48))),
        ("slots dtype", dict(slots=sl.int())), ("slots shape", dict(slots=torch.zeros(4, dtype=torch.int64))),
        ("no slots, short table", dict(slots=None, stored=torch.zeros(2, 8))),
    ]
    for what, over in bad:
        kw = dict(good, **over)
        with pytest.raises(RuntimeError, match="der_loss"):
            ops.der_loss(kw["logits"], kw["y0"], kw["y2"], kw["stored"], kw["slots"], 4, 3, 2, 0.1, 0.5)
    for n0, n1, n2 in ((0, 3, 6), (4, -1, 6), (4, 3, 3), (5, 3, 2)):
        with pytest.raises(RuntimeError, match="der_loss"):
            ops.der_loss(s, y0, y2, st, sl, n0, n1, n2, 0.1, 0.5)
    for what, dl in (("dl_out dtype", torch.zeros(9, 8, dtype=torch.float64)), ("dl_out shape", torch.zeros(10, 8)), ("dl_out layout", wide[:, :8])):
        with pytest.raises(RuntimeError, match="dl_out"):
            ops.der_loss(s, y0, y2, st, sl, 4, 3, 2, 0.1, 0.5, dl_out=dl)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.der_loss(s, y0, y2, st, sl, 4, 3, 2, 0.1, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.der_loss(s[:4].contiguous(), y0, None, None, None, 4, 0, 0, 0.1, 0.5)


# ---- registries ---------------------------------------------------------------------------------------------------------------------------

def test_der_resolves_by_name_and_every_older_table_keeps_its_keys():
    from ocl_amd import name_match
    from ocl_amd.agents.der import Der
    from ocl_amd.agents.base import ContinualLearner
    assert name_match.get_agent("DER") is Der and issubclass(Der, ContinualLearner)
    assert set(name_match.logit_replay_agents.keys()) == {"DER"} and name_match.logit_replay_agents["DER"] is Der
    assert set(name_match.agents.keys()) == {"ER", "SCR"}
    assert set(name_match.extra_agents.keys()) == {"AGEM"}
    assert set(name_match.regularization_agents.keys()) == {"EWC"}
    assert set(name_match.distillation_agents.keys()) == {"LWF"}
    assert set(name_match.offline_agents.keys()) == {"GDUMB"}
    assert set(name_match.exemplar_agents.keys()) == {"ICARL"}
    assert Der._force_autograd is False
    assert "DER" not in " ".join(ffi.KNOWN_ENV)


def test_constructor_refuses_another_update_or_retrieve_method_before_it_builds_a_memory():
    from types import SimpleNamespace
    from ocl_amd.agents.der import Der
    trick = {k: False for k in ('labels_trick', 'kd_trick', 'separated_softmax', 'review_trick', 'ncm_trick', 'kd_trick_star')}
    for update, retrieve in (("GSS", "random"), ("ASER", "random"), ("random", "MIR"), ("random", "ASER")):
        params = SimpleNamespace(data="cifar10", cuda=True, epoch=1, batch=10, verbose=False, agent="DER", trick=trick, error_analysis=False,
                                 update=update, retrieve=retrieve, mem_size=30, eps_mem_batch=10, mem_iters=1)
        with pytest.raises(ValueError, match="do not carry the logit field"):
            Der(torch.nn.Linear(2, 2), None, params)


# ---- the float64 statement ------------------------------------------------------------------------------------------------------------------

def _torch64(s, y0, y2, stored, slots, n0, n1, n2, alpha, beta):
    x = torch.from_numpy(np.asarray(s, dtype=np.float64)).requires_grad_(True)
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    ce = F.cross_entropy(x[:n0], torch.from_numpy(y0))
    mse = ce_m = torch.zeros((), dtype=torch.float64)
    if n1:
        mse = F.mse_loss(x[n0:n0 + n1], torch.from_numpy(np.asarray(stored, dtype=np.float64))[torch.from_numpy(slots)])
    if n2:
        ce_m = F.cross_entropy(x[n0 + n1:], torch.from_numpy(y2))
    loss = ce + alpha * mse + beta * ce_m
    loss.backward()
    return np.array([float(v.detach()) for v in (loss, ce, mse, ce_m)]), x.grad.numpy()


@pytest.mark.parametrize("c,scale", [(5, 1), (100, 30), (257, 300)])
@pytest.mark.parametrize("n0,n1,n2", SHAPES)
def test_float64_statement_equals_torch_float64_autograd(n0, n1, n2, c, scale):
    s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, scale)
    l64, g64 = ref_der(s, y0, y2, stored, slots, n0, n1, n2, 0.1, 0.5)
    lt, gt = _torch64(s, y0, y2, stored, slots, n0, n1, n2, 0.1, 0.5)
    assert np.abs(l64 - lt).max() <= 1e-12 * max(1.0, np.abs(lt).max()), (l64, lt)
    assert np.abs(g64 - gt).max() <= 1e-12 * np.abs(gt).max(), np.abs(g64 - gt).max()
    if n1 == 0:
        assert l64[2] == 0.0
    if n2 == 0:
        assert l64[3] == 0.0


def test_float64_statement_on_one_row_per_block_worked_out_by_hand():
    """Block 0: s = [0, log 3], y = 0: softmax = [1/4, 3/4], ce = log 4.  Block 1: s = [1, -1] against z = [0, 1]: mse = (1 + 4) / 2,
    gradient alpha * 2 * [1, -2] / 2.  Block 2: s = [log 4, 0], y = 1: softmax = [4/5, 1/5], ce_m = log 5."""
    s = np.array([[0.0, math.log(3.0)], [1.0, -1.0], [math.log(4.0), 0.0]])
    stored = np.array([[9.0, 9.0], [0.0, 1.0]])
    a, b = float(np.float32(0.1)), 0.5
    loss4, dl = ref_der(s, [0], [1], stored, [1], 1, 1, 1, 0.1, 0.5)
    assert loss4 == pytest.approx([math.log(4.0) + a * 2.5 + b * math.log(5.0), math.log(4.0), 2.5, math.log(5.0)], rel=1e-14)
    assert dl == pytest.approx(np.array([[-0.75, 0.75], [a * 1.0, a * -2.0], [b * 0.8, b * -0.8]]), rel=1e-13)
    same4, same_dl = ref_der(s, [0], [1], stored[1:], None, 1, 1, 1, 0.1, 0.5)      # slots None: row 0 of the table
    assert np.array_equal(same4, loss4) and np.array_equal(same_dl, dl)


@pytest.mark.parametrize("c,scale", [(5, 1), (100, 30), (257, 300)])
@pytest.mark.parametrize("n0,n1,n2", SHAPES)
def test_plain_float32_statement_is_torchs_own_functions_and_agrees_with_the_float64_one(n0, n1, n2, c, scale):
    s, y0, y2, stored, slots, m = kernel_case(n0, n1, n2, c, scale)
    l32, g32 = torch32_der(s, y0, y2, stored, slots, n0, n1, n2, 0.1, 0.5)
    assert l32.dtype == g32.dtype == np.float32
    x = torch.from_numpy(s).requires_grad_(True)
    a, b = float(np.float32(0.1)), float(np.float32(0.5))
    ce = F.cross_entropy(x[:n0], torch.from_numpy(y0))
    loss = ce
    if n1:
        mse = F.mse_loss(x[n0:n0 + n1], torch.from_numpy(stored)[torch.from_numpy(slots)])
        loss = loss + a * mse
        assert float(mse.detach()) == l32[2]
    if n2:
        ce_m = F.cross_entropy(x[n0 + n1:], torch.from_numpy(y2))
        loss = loss + b * ce_m
        assert float(ce_m.detach()) == l32[3]
    loss.backward()
    assert float(loss.detach()) == l32[0] and float(ce.detach()) == l32[1] and np.array_equal(x.grad.numpy(), g32)
    l64, g64 = ref_der(s, y0, y2, stored, slots, n0, n1, n2, 0.1, 0.5)
    assert np.abs(l32 - l64).max() <= 2e-6 * max(1.0, np.abs(l64).max()), (l32, l64)
    assert np.abs(g32 - g64).max() <= 2e-6 * np.abs(g64).max(), np.abs(g32 - g64).max()


# ---- the reservoir statement with its logit field ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(10, 10, 10, 10, 10, 10), (10, 70, 10, 25), (45, 3, 60)], ids=str)
def test_reservoir_statement_leaves_what_the_oracles_leaves_and_draws_as_much(sizes):
    """From one RNG state: images, labels, counters and the torch generator's state afterwards are those of O.reservoir_update, and the
    written slots are its returned list; every filled slot's logit row is the row that came with the image now in it (the rows encode
    the item's running index, and so does the image's first pixel)."""
    mem, n_cls = 30, 4
    a, b = O.OracleBuffer(mem, (3, 2, 2)), der_ref.der_buffer(mem, (3, 2, 2), n_cls)
    torch.manual_seed(5)
    seen = 0
    for n in sizes:
        ids = torch.arange(seen, seen + n, dtype=torch.float32)
        x = ids.reshape(n, 1, 1, 1).expand(n, 3, 2, 2).contiguous()
        y = (torch.arange(seen, seen + n) % 7).long()
        rows = ids.reshape(n, 1).expand(n, n_cls).contiguous() + 0.25
        seen += n
        st = torch.get_rng_state()
        room = mem - a.current_index
        slots = O.reservoir_update(a, x, y)
        if 0 < room < n:                          # a straddling batch: the reference's list names the overwritten slots alone
            slots = list(range(mem - room, mem)) + [s for s in slots if s < mem - room]
        after = torch.get_rng_state()
        torch.set_rng_state(st)
        pairs = der_ref.der_reservoir(b, x, y, rows)
        assert torch.equal(after, torch.get_rng_state()), "another amount was drawn"
        written = list(dict.fromkeys(s for s, _ in pairs))
        assert sorted(written) == sorted(slots)
        assert torch.equal(a.img, b.img) and torch.equal(a.label, b.label)
        assert (a.current_index, a.n_seen_so_far) == (b.current_index, b.n_seen_so_far)
        k = b.current_index
        assert torch.equal(b.logits[:k], b.img[:k, 0, 0, 0].reshape(k, 1).expand(k, n_cls) + 0.25)
        assert bool((b.logits[k:] == 0).all())
    assert b.current_index == mem and b.n_seen_so_far == sum(sizes)


# ---- the kernel uses no scratch ------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_der_kernels_use_no_scratch_and_spill_nothing():
    """csrc/der.hip for gfx950 with the compiler's resource remarks, parsed as tests/test_cpu_lwf.py parses distill.hip's: every
    instantiation (row in registers or strided, with and without replay blocks)."""
    src = ROOT + "/online-continual-learning_amd/csrc/der.hip"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            cur = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur).replace("void ", "").replace("ocl::", "")
            res[cur] = {}
        elif cur:
            for key in ("ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size"):
                if t.startswith(key):
                    res[cur][key] = int(re.search(r":\s*(\d+)", t).group(1))
    hits = {k: v for k, v in res.items() if re.fullmatch(r"der_loss_kernel<(true|false), (true|false)>", k)}
    assert len(hits) == 4 and len(res) == 4, sorted(res)
    for k, v in hits.items():
        lds = 80 if k.endswith("true>") else 16      # the per-wave partials: one float sum, and with replay blocks two double sums
        assert v == {"ScratchSize": 0, "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size": lds}, (k, v)
