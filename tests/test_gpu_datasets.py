"""GPU: --data core50 (128 x 128, 2560 features) and openloris (50 x 50: 50 -> 25 -> 13 -> 7, the 7 x 7 map cropped by avg_pool2d(4)),
and float task arrays (the reference's new-instance streams) through csrc/loader.hip.

* the float loader kernel, bit for bit against `torch.from_numpy(x[idx].transpose(0, 3, 1, 2).copy()).float()`;
* the network against oracle.OracleNet as tests/test_gpu_net.py::test_train_forward_backward_vs_oracle does (state from the product model's
  own state_dict, ReLU patterns teacher-forced, the same tolerances and the same ReLU-ambiguity allowance);
* every kernel form the planner gives at these sizes that the 32 / 84 grid lacks (tests/datasets_cases.py), and every layer shape of the
  new lattices, one layer at a time, integer-exact, through the cases of tests/test_gpu_layers.py;
* whole ER steps teacher-forced against the oracle's er_step, as tests/test_gpu_steps.py::test_cosim_er_random does, at both shapes and
  on a float64 (new-instance) task; one NCM evaluate() with 2560-wide features; one ASER retrieval at 50 x 50.

The ReLU-ambiguity allowance (n_mis <= 5 + 2e-5 * n_tot, worst ambiguous |pre-activation| < 1e-5 of the maximum) is not exceeded by the
reference arithmetic alone at these sizes: the oracle against itself with every weight moved by one ulp in a random direction gives, on
the cases below, 0 .. 5 mismatches of 4.4e5 .. 1.7e7 and a worst ratio of 1.0e-6 (profiles/datasets_parity.txt).

With OCL_PARITY_REPORT=<file> the figures go to datasets_parity.txt next to it (profiles/datasets_parity.txt)."""
import os
import zlib

import numpy as np
import pytest
import torch

import datasets_cases as DC
import test_gpu_layers as TL
import test_gpu_net as TN
import test_gpu_steps as TS
from oracle import ocl_oracle as O
from oracle.synth import class_images, seed_all

pytestmark = pytest.mark.gpu

HW = {"openloris": 50, "core50": 128, "cifar10": 32, "cifar100": 32}
REPORT = []


def record(case, quantity, err, bound):
    REPORT.append((case, quantity, err, bound, err / bound if bound else 0.0))


@pytest.fixture(scope="module")
def lib(cuda):
    from ocl_amd import ffi
    L = ffi.lib()
    torch.set_num_threads(16)
    yield L
    L.ocl_set_deterministic(0)
    path = os.environ.get("OCL_PARITY_REPORT")
    if path and REPORT:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "datasets_parity.txt"), "w") as f:
            f.write("# parity at the core50 (128 x 128) and openloris (50 x 50) shapes and on float tasks (tests/test_gpu_datasets.py): worst error,\n"
                    "# the bound it is held to (those of tests/test_gpu_net.py and tests/test_gpu_steps.py), and error / bound (must be < 1)\n")
            f.write("%-44s %-22s %12s %12s %8s\n" % ("case", "quantity", "error", "bound", "ratio"))
            for row in REPORT:
                f.write("%-44s %-22s %12.4g %12.4g %8.3f\n" % row)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float loader
# ---------------------------------------------------------------------------------------------------------------------------------------
def _special_values(x):
    """Sprinkle a float64 array with the values whose float32 rounding and bits matter: ties (to even, both directions), -0.0, a value
    that becomes a float32 denormal, 1.0 and a NaN."""
    flat = x.reshape(-1)
    vals = [1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24, 0.5 + 2.0 ** -25, -0.0, 1e-40, 1.0, float("nan"), 2.0 ** -149]
    for i, v in enumerate(vals):
        flat[i::len(vals) * 13][:64] = v
    return x


def _indices(n, rows, rng):
    """n picks of `rows` rows with repeats, always containing the last row (and row 0 when there is room)."""
    idx = rng.integers(0, rows, n)
    idx[-1] = rows - 1
    if n > 2:
        idx[0] = 0
        idx[1] = idx[-1] if n < 4 else idx[2]
    return idx.astype(np.int64)


@pytest.mark.parametrize("n", [1, 10, 128])
@pytest.mark.parametrize("h,w,c,misalign", [(5, 7, 3, False), (32, 32, 3, False), (32, 32, 3, True), (50, 50, 3, False), (128, 128, 3, False),
                                            (6, 6, 4, False), (20, 20, 1, False), (4, 4, 17, False)])
def test_f32_loader_kernel_is_bit_exact(cuda, h, w, c, misalign, n):
    """(5, 7, 3): 105 floats per row, the scalar form; misalign: the task is a view one float into its allocation, so its base is only
    4-byte aligned (scalar form on a shape that otherwise takes the 16-byte loads); the others: the tile form, with a last tile of
    less than 256 pixels at 50 x 50 (2500 = 9 * 256 + 196).  Beyond the issue's shapes: 4 channels and 1 channel on the tile form (one
    tile of 36 pixels; tiles of 256 + 144), and 17 channels, more than the tile form holds in LDS (scalar form)."""
    from ocl_amd import ops
    rows = 7 if h * w > 5000 else 19
    rng = np.random.default_rng(h * 1000 + n)
    x64 = _special_values(rng.random((rows, h, w, c)))
    x32 = x64.astype(np.float32)
    idx = _indices(n, rows, rng)
    ref = torch.from_numpy(x64[idx].transpose(0, 3, 1, 2).copy()).float()
    if misalign:
        store = torch.empty(x32.size + 1, dtype=torch.float32, device=cuda)
        task = store[1:].view(rows, h, w, c)
        task.copy_(torch.from_numpy(x32))
        assert task.data_ptr() % 16 == 4
    else:
        task = torch.from_numpy(x32).to(cuda)
        assert task.data_ptr() % 16 == 0
    got = ops.gather_f32_images(task, torch.from_numpy(idx).to(cuda)).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), ref.numpy().view(np.uint32)), "bits differ"
    assert np.array_equal(task.cpu().numpy().view(np.uint32), x32.view(np.uint32)), "the task was written"
    assert ops.gather_f32_images(task, torch.zeros(0, dtype=torch.long, device=cuda)).shape == (0, c, h, w)


def test_f32_loader_refuses_what_it_cannot_read(cuda):
    from ocl_amd import ops
    idx = torch.zeros(2, dtype=torch.long, device=cuda)
    with pytest.raises(RuntimeError):
        ops.gather_f32_images(torch.zeros(3, 5, 7, 3, dtype=torch.float64, device=cuda), idx)
    with pytest.raises(RuntimeError):
        ops.gather_f32_images(torch.zeros(3, 5, 7, 3), idx)
    with pytest.raises(RuntimeError):
        ops.gather_f32_images(torch.zeros(3, 5, 7, 3, device=cuda), idx.int())


@pytest.mark.parametrize("as_torch", [False, True])
def test_device_loader_float64_task_end_to_end(cuda, as_torch):
    """A float64 task through DeviceLoader: the batches are the reference's `transform(x[idx]).float()` in the order of the reference's
    DataLoader under the same seed, with the same RNG state afterwards; labels and host mirrors as on the uint8 path."""
    from ocl_amd.data import DeviceLoader
    from torch.utils import data as tdata
    n, bs = 53, 10
    rng = np.random.default_rng(3)
    x64 = _special_values(rng.random((n, 50, 50, 3)))
    ys = rng.integers(0, 69, n)
    torch.manual_seed(5)
    order = [b[1].numpy() for b in tdata.DataLoader(tdata.TensorDataset(torch.zeros(n, 1), torch.arange(n)), batch_size=bs, shuffle=True,
                                                    drop_last=True)]
    after_ref = torch.rand(3)
    torch.manual_seed(5)
    dl = DeviceLoader(torch.from_numpy(x64) if as_torch else x64, ys, bs, shuffle=True, drop_last=True)
    seen = 0
    for i, (bx, by) in enumerate(dl):
        ref = torch.from_numpy(x64[order[i]].transpose(0, 3, 1, 2).copy()).float()
        assert np.array_equal(bx.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32)), i
        assert np.array_equal(dl.last_index_host, order[i]) and np.array_equal(by.cpu().numpy(), ys[order[i]])
        assert np.array_equal(by.host, ys[order[i]]) and np.array_equal(dl.last_y_host, ys[order[i]])
        seen += 1
    assert seen == len(order) == n // bs and torch.equal(torch.rand(3), after_ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the network against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
TRAIN_CASES = [
    # agent, data, head, n, BatchNorm groups
    ("ER", "openloris", None, 1, 1),
    ("ER", "openloris", None, 3, 1),
    ("ER", "openloris", None, 10, 1),
    ("ER", "openloris", None, 20, 2),
    ("ER", "core50", None, 2, 1),
    ("ER", "core50", None, 6, 2),
    ("SCR", "openloris", "mlp", 8, 2),     # the SCR `mlp` pass at 50 x 50
]


@pytest.mark.parametrize("agent,data,head,n,groups", TRAIN_CASES)
def test_train_forward_backward_vs_oracle(cuda, lib, agent, data, head, n, groups):
    """tests/test_gpu_net.py::test_train_forward_backward_vs_oracle at the new shapes: raw conv outputs per layer (one group), the output,
    the loss, every parameter gradient, the running statistics and num_batches_tracked, with that test's tolerances and allowance."""
    hw = HW[data]
    case = "%s %s n=%d g=%d" % (agent, data, n, groups)
    m, sd = TN.build(agent, data, head or "mlp", cuda=cuda, max_batch=max(8, n))
    m._ensure_bound()
    assert m.feature_dim == (2560 if data == "core50" else 160)
    pre = "encoder." if head is not None else ""
    rng = np.random.default_rng(n)
    x = rng.random((n, 3, hw, hw)).astype(np.float32)
    y = rng.integers(0, 10, n).astype(np.int64)
    xt = torch.from_numpy(x)
    per = n // groups
    m.train()
    xd = torch.from_numpy(x).to(cuda)
    out = m.forward(xd) if groups == 1 else m.forward_views([xd[g * per:(g + 1) * per] for g in range(groups)])
    torch.cuda.synchronize()
    st = O.clone_state(sd)
    net = O.OracleNet(st, head=head, training=True)
    net.rec = {}
    probe = O.OracleNet(O.clone_state(sd, requires_grad=False), head=head, training=True)
    probe.pre_act = {}
    with torch.no_grad():
        probe.forward(xt[:per])
    shapes = {k: (n,) + tuple(v.shape[1:]) for k, v in probe.pre_act.items()}
    masks = TN.engine_masks(m, shapes, pre)
    outs, n_mis, n_tot, worst_amb = [], 0, 0, 0.0
    for g in range(groups):
        net.mask_override = {k: v[g * per:(g + 1) * per] for k, v in masks.items()}
        net.pre_act = {}
        outs.append(net.forward(xt[g * per:(g + 1) * per]))
        for k, pa in net.pre_act.items():
            mis = (pa > 0).float() != net.mask_override[k]
            n_mis += int(mis.sum())
            n_tot += pa.numel()
            if mis.any():
                worst_amb = max(worst_amb, float(pa[mis].abs().max() / pa.abs().max()))
    o_ref = torch.cat(outs, 0)
    print("relu pattern mismatches: %d of %d, worst |pre-activation| / max = %.2e" % (n_mis, n_tot, worst_amb))
    record(case, "relu mismatches", n_mis, 5 + 2e-5 * n_tot)
    record(case, "worst ambiguous", worst_amb, 1e-5)
    assert n_mis <= 5 + 2e-5 * n_tot and worst_amb < 1e-5, "activation patterns differ beyond fp32 round-off"
    if groups == 1:
        rows = TN.layer_report(m, net.rec, n)
        print("\n".join("%-40s %.3e" % r for r in rows))
        record(case, "raw conv outputs", max(r[1] for r in rows), 1e-4)
        assert max(r[1] for r in rows) < 1e-4, "raw conv outputs diverge: %s" % (max(rows, key=lambda r: r[1]),)
    err_out = float(np.abs(out.detach().cpu().numpy() - o_ref.detach().numpy()).max())
    print("out err", err_out)
    record(case, "output", err_out, 1e-4)
    assert err_out < 1e-4
    w = torch.linspace(-1, 1, o_ref.numel()).view_as(o_ref)
    if head is None:
        from ocl_amd.loss import cross_entropy_mean
        loss_ref = torch.nn.functional.cross_entropy(o_ref, torch.from_numpy(y))
        loss = cross_entropy_mean(out, torch.from_numpy(y).to(cuda))
    else:
        loss_ref = (o_ref * w).sum()
        loss = (out * w.to(cuda)).sum()
    lim = 1e-4 * max(1.0, abs(float(loss_ref.detach())))
    record(case, "loss", abs(float(loss.detach()) - float(loss_ref.detach())), lim)
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < lim
    loss_ref.backward()
    loss.backward()
    torch.cuda.synchronize()
    worst, rows = 0.0, []
    for k, p in m.named_parameters():
        gref = st[k].grad
        if gref is None:
            assert float(p.grad.abs().max()) == 0.0, "%s should have a zero gradient" % k
            continue
        e = np.abs(p.grad.cpu().numpy() - gref.numpy()).max() / (1e-12 + float(gref.abs().max()))
        rows.append((k, e, float(gref.abs().max())))
        worst = max(worst, e)
    print("\n".join("%-44s rel %.3e  max|g| %.3e" % r for r in rows))
    record(case, "parameter gradients", worst, 2e-4)
    assert worst < 2e-4, max(rows, key=lambda r: r[1])
    sd_new = m.state_dict()
    worst_rs = 0.0
    for k in sd_new:
        if k.endswith("running_mean") or k.endswith("running_var"):
            e = TN.relmax(sd_new[k].cpu().numpy(), st[k].numpy())
            worst_rs = max(worst_rs, e)
            assert e < 1e-4, k
        if k.endswith("num_batches_tracked"):
            assert int(sd_new[k]) == int(st[k]) == groups
    record(case, "running statistics", worst_rs, 1e-4)


@pytest.mark.parametrize("agent,data,head,n", [("ER", "openloris", None, 33), ("ER", "core50", None, 5), ("SCR", "openloris", "mlp", 9)])
def test_eval_forward_features_vs_oracle(cuda, lib, agent, data, head, n):
    """Eval-mode features and outputs: at core50 the 4 x 4 x 160 pooled map in the reference's `view` order (channel, row, column: 2560
    wide), at openloris the one 4 x 4 window avg_pool2d(4) keeps of the 7 x 7 map; n above max_batch is chunked."""
    hw = HW[data]
    m, sd = TN.build(agent, data, head or "mlp", cuda=cuda, max_batch=16 if data == "openloris" else 4)
    rng = np.random.default_rng(2)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.from_numpy(rng.standard_normal(sd[k].shape).astype(np.float32) * 0.1)
        if k.endswith("running_var"):
            sd[k] = torch.from_numpy((0.5 + rng.random(sd[k].shape)).astype(np.float32))
    m.load_state_dict(sd)
    x = rng.random((n, 3, hw, hw)).astype(np.float32)
    net = O.OracleNet(O.clone_state(sd, requires_grad=False), head=head, training=False)
    with torch.no_grad():
        f_ref = net.features(torch.from_numpy(x)).numpy()
        o_ref = net.forward(torch.from_numpy(x)).numpy()
    m.eval()
    mb = m._engine_desc().max_batch
    with torch.no_grad():
        f = m.features_batched(torch.from_numpy(x).to(cuda)).cpu().numpy()
        o = torch.cat([m.forward(torch.from_numpy(x[i:i + mb]).to(cuda)) for i in range(0, n, mb)]).cpu().numpy()
    case = "eval %s %s n=%d" % (agent, data, n)
    assert f.shape == f_ref.shape == (n, 2560 if data == "core50" else 160)
    record(case, "features", TN.relmax(f, f_ref), 1e-4)
    record(case, "output", float(np.abs(o - o_ref).max()), 1e-4)
    assert TN.relmax(f, f_ref) < 1e-4 and np.abs(o - o_ref).max() < 1e-4
    sd2 = m.state_dict()
    for k in sd:
        if "running" in k or "num_batches" in k:
            assert torch.equal(sd2[k].cpu(), sd[k]), "eval forward must not touch BatchNorm buffers"


def test_scr_core50_is_refused_at_bind_time_with_the_shape_message(cuda):
    """The reference's SupConResNet for core50 has a 160-wide head over 2560 features and fails at its first forward; here the bind-time
    shape check names the first tensor that does not fit."""
    m, _ = TN.build("SCR", "core50", "mlp", cuda=cuda, max_batch=2)
    with pytest.raises(RuntimeError, match=r"parameter head\.0\.weight: module shape \(160, 160\), engine shape \(2560, 2560\)"):
        m.forward(torch.zeros(2, 3, 128, 128, device=cuda))


def test_default_max_batch_holds_the_default_test_batch_at_core50(cuda):
    """No model.max_batch: one eval forward of 128 images of 128 x 128 (the default --test_batch) fits the engine."""
    from types import SimpleNamespace
    from ocl_amd.setup_elements import setup_architecture
    torch.manual_seed(11)
    m = setup_architecture(SimpleNamespace(agent="ER", data="core50", head="mlp")).cuda()
    m.n_slots = 1
    m.eval()
    x = torch.rand(128, 3, 128, 128, device=cuda)
    with torch.no_grad():
        out = m.forward(x)
        again = m.forward(x[:4])
    assert m._desc.max_batch == 128 and out.shape == (128, 50) and bool(torch.isfinite(out).all())
    assert float((again - out[:4]).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------------
# layer forms and lattices
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def new_entries(monkeypatch):
    """The cases of tests/test_gpu_layers.py look their layer up through find_entry: point it at datasets_cases.NEW_FORMS."""
    monkeypatch.setattr(TL, "find_entry", DC.find_entry)


@pytest.mark.parametrize("key,det", [(k, 0) for k in DC.EXACT_CONV_KEYS] + [(k, 1) for k in DC.EXACT_CONV_KEYS if k.endswith("/stats") or k.endswith("/bnb")])
def test_new_conv_form_is_exact(lib, new_entries, key, det):
    lib.ocl_set_deterministic(det)
    try:
        TL._conv_form_is_exact(lib, key, det)
    finally:
        lib.ocl_set_deterministic(0)


@pytest.mark.parametrize("key", DC.WGRAD_KEYS)
def test_new_wgrad_form_is_exact(lib, new_entries, key):
    TL.test_wgrad_form_is_exact(lib, key)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("key", DC.XF_KEYS)
def test_new_input_transform_form_against_float64_batchnorm(lib, new_entries, key, det):
    TL.test_input_transform_against_float64_batchnorm(lib, key, det)


@pytest.mark.parametrize("n,groups", [(1, 1), (3, 1), (10, 2)])
@pytest.mark.parametrize("cin,cout,k,stride,hw", DC.LATTICE_SHAPES)
def test_lattice_layer_shapes_exact(lib, cin, cout, k, stride, hw, n, groups):
    """Forward, data gradient (merged and per-phase launches) and weight gradient of every layer shape of the new lattices, integer-exact
    (small-integer operands: every partial sum is exact in fp32, so the result is bit-equal to float64 whatever the tiling)."""
    from ocl_amd import ffi
    if hw == 128 and n == 10:
        n, groups = 4, 2      # (128 x 128: four images are 65 536 pixels, already past every threshold the 10-image pass crosses at 50 x 50)
    g = torch.Generator().manual_seed(zlib.crc32(repr((cin, cout, k, stride, hw, n)).encode()) % 10007)
    d = TL._desc(cin, cout, k, stride, hw, n, groups, 0)
    cinT, ho, wo, _ = TL.shape_of(d)
    assert (ho, wo) == (((hw + 1) // 2,) * 2 if stride == 2 else (hw, hw))
    w = TL.ints((cout, cin, k, k), g)
    x = TL.ints((n, hw, hw, cinT), g)
    if cin == 3:
        x[..., 3] = 0
    got, _, _ = TL.run_conv(lib, d, x, w)
    TL.assert_exact(got, TL.ref_fwd(x, w, d), "fwd %r" % ((cin, cout, k, stride, hw),))
    dy = TL.ints((n, ho, wo, cout), g)
    if cin != 3:
        for merge in (1, 0):
            dd = TL._desc(cin, cout, k, stride, hw, n, groups, 1, merge=merge)
            got, _, _ = TL.run_conv(lib, dd, dy, w)
            ref = TL.ref_dgrad(dy, w, dd)
            if k == 1 and stride == 2:     # only the even pixels are written; run_conv starts the others at 0
                full, ref = ref, torch.zeros_like(ref)
                ref[:, ::2, ::2] = full[:, ::2, ::2]
            TL.assert_exact(got, ref, "dgrad merge=%d %r" % (merge, (cin, cout, k, stride, hw)))
    wd = ffi.TestWgradDesc(cin=cin, cout=cout, k=k, stride=stride, hin=hw, win=hw, n=n)
    got, _ = TL.run_wgrad(lib, [wd], [x], [dy])
    TL.assert_exact(got[0], TL.ref_wgrad(x, dy, wd), "wgrad %r" % ((cin, cout, k, stride, hw),))


# ---------------------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------------------
class _OracleEr(object):
    """The ER loop of oracle.OracleAgent.train_learner over O.er_step for a task that is float already (the caller applies the
    reference's transform), at any input size: O.OracleAgent itself knows the 32 / 84 datasets only."""

    def __init__(self, state_dict, mem_size, hw, eps_mem_batch, batch):
        self.state = O.clone_state(state_dict)
        self.names = [k for k in self.state if self.state[k].requires_grad]
        self.buf = O.OracleBuffer(mem_size, (3, hw, hw))
        self.p = dict(eps_mem_batch=eps_mem_batch, lr=0.1)
        self.batch = batch
        self.log = []

    def train_learner(self, xs, ys):
        loader = torch.utils.data.DataLoader(O._Idx(len(ys)), batch_size=self.batch, shuffle=True, drop_last=True)
        for idx in loader:
            self.log.append(O.er_step(self.state, self.names, self.buf, xs[idx], ys[idx], self.p, "random"))

    def state_dict(self):
        return O.OrderedDict((k, v.detach()) for k, v in self.state.items())


def _noise_task(x_u8, factor, gen):
    """The reference's noise task (continuum/non_stationary.py): clip(x / 255 + f * N(0, 0.1), 0, 1), float64 HWC."""
    x = x_u8 / 255
    return np.clip(x + factor * gen.normal(loc=0.0, scale=0.1, size=x.shape), 0, 1)


def _er_cosim(cuda, data, batch, eps, n_steps, floats):
    hw = HW[data]
    cfg = dict(agent="ER", retrieve="random", update="random", data=data, mem_size=2 * batch, eps_mem_batch=eps, seed=0, tasks=[[0, 1]])
    params, model, agent = TS.build_agent(cfg, batch=batch)
    model.max_batch = 2 * max(batch, eps)
    from ocl_amd import debug
    oa = _OracleEr(model.state_dict(), cfg["mem_size"], hw, eps, batch)
    rng = np.random.default_rng(9000)
    ys_all = np.repeat(np.array([0, 1], dtype=np.int64), (n_steps * batch + 1) // 2)[:n_steps * batch]
    rng.shuffle(ys_all)
    x_u8 = np.concatenate([class_images(int(c), 1, (hw, hw), rng) for c in ys_all], 0)
    x_task = _noise_task(x_u8, 0.4, np.random.default_rng(77)) if floats else x_u8
    assert x_task.dtype == (np.float64 if floats else np.uint8)
    seed_all(1000)
    worst = 0.0
    case = "er step %s%s %d+%d" % (data, " float64 task" if floats else "", batch, eps)
    for it in range(n_steps):
        x, y = x_task[it * batch:(it + 1) * batch], ys_all[it * batch:(it + 1) * batch]
        # the reference's transform on the host: ToTensor scales uint8 by 1 / 255 and only transposes a float array; then .float()
        xs = O.to_tensor(x) if not floats else torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).float()
        model.load_state_dict(oa.state_dict())
        w0 = TS._flat(oa.state, oa.names)
        st = TS._rng_get()
        oa.train_learner(xs, torch.from_numpy(y))
        st_o = TS._rng_get()
        TS._rng_set(st)
        debug.LOG = []
        try:
            agent.train_learner(x, y)
            ev = list(debug.LOG)
        finally:
            debug.LOG = None
        ol = oa.log[-1]
        assert TS._rng_equal(st_o, TS._rng_get()), "host RNG streams diverged at iteration %d" % it
        # (losses: the bound of tests/test_gpu_net.py, 1e-4 * max(1, |loss|) -- at lr 0.1 a third step's loss can be far above 1)
        e_loss, lim = abs([e["loss"] for t, e in ev if t == "er_loss"][0] - ol["loss"]), 1e-4 * max(1.0, abs(ol["loss"]))
        record(case, "loss (step %d)" % it, e_loss, lim)
        assert e_loss < lim
        assert np.array_equal([e["indices"] for t, e in ev if t == "random_retrieve"][0], ol["idx"])
        if "loss_mem" in ol:
            e_mem, lim = abs([e["loss"] for t, e in ev if t == "er_loss_mem"][0] - ol["loss_mem"]), 1e-4 * max(1.0, abs(ol["loss_mem"]))
            record(case, "memory loss (step %d)" % it, e_mem, lim)
            assert e_mem < lim
        assert [list(e["slots"]) for t, e in ev if t == "reservoir"][0] == list(ol["slots"])
        b = agent.buffer
        assert np.array_equal(b.buffer_label.cpu().numpy(), oa.buf.label.numpy()) and np.array_equal(b.label_host, oa.buf.label.numpy())
        assert torch.equal(b.buffer_img.cpu(), oa.buf.img), "memory rows differ (slot indices or image bits)"
        assert [b.current_index, b.n_seen_so_far] == [oa.buf.current_index, oa.buf.n_seen_so_far]
        w1_o, w1_m = TS._flat(oa.state, oa.names), model.flat_params().double().cpu().numpy()
        upd = float(np.linalg.norm((w1_m - w0) - (w1_o - w0)) / (1e-30 + np.linalg.norm(w1_o - w0)))
        print(case, "it", it, "update err", upd)
        worst = max(worst, upd)
    record(case, "SGD update (worst step)", worst, 1e-2)
    assert worst < 1e-2
    assert any("loss_mem" in l for l in oa.log), "no step replayed memory"
    assert oa.buf.n_seen_so_far > oa.buf.mem_size == oa.buf.current_index, "the reservoir never went past the fill"


@pytest.mark.parametrize("data,batch,eps,floats", [("openloris", 10, 10, False), ("core50", 4, 4, False), ("cifar10", 10, 10, True)])
def test_er_steps_teacher_forced_vs_oracle(cuda, lib, data, batch, eps, floats):
    """ER + random retrieval + reservoir, 3 steps from the oracle's state each, as tests/test_gpu_steps.py::test_cosim_er_random compares them:
    both losses within 1e-4 * max(1, |loss|), retrieved indices, reservoir slots, memory rows, labels, counters and host RNG state exact, the SGD update
    within 1e-2 norm-wise.  openloris and core50 on a uint8 task; cifar10 shape on a float64 task (a new-instance stream: the noise
    transform restated with a fixed generator), which the loader only transposes."""
    _er_cosim(cuda, data, batch, eps, 3, floats)


def test_ncm_evaluate_with_2560_wide_features(cuda, lib):
    """ncm_trick on a core50-shaped model: class means over 40 memory rows, two test loaders of 16.  Against the oracle's features of the
    same rows: every prediction the oracle makes with a margin is the engine's; the class means' width is 2560."""
    from ocl_amd import debug
    from ocl_amd.data import setup_test_loader
    trick = dict(TS.TRICK, ncm_trick=True)
    cfg = dict(agent="ER", retrieve="random", update="random", data="core50", mem_size=40, eps_mem_batch=4, seed=3, tasks=[[0, 1, 2, 3]])
    params, model, agent = TS.build_agent(cfg, batch=4, test_batch=16, trick=trick)
    model.max_batch = 16
    rng = np.random.default_rng(12)
    classes = [0, 1, 2, 3]
    ys = np.array(classes * 10, dtype=np.int64)
    xs = O.to_tensor(np.concatenate([class_images(int(c), 1, (128, 128), rng) for c in ys], 0))
    agent.buffer.update(xs.to(cuda), torch.from_numpy(ys).to(cuda), y_host=ys)
    assert agent.buffer.current_index == 40
    agent.old_labels = list(classes)
    tests = []
    for t in range(2):
        ty = np.array(classes * 4, dtype=np.int64)
        tests.append((np.concatenate([class_images(int(c), 1, (128, 128), rng) for c in ty], 0), ty))
    loaders = setup_test_loader(tests, params)
    debug.LOG = []
    try:
        acc = agent.evaluate(loaders)
        ev = [e for t, e in debug.LOG if t == "evaluate"]
    finally:
        debug.LOG = None
    assert model.feature_dim == 2560 and len(ev) == 2
    net = O.OracleNet(O.clone_state(model.state_dict(), requires_grad=False), head=None, training=False)
    with torch.no_grad():
        means = O.ncm_means(O.deep_features(net, xs), torch.from_numpy(ys), classes)
        assert means.shape == (4, 2560)
        checked = 0
        for t, (tx, ty) in enumerate(tests):
            f = net.features(O.to_tensor(tx)[torch.from_numpy(ev[t]["index"])])
            f = f / f.norm(dim=1, keepdim=True)
            d = ((f[:, None, :] - means[None, :, :]) ** 2).sum(-1)
            top2 = d.sort(1)[0][:, :2]
            clear = (top2[:, 1] - top2[:, 0]) > 1e-4 * top2[:, 1]
            pred = torch.tensor(classes)[d.min(1)[1]]
            assert sorted(ev[t]["index"].tolist()) == list(range(16))
            assert np.array_equal(ev[t]["pred"][clear.numpy()], pred.numpy()[clear.numpy()]), t
            checked += int(clear.sum())
            assert abs(acc[t] - float((torch.from_numpy(ev[t]["pred"]) == torch.from_numpy(ty[ev[t]["index"]])).float().mean())) < 1e-12
    assert checked >= 24, "too few predictions with a margin to compare (%d of 32)" % checked


def test_aser_retrieval_at_openloris_shape(cuda, lib):
    """One ASER retrieval (aser_type neg_sv: candidates scored against the incoming batch) over a 50 x 50 memory: the kernel's neighbour
    order is a valid order of the ORACLE's feature distances, the scores are the oracle's Shapley values under that order (1e-5), and the
    rows returned are a valid top-10 -- tests/test_gpu_steps.py::test_cosim_aser_tie_aware's checks of a retrieval."""
    from ocl_amd import debug
    cfg = dict(agent="ER", retrieve="ASER", update="random", data="openloris", mem_size=120, eps_mem_batch=10, seed=5, tasks=[list(range(12))],
               k=3, n_smp_cls=3.0, aser_type="neg_sv")
    params, model, agent = TS.build_agent(cfg)
    model.max_batch = 64
    rng = np.random.default_rng(21)
    ys = np.repeat(np.arange(12, dtype=np.int64), 10)
    xs = O.to_tensor(np.concatenate([class_images(int(c), 1, (50, 50), rng) for c in ys], 0))
    b = agent.buffer
    b.update(xs.to(cuda), torch.from_numpy(ys).to(cuda), y_host=ys)
    assert b.current_index == 120
    b.n_seen_so_far = 500      # the memory has cycled: retrieval by Shapley value
    cy = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int64)
    cx = O.to_tensor(np.concatenate([class_images(int(c), 1, (50, 50), rng) for c in cy], 0))
    debug.LOG = []
    try:
        mem_x, mem_y = b.retrieve(x=cx.to(cuda), y=torch.from_numpy(cy).to(cuda))
        r = [e for t, e in debug.LOG if t == "aser_retrieve"][0]
    finally:
        debug.LOG = None
    cand = r["cand_ind"]
    assert len(cand) == 36 == len(set(cand.tolist())) and mem_x.shape == (10, 3, 50, 50)
    assert np.array_equal(np.bincount(ys[cand], minlength=12), np.full(12, 3)), "candidates are not class-balanced"
    net = O.OracleNet(O.clone_state(model.state_dict(), requires_grad=False), head=None, training=False)
    f_e, f_c = O.deep_features(net, cx).numpy(), O.deep_features(net, xs[torch.from_numpy(cand)]).numpy()
    sv_adv = TS._sv_given_order((f_e, cy, f_c, ys[cand]), r["order_adv"], 3)
    score = O.aser_score(sv_adv, None, "neg_sv")
    record("aser retrieve openloris", "scores", float(np.abs(r["sv"] - score).max()), 1e-5)
    assert np.abs(r["sv"] - score).max() < 1e-5
    thr = np.sort(score)[::-1][9]
    pos = {c: j for j, c in enumerate(cand.tolist())}
    assert len(r["ret"]) == 10 and min(score[pos[c]] for c in r["ret"].tolist()) >= thr - 1e-5, "not a valid top-10"
    assert torch.equal(mem_x.cpu(), xs[torch.from_numpy(r["ret"])]) and np.array_equal(mem_y.cpu().numpy(), ys[r["ret"]])
