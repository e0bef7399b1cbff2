"""CPU: --data core50 / openloris and float task arrays (new-instance streams), host side.

* the engine's parameter layout at 128x128 / 50 classes and 50x50 / 69 classes carries the names and shapes of the reference's
  named_parameters() (tests/golden/datasets.npz, recorded from the reference by scripts/make_datasets_golden.py);
* setup_architecture builds modules whose state_dict keys and seeded initial weights equal the reference's (same seed, same draws);
* SCR + core50 is what the reference builds (a 160-wide head over 2560 features), which the engine's layout does not accept;
* DeviceLoader takes uint8, float32 and float64 and nothing else; the index loader's order and the torch-RNG state after an epoch do not
  depend on the array's dtype.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi
from conftest import gold
from oracle.synth import digest_state

SEED = 11   # scripts/make_datasets_golden.py


def _layout(desc):
    L = ffi.lib()
    h = ffi.vp(0)
    ffi.check(L.ocl_net_create(C.byref(desc), C.byref(h)), "create")
    nb, off, nd, sh = C.create_string_buffer(64), ffi.i64(0), ffi.i32(0), (ffi.i64 * 4)()
    out = []
    for i in range(L.ocl_net_num_tensors(h)):
        ffi.check(L.ocl_net_tensor_info(h, i, nb, C.byref(off), C.byref(nd), sh))
        out.append((nb.value.decode(), off.value, tuple(sh[k] for k in range(nd.value))))
    info = dict(n=L.ocl_net_param_count(h), fd=L.ocl_net_feature_dim(h), od=L.ocl_net_out_dim(h), nbn=L.ocl_net_num_bn(h),
                ws=L.ocl_net_workspace_bytes(h))
    L.ocl_net_destroy(h)
    return out, info


def _ref_params(g, name):
    return [(str(k), tuple(int(v) for v in s if v >= 0)) for k, s, p in zip(g[name + "_keys"], g[name + "_shapes"], g[name + "_is_param"]) if p]


def _build(agent, data, head="mlp"):
    from ocl_amd.setup_elements import setup_architecture
    torch.manual_seed(SEED)
    return setup_architecture(SimpleNamespace(agent=agent, data=data, head=head))


@pytest.mark.parametrize("name,desc,n_params,fd,od", [
    ("er_core50", (128, 128, 20, 50, 0, 0, 4, 2), 1093140 + 2560 * 50 + 50, 2560, 50),
    ("er_openloris", (50, 50, 20, 69, 0, 0, 4, 2), 1093140 + 160 * 69 + 69, 160, 69),
    ("scr_openloris", (50, 50, 20, 100, 1, 128, 4, 2), None, 160, 128),
])
def test_engine_layout_equals_reference_named_parameters(name, desc, n_params, fd, od):
    lay, info = _layout(ffi.NetDesc(*desc))
    ref = _ref_params(gold("datasets"), name)
    assert [(k, s) for k, _, s in lay] == ref
    off = 0
    for (k, o, s) in lay:      # flat offsets are the cumulative sizes: the layout of get_grad_vector
        assert o == off, k
        off += int(np.prod(s))
    assert info["n"] == off and info["fd"] == fd and info["od"] == od and info["nbn"] == 20
    if n_params is not None:
        assert info["n"] == n_params
        assert info["n"] == {"er_core50": 1221190, "er_openloris": 1104249}[name]


@pytest.mark.parametrize("name,agent,data", [("er_core50", "ER", "core50"), ("er_openloris", "ER", "openloris"),
                                             ("scr_openloris", "SCR", "openloris"), ("scr_core50", "SCR", "core50")])
def test_state_dict_and_seeded_weights_equal_the_reference(name, agent, data):
    g = gold("datasets")
    m = _build(agent, data)
    after = torch.rand(4).numpy()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[name + "_keys"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(int(x) for x in s if x >= 0) for s in g[name + "_shapes"]]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in _ref_params(g, name)]
    assert np.array_equal(digest_state(sd), g[name + "_digest"]), "seeded initialisation differs from the reference's"
    assert np.array_equal(after, g[name + "_draw_after"]), "the construction consumed another number of torch-RNG draws"


def test_models_carry_the_engine_descriptions_of_the_issue():
    """in_hw, classifier width, default max_batch (128 above 84x84: the default --test_batch fits one forward; model.max_batch
    overrides) -- and the engine accepts the descriptions (workspace size > 0)."""
    for data, hw, ncls, fd, mb in (("core50", 128, 50, 2560, 128), ("openloris", 50, 69, 160, 256), ("mini_imagenet", 84, 100, 640, 256),
                                   ("cifar10", 32, 10, 160, 512)):
        m = _build("ER", data)
        d = m._engine_desc()
        assert (d.in_h, d.in_w, d.nf, d.n_classes, d.head, d.max_batch, d.n_slots) == (hw, hw, 20, ncls, 0, mb, 3)
        assert tuple(m.linear.weight.shape) == (ncls, fd)
    m = _build("ER", "core50")
    m.max_batch = 8
    assert m._engine_desc().max_batch == 8
    lay, info = _layout(m._engine_desc())
    assert info["ws"] > 0 and info["fd"] == 2560
    s = _build("SCR", "core50")
    assert s._engine_desc().max_batch == 128 and _build("SCR", "openloris")._engine_desc().max_batch == 256


def test_scr_core50_is_the_reference_model_and_the_engine_layout_refuses_it():
    """The reference builds SupConResNet(head=...) with dim_in = 160 over an encoder that yields 2560 features, and fails at its first
    forward.  setup_architecture returns the same module (golden shapes above); the engine's layout for that description has a 2560-wide
    head, so the shape check at bind time (resnet._ensure_bound) refuses the pair -- restated here on the layout, bound on the GPU in
    tests/test_gpu_datasets.py."""
    m = _build("SCR", "core50")
    assert tuple(m.head[0].weight.shape) == (160, 160) and tuple(m.head[2].weight.shape) == (128, 160)
    lay, info = _layout(m._engine_desc())
    eng = {k: s for k, _, s in lay}
    assert info["fd"] == 2560 and eng["head.0.weight"] == (2560, 2560) and eng["head.2.weight"] == (128, 2560)
    named = dict(m.named_parameters())
    bad = [k for k, _, s in lay if tuple(named[k].shape) != s]
    assert bad == ["head.0.weight", "head.0.bias", "head.2.weight"]
    # openloris: 160 features, the pair fits
    m = _build("SCR", "openloris")
    lay, _ = _layout(m._engine_desc())
    named = dict(m.named_parameters())
    assert all(tuple(named[k].shape) == s for k, _, s in lay)


def test_unknown_dataset_is_a_key_error_as_in_the_reference():
    with pytest.raises(KeyError):
        _build("ER", "imagenet")


# ---- the loader ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [lambda a: a, torch.from_numpy], ids=["numpy", "torch"])
def test_device_loader_refuses_other_dtypes_and_names_the_three(make):
    from ocl_amd.data import DeviceLoader
    x = np.zeros((4, 5, 7, 3), dtype=np.int16)
    with pytest.raises(TypeError) as e:
        DeviceLoader(make(x), np.arange(4), 2, shuffle=False, device=torch.device("cpu"))
    assert all(w in str(e.value) for w in ("uint8", "float32", "float64"))
    with pytest.raises(TypeError):
        DeviceLoader(make(np.zeros((4, 5, 7), dtype=np.float32)), np.arange(4), 2, shuffle=False, device=torch.device("cpu"))


def _epoch(loader_x, n, bs, monkeypatch):
    """One epoch of a DeviceLoader whose three device ops are replaced by their torch-CPU statements (the kernels themselves:
    tests/test_gpu_datasets.py): the batches, the host mirrors, and a torch-RNG draw afterwards."""
    from ocl_amd import data, ops
    monkeypatch.setattr(ops, "gather_u8_images", lambda x, idx: x[idx].permute(0, 3, 1, 2).contiguous().float().div(255))
    monkeypatch.setattr(ops, "gather_f32_images", lambda x, idx: x[idx].permute(0, 3, 1, 2).contiguous())
    monkeypatch.setattr(ops, "gather_rows", lambda src, idx: src[idx])
    ys = np.arange(n) % 7
    torch.manual_seed(5)
    dl = data.DeviceLoader(loader_x, ys, bs, shuffle=True, drop_last=True, device=torch.device("cpu"))
    rows = []
    for bx, by in dl:
        rows.append((bx.clone(), by.clone(), dl.last_index_host.copy(), dl.last_y_host.copy(), by.host.copy()))
    return dl, rows, torch.rand(3)


def test_float_task_keeps_the_index_loaders_order_and_rng_draws(monkeypatch):
    n, bs = 53, 10
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (n, 5, 7, 3)).astype(np.uint8)
    f64 = u8.astype(np.float64) / 255
    _, ru, after_u = _epoch(u8, n, bs, monkeypatch)
    for x in (f64, f64.astype(np.float32), torch.from_numpy(f64), torch.from_numpy(f64.astype(np.float32))):
        dl, rf, after_f = _epoch(x, n, bs, monkeypatch)
        assert dl.x.dtype == torch.float32 and len(dl) == n // bs == len(rf) == len(ru)
        assert torch.equal(after_f, after_u), "another number of torch-RNG draws than the uint8 path"
        for (bxu, byu, iu, yu, hu), (bxf, byf, i_f, yf, hf) in zip(ru, rf):
            assert np.array_equal(iu, i_f) and np.array_equal(yu, yf) and np.array_equal(hu, hf) and torch.equal(byu, byf)
            # the contract: dataset_transform.__getitem__ on a non-uint8 array = transpose + .float()
            ref = torch.from_numpy(f64[i_f].transpose(0, 3, 1, 2).copy()).float()
            assert torch.equal(bxf, ref)
    # and the reference's own loader over the same length draws the same order
    from torch.utils import data as tdata
    torch.manual_seed(5)
    ref_order = [b[1].numpy() for b in tdata.DataLoader(tdata.TensorDataset(torch.zeros(n, 1), torch.arange(n)), batch_size=bs, shuffle=True,
                                                        drop_last=True)]
    assert all(np.array_equal(a, r[2]) for a, r in zip(ref_order, ru)) and torch.equal(torch.rand(3), after_u)


def test_float64_is_rounded_once_to_nearest_even_on_the_host():
    """astype(np.float32) of the task == the reference's per-item .float(): ties to even, -0.0, a denormal, 1.0 and a NaN included."""
    from ocl_amd.data import DeviceLoader
    tie_up = 1.0 + 3 * 2.0 ** -24      # halfway between 1 + 2^-23 and 1 + 2^-22: rounds to the even neighbour 1 + 2^-22
    tie_down = 1.0 + 2.0 ** -24        # halfway between 1 and 1 + 2^-23: rounds to 1
    vals = np.array([tie_up, tie_down, -0.0, 1e-40, 1.0, np.nan, 0.1, 254 / 255], dtype=np.float64)
    x = np.resize(vals, (2, 2, 2, 3))
    dl = DeviceLoader(x, np.arange(2), 2, shuffle=False, device=torch.device("cpu"))
    ref = torch.from_numpy(x).float()
    assert dl.x.dtype == torch.float32 and np.array_equal(dl.x.numpy().view(np.uint32), ref.numpy().view(np.uint32))
    got = dl.x.numpy().reshape(-1)[:5]
    assert got[0] == np.float32(1 + 2.0 ** -22) and got[1] == np.float32(1.0) and np.signbit(got[2]) and got[2] == 0 and 0 < got[3] < 1.2e-38


def test_the_new_entry_point_is_exported_and_declared():
    import os
    from conftest import ROOT
    assert ffi.SIGNATURES["ocl_gather_f32_hwc_to_f32_chw"] == ffi.SIGNATURES["ocl_gather_u8_hwc_to_f32_chw"]
    assert hasattr(ffi.lib(), "ocl_gather_f32_hwc_to_f32_chw")
    assert "loader.hip" in open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", "loader.hip")).read()
    assert "gather_f32_hwc_f32_chw_kernel" in src
    # argument checks need no GPU: they come before any launch
    L = ffi.lib()
    assert L.ocl_gather_f32_hwc_to_f32_chw(None, None, 0, 5, 7, 3, None, None) == 0          # n = 0: nothing to do
    assert L.ocl_gather_f32_hwc_to_f32_chw(None, None, 1, 5, 7, 3, None, None) < 0
    assert b"null pointer" in L.ocl_last_error()
    assert L.ocl_gather_f32_hwc_to_f32_chw(None, None, 1, 0, 7, 3, None, None) < 0 and b"bad shape" in L.ocl_last_error()
    assert L.ocl_gather_f32_hwc_to_f32_chw(ffi.vp(16), ffi.vp(16), 1, 5, 7, 3, ffi.vp(18), None) < 0 and b"4-byte aligned" in L.ocl_last_error()


# ---- the planner at the new sizes ---------------------------------------------------------------------------------------------------------

def test_every_form_of_the_new_sizes_has_a_single_layer_case():
    """ocl_test_net_forms over hw {50, 128} x n {1 .. 64} x groups {1, 2} x train {0, 1} (datasets_cases.pass_grid): a form key outside
    the 32 / 84 grid of tests/layer_forms.py has a single-layer case in datasets_cases.NEW_FORMS, at a pass / layer where the planner still
    gives it -- a later planner change cannot add an untested form at these sizes."""
    import datasets_cases as DC
    L = ffi.lib()
    forms = DC.new_forms(L)
    assert sorted(forms) == sorted(DC.NEW_FORMS), (sorted(set(forms) - set(DC.NEW_FORMS)), sorted(set(DC.NEW_FORMS) - set(forms)))
    for key in DC.NEW_FORMS:
        e = DC.find_entry(L, key)
        d = e.desc if e.dir < 2 else e.wdesc
        assert d.hin >= 4 and d.n == DC.NEW_FORMS[key][1]
    assert sorted(DC.EXACT_CONV_KEYS + DC.XF_KEYS + DC.WGRAD_KEYS) == sorted(DC.NEW_FORMS)
