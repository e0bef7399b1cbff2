"""CPU: the host side of the fused Adam optimiser (optim.FusedAdam, ocl_adam_step) and the float64 statement of its update rule.

`ref_adam` is one Adam step in float64 in the order of torch's _single_tensor_adam (amsgrad off, maximize off, L2 weight decay added to
the gradient); it is pinned here against torch.optim.Adam(foreach=False) in float64, and tests/test_gpu_adam.py judges the kernel
against it (together with `adam_bounds`, the first-order propagation of fp32 round-off through the same formula, and `make_grads`,
the gradients both files use)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ocl_amd  # noqa: F401
from ocl_amd import ffi

U = 2.0 ** -24      # half an fp32 ulp, relative
OCL_ERR_ARG = -1    # include/ocl_hip.h


def f32(x):
    """The value a Python float has once it has crossed the C-ABI as a `float` argument."""
    return float(np.float32(x))


def make_grads(rng, n, step):
    """Gradient magnitudes from 1e-7 to 1 (log-uniform), random signs; on every fourth step 30 % of them exactly zero."""
    g = np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-7.0, 0.0, n)
    if step % 4 == 0:
        g[rng.random(n) < 0.3] = 0.0
    return g.astype(np.float32)


def ref_adam(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, gs=1.0, skip=(0, 0)):
    """One step in float64.  p, g, m, v: arrays (any float dtype), step: this step's 1-based number; elements skip[0] .. skip[1] - 1
    keep p, m, v.  Returns the new p, m, v and the intermediates adam_bounds needs."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gp = wd * p + g * gs
    m1 = m + (1.0 - beta1) * (gp - m)
    v1 = beta2 * v + (1.0 - beta2) * gp * gp
    step_size = lr / (1.0 - beta1 ** step)
    bc2_sqrt = (1.0 - beta2 ** step) ** 0.5
    den = np.sqrt(v1) / bc2_sqrt + eps
    p1 = p - step_size * (m1 / den)
    keep = np.zeros(p.shape, dtype=bool)
    keep[skip[0]:skip[1]] = True
    p1, m1, v1 = np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)
    return SimpleNamespace(p=p1, m=m1, v=v1, p0=p, g=g, m0=m, v0=v, gp=gp, den=den, step_size=step_size, bc2_sqrt=bc2_sqrt, keep=keep,
                           beta1=beta1, beta2=beta2, wd=wd, gs=gs)


def adam_bounds(r):
    """(e_p, e_m, e_v): fp32 round-off of one step propagated to first order, one half-ulp (U = 2^-24) per operation; zero (exact
    equality) inside the skip range.  r: what ref_adam returned."""
    gp = np.abs(r.gp)
    e_g = U * (np.abs(r.g * r.gs) + np.abs(r.wd * r.p0))
    e_m = U * (np.abs(r.m0) + gp) + (1.0 - r.beta1) * e_g
    e_v = U * (r.beta2 * np.abs(r.v0) + (1.0 - r.beta2) * gp * gp) + 2.0 * (1.0 - r.beta2) * gp * e_g
    sq = np.sqrt(r.v) * r.bc2_sqrt
    e_den = U * r.den + np.divide(e_v, 2.0 * sq, out=np.zeros_like(sq), where=sq > 0)
    delta = np.abs(r.p - r.p0)
    e_p = U * (np.abs(r.p0) + 3.0 * delta) + (r.step_size / r.den) * e_m + delta * e_den / r.den
    z = np.zeros_like(e_p)
    return np.where(r.keep, z, e_p), np.where(r.keep, z, e_m), np.where(r.keep, z, e_v)


def worst_ratios(got_p, got_m, got_v, r):
    """max |got - ref| / bound for p, m, v (0 where both are zero, inf where a zero bound is exceeded)."""
    out = []
    for got, ref, e in zip((got_p, got_m, got_v), (r.p, r.m, r.v), adam_bounds(r)):
        d = np.abs(np.asarray(got, dtype=np.float64) - ref)
        ratio = np.divide(d, e, out=np.where(d > 0, np.inf, 0.0), where=e > 0)
        out.append(float(ratio.max()))
    return out


# ---- factory and constructor -------------------------------------------------------------------------------------------------------

def test_setup_opt_adam_is_the_fused_optimiser():
    from ocl_amd import optim
    from ocl_amd.resnet import Reduced_ResNet18
    from ocl_amd.setup_elements import setup_opt
    model = Reduced_ResNet18(10)
    opt = setup_opt('Adam', model, 1e-3, 0)
    assert type(opt) is optim.FusedAdam and opt.model is model
    assert len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-3, (0.9, 0.999), 1e-8, 0, False)
    assert len(g["params"]) == len(list(model.parameters())) == 62
    assert model._net is None, "constructing the optimiser must not bind the engine"
    assert opt.step_count == 0 and opt.exp_avg is None and opt.exp_avg_sq is None
    opt.zero_grad()
    assert opt.step() is None and opt.step_count == 0      # no backward since zero_grad(): nothing to step, nothing counted (and no device needed)
    with pytest.raises(RuntimeError):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(1))]))
    with pytest.raises(RuntimeError):
        optim.FusedAdam(torch.nn.Linear(3, 2), lr=1e-3)
    sd = opt.state_dict()
    assert sd["step"] == 0 and sd["exp_avg"] is None and sd["exp_avg_sq"] is None


def test_state_dict_round_trip_on_the_host():
    from ocl_amd import optim
    from ocl_amd.resnet import Reduced_ResNet18
    a, b = optim.FusedAdam(Reduced_ResNet18(10), lr=1e-3), optim.FusedAdam(Reduced_ResNet18(10), lr=5e-2, weight_decay=1e-4)
    n = sum(p.numel() for p in a.param_groups[0]["params"])
    a.step_count, a.exp_avg, a.exp_avg_sq = 7, torch.randn(n), torch.rand(n)
    b.load_state_dict(a.state_dict())
    assert b.step_count == 7 and torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    assert b.exp_avg.data_ptr() != a.exp_avg.data_ptr()
    assert b.param_groups[0]["lr"] == 1e-3 and b.param_groups[0]["weight_decay"] == 0.0
    with pytest.raises(RuntimeError):
        b.load_state_dict(dict(step=1, exp_avg=torch.zeros(3), exp_avg_sq=torch.zeros(3)))


# ---- C-ABI: argument checks run on the host, before any launch ------------------------------------------------------------------------

def _call(**over):
    buf = (C.c_float * 64)()
    a = (C.addressof(buf) + 15) // 16 * 16      # 16-byte aligned host address: never dereferenced, every case below is refused first
    kw = dict(params=a, grads=a + 16, exp_avg=a + 32, exp_avg_sq=a + 48, n=4, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, gs=1.0,
              step=1, skip_begin=0, skip_end=0)
    kw.update(over)
    rc = ffi.lib().ocl_adam_step(ffi.vp(kw["params"]), ffi.vp(kw["grads"]), ffi.vp(kw["exp_avg"]), ffi.vp(kw["exp_avg_sq"]), kw["n"], kw["lr"],
                                 kw["beta1"], kw["beta2"], kw["eps"], kw["wd"], kw["gs"], kw["step"], kw["skip_begin"], kw["skip_end"], ffi.vp(0))
    return rc, ffi.lib().ocl_last_error().decode()


def test_abi_signature_is_registered():
    assert "ocl_adam_step" in ffi.SIGNATURES
    res, args = ffi.SIGNATURES["ocl_adam_step"]
    assert res is C.c_int and len(args) == 15
    assert args[4] is ffi.i64 and args[5:11] == [ffi.f32] * 6 and args[11:14] == [ffi.i64] * 3


@pytest.mark.parametrize("over", [
    dict(params=0), dict(grads=0), dict(exp_avg=0), dict(exp_avg_sq=0),
    dict(n=0), dict(n=-4),
    dict(step=0), dict(step=-1),
    dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(eps=-1e-8),
    dict(skip_begin=2, skip_end=5), dict(skip_begin=3, skip_end=2), dict(skip_begin=-1, skip_end=2),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_abi_refuses_bad_arguments_without_a_device(over):
    rc, msg = _call(**over)
    assert rc == OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("adam:"), msg


def test_abi_refuses_a_misaligned_pointer_without_a_device():
    buf = (C.c_float * 64)()
    a = (C.addressof(buf) + 15) // 16 * 16
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        rc, msg = _call(**{name: a + 4})
        assert rc == OCL_ERR_ARG and "aligned" in msg, (name, rc, msg)


def test_abi_refuses_overlapping_arrays_without_a_device():
    """params, grads, exp_avg and exp_avg_sq are four disjoint arrays: an aliased pair would be read and written by different
    threads in no order."""
    buf = (C.c_float * 64)()
    a = (C.addressof(buf) + 15) // 16 * 16
    arrays = dict(params=a, grads=a + 256, exp_avg=a + 512, exp_avg_sq=a + 768)     # n = 16: 64 bytes each
    for over in (dict(exp_avg=a),                  # exp_avg on params
                 dict(exp_avg_sq=a + 256 - 16),    # exp_avg_sq ending inside grads
                 dict(grads=a + 48)):              # grads starting inside params
        rc, msg = _call(**dict(arrays, n=16, **over))
        assert rc == OCL_ERR_ARG and msg.startswith("adam:") and "overlap" in msg, (over, rc, msg)
    rc, msg = _call(**dict(arrays, n=16, step=0))                                   # the arrays themselves are accepted
    assert rc == OCL_ERR_ARG and "step" in msg, (rc, msg)


# ---- the float64 reference against torch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("gs", [1.0, 0.1])
def test_ref_adam_equals_torch_adam_in_float64(wd, gs):
    """12 steps of torch.optim.Adam(foreach=False) on a float64 CPU tensor; every step is judged on its own, from torch's incoming
    p / exp_avg / exp_avg_sq.  Agreement to 1e-12 relative to the magnitudes that enter each sum (|m| + |g'| for m, |p| + |step| for p,
    v itself for v, which has no cancellation); measured: below 1e-15."""
    n, lr = 4001, 1e-3
    rng = np.random.default_rng(17)
    p = torch.nn.Parameter(torch.from_numpy(0.1 * rng.standard_normal(n)))
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd, foreach=False)
    worst = 0.0
    for t in range(1, 13):
        g = make_grads(rng, n, t)
        if t % 4 == 0:
            assert 0.25 < (g == 0).mean() < 0.35
        st = opt.state.get(p, {})
        p0 = p.detach().numpy().copy()
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n)
        p.grad = torch.from_numpy(g.astype(np.float64) * gs)
        opt.step()
        st = opt.state[p]
        assert int(st["step"]) == t
        r = ref_adam(p0, g, m0, v0, t, lr, wd=wd, gs=gs)
        delta = np.abs(r.p - r.p0)
        for got, ref, scale in ((p.detach().numpy(), r.p, np.abs(p0) + delta), (st["exp_avg"].numpy(), r.m, np.abs(m0) + np.abs(r.gp)),
                                (st["exp_avg_sq"].numpy(), r.v, r.v)):
            d = np.abs(got - ref)
            assert (d <= 1e-12 * scale).all(), (t, float((d / np.maximum(scale, 1e-300)).max()))
            worst = max(worst, float(np.divide(d, scale, out=np.zeros_like(d), where=scale > 0).max()))
    print("ref_adam vs torch float64: worst relative difference %.3g" % worst)


def test_ref_adam_skip_range_and_zero_gradient():
    rng = np.random.default_rng(3)
    n = 50
    p, m, v = rng.standard_normal(n), rng.standard_normal(n), rng.random(n)
    r = ref_adam(p, make_grads(rng, n, 1), m, v, 3, 1e-3, wd=1e-4, skip=(7, 23))
    for new, old in ((r.p, p), (r.m, m), (r.v, v)):
        assert np.array_equal(new[7:23], old[7:23]) and (new[:7] != old[:7]).all() and (new[23:] != old[23:]).all()
    assert all((e[7:23] == 0).all() and (e[:7] > 0).all() for e in adam_bounds(r))
    r = ref_adam(p, np.zeros(n), np.zeros(n), np.zeros(n), 1, 1e-3)
    assert np.array_equal(r.p, p) and not r.m.any() and not r.v.any()


def test_bounds_hold_for_torch_fp32_adam_on_the_cpu():
    """The yardstick of the GPU test applied to an independent fp32 implementation: torch's own fp32 CPU Adam, teacher-forced over 12
    steps, stays inside 4 x the bounds (it measures about 1, 1 and 2.2 of them for p, m, v)."""
    n, lr, wd, gs = 100003, f32(1e-3), f32(1e-4), f32(0.1)
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-8)
    rng = np.random.default_rng(5)
    p = torch.nn.Parameter(torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, 13):
        g = make_grads(rng, n, t)
        st = opt.state.get(p, {})
        p0 = p.detach().numpy().copy()
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n, dtype=np.float32)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, dtype=np.float32)
        p.grad = torch.from_numpy(g) * torch.tensor(gs, dtype=torch.float32)
        opt.step()
        st = opt.state[p]
        r = ref_adam(p0, g, m0, v0, t, lr, b1, b2, eps, wd, gs)
        worst = [max(a, b) for a, b in zip(worst, worst_ratios(p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), r))]
    print("torch fp32 CPU Adam, worst |err| / bound (p, m, v): %.2f %.2f %.2f" % tuple(worst))
    assert max(worst) <= 4.0, worst
