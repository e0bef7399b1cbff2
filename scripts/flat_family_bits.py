#!/usr/bin/env python
"""The flat-array kernels (csrc/flat_dev.h: sgd_flat, adam_flat_kernel, agem_*, clip_*, ewc_*) bit for bit: every kernel through its
`ops.` function at every size at which the streaming loop or the reduction takes another corner (1, 3, 4, 5, 1003, 4099, and 1094750 and
1109240, where the reduction grid is capped and a thread makes several trips), on both sides of every decision, from seeded numpy
inputs.  One line per case: the SHA-256 of every output array's bytes, the info words, penalty, min / max and workspace included.

  python scripts/flat_family_bits.py [SEED]                          # the library of the tree
  OCL_LIB=<another build> python scripts/flat_family_bits.py [SEED]  # the same cases on another build of libocl_hip.so

Two builds compute the same thing exactly when the two outputs are the same text (`profiles/flat_family_bits.txt`).  A differing line
is a changed summation order or a changed contraction in that kernel.  Nothing is compared here: the script prints."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (1, 3, 4, 5, 1003, 4099, 1094750, 1109240)
NAN_WITH_PAYLOAD = 0x7fc12345


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(op, case, n, **arrays):
    print("%-14s %-34s n=%-8d %s" % (op, case, n, " ".join("%s=%s" % (k, sha(v)) for k, v in arrays.items())), flush=True)


class Inputs:
    """Seeded float32 arrays of one case, uploaded to the device."""
    def __init__(self, seed, n, op, dev):
        self.rng = np.random.default_rng([seed, n, sum(op.encode())])
        self.n, self.dev = n, dev

    def normal(self, scale=1.0):
        return (scale * self.rng.standard_normal(self.n)).astype(np.float32)

    def positive(self, scale=1.0):
        return (scale * self.rng.random(self.n)).astype(np.float32)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)


def agem(ops, lib, seed, n, dev):
    i = Inputs(seed, n, "agem", dev)
    r, noise = i.normal(), i.normal(0.1)
    with_nan = 0.5 * r + noise
    with_nan.view(np.uint32)[[0, n - 1]] = NAN_WITH_PAYLOAD          # in the first vector and in the tail (or the last vector)
    for case, g in (("projected", -0.5 * r + noise), ("not-projected", 0.5 * r + noise), ("not-projected-nan-in-g", with_nan)):
        g_d, r_d = i.up(g.astype(np.float32)), i.up(r)
        ws = torch.zeros(lib.ocl_agem_workspace_doubles(n), dtype=torch.float64, device=dev)
        info = torch.zeros(4, device=dev)
        ops.agem_project(g_d, r_d, workspace=ws, info=info)
        line("agem_project", case, n, g_ref=r_d, info=info, workspace=ws)


def clip(ops, lib, seed, n, dev):
    i = Inputs(seed, n, "clip", dev)
    g = i.normal()
    for case, max_norm in (("clipped", 0.1), ("not-clipped", 1e9), ("max_norm-0", 0.0)):
        g_d = i.up(g)
        ws = torch.zeros(lib.ocl_clip_workspace_doubles(n), dtype=torch.float64, device=dev)
        info = torch.zeros(4, device=dev)
        total = ops.clip_grad_norm_(g_d, max_norm, workspace=ws, info=info)
        line("clip_grad_norm", case, n, g=g_d, total=total, info=info, workspace=ws)


def ewc(ops, lib, seed, n, dev):
    i = Inputs(seed, n, "ewc", dev)
    g, t, p, q, f = i.normal(), i.positive(), i.normal(), i.normal(), i.positive()
    for has_prev in (False, True):
        for scale in (0.0, 2.5):
            for want in (False, True):
                g_d, t_d = i.up(g), i.up(t)
                ws = torch.zeros(lib.ocl_ewc_workspace_doubles(n), dtype=torch.float64, device=dev)
                pen = torch.zeros(1, device=dev)
                ops.ewc_accumulate(g_d, t_d, i.up(p), i.up(q) if has_prev else None, i.up(f) if has_prev else None, scale=scale,
                                   workspace=ws if want else None, penalty_out=pen if want else None)
                line("ewc_accumulate", "prev-%d,scale-%g,penalty_out-%d" % (has_prev, scale, want), n, grads=g_d, tmp_fisher=t_d, penalty=pen,
                     workspace=ws)
    run_d, t_d = i.up(f), i.up(t)
    ops.ewc_fisher_ema(run_d, t_d, 0.1, 0.45)
    line("ewc_fisher_ema", "keep-0.1,gain-0.45", n, running=run_d, tmp_fisher=t_d)
    far = (0, (3 * n) // 4)                                           # the two extremes in different blocks where there are several
    tail = (n - 1, max(n - 2, 0))                                     # ... and in the scalar tail (or the last vector)
    for case, (at_min, at_max) in (("extremes-in-different-blocks", far), ("extremes-in-the-tail", tail)):
        run = f.copy() + 1.0
        run[at_max] = 7.5
        run[at_min] = 0.25
        run_d, out = i.up(run), torch.zeros(n, device=dev)
        ws = torch.zeros(lib.ocl_ewc_workspace_doubles(n), dtype=torch.float64, device=dev)
        mm = torch.zeros(2, device=dev)
        ops.ewc_fisher_normalize(run_d, out, workspace=ws, minmax_out=mm)
        line("ewc_normalize", case, n, fisher_hat=out, minmax=mm, workspace=ws)


def adam(ops, lib, seed, n, dev):
    i = Inputs(seed, n, "adam", dev)
    p, g, m, v = i.normal(0.1), i.normal(), i.normal(0.01), i.positive(0.01)
    b = n // 3
    for step in (1, 7):
        for case, skip in (("empty", (0, 0)), ("straddling", (b, min(n, b + n // 2 + 1))), ("whole-array", (0, n))):
            p_d, m_d, v_d = i.up(p), i.up(m), i.up(v)
            ops.adam_step(p_d, i.up(g), m_d, v_d, step, 1e-3, weight_decay=1e-4, grad_scale=0.1, skip=skip)
            line("adam_step", "step-%d,skip-%s[%d,%d)" % (step, case, skip[0], skip[1]), n, params=p_d, exp_avg=m_d, exp_avg_sq=v_d)


def sgd(ops, lib, seed, n, dev):
    i = Inputs(seed, n, "sgd", dev)
    p, g = i.normal(0.1), i.normal()
    p_d = i.up(p)
    ops.sgd_step(p_d, i.up(g), 0.1, weight_decay=1e-4, grad_scale=0.1)
    line("sgd_step", "in-place", n, params=p_d)
    p_d, out = i.up(p), torch.zeros(n, device=dev)
    ops.sgd_step(p_d, i.up(g), 0.1, weight_decay=1e-4, grad_scale=0.1, out=out)
    line("sgd_step", "with-out", n, params=p_d, out=out)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    if not torch.cuda.is_available():
        raise SystemExit("flat_family_bits.py runs the kernels on an MI355X; no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi, ops
    ffi.init()
    print("flat_family_bits: seed %d, sizes %s" % (seed, " ".join(str(n) for n in SIZES)))
    for n in SIZES:
        for family in (sgd, adam, agem, clip, ewc):
            family(ops, ffi.lib(), seed, n, dev)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
