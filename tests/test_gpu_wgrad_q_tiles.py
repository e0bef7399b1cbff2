"""GPU: the tile loop of the 4x4x1 weight-gradient form (conv_wgrad_kernel<1, 1, PF, RGW > 0>: two LDS tile buffers, one barrier per
tile) at every tile count per workgroup at which the loop behaves differently, through the single-layer hook ocl_test_wgrad.

Layer 1's convolution (20 -> 20 channels, 3x3, stride 1) with tier-1 data: inputs and gradients are integers from {-2 .. 2}, so every
partial sum stays below 2^24 (at most 70 * 1024 pixels * 5 * 2), the fp32 result is exact in any order, and the weight gradient must
be BIT-equal to torch's float64 one: a tile that is read from the wrong buffer, read before it is written, or overwritten while it is
still being read is an O(1) error.

  32 x 32, N = 1     8 tiles, one per workgroup: the loop body never swaps buffers
  32 x 32, N = 40    two tiles per workgroup: one swap
  32 x 32, N = 65    520 tiles over 174 workgroups: three tiles (odd) in most, two (even) in the last ones of the same launch
  84 x 84, N = 1     7056 pixels in tiles of 64: the last tile of the image is ragged
and the same with the input transform (the producer's BatchNorm + ReLU applied while the patch is staged; its table lies behind both
buffers): two BatchNorm groups with different power-of-two scales and integer shifts per channel, N = 2 / 40 / 68 / 2 (the groups
halve the images, so N is even; 68 images: three tiles and two).

OCL_WGRAD_Q=2 lifts the planner's size gate for the form and is read once per process: the cases run in ONE child process (this file
run as a script), which prints a JSON record per case; the tests check the records."""
import json
import os
import subprocess
import sys

import pytest

# (input size, images, groups of the input transform or 0, pixel splits the planner gives = workgroups, pixel tiles)
CASES = [(32, 1, 0, 8, 8), (32, 40, 0, 160, 320), (32, 65, 0, 174, 520), (84, 1, 0, 111, 111),
         (32, 2, 2, 16, 16), (32, 40, 2, 160, 320), (32, 68, 2, 182, 544), (84, 2, 2, 222, 222)]
# tiles per workgroup (workgroup b takes tiles b, b + S, ...): the first and the last workgroup's
TILES_PER_WG = {(32, 1, 0): (1, 1), (32, 40, 0): (2, 2), (32, 65, 0): (3, 2), (84, 1, 0): (1, 1),
                (32, 2, 2): (1, 1), (32, 40, 2): (2, 2), (32, 68, 2): (3, 2), (84, 2, 2): (1, 1)}
CIN = COUT = 20


def case_id(c):
    return "hw%d_n%d_xf%d" % c[:3]


def _worker():
    import ctypes as C
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    import torch
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi
    from guarded import FILL, SLACK, dev
    ffi.init()
    lib = ffi.lib()
    torch.set_num_threads(16)
    out = {}
    for hw, n, xfg, _, _ in CASES:
        g = torch.Generator().manual_seed(1000 * hw + 10 * n + xfg)
        x = torch.randint(-2, 3, (n, hw, hw, CIN), generator=g).double()
        dy = torch.randint(-2, 3, (n, hw, hw, COUT), generator=g).double()
        d = ffi.TestWgradDesc()
        d.cin, d.cout, d.k, d.stride, d.hin, d.win, d.n, d.xf_groups = CIN, COUT, 3, 1, hw, hw, n, xfg
        o = ffi.TestWgradOps()
        keep = [dev(x.float()), dev(dy.float())]
        flat = torch.full((COUT * CIN * 9 + SLACK,), float(FILL), device="cuda")
        flat[: COUT * CIN * 9].fill_(float("nan"))
        o.x, o.dy, o.grad = C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()), C.c_void_p(flat.data_ptr())
        xin = x
        if xfg:
            # scale = gamma * invstd in {1, 2}, shift = beta - mean * scale: integers; relu(x * scale + shift) stays an integer <= 2 * 2 + 1
            gamma = 2.0 ** torch.randint(0, 2, (CIN,), generator=g).double()
            beta = torch.randint(-1, 2, (CIN,), generator=g).double()
            mean = torch.randint(-1, 2, (xfg, CIN), generator=g).double()
            invstd = torch.ones(xfg, CIN, dtype=torch.float64)
            for name, t in (("xf_mean", mean), ("xf_invstd", invstd), ("xf_gamma", gamma), ("xf_beta", beta)):
                keep.append(dev(t.float()))
                setattr(o, name, C.c_void_p(keep[-1].data_ptr()))
            o.xf = 1
            grp = (torch.arange(n) // (n // xfg)).clamp(max=xfg - 1)
            xin = torch.clamp(x * gamma + (beta - mean[grp] * gamma)[:, None, None, :], min=0)
        f = ffi.TestWgradForm()
        rc = lib.ocl_test_wgrad(C.byref(d), C.byref(o), 1, 0, 0, C.byref(f), None)
        rec = dict(rc=rc, error=lib.ocl_last_error().decode() if rc else "", q_rgw=f.q_rgw, s=f.s, grid=[f.grid_x, f.grid_y])
        if rc == 0:
            torch.cuda.synchronize()
            got = flat[: COUT * CIN * 9].double().cpu().view(COUT, CIN, 3, 3)
            ref = torch.nn.grad.conv2d_weight(xin.permute(0, 3, 1, 2).contiguous(), (COUT, CIN, 3, 3), dy.permute(0, 3, 1, 2).contiguous(),
                                              stride=1, padding=1)
            bad = ~(got == ref)   # (a NaN left in the gradient counts)
            rec.update(differ=int(bad.sum()), total=bad.numel(), past_end=int((flat[COUT * CIN * 9:] != FILL).sum()),
                       max_abs_ref=float(ref.abs().max()))
            if bool(bad.any()):
                i = tuple(bad.nonzero()[0].tolist())
                rec["first"] = [list(i), float(got[i]), float(ref[i])]
        out[case_id((hw, n, xfg))] = rec
    print("RESULTS " + json.dumps(out))


if __name__ == "__main__":
    _worker()
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def records(cuda):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OCL_WGRAD_Q="2"))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULTS ")]
    assert lines, r.stdout + r.stderr
    return json.loads(lines[-1][len("RESULTS "):])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_4x4x1_form_is_exact_at_this_tile_count(case, records):
    hw, n, xfg, splits, tiles = case
    rec = records[case_id(case)]
    assert rec["rc"] == 0, rec
    assert rec["q_rgw"] == 3 and rec["s"] == splits and rec["grid"] == [splits, 1], "the planner no longer gives this case its tile counts: %r" % rec
    first, last = TILES_PER_WG[case[:3]]
    assert (len(range(0, tiles, splits)), len(range(splits - 1, tiles, splits))) == (first, last)
    assert rec["past_end"] == 0, rec
    assert rec["max_abs_ref"] < 2 ** 24
    assert rec["differ"] == 0, "%d of %d gradient entries differ from float64 (first [index, got, want]: %r)" % (
        rec["differ"], rec["total"], rec.get("first"))
