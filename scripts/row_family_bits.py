#!/usr/bin/env python
"""The per-row loss kernels (csrc/row_dev.h: ce_kernel, ce_seg_kernel, kd_kernel, mir_kernel, ce_kd_blend_kernel, bce_distill_kernel,
row_argmax_groupsum_kernel) bit for bit: every kernel through its `ops.` function at the smallest shapes on both sides of every decision
-- c = 1, 63, 64, 65 (the lane boundary), 255, 256, 257, 300 (registers / strided loop), n = 1, 3, 4, 5, 9 (short of, at and past the
four waves of the row loop and the four rows of a row-statistics workgroup) -- crossed with the options of each, from seeded numpy
inputs; then labels outside the row, non-finite logits in a student's and in a teacher's row, and a teacher that is the student.  One
line per case: the SHA-256 of every output array's bytes.

  python scripts/row_family_bits.py [SEED]                          # the library of the tree
  OCL_LIB=<another build> python scripts/row_family_bits.py [SEED]  # the same cases on another build of libocl_hip.so

Two builds compute the same thing exactly when the two outputs are the same text.  A differing line is a changed summation order or a
changed contraction in that kernel.  Nothing is compared here: the script prints.

  python scripts/row_family_bits.py --digest OUT_A OUT_B            # the two saved texts folded per operation and column count

(`profiles/row_family_bits.txt`: the texts themselves are 2391 lines each.)

  rocprofv3 --kernel-trace --stats -d OUT/<leg> -o p -- python scripts/row_family_bits.py --launches N
  python scripts/row_family_bits.py --summarise OUT/parent1 OUT/tree1 OUT/parent2 [OUT/tree2 OUT/parent3 ...]

--launches issues every kernel N times at the shapes the agents use (n = 10 and 20 rows of c = 100 logits; the BCE loss at n_old = 90
of 100; the row statistics at n = 128) for a kernel trace; --summarise reads such traces in the order they were taken (parent, tree, parent, ...)
and prints, per round, each kernel's mean duration and whether the tree's is within the parent's own run-to-run difference (`profiles/row_family_kernel_times.txt`)."""
import glob
import hashlib
import os
import sqlite3
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLS = (1, 63, 64, 65, 255, 256, 257, 300)
ROWS = (1, 3, 4, 5, 9)
SPECIAL = ((5, 65), (9, 300))                   # (n, c) of the label, non-finite and teacher-equals-student cases: both row forms
TEMPS = (1.0, 2.0, 3.0)
WEIGHTS = ((1.0, 0.0), (0.5, 0.5), (1.0 / 3.0, 2.0 / 3.0))
MODES = ("grad", "no-grad", "dl_out")
FAMILY = ("ce_kernel", "ce_seg_kernel", "kd_kernel", "mir_kernel", "ce_kd_blend_kernel", "bce_distill_kernel", "row_argmax_groupsum_kernel")


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(op, case, n, c, **arrays):
    print("%-20s %-58s n=%-2d c=%-3d %s" % (op, case, n, c, " ".join("%s=%s" % (k, sha(v)) for k, v in arrays.items())), flush=True)


class Inputs:
    """Seeded arrays of one (n, c), uploaded to the device."""
    def __init__(self, seed, n, c, dev):
        self.rng = np.random.default_rng([seed, n, c])
        self.n, self.c, self.dev = n, c, dev
        self.s = self.logits()
        self.t = self.logits()
        self.y = self.rng.integers(0, c, n).astype(np.int64)
        self.seg = (np.arange(c) % 2).astype(np.int32)          # two segments and, from three columns on, one column in none
        if c >= 3:
            self.seg[c // 2] = -1

    def logits(self):
        return (3.0 * self.rng.standard_normal((self.n, self.c))).astype(np.float32)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def grad_args(self, mode):
        """(keyword arguments, the buffer dl_out is a row block of | None): rows 1 .. n of a buffer of n + 3 rows of 7.0"""
        if mode != "dl_out":
            return {"want_grad": mode == "grad"}, None
        big = torch.full((self.n + 3, self.c), 7.0, dtype=torch.float32, device=self.dev)
        return {"dl_out": big[1:1 + self.n]}, big


def with_nonfinite(a):
    """NaN, +inf and -inf planted in rows 0, 1 and 2 (one row takes all of them where there are fewer rows)."""
    a = a.copy()
    n, c = a.shape
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        a[k % n, (k * 31 + 1) % c] = v
    return a


def ce(ops, i, s=None, y=None, tag=""):
    s_d, y_d = i.up(i.s if s is None else s), i.up(i.y if y is None else y)
    for red in ("none", "mean"):
        for mode in MODES:
            kw, big = i.grad_args(mode)
            loss, dl = ops.cross_entropy(s_d, y_d, reduction=red, **kw)
            line("cross_entropy", "%sreduction-%s,%s" % (tag, red, mode), i.n, i.c, loss=loss, dlogits=dl if big is None else big)


def ce_seg(ops, i, s=None, y=None, tag=""):
    s_d, y_d, seg_d = i.up(i.s if s is None else s), i.up(i.y if y is None else y), i.up(i.seg)
    for want in (True, False):
        loss, dl = ops.cross_entropy_segmented(s_d, y_d, seg_d, want_grad=want)
        line("cross_entropy_seg", "%swant_grad-%d" % (tag, want), i.n, i.c, loss=loss, dlogits=dl)


def kd(ops, i, s=None, t=None, tag=""):
    s_d, t_d = i.up(i.s if s is None else s), i.up(i.t if t is None else t)
    for T in TEMPS:
        for want in (True, False):
            loss, ds = ops.kd_loss(s_d, t_d, T=T, want_grad=want)
            line("kd_loss", "%sT-%g,want_grad-%d" % (tag, T, want), i.n, i.c, loss=loss, dscores=ds)


def mir(ops, i, pre=None, y=None, tag=""):
    out = ops.mir_scores(i.up(i.s if pre is None else pre), i.up(i.t), i.up(i.y if y is None else y))
    line("mir_scores", "%spost-minus-pre" % tag, i.n, i.c, scores=out)


def blend(ops, i, s=None, t=None, y=None, tag="", teachers=(False, True)):
    s_d, t_d, y_d = i.up(i.s if s is None else s), i.up(i.t if t is None else t), i.up(i.y if y is None else y)
    for teacher in teachers:
        for T in (TEMPS if teacher else TEMPS[:1]):
            for w_new, w_old in WEIGHTS:
                # the three gradient modes at one (T, weights) with a teacher and at the plain cross-entropy without one
                for mode in (MODES if (T, w_new) == ((2.0, 0.5) if teacher else (1.0, 1.0)) else MODES[:1]):
                    kw, big = i.grad_args(mode)
                    loss, dl = ops.ce_kd_blend(s_d, y_d, t_d if teacher else None, T, w_new, w_old, **kw)
                    line("ce_kd_blend", "%steacher-%d,T-%g,w-%.3g/%.3g,%s" % (tag, teacher, T, w_new, w_old, mode), i.n, i.c, loss3=loss,
                         dlogits=dl if big is None else big)


def bce(ops, i, s=None, t=None, pos_outside=False, tag=""):
    s_d, t_d = i.up(i.s if s is None else s), i.up(i.t if t is None else t)
    for n_cls in sorted({i.c, max(1, i.c - 2)}):
        for n_old in sorted({0, n_cls // 2, n_cls}):
            for n_stream in sorted({1, i.n}):
                # the stream rows' target columns: among the new columns where there are any
                pos = i.y[:n_stream] % max(1, n_cls - n_old) + min(n_old, n_cls - 1)
                if pos_outside:
                    pos = pos.copy()
                    pos[0] = i.c + 5
                    pos[-1] = -3
                for mode in (MODES if (n_cls, n_stream) == (i.c, i.n) else MODES[:1]):   # the three gradient modes at every n_old
                    kw, big = i.grad_args(mode)
                    loss, dl = ops.bce_distill(s_d, t_d if n_old else None, i.up(pos), n_stream, n_cls, n_old, **kw)
                    line("bce_distill", "%sn_cls-%d,n_old-%d,n_stream-%d,%s" % (tag, n_cls, n_old, n_stream, mode), i.n, i.c, loss3=loss,
                         dlogits=dl if big is None else big)


def rowstats(ops, i, x=None, tag=""):
    x_d = i.up(i.s if x is None else x)
    groups = (("none", None, 0), ("empty", i.seg, 5), ("full", np.full(i.c, 2, np.int32), 2), ("segment-1", i.seg, 1))
    for name, group, sel in groups:
        am, sm = ops.row_argmax_groupsum(x_d, None if group is None else i.up(group), sel)
        line("row_argmax_groupsum", "%scol_group-%s" % (tag, name), i.n, i.c, argmax=am, sums=sm)
    am, _ = ops.row_argmax_groupsum(x_d, want_sum=False)
    _, sm = ops.row_argmax_groupsum(x_d, i.up(i.seg), 0, want_argmax=False)
    line("row_argmax_groupsum", "%sone-result-each" % tag, i.n, i.c, argmax=am, sums=sm)


def bits(ops, seed, dev):
    print("row_family_bits: seed %d, columns %s, rows %s" % (seed, " ".join(map(str, COLS)), " ".join(map(str, ROWS))))
    for c in COLS:
        for n in ROWS:
            i = Inputs(seed, n, c, dev)
            for family in (ce, ce_seg, kd, mir, blend, bce, rowstats):
                family(ops, i)
    for n, c in SPECIAL:
        i = Inputs(seed, n, c, dev)
        y_out = i.y.copy()
        y_out[0], y_out[-1] = c, -1                              # just past the row and before it
        for family in (ce, ce_seg, mir, blend):
            family(ops, i, y=y_out, tag="label-outside,")
        bce(ops, i, pos_outside=True, tag="pos-outside,")
        bad_s, bad_t = with_nonfinite(i.s), with_nonfinite(i.t)
        for family in (ce, ce_seg, kd, blend, bce):
            family(ops, i, s=bad_s, tag="nonfinite-student,")
        mir(ops, i, pre=bad_s, tag="nonfinite-pre,")
        rowstats(ops, i, x=bad_s, tag="nonfinite,")
        blend(ops, i, t=bad_t, tag="nonfinite-teacher,", teachers=(True,))
        bce(ops, i, t=bad_t, tag="nonfinite-teacher,")
        kd(ops, i, t=i.s, tag="teacher-is-student,")
        blend(ops, i, t=i.s, tag="teacher-is-student,", teachers=(True,))
        bce(ops, i, t=i.s, tag="teacher-is-student,")
        mir(ops, i, pre=i.t, tag="pre-is-post,")


def launches(ops, count, dev):
    """Every kernel `count` times at each of the agents' shapes, nothing read back in between."""
    for n in (10, 20):
        i = Inputs(0, n, 100, dev)
        s, t, y, seg = i.up(i.s), i.up(i.t), i.up(i.y), i.up(i.seg)
        pos = i.up(i.y % 10 + 90)
        dl = torch.empty_like(s)
        for _ in range(count):
            ops.cross_entropy(s, y, dl_out=dl)
            ops.cross_entropy_segmented(s, y, seg)
            ops.kd_loss(s, t)
            ops.mir_scores(s, t, y)
            ops.ce_kd_blend(s, y, t, 2.0, 0.5, 0.5, dl_out=dl)
            ops.bce_distill(s, t, pos, n, 100, 90, dl_out=dl)
        torch.cuda.synchronize()
    i = Inputs(0, 128, 100, dev)
    x, seg = i.up(i.s), i.up(i.seg)
    for _ in range(count):
        ops.row_argmax_groupsum(x, seg, 1)
    torch.cuda.synchronize()
    print("row_family_bits: %d launches of every kernel at each of its shapes" % count)


def kernel_means(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start) from kernels group by name").fetchall()
    named = {r[0].split("(")[0].replace("void ", "").replace("ocl::", ""): (r[1], r[2] / 1e3) for r in rows}
    return {k: v for k, v in named.items() if k.split("<")[0] in FAMILY}


def summarise(dirs):
    """dirs: traces in the order they were taken, parent, tree, parent[, tree, parent ...]; a round is a tree run and its two neighbours"""
    runs = [kernel_means(d) for d in dirs]
    print("mean kernel duration in us (launches): parent, tree, parent; the tree passes when it is no higher than the slower parent run")
    print("by more than the two parent runs differ from each other")
    for r in range(0, len(runs) - 2, 2):
        print("round %d" % (r // 2 + 1))
        for k in sorted(runs[r + 1]):
            (na, pa), (nb, tr), (nc, pc) = runs[r][k], runs[r + 1][k], runs[r + 2][k]
            bound = max(pa, pc) + abs(pa - pc)
            print("  %-42s %7.3f (%d)  %7.3f (%d)  %7.3f (%d)   bound %7.3f  %s" % (k, pa, na, tr, nb, pc, nc, bound, "pass" if tr <= bound else "ABOVE"))


def digest(path_a, path_b):
    """Two saved outputs side by side, folded: per operation and column count the number of case lines and the SHA-256 of those lines."""
    def groups(path):
        g = {}
        for ln in open(path).read().splitlines()[1:]:
            g.setdefault((ln.split()[0], int(ln.split(" c=")[1].split()[0])), []).append(ln)
        return {k: (len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()) for k, v in g.items()}
    a, b = groups(path_a), groups(path_b)
    for k in sorted(set(a) | set(b)):
        (na, ha), (nb, hb) = a.get(k, (0, "-")), b.get(k, (0, "-"))
        print("%-20s c=%-3d %4d %s  %4d %s  %s" % (k[0], k[1], na, ha, nb, hb, "same" if (na, ha) == (nb, hb) else "DIFFERENT"))
    same = open(path_a).read() == open(path_b).read()
    print("%d and %d lines: %s" % (sum(v[0] for v in a.values()) + 1, sum(v[0] for v in b.values()) + 1,
                                   "identical, byte for byte" if same else "NOT identical"))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--digest":
        digest(sys.argv[2], sys.argv[3])
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("row_family_bits.py runs the kernels on an MI355X; no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import ocl_amd  # noqa: F401
    from ocl_amd import ffi, ops
    ffi.init()
    if len(sys.argv) > 1 and sys.argv[1] == "--launches":
        launches(ops, int(sys.argv[2]), dev)
    else:
        bits(ops, int(sys.argv[1]) if len(sys.argv) > 1 else 0, dev)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
