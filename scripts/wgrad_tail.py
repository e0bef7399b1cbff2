#!/usr/bin/env python
"""The weight-gradient tail of the large-pass backward from a rocprofv3 rocpd database (`rocprofv3 --kernel-trace --stats`), for
`steps` consecutive training steps (a step = the kernels between two launches of pack_weights_kernel), counted from the end:
  * idle time on the weight-gradient queue between its first conv_wgrad_kernel and its last kernel of the step (sum of the gaps
    between consecutive kernels there, and the largest single gap);
  * time from the end of the dependent chain's last kernel (the last kernel in front of sgd_flat on sgd_flat's queue that is not a
    weight gradient or its reduction: the stem's BatchNorm backward) to the start of sgd_flat;
  * start and duration of each of the last six conv_wgrad_kernel launches.
Then the per-kernel statistics of the whole run (name, calls, total, average).
    python scripts/wgrad_tail.py results.db [steps, default 3] [skip this many steps at the end, default 1] > profiles/...txt"""
import sqlite3
import sys


def short(name):
    return name.replace("void ocl::", "").replace("ocl::", "")[:72]


def main(path, steps=3, skip=1):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)").fetchall()]
    extra = [k for k in ("queue_id", "stream_id") if k in cols]
    rows = c.execute("select name, start, end%s from kernels order by start" % "".join(", " + k for k in extra)).fetchall()
    marks = [i for i, r in enumerate(rows) if "pack_weights_kernel" in r[0]]
    if len(marks) < steps + skip + 1:
        print("not enough pack_weights_kernel launches (%d)" % len(marks))
        return
    print("# %s: %d kernels, %d steps; queue columns %s" % (path.split("/")[-1], len(rows), len(marks), extra))
    for k in range(steps):
        a, b = marks[-skip - steps + k - 1], marks[-skip - steps + k]
        win = rows[a:b]
        t0 = win[0][1]
        us = lambda t: (t - t0) / 1e3
        wg = [r for r in win if "conv_wgrad_kernel" in r[0]]
        sgd = [r for r in win if "sgd_flat" in r[0]]
        if not wg or not sgd:
            print("step -%d: no conv_wgrad_kernel / sgd_flat launch" % (skip + steps - k))
            continue
        sgd = sgd[-1]
        count = {}
        for r in wg:
            count[r[3:]] = count.get(r[3:], 0) + 1
        side = max(count, key=count.get)
        first = min(r[1] for r in wg if r[3:] == side)
        on_side = sorted((r for r in win if r[3:] == side and r[1] >= first and r[1] < sgd[1]), key=lambda r: r[1])
        gaps = [max(0, y[1] - x[2]) for x, y in zip(on_side, on_side[1:])]
        big = max(range(len(gaps)), key=gaps.__getitem__) if gaps else -1
        chain = [r for r in win if r[3:] == sgd[3:] and r[2] <= sgd[1] and "wgrad" not in r[0]]
        last = max(chain, key=lambda r: r[2])
        print("step -%d: %.1f us from pack_weights to the end of sgd_flat; %d weight-gradient launches, %d on queue %s" % (
            skip + steps - k, us(sgd[2]), len(wg), count[side], "/".join(map(str, side))))
        print("  weight-gradient queue, %.1f .. %.1f us: busy %.1f us, idle %.1f us in %d gaps; largest gap %.1f us at %.1f us" % (
            us(first), us(on_side[-1][2]), sum(r[2] - r[1] for r in on_side) / 1e3, sum(gaps) / 1e3, len(gaps),
            gaps[big] / 1e3 if gaps else 0.0, us(on_side[big][2]) if gaps else 0.0))
        print("  chain end (%s, ends %.1f us) -> sgd_flat start (%.1f us): %.1f us" % (short(last[0]), us(last[2]), us(sgd[1]), (sgd[1] - last[2]) / 1e3))
        for r in sorted(wg, key=lambda r: r[1])[-6:]:
            print("  %9.1f us  +%6.1f us  q=%s  %s" % (us(r[1]), (r[2] - r[1]) / 1e3, "/".join(map(str, r[3:])), short(r[0])))
    stats = {}
    for r in rows:
        s = stats.setdefault(r[0], [0, 0])
        s[0] += 1
        s[1] += r[2] - r[1]
    total = sum(s[1] for s in stats.values())
    print("# per-kernel statistics of the run: calls, total us, average us, share")
    for name, (n, t) in sorted(stats.items(), key=lambda kv: -kv[1][1])[:40]:
        print("  %6d  %10.1f  %8.2f  %5.1f %%  %s" % (n, t / 1e3, t / 1e3 / n, 100.0 * t / total, short(name)))


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:4]])
