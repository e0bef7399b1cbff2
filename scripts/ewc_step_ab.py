#!/usr/bin/env python
"""--agent EWC: the fused bookkeeping (ops.ewc_accumulate: one launch between backward and opt.step(); ops.ewc_fisher_ema every
fisher_update_after steps; ops.ewc_fisher_normalize at a task's end) against the reference's own statements over the p / p.grad views
(agents/ewc_pp.py:76-106: a 62-tensor autograd graph for the penalty, 62 launches of `tmp += grad ** 2`, the per-tensor moving average,
the max / min lists), on the EWC++ agent at BASELINE configs[0] sizes (cifar10 shape, batch 10, SGD) with task_seen >= 1, so that every
step carries the penalty (MI355X).  There is no replay memory: the step is one batch pass plus this bookkeeping.

  python scripts/ewc_step_ab.py                          # timing: both sides in one process, alternating A/B/A/B, 20 warm-up + 200
                                                         # timed steps per leg, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/fused -o p -- python scripts/ewc_step_ab.py --profile fused
  rocprofv3 --kernel-trace --stats -d OUT/torch -o p -- python scripts/ewc_step_ab.py --profile torch
                                                         # one run per side: kernel trace of 20 + 200 steps, nothing timed
  python scripts/ewc_step_ab.py --summarise OUT          # launches per step of the bookkeeping from the two databases

Every leg is one train_learner call: the warm-up call ends a task (prev_params and the normalised Fisher exist from then on), and each
timed call ends one too (one parameter copy and the normalisation inside the window, on both sides).  The comparator is the agent's
private `_force_torch_bookkeeping` attribute (the product has no switch for it)."""
import argparse
import glob
import os
import random
import sqlite3
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload's sizes and the synthetic stream of the benchmark)

WARMUP, STEPS, ROUNDS = 20, 200, 5
EWC = dict(lambda_=100, alpha=0.9, fisher_update_after=50, learning_rate=0.01)      # (at lr 0.1 and lambda_ 100 EWC++ itself diverges)
CONFIG = "BASELINE configs[0] shape: EWC++, cifar10, batch 10, SGD lr 0.01, lambda_ 100, alpha 0.9, fisher_update_after 50, task_seen >= 1"
SIDES = ("fused", "torch")


def build(side, device, seed=0):
    """The EWC++ agent on bench.py's ER workload sizes."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.setup_elements import setup_architecture, setup_opt, n_classes, input_size_match
    params = bench.make_params(dict(bench.WORKLOADS["er"], agent="EWC", **EWC))
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent("EWC")(model, opt, params)
    agent._force_torch_bookkeeping = side == "torch"
    hw, ncls = input_size_match[params.data][1], n_classes[params.data]
    return params, model, agent, hw, ncls


def stream(steps, bs, hw, ncls, seed, device):
    x, y = bench.synth_u8(steps * bs, hw, ncls, seed)
    return torch.from_numpy(x).to(device), y


def timing(device):
    print("ewc_step_ab: %s, torch %s, %d warm-up + %d timed steps per leg, %d legs per side alternating fused / torch in one process"
          % (torch.cuda.get_device_name(device), torch.__version__, WARMUP, STEPS, ROUNDS))
    sides = {side: build(side, device) for side in SIDES}
    params, _, _, hw, ncls = sides["fused"]
    bs = params.batch
    warm = stream(WARMUP, bs, hw, ncls, 1, device)
    for side in SIDES:
        sides[side][2].train_learner(*warm)
        assert sides[side][2].task_seen == 1 and sides[side][2].prev_params is not None
    torch.cuda.synchronize()
    ms = {side: [] for side in SIDES}
    for r in range(ROUNDS):
        timed = stream(STEPS, bs, hw, ncls, 10 + r, device)
        for side in SIDES:
            agent = sides[side][2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train_learner(*timed)          # exactly STEPS iterations (drop_last, len = STEPS * batch)
            torch.cuda.synchronize()
            ms[side].append((time.perf_counter() - t0) / STEPS * 1e3)
    print("%s; %d parameters" % (CONFIG, sides["fused"][1].flat_params().numel()))
    for side in SIDES:
        v = ms[side]
        print("  %-5s  ms/step median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
              % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
    f, s = statistics.median(ms["fused"]), statistics.median(ms["torch"])
    print("  fused / torch = %.3f  (%.4f ms per step %s)" % (f / s, abs(s - f), "saved" if f <= s else "LOST"))
    print("the fused bookkeeping is not slower than the reference's statements: %s" % ("yes" if f <= s else "NO"))
    return 0 if f <= s else 1


def profile(side, device):
    params, model, agent, hw, ncls = build(side, device)
    agent.train_learner(*stream(WARMUP, params.batch, hw, ncls, 1, device))
    agent.train_learner(*stream(STEPS, params.batch, hw, ncls, 10, device))
    torch.cuda.synchronize()
    print("profiled %s: %d steps" % (side, WARMUP + STEPS))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(out):
    steps = WARMUP + STEPS
    print("rocprofv3 --kernel-trace --stats, one run per side: %d + %d steps in two train_learner calls (the second carries the penalty; "
          "device copies run as the runtime's copyBuffer kernel and are counted)" % (WARMUP, STEPS))
    st = {side: kernel_stats(os.path.join(out, side)) for side in SIDES}
    total = {side: sum(v[0] for v in st[side].values()) for side in st}
    for side in SIDES:
        other_side = "torch" if side == "fused" else "fused"
        only = {k: v for k, v in st[side].items() if st[other_side].get(k, (0,))[0] != v[0]}
        print("  %-5s  %d kernel launches in all; kernels whose launch count differs from the other side:" % (side, total[side]))
        for k, v in sorted(only.items(), key=lambda kv: -kv[1][0]):
            other = st[other_side].get(k, (0,))[0]
            print("    %6d calls (other side %6d)  %7.2f per step  avg %8.1f ns  min %7d  max %7d  %s"
                  % (v[0], other, (v[0] - other) / steps, v[1], v[2], v[3], k[:110]))
    mine = {k: v for k, v in st["fused"].items() if "ewc_" in k}
    assert mine and not any("ewc_" in k for k in st["torch"]), sorted(mine)
    calls = sum(v[0] for v in mine.values())
    print("  bookkeeping launches per step: fused %.2f (%s: %d calls / %d steps), torch %.2f (all launches of the torch run minus all "
          "launches of the fused run, per step, plus the fused side's own)"
          % (calls / steps, " + ".join("%d %s" % (v[0], k.split("(")[0].split("<")[0].replace("void ", "")) for k, v in sorted(mine.items())), calls, steps,
             (total["torch"] - total["fused"]) / steps + calls / steps))
    n = 1094750
    for k, v in sorted(mine.items()):
        if "ewc_accumulate" not in k:
            continue
        reads = 5 if "<true, true" in k.replace("(bool)1", "true").replace("(bool)0", "false") else 2
        nbytes = 4.0 * (reads + (2 if reads == 5 else 1)) * n
        print("  %s: %d calls, avg %.2f us per call (min %.2f, max %.2f); %.0f B x %d elements = %.1f MB per call -> %.2f TB/s"
              % (k.split("(")[0], v[0], v[1] / 1e3, v[2] / 1e3, v[3] / 1e3, nbytes / n, n, nbytes / 1e6, nbytes / (v[1] * 1e-9) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", metavar="SIDE", choices=SIDES)
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("ewc_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile, device)
        return 0
    return timing(device)


if __name__ == "__main__":
    sys.exit(main())
