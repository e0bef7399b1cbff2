#!/usr/bin/env python
"""--agent LWF: one training step with a teacher (task_seen = 1: forward, the teacher's forward, CE blended with the distillation loss,
backward, SGD step) as the fused path runs it (agents/lwf.py: taped forward, ONE launch of ops.ce_kd_blend, backward_taped) against
the reference's statements (agents/lwf.py:36-48 of the reference) written over model.forward, criterion, kd_manager.get_kd_loss and
autograd alone, on the same engine, at BASELINE config-1 sizes (cifar10-shaped stream, batch 10, SGD 0.1; MI355X).

  python scripts/lwf_step_ab.py [--out FILE]             # timing: both sides in one process, alternating A/B/A/B, 100 warm-up + 500
                                                         # timed steps per leg, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/fused -o p -- python scripts/lwf_step_ab.py --profile fused
  rocprofv3 --kernel-trace --stats -d OUT/comparator -o p -- python scripts/lwf_step_ab.py --profile comparator
                                                         # one run per side: kernel trace of 600 steps, nothing timed
  python scripts/lwf_step_ab.py --summarise OUT          # launches per step from the two databases

The comparator uses nothing this agent added: the same script runs on a commit that has no agents/lwf.py, where it times the comparator
alone -- that run is the baseline of the commit that adds the agent.  Nothing is asserted about the ratio: the script reports what it
measures, and whether the fused step's median is above the comparator's by more than the comparator's own max / min spread."""
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

import bench  # noqa: E402  (the parameter namespace of the benchmark)

WARMUP, TIMED, ROUNDS, N_BATCHES = 100, 500, 7, 64
CONFIG = "BASELINE config-1 sizes: cifar10-shaped stream, batch 10, Reduced ResNet18, SGD lr 0.1; task_seen = 1 (the teacher runs)"


def have_fused():
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    try:
        name_match.get_agent("LWF")
        return True
    except KeyError:
        return False


def build(side, device, seed=0):
    """A learner after its first task's end: task_seen = 1 and a teacher snapshot.  `fused` is the registered agent; `comparator` a bare
    ContinualLearner (its train_learner is never called: the steps below are the reference's statements)."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.agents.base import ContinualLearner
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    params = bench.make_params(dict(agent="LWF", data="cifar10", batch=10))
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    if side == "fused":
        agent = name_match.get_agent("LWF")(model, opt, params)
    else:
        agent = type("Plain", (ContinualLearner,), dict(train_learner=lambda self, x, y: None))(model, opt, params)
    model.train()
    agent._freeze_long_lived_objects()        # as before_train() does at the first training call
    agent.after_train()                       # base.py:90-91: params.agent == 'LWF' takes the teacher's snapshot
    assert agent.task_seen == 1 and agent.kd_manager.teacher_model is not None
    rng = np.random.default_rng(seed + 1000)
    batches = [(torch.from_numpy(rng.random((params.batch, 3, 32, 32), dtype=np.float32)).to(device),
                torch.from_numpy(rng.integers(0, 10, params.batch).astype(np.int64)).to(device)) for _ in range(N_BATCHES)]
    return agent, batches


def comparator_step(agent, x, y):
    """agents/lwf.py:36-48 of the reference over what every commit exports."""
    from ocl_amd.loss import unit_gradient
    logits = agent.forward(x)
    loss_old = agent.kd_manager.get_kd_loss(logits, x)
    loss_new = agent.criterion(logits, y)
    loss = 1 / (agent.task_seen + 1) * loss_new + (1 - 1 / (agent.task_seen + 1)) * loss_old
    agent.opt.zero_grad()
    loss.backward(unit_gradient(loss))
    agent.opt.step()


def run_leg(side, agent, batches, n_steps, start_weights):
    """n_steps from the given weights and the teacher the learner holds; returns seconds per step."""
    with torch.no_grad():
        agent.model.flat_params().copy_(start_weights)
    step = (lambda x, y: agent._step(x, y, None)) if side == "fused" else (lambda x, y: comparator_step(agent, x, y))
    with agent.model.same_weights():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            step(*batches[i % len(batches)])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_steps


def timing(device, out):
    sides = ("fused", "comparator") if have_fused() else ("comparator",)
    built = {side: build(side, device) for side in sides}
    start = built[sides[0]][0].model.flat_params().clone()
    for side in sides:
        built[side][0].kd_manager.teacher_model.copy_(start)
        run_leg(side, *built[side], WARMUP, start)
    ms = {side: [] for side in sides}
    for r in range(ROUNDS):
        for side in sides:
            ms[side].append(run_leg(side, *built[side], TIMED, start) * 1e3)
    lines = ["lwf_step_ab: %s, torch %s, %d warm-up + %d timed steps per leg, %d legs per side%s in one process"
             % (torch.cuda.get_device_name(device), torch.__version__, WARMUP, TIMED, ROUNDS, " alternating fused / comparator" if len(sides) == 2 else ""),
             "%s; %d parameters" % (CONFIG, start.numel())]
    for side in sides:
        v = ms[side]
        lines.append("  %-10s  ms/step median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
                     % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
    if len(sides) == 2:
        f, c = statistics.median(ms["fused"]), statistics.median(ms["comparator"])
        spread = max(ms["comparator"]) / min(ms["comparator"])
        lines.append("  fused / comparator = %.3f  (%.4f ms per step %s); the comparator's own max / min spread %.3f" % (f / c, abs(c - f), "saved" if f <= c else "LOST", spread))
        lines.append("the fused step's median is not above the comparator's by more than the comparator's spread: %s" % ("yes" if f <= c * spread else "NO"))
        # the two sides compute the same step: one step from the same weights, teacher and batch
        w = {}
        for side in sides:
            run_leg(side, *built[side], 1, start)
            w[side] = built[side][0].model.flat_params().double() - start.double()
        lines.append("one step from the same state: update difference %.2e norm-wise"
                     % float((w["fused"] - w["comparator"]).norm() / w["comparator"].norm()))
    else:
        lines.append("(this commit has no LWF agent: the comparator alone, the baseline of the commit that adds it)")
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def profile(side, device):
    agent, batches = build(side, device)
    start = agent.model.flat_params().clone()
    run_leg(side, agent, batches, WARMUP + TIMED, start)
    print("profiled %s: %d steps" % (side, WARMUP + TIMED))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(out, steps=WARMUP + TIMED):
    print("rocprofv3 --kernel-trace --stats, one run per side: %d steps each (plus the set-up's launches, the same on both sides)" % steps)
    sides = [s for s in ("fused", "comparator") if os.path.isdir(os.path.join(out, s))]
    st = {side: kernel_stats(os.path.join(out, side)) for side in sides}
    total = {side: sum(v[0] for v in st[side].values()) for side in st}
    for side in sides:
        print("  %-10s  %d kernel launches in all: %.2f per step" % (side, total[side], total[side] / steps))
    if len(sides) == 2:
        for side, other_side in (("fused", "comparator"), ("comparator", "fused")):
            only = {k: v for k, v in st[side].items() if st[other_side].get(k, (0,))[0] != v[0]}
            print("  %s: kernels whose launch count differs from the other side's:" % side)
            for k, v in sorted(only.items(), key=lambda kv: -kv[1][0]):
                other = st[other_side].get(k, (0,))[0]
                print("    %6d calls (other side %6d)  %+7.2f per step  avg %8.1f ns  min %7d  max %7d  %s"
                      % (v[0], other, (v[0] - other) / steps, v[1], v[2], v[3], k[:110]))
        print("  launches per step: fused %.2f, comparator %.2f (difference %.2f)"
              % (total["fused"] / steps, total["comparator"] / steps, (total["comparator"] - total["fused"]) / steps))
    for side in sides:
        for k, v in sorted(st[side].items()):
            if "ce_kd_blend" in k or "kd_kernel" in k or "ce_kernel" in k or "pack" in k.lower():
                print("  %-10s %s: %d calls, avg %.2f us (min %.2f, max %.2f)" % (side, k.split("(")[0][:90], v[0], v[1] / 1e3, v[2] / 1e3, v[3] / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", metavar="SIDE", choices=("fused", "comparator"))
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--out", metavar="FILE", help="also write the timing report to FILE")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("lwf_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile, device)
        return 0
    return timing(device, args.out)


if __name__ == "__main__":
    sys.exit(main())
