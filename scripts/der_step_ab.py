#!/usr/bin/env python
"""--agent DER: one DER++ training step from a full memory (two uniform draws, a forward over stream batch + logit-replay batch +
label-replay batch, CE + alpha * MSE against the stored logits + beta * CE, backward, SGD step) as the fused path runs it
(agents/der.py: ONE taped pass of three BatchNorm groups, ONE launch of ops.der_loss, backward_taped) against the same statements over
model.forward per batch, criterion, F.mse_loss, a gather of the stored rows and autograd (`_force_autograd`), on the same engine:
cifar100-shaped 32x32 input, batch 10, eps_mem_batch 10, mem_size 5000 (full), alpha 0.1, beta 0.5, SGD 0.1; MI355X.  Beside the two,
from the same call: ER's merged step (its draw + one taped pass of two groups, 20 images, two CE launches), which shows what the second
replay batch costs.

  python scripts/der_step_ab.py [--out FILE]             # timing: the three sides in one process, alternating, 100 warm-up + 500
                                                         # timed steps per leg, 7 legs each, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/fused -o p -- python scripts/der_step_ab.py --profile fused
  rocprofv3 --kernel-trace --stats -d OUT/comparator -o p -- python scripts/der_step_ab.py --profile comparator
                                                         # one run per side: kernel trace of 600 steps, nothing timed
  python scripts/der_step_ab.py --summarise OUT [--out FILE]   # launches per step and the loss kernels' own times (appended to FILE)

Nothing is asserted about the ratio: the script reports what it measures, and whether the fused step's median lies below the
comparator's by more than the comparator's own max / min spread."""
import argparse
import glob
import os
import random
import re
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
CONFIG = "cifar100-shaped 32x32 input, batch 10, eps_mem_batch 10, mem_size 5000 (full), alpha 0.1, beta 0.5, Reduced ResNet18, SGD lr 0.1"
SIDES = ("fused", "comparator", "er")


def build(side, device, seed=0):
    """A learner in front of a full memory.  `fused` is the registered agent, `comparator` the same agent with `_force_autograd`, `er`
    the ER agent (random retrieval, reservoir update) over a memory with the same images and labels."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    from ocl_amd.utils import AverageMeter
    params = bench.make_params(dict(agent="ER" if side == "er" else "DER", data="cifar100", batch=10, eps_mem_batch=10, mem_size=5000,
                                    der_alpha=0.1, der_beta=0.5))
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent(params.agent)(model, opt, params)
    agent._force_autograd = side == "comparator"
    model.train()
    agent._freeze_long_lived_objects()        # as before_train() does at the first training call
    rng = np.random.default_rng(seed + 1000)
    b = agent.buffer
    b.buffer_img.copy_(torch.from_numpy(rng.random(tuple(b.buffer_img.shape), dtype=np.float32)))
    b.buffer_label.copy_(torch.from_numpy(rng.integers(0, 100, params.mem_size).astype(np.int64)))
    b.sync_host_labels()
    b.current_index = b.n_seen_so_far = params.mem_size
    if side != "er":
        b.buffer_logits.copy_(torch.from_numpy(rng.standard_normal(tuple(b.buffer_logits.shape)).astype(np.float32) * 0.3))
    batches = [(torch.from_numpy(rng.random((params.batch, 3, 32, 32), dtype=np.float32)).to(device),
                torch.from_numpy(rng.integers(0, 100, params.batch).astype(np.int64)).to(device)) for _ in range(N_BATCHES)]
    meters = ((AverageMeter(), AverageMeter()), (AverageMeter(), AverageMeter()))
    if side == "er":
        def step(x, y):
            mem_x, mem_y = agent.buffer.retrieve(x=x, y=y)
            agent._merged_step(x, y, mem_x, mem_y, meters)
    else:
        def step(x, y):
            agent._step(x, y, meters[0])
    return agent, batches, step


def run_leg(agent, batches, step, n_steps, start_weights, seed=0):
    """n_steps from the given weights and the memory the learner holds, the draws from a seeded generator; returns seconds per step."""
    with torch.no_grad():
        agent.model.flat_params().copy_(start_weights)
    np.random.seed(seed)
    with agent.model.same_weights():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            step(*batches[i % len(batches)])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_steps


def timing(device, out):
    built = {side: build(side, device) for side in SIDES}
    start = built["fused"][0].model.flat_params().clone()
    for side in SIDES:
        run_leg(*built[side], WARMUP, start)
    ms = {side: [] for side in SIDES}
    for r in range(ROUNDS):
        for side in SIDES:
            ms[side].append(run_leg(*built[side], TIMED, start) * 1e3)
    lines = ["der_step_ab: %s, torch %s, %d warm-up + %d timed steps per leg, %d legs per side alternating %s in one process"
             % (torch.cuda.get_device_name(device), torch.__version__, WARMUP, TIMED, ROUNDS, " / ".join(SIDES)),
             "%s; %d parameters" % (CONFIG, start.numel())]
    for side in SIDES:
        v = ms[side]
        lines.append("  %-10s  ms/step median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
                     % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
    f, c, e = (statistics.median(ms[side]) for side in SIDES)
    spread = max(ms["comparator"]) / min(ms["comparator"])
    lines.append("  fused / comparator = %.3f  (%.4f ms per step %s); the comparator's own max / min spread %.3f; the fused side's %.3f"
                 % (f / c, abs(c - f), "saved" if f <= c else "LOST", spread, max(ms["fused"]) / min(ms["fused"])))
    lines.append("the fused step's median lies below the comparator's by more than the comparator's spread (a gain): %s" % ("yes" if f * spread < c else "NO"))
    lines.append("  DER++ fused step (30 images, three groups) / ER merged step (20 images, two groups) = %.3f  (%.4f ms for the second replay batch)"
                 % (f / e, f - e))
    # the two sides compute the same step: one step from the same weights, memory, batch and draws
    w = {}
    for side in ("fused", "comparator"):
        run_leg(*built[side], 1, start)
        w[side] = built[side][0].model.flat_params().double() - start.double()
    lines.append("one step from the same state: update difference %.2e norm-wise" % float((w["fused"] - w["comparator"]).norm() / w["comparator"].norm()))
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def profile(side, device):
    agent, batches, step = build(side, device)
    start = agent.model.flat_params().clone()
    run_leg(agent, batches, step, WARMUP + TIMED, start)
    print("profiled %s: %d steps" % (side, WARMUP + TIMED))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(directory, out, steps=WARMUP + TIMED):
    lines = ["rocprofv3 --kernel-trace --stats, one run per side: %d steps each (plus the set-up's launches, the same on both sides)" % steps]
    sides = [s for s in ("fused", "comparator") if os.path.isdir(os.path.join(directory, s))]
    st = {side: kernel_stats(os.path.join(directory, side)) for side in sides}
    total = {side: sum(v[0] for v in st[side].values()) for side in st}
    for side in sides:
        lines.append("  %-10s  %d kernel launches in all: %.2f per step" % (side, total[side], total[side] / steps))
    if len(sides) == 2:
        for side, other_side in (("fused", "comparator"), ("comparator", "fused")):
            only = {k: v for k, v in st[side].items() if st[other_side].get(k, (0,))[0] != v[0]}
            lines.append("  %s: kernels whose launch count differs from the other side's:" % side)
            for k, v in sorted(only.items(), key=lambda kv: -kv[1][0]):
                other = st[other_side].get(k, (0,))[0]
                lines.append("    %6d calls (other side %6d)  %+7.2f per step  avg %8.1f ns  min %7d  max %7d  %s"
                             % (v[0], other, (v[0] - other) / steps, v[1], v[2], v[3], k[:110]))
        lines.append("  launches per step: fused %.2f, comparator %.2f (difference %.2f)"
                     % (total["fused"] / steps, total["comparator"] / steps, (total["comparator"] - total["fused"]) / steps))
    for side in sides:
        for k, v in sorted(st[side].items()):
            if re.search(r"\b(der_loss_kernel|ce_kernel)\b|mse", k):
                lines.append("  %-10s %s: %d calls, avg %.2f us (min %.2f, max %.2f)" % (side, k.split("(")[0][:90], v[0], v[1] / 1e3, v[2] / 1e3, v[3] / 1e3))
    print("\n".join(lines))
    if out:
        with open(out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", metavar="SIDE", choices=("fused", "comparator"))
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--out", metavar="FILE", help="write the timing report to FILE (--summarise: append to it)")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("der_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile, device)
        return 0
    return timing(device, args.out)


if __name__ == "__main__":
    sys.exit(main())
