#!/usr/bin/env python
"""--agent ICARL: one iteration of the last task of split CIFAR-100 (task_seen = 9: 90 old columns, 100 seen; 10 stream rows + 10 memory
rows drawn from a full memory of 5000; the student's pass, the teacher's pass, the BCE against the distilled target, backward, SGD
step, reservoir update) as the fused path runs it (agents/icarl.py: taped forward, ONE launch of ops.bce_distill, backward_taped)
against `Icarl._force_autograd`, the reference's statements (agents/icarl.py:46-63 of the reference: one-hot scatter, cat with zeros,
sigmoid, one column copy per old class, F.binary_cross_entropy_with_logits, autograd) on the same engine, at the sizes of the
reference README's iCaRL line (cifar100-shaped stream, batch 10, mem_size 5000, SGD 0.1; MI355X).

  python scripts/icarl_step_ab.py [--out FILE]           # timing: both sides in one process, alternating A/B/A/B, 100 warm-up + 500
                                                         # timed iterations per leg, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/fused -o p -- python scripts/icarl_step_ab.py --profile fused
  rocprofv3 --kernel-trace --stats -d OUT/comparator -o p -- python scripts/icarl_step_ab.py --profile comparator
                                                         # one run per side: kernel trace of 600 iterations, nothing timed
  python scripts/icarl_step_ab.py --summarise OUT        # launches per iteration from the two databases

Every leg starts from the same weights, teacher, memory and host RNG state, and its exclusion list starts empty, as a train_learner
call's does.  Nothing is asserted about the ratio: the script reports what it measures, and whether the fused median is below the
comparator's by more than the comparator's own max / min spread."""
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
TASK_SEEN, MEM = 9, 5000
CONFIG = ("the reference README's iCaRL line: cifar100-shaped stream, batch 10, mem_size %d (full), Reduced ResNet18, SGD lr 0.1; task_seen = %d "
          "(n_old = 90, n_cls = 100; 10 stream + 10 memory rows)" % (MEM, TASK_SEEN))


def seed_host(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def build(side, device, seed=0):
    """An Icarl learner inside its tenth task: nine tasks of ten classes seen, a teacher snapshot, a full memory of old-class images."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    params = bench.make_params(dict(agent="ICARL", data="cifar100", batch=10, mem_size=MEM))
    seed_host(seed)
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent("ICARL")(model, opt, params)
    agent._force_autograd = side == "comparator"
    model.train()
    agent._freeze_long_lived_objects()        # as before_train() does at the first training call
    agent.old_labels = list(range(10 * TASK_SEEN))
    agent.new_labels = list(range(10 * TASK_SEEN, 10 * TASK_SEEN + 10))
    agent.task_seen = TASK_SEEN
    agent.prev.update_teacher(model)
    rng = np.random.default_rng(seed + 1000)
    buf = agent.buffer
    buf.buffer_img.copy_(torch.from_numpy(rng.random(tuple(buf.buffer_img.shape), dtype=np.float32)))
    labels = rng.integers(0, 10 * TASK_SEEN, MEM).astype(np.int64)
    buf.buffer_label.copy_(torch.from_numpy(labels))
    buf.label_host[:] = labels
    batches = []
    for _ in range(N_BATCHES):
        y = rng.integers(10 * TASK_SEEN, 10 * TASK_SEEN + 10, params.batch).astype(np.int64)
        batches.append((torch.from_numpy(rng.random((params.batch, 3, 32, 32), dtype=np.float32)).to(device), torch.from_numpy(y).to(device), y))
    return agent, batches


def run_leg(agent, batches, n_steps, start_weights, seed=7):
    """n_steps iterations of update_representation's loop body from the given weights, the teacher the learner holds, a full memory whose
    stream counter stands at nine tasks, and a fresh exclusion list; returns seconds per iteration."""
    with torch.no_grad():
        agent.model.flat_params().copy_(start_weights)
    agent.buffer.current_index, agent.buffer.n_seen_so_far = MEM, MEM * TASK_SEEN
    seed_host(seed)
    updated_idx = []
    with agent.model.same_weights():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            x, y, y_host = batches[i % len(batches)]
            agent._step(x, y, y_host, updated_idx)
            updated_idx += agent.buffer.update(x, y, y_host=y_host)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_steps


def timing(device, out):
    sides = ("fused", "comparator")
    built = {side: build(side, device) for side in sides}
    start = built[sides[0]][0].model.flat_params().clone()
    for side in sides:
        built[side][0].prev.teacher_model.copy_(start)
        run_leg(*built[side], WARMUP, start)
    ms = {side: [] for side in sides}
    for r in range(ROUNDS):
        for side in sides:
            ms[side].append(run_leg(*built[side], TIMED, start) * 1e3)
    lines = ["icarl_step_ab: %s, torch %s, %d warm-up + %d timed iterations per leg, %d legs per side alternating fused / comparator in one process"
             % (torch.cuda.get_device_name(device), torch.__version__, WARMUP, TIMED, ROUNDS),
             "%s; %d parameters" % (CONFIG, start.numel())]
    for side in sides:
        v = ms[side]
        lines.append("  %-10s  ms/iteration median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
                     % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
    f, c = statistics.median(ms["fused"]), statistics.median(ms["comparator"])
    spread = max(ms["comparator"]) / min(ms["comparator"])
    lines.append("  fused / comparator = %.3f  (%.4f ms per iteration %s); the comparator's own max / min spread %.3f" % (f / c, abs(c - f), "saved" if f <= c else "LOST", spread))
    lines.append("the fused median is below the comparator's by more than the comparator's spread: %s" % ("yes" if f * spread < c else "NO"))
    # the two sides compute the same step: one iteration from the same weights, teacher, memory, batch and RNG state
    w = {}
    for side in sides:
        run_leg(*built[side], 1, start)
        w[side] = built[side][0].model.flat_params().double() - start.double()
    lines.append("one step from the same state: update difference %.2e norm-wise"
                 % float((w["fused"] - w["comparator"]).norm() / w["comparator"].norm()))
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def profile(side, device):
    agent, batches = build(side, device)
    start = agent.model.flat_params().clone()
    run_leg(agent, batches, WARMUP + TIMED, start)
    print("profiled %s: %d iterations" % (side, WARMUP + TIMED))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(out, steps=WARMUP + TIMED):
    print("rocprofv3 --kernel-trace --stats, one run per side: %d iterations each (plus the set-up's launches, the same on both sides)" % steps)
    sides = [s for s in ("fused", "comparator") if os.path.isdir(os.path.join(out, s))]
    st = {side: kernel_stats(os.path.join(out, side)) for side in sides}
    total = {side: sum(v[0] for v in st[side].values()) for side in st}
    for side in sides:
        print("  %-10s  %d kernel launches in all: %.2f per iteration" % (side, total[side], total[side] / steps))
    if len(sides) == 2:
        for side, other_side in (("fused", "comparator"), ("comparator", "fused")):
            only = {k: v for k, v in st[side].items() if st[other_side].get(k, (0,))[0] != v[0]}
            print("  %s: kernels whose launch count differs from the other side's:" % side)
            for k, v in sorted(only.items(), key=lambda kv: -kv[1][0]):
                other = st[other_side].get(k, (0,))[0]
                print("    %6d calls (other side %6d)  %+7.2f per iteration  avg %8.1f ns  min %7d  max %7d  %s"
                      % (v[0], other, (v[0] - other) / steps, v[1], v[2], v[3], k[:110]))
        print("  launches per iteration: fused %.2f, comparator %.2f (difference %.2f)"
              % (total["fused"] / steps, total["comparator"] / steps, (total["comparator"] - total["fused"]) / steps))
    for side in sides:
        for k, v in sorted(st[side].items()):
            if "bce_distill" in k or "pack" in k.lower():
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
        raise SystemExit("icarl_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile, device)
        return 0
    return timing(device, args.out)


if __name__ == "__main__":
    sys.exit(main())
