#!/usr/bin/env python
"""--agent GDUMB: the memory-training step (agents/gdumb.py:78-83: forward, CE, backward, global-norm clip, SGD step) with the fused clip
(ops.clip_grad_norm_: two launches on the flat gradient array) against torch.nn.utils.clip_grad_norm_ over the 62 p.grad views, on the
same engine, at the sizes of the reference README's line (cifar100, mem_size 1000 full and balanced, batch 10, clip 10, SGD 0.1; MI355X).

  python scripts/gdumb_step_ab.py                        # timing: both sides in one process, alternating A/B/A/B, 100 warm-up + 500
                                                         # timed memory steps per leg, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/fused -o p -- python scripts/gdumb_step_ab.py --profile fused
  rocprofv3 --kernel-trace --stats -d OUT/torch -o p -- python scripts/gdumb_step_ab.py --profile torch
                                                         # one run per side: kernel trace of fill + 600 steps, nothing timed
  python scripts/gdumb_step_ab.py --summarise OUT        # launches per step of the clip from the two databases

Every leg starts from a fresh network (as train_mem does) built outside the timed window and steps through whole epochs of the memory;
only `_mem_step` calls are timed.  The comparator is the agent's private `_force_torch_clip` attribute (the product has no switch for
it).  Nothing is asserted about the ratio: the script reports what it measures."""
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

WARMUP_EPOCHS, TIMED_EPOCHS, ROUNDS = 1, 5, 5
CONFIG = "reference README line: GDUMB, cifar100, mem_size 1000 (full, 10 per class), batch 10, clip 10, SGD lr 0.1"
SIDES = ("fused", "torch")


def build(side, device, seed=0):
    """The GDumb agent with its memory filled by the greedy sampler from a stream of 20 images per class."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.setup_elements import setup_architecture, setup_opt, n_classes, input_size_match
    from ocl_amd.gdumb_memory import GdumbMemory
    params = bench.make_params(dict(agent="GDUMB", data="cifar100", mem_size=1000, batch=10, mem_epoch=30, clip=10.0, minlr=0.0005))
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent("GDUMB")(model, opt, params)
    agent._force_torch_clip = side == "torch"
    hw, ncls = input_size_match[params.data][1], n_classes[params.data]
    rng = np.random.default_rng(seed + 1000)
    agent.memory = GdumbMemory(params.mem_size, input_size_match[params.data], device, batch=params.batch)
    ys = rng.permutation(np.repeat(np.arange(ncls, dtype=np.int64), 20))
    for s in range(0, len(ys), params.batch):
        xs = torch.from_numpy(rng.random((params.batch, 3, hw, hw), dtype=np.float32)).to(device)
        agent.memory.update(xs, ys[s:s + params.batch])
    assert sum(agent.memory.balancer.mem_c.values()) == params.mem_size
    return params, agent


def epochs(agent, n_epochs, rng):
    """Mini-batches of n_epochs passes over the memory, gathered before the timed window."""
    from ocl_amd import ops
    slots, _ = agent.memory.order()
    bs = agent.params.batch
    out = []
    for _ in range(n_epochs):
        order = slots[rng.permutation(len(slots))]
        mem_x, mem_y = ops.gather_pair(agent.memory.img, agent.memory.label, torch.from_numpy(order))
        out += [(mem_x[bs * j:bs * (j + 1)], mem_y[bs * j:bs * (j + 1)]) for j in range(len(slots) // bs)]
    return out


def run_leg(agent, n_epochs, rng):
    """A fresh network, then n_epochs of memory steps; returns seconds per step."""
    agent._fresh_learner()
    agent.model.train()
    batches = epochs(agent, n_epochs, rng)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, y in batches:
        agent._mem_step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(batches), len(batches)


def timing(device):
    sides = {side: build(side, device) for side in SIDES}
    for side in SIDES:
        _, steps = run_leg(sides[side][1], WARMUP_EPOCHS, np.random.default_rng(1))
    warm = steps
    ms = {side: [] for side in SIDES}
    for r in range(ROUNDS):
        for side in SIDES:
            torch.manual_seed(10 + r)                     # both sides of a round start from the same fresh weights and see the same batches
            sec, steps = run_leg(sides[side][1], TIMED_EPOCHS, np.random.default_rng(10 + r))
            ms[side].append(sec * 1e3)
    print("gdumb_step_ab: %s, torch %s, %d warm-up + %d timed memory steps per leg, %d legs per side alternating fused / torch in one process"
          % (torch.cuda.get_device_name(device), torch.__version__, warm, steps, ROUNDS))
    print("%s; %d parameters" % (CONFIG, sides["fused"][1].model.flat_params().numel()))
    for side in SIDES:
        v = ms[side]
        print("  %-5s  ms/step median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
              % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
    f, s = statistics.median(ms["fused"]), statistics.median(ms["torch"])
    print("  fused / torch = %.3f  (%.4f ms per step %s)" % (f / s, abs(s - f), "saved" if f <= s else "LOST"))
    # how many of a leg's steps clip (untimed: the debug log fetches the info words every step)
    from ocl_amd import debug
    torch.manual_seed(10)
    debug.LOG = []
    try:
        run_leg(sides["fused"][1], TIMED_EPOCHS, np.random.default_rng(10))
        ev = [e for t, e in debug.LOG if t == "gdumb_clip"]
    finally:
        debug.LOG = None
    norms = [e["total_norm"] for e in ev]
    print("  census of one fused leg (untimed): %d of %d steps clip; total norm min %.3f median %.3f max %.3f"
          % (sum(e["clipped"] for e in ev), len(ev), min(norms), statistics.median(norms), max(norms)))
    print("the fused clip is not slower than torch's statements on the same engine: %s" % ("yes" if f <= s else "NO"))
    return 0


def profile(side, device):
    params, agent = build(side, device)
    _, steps = run_leg(agent, WARMUP_EPOCHS + TIMED_EPOCHS, np.random.default_rng(1))
    print("profiled %s: %d steps" % (side, steps))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(out, steps=(WARMUP_EPOCHS + TIMED_EPOCHS) * 100):
    print("rocprofv3 --kernel-trace --stats, one run per side: memory fill + %d memory steps each" % steps)
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
    mine = {k: v for k, v in st["fused"].items() if "clip_" in k}
    assert len(mine) == 2 and not any("clip_" in k for k in st["torch"]), sorted(mine)
    calls = sum(v[0] for v in mine.values())
    print("  clip launches per step: fused %.2f (clip_sumsq_kernel + clip_apply_kernel: %d calls / %d steps), torch %.2f (all launches of the "
          "torch run minus all launches of the fused run, per step, plus the fused side's two)"
          % (calls / steps, calls, steps, (total["torch"] - total["fused"]) / steps + calls / steps))
    n = 1109240
    for k, v in sorted(mine.items()):
        print("  %s: avg %.2f us per call (min %.2f, max %.2f); %d elements, 4 B read each (the apply kernel reads and writes 4 B more per "
              "element on a step that clips)" % (k.split("(")[0], v[1] / 1e3, v[2] / 1e3, v[3] / 1e3, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", metavar="SIDE", choices=SIDES)
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("gdumb_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile, device)
        return 0
    return timing(device)


if __name__ == "__main__":
    sys.exit(main())
