#!/usr/bin/env python
"""--optimizer Adam: the fused optimiser (optim.FusedAdam, one adam_flat_kernel launch per step) against stock torch.optim.Adam over the
model's 62 parameter views, on the ER agent at BASELINE configs[0] sizes and the SCR agent at configs[1] sizes (MI355X).

  python scripts/adam_step_ab.py                         # timing: both sides in one process, alternating A/B/A/B, 20 warm-up + 200
                                                         # timed steps per leg, host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT/er_fused -o p -- python scripts/adam_step_ab.py --profile er fused
  ...                                                    # one run per (config, side): kernel trace of fill + 220 steps, nothing timed
  python scripts/adam_step_ab.py --summarise OUT         # launches per step and adam_flat_kernel's time from the four databases

The stock optimiser is constructed here (the product has no switch for it): torch.optim.Adam(model.parameters(), lr, weight_decay)."""
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

import bench  # noqa: E402  (the workloads' sizes and the synthetic stream of the benchmark)

WARMUP, STEPS, ROUNDS = 20, 200, 5
LR = 1e-3
CONFIGS = {"er": "BASELINE configs[0]: ER random/random, cifar10 shape, mem_size 1000, batch 10 + 10",
           "scr": "BASELINE configs[1]: SCR random/random, cifar100 shape, mem_size 5000, eps_mem_batch 100"}


def build(workload, side, device, seed=0):
    """bench.build_agent with --optimizer Adam: the agent, its replay memory filled, the optimiser of `side`."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.optim import FusedAdam
    from ocl_amd.setup_elements import setup_architecture, setup_opt, n_classes, input_size_match
    params = bench.make_params(dict(bench.WORKLOADS[workload], optimizer="Adam", learning_rate=LR))
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    model = setup_architecture(params).to(device)
    if side == "fused":
        opt = setup_opt("Adam", model, LR, params.weight_decay)
        assert type(opt) is FusedAdam
    else:
        opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=params.weight_decay)
    agent = name_match.agents[params.agent](model, opt, params)
    hw, ncls = input_size_match[params.data][1], n_classes[params.data]
    rng = np.random.default_rng(seed + 1000)
    for s in range(0, params.mem_size, 500):
        n = min(500, params.mem_size - s)
        ys = rng.integers(0, ncls, n).astype(np.int64)
        xs = torch.from_numpy(rng.random((n, 3, hw, hw), dtype=np.float32)).to(device)
        agent.buffer.update(xs, torch.from_numpy(ys).to(device), y_host=ys)
    return params, model, agent, hw, ncls


def stream(steps, bs, hw, ncls, seed, device):
    x, y = bench.synth_u8(steps * bs, hw, ncls, seed)
    return torch.from_numpy(x).to(device), y


def timing(device):
    print("adam_step_ab: %s, torch %s, %d warm-up + %d timed steps per leg, %d legs per side alternating fused / stock in one process"
          % (torch.cuda.get_device_name(device), torch.__version__, WARMUP, STEPS, ROUNDS))
    ok = True
    for workload in ("er", "scr"):
        sides = {}
        for side in ("fused", "stock"):
            params, model, agent, hw, ncls = build(workload, side, device)
            sides[side] = (params, model, agent)
        bs = params.batch
        warm = stream(WARMUP, bs, hw, ncls, 1, device)
        for side in ("fused", "stock"):
            sides[side][2].train_learner(*warm)
        torch.cuda.synchronize()
        ms = {"fused": [], "stock": []}
        for r in range(ROUNDS):
            timed = stream(STEPS, bs, hw, ncls, 10 + r, device)
            for side in ("fused", "stock"):
                agent = sides[side][2]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                agent.train_learner(*timed)          # exactly STEPS iterations (drop_last, len = STEPS * batch)
                torch.cuda.synchronize()
                ms[side].append((time.perf_counter() - t0) / STEPS * 1e3)
        n = sides["fused"][1].flat_params().numel()
        print("%s  (%s; %d parameters)" % (workload.upper(), CONFIGS[workload], n))
        for side in ("fused", "stock"):
            v = ms[side]
            print("  %-5s  ms/step median %.4f  min %.4f  max %.4f  max/min %.3f   legs %s"
                  % (side, statistics.median(v), min(v), max(v), max(v) / min(v), " ".join("%.4f" % t for t in v)))
        f, s = statistics.median(ms["fused"]), statistics.median(ms["stock"])
        print("  fused / stock = %.3f  (%.4f ms per step %s)" % (f / s, abs(s - f), "saved" if f <= s else "LOST"))
        assert sides["fused"][2].opt.step_count == WARMUP + ROUNDS * STEPS
        ok = ok and f <= s
        del sides
    print("FusedAdam is not slower than torch.optim.Adam on either config: %s" % ("yes" if ok else "NO"))
    return 0 if ok else 1


def profile(workload, side, device):
    params, model, agent, hw, ncls = build(workload, side, device)
    agent.train_learner(*stream(WARMUP + STEPS, params.batch, hw, ncls, 1, device))
    torch.cuda.synchronize()
    print("profiled %s %s: %d steps" % (workload, side, WARMUP + STEPS))


def kernel_stats(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    return {r[0]: r[1:] for r in rows}


def summarise(out):
    steps = WARMUP + STEPS
    hbm_peak = 8.0e12       # MI355X HBM3E peak, bytes/s
    print("rocprofv3 --kernel-trace --stats, one run per (config, side): replay-memory fill + %d steps each" % steps)
    for workload in ("er", "scr"):
        st = {side: kernel_stats(os.path.join(out, "%s_%s" % (workload, side))) for side in ("fused", "stock")}
        total = {side: sum(v[0] for v in st[side].values()) for side in st}
        print("%s  (%s)" % (workload.upper(), CONFIGS[workload]))
        for side in ("fused", "stock"):
            only = {k: v for k, v in st[side].items() if k not in st["stock" if side == "fused" else "fused"] or
                    st["stock" if side == "fused" else "fused"][k][0] != v[0]}
            print("  %-5s  %d kernel launches in all; kernels whose launch count differs from the other side:" % (side, total[side]))
            for k, v in sorted(only.items(), key=lambda kv: -kv[1][0]):
                other = st["stock" if side == "fused" else "fused"].get(k, (0,))[0]
                print("    %6d calls (other side %6d)  %7.2f per step  avg %8.1f ns  min %7d  max %7d  %s"
                      % (v[0], other, (v[0] - other) / steps, v[1], v[2], v[3], k[:110]))
        adam = [(k, v) for k, v in st["fused"].items() if "adam_flat_kernel" in k]
        assert len(adam) == 1 and not any("adam_flat_kernel" in k for k in st["stock"])
        calls, avg, mn, mx = adam[0][1]
        n = {"er": 1094750, "scr": 1155608}[workload]
        print("  optimiser launches per step: fused %.2f (adam_flat_kernel: %d calls / %d steps), stock %.2f (all launches of the stock run minus all "
              "launches of the fused run, per step, plus the fused side's one)" % (calls / steps, calls, steps, (total["stock"] - total["fused"]) / steps + calls / steps))
        bw = 28.0 * n / (avg * 1e-9)
        print("  adam_flat_kernel: avg %.2f us per call (min %.2f, max %.2f); 28 B x %d elements = %.1f MB per call -> %.2f TB/s achieved (%.0f %% of the %.0f TB/s "
              "HBM peak)" % (avg / 1e3, mn / 1e3, mx / 1e3, n, 28.0 * n / 1e6, bw / 1e12, 100 * bw / hbm_peak, hbm_peak / 1e12))
        print("  -> %s" % ("bandwidth-bound at this size, not launch-bound: the kernel moves its bytes at more than half of the HBM peak (%.0f %% of the 6.3 TB/s a float4 copy "
                           "reaches; p, m and v, 3 x %.1f MB, fit the Infinity Cache between two steps, so this is not a pure HBM rate)" % (100 * bw / 6.3e12, 4.0 * n / 1e6) if bw > 0.5 * hbm_peak else
                           "not at the HBM roof at this size: %.1f MB in %.1f us is latency / launch-shaped (a few trips per wave over a grid of at most 2048 "
                           "workgroups); the step gains from the launches and host work removed, not from the kernel's rate" % (28.0 * n / 1e6, avg / 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", nargs=2, metavar=("CONFIG", "SIDE"))
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile:
        profile(args.profile[0], args.profile[1], device)
        return 0
    return timing(device)


if __name__ == "__main__":
    sys.exit(main())
