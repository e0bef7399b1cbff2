#!/usr/bin/env python
"""--error_analysis True: evaluate() after the last task of a cifar100-shaped stream (10 test loaders x 1000 images, test_batch 128: 8
batches per loader, the last of 104 rows; 100 logit columns; task_seen = 10, so nine loaders are old tasks' and the last the new task's)
in three legs on the same ER learner and the same loaders:

  off         params.error_analysis False: evaluate() as it was before the flag existed
  fused       error_analysis.ErrorAnalysis: ONE ops.row_argmax_groupsum launch per batch and one per evaluate, one copy per loader
  comparator  `_force_torch_error_analysis`, error_analysis.TorchErrorAnalysis: the reference's statements (agents/base.py:182-205,
              :217-220 of the reference: one .item() per predicted label, one (wrong == i).sum().item() per class of the comparison set, a
              column gather with mean().item()) on the engine's logits

  python scripts/error_analysis_ab.py [--out FILE]      # timing: the legs interleaved off / fused / comparator in one process, 1 warm-up +
                                                         # 7 timed evaluates per leg, host clock (evaluate() ends on a host read); then
                                                         # the kernel alone at n = 128, c = 100: 2000 launches between two events
  rocprofv3 --kernel-trace --stats -d OUT -o p -- python scripts/error_analysis_ab.py --profile
                                                         # kernel trace of 8 fused evaluates, nothing timed
  python scripts/error_analysis_ab.py --summarise OUT   # the kernel's own duration from that database

Nothing is asserted: the script reports what it measures, whether the fused median is below the comparator's by more than the
comparator's own max / min spread, and fused - off."""
import argparse
import contextlib
import glob
import io
import os
import sqlite3
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the parameter namespace of the benchmark)

ROUNDS, N_TASKS, PER_LOADER, TEST_BATCH = 7, 10, 1000, 128
LEGS = ("off", "fused", "comparator")
LISTS = ("error_list", "new_class_score", "old_class_score", "fc_norm_new", "fc_norm_old", "bias_norm_new", "bias_norm_old")
CONFIG = ("cifar100-shaped stream after its last task: %d loaders x %d images, test_batch %d, 100 columns, Reduced ResNet18, ER"
          % (N_TASKS, PER_LOADER, TEST_BATCH))


def build(device, seed=0):
    """An ER learner after its tenth task (ten classes per task) and the ten test loaders."""
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.data import setup_test_loader
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    params = bench.make_params(dict(agent="ER", data="cifar100", test_batch=TEST_BATCH, mem_size=1000))
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent("ER")(model, opt, params)
    agent.old_labels = list(range(10 * N_TASKS))
    agent.new_labels_zombie = list(range(10 * (N_TASKS - 1), 10 * N_TASKS))
    agent.class_task_map = {c: c // 10 for c in range(10 * N_TASKS)}
    agent.task_seen = N_TASKS
    rng = np.random.default_rng(seed + 1000)
    tests = [(rng.integers(0, 256, (PER_LOADER, 32, 32, 3), dtype=np.uint8), rng.integers(10 * t, 10 * t + 10, PER_LOADER).astype(np.int64))
             for t in range(N_TASKS)]
    return agent, setup_test_loader(tests, params)


def set_leg(agent, leg):
    agent.params.error_analysis = leg != "off"
    agent._force_torch_error_analysis = leg == "comparator"
    for k in LISTS:
        del getattr(agent, k)[:]            # (every evaluate prints the lists: they do not grow from leg to leg)


def one_evaluate(agent, loaders, leg, seed=7):
    """Milliseconds of one evaluate() of the leg, from the same host RNG state (the loaders shuffle); what it printed is dropped."""
    set_leg(agent, leg)
    torch.manual_seed(seed)
    torch.cuda.synchronize()
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        acc = agent.evaluate(loaders)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return ms, acc


def counters():
    """Wraps the op, the copy and the comparator's host read: [launches, copies, item reads]."""
    from ocl_amd import ops, error_analysis as EA
    n = [0, 0, 0]
    inner_op, inner_copy, inner_item = ops.row_argmax_groupsum, EA.to_host, EA.item

    def op(*a, **k):
        n[0] += 1
        return inner_op(*a, **k)

    def to_host(t):
        n[1] += 1
        return inner_copy(t)

    def item(t):
        n[2] += 1
        return inner_item(t)

    ops.row_argmax_groupsum, EA.to_host, EA.item = op, to_host, item
    return n


def kernel_alone(device, n=128, c=100, launches=2000):
    """Microseconds per ops.row_argmax_groupsum call at [n, c], back to back on one stream between two events (launch gaps included: an
    upper bound on the kernel's own time), through the Python wrapper and through the C entry point alone."""
    from ocl_amd import ops, ffi
    x = torch.randn(n, c, device=device)
    group = torch.from_numpy((np.arange(c) >= 90).astype(np.int32)).to(device)
    am, sm = torch.empty(n, dtype=torch.int64, device=device), torch.empty(n, dtype=torch.float64, device=device)
    lib, stream = ffi.lib(), ffi.stream()
    px, pg, pa, ps = ffi.ptr(x), ffi.ptr(group), ffi.ptr(am), ffi.ptr(sm)
    out = []
    for call in (lambda: ops.row_argmax_groupsum(x, group, 0, argmax_out=am, sum_out=sm), lambda: lib.ocl_row_argmax_groupsum(px, n, c, pg, 0, pa, ps, stream)):
        for _ in range(200):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return out


def timing(device, out):
    agent, loaders = build(device)
    n = counters()
    per = {}
    accs = {}
    for leg in LEGS:                                    # warm-up, and the counts per evaluate
        n[:] = [0, 0, 0]
        _, accs[leg] = one_evaluate(agent, loaders, leg)
        per[leg] = list(n)
    ms = {leg: [] for leg in LEGS}
    for r in range(ROUNDS):
        for leg in LEGS:
            ms[leg].append(one_evaluate(agent, loaders, leg)[0])
    batches = sum(len(l) for l in loaders)
    lines = ["error_analysis_ab: %s, torch %s, 1 warm-up + %d timed evaluates per leg, interleaved off / fused / comparator in one process"
             % (torch.cuda.get_device_name(device), torch.__version__, ROUNDS),
             "%s; %d test batches per evaluate" % (CONFIG, batches)]
    for leg in LEGS:
        v = ms[leg]
        syncs = len(loaders) if leg == "off" else per[leg][1] + per[leg][2]
        lines.append("  %-10s  ms/evaluate median %.3f  min %.3f  max %.3f  max/min %.3f   row_argmax_groupsum launches %d  host synchronisations %d%s   legs %s"
                     % (leg, statistics.median(v), min(v), max(v), max(v) / min(v), per[leg][0], syncs,
                        " (one .cpu() per loader)" if leg == "off" else " (%d copies, %d .item() reads)" % (per[leg][1], per[leg][2]),
                        " ".join("%.3f" % t for t in v)))
    a, f, c = (statistics.median(ms[leg]) for leg in LEGS)
    spread = max(ms["comparator"]) / min(ms["comparator"])
    lines.append("  fused / comparator = %.3f  (%.3f ms per evaluate %s); the comparator's own max / min spread %.3f" % (f / c, abs(c - f), "saved" if f <= c else "LOST", spread))
    lines.append("the fused median is below the comparator's by more than the comparator's spread: %s" % ("yes" if f * spread < c else "NO"))
    lines.append("  fused - off = %+.3f ms per evaluate = %+.2f us per test batch (%d launches and %d copies more than off, %d torch.max / compare / sum "
                 "launches and %d stacked copies fewer)" % (f - a, (f - a) * 1e3 / batches, per["fused"][0], per["fused"][1], 3 * batches, len(loaders)))
    lines.append("  acc_array: fused == off bit for bit: %s; comparator == off: %s"
                 % (accs["fused"].tobytes() == accs["off"].tobytes(), accs["comparator"].tobytes() == accs["off"].tobytes()))
    wrapped, bare = kernel_alone(device)
    lines.append("  the kernel alone at n = 128, c = 100 (32 workgroups of 4 waves), 2000 calls back to back between two events: %.2f us per call through "
                 "ops.row_argmax_groupsum, %.2f us through the C entry point" % (wrapped, bare))
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def profile(device):
    agent, loaders = build(device)
    for _ in range(ROUNDS + 1):
        one_evaluate(agent, loaders, "fused")
    print("profiled fused: %d evaluates" % (ROUNDS + 1))


def summarise(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    print("rocprofv3 --kernel-trace --stats: %d fused evaluates" % (ROUNDS + 1))
    for name, calls, avg, lo, hi in sorted(rows):
        if "row_argmax_groupsum" in name:
            print("  %s: %d calls (%.1f per evaluate), avg %.2f us (min %.2f, max %.2f)" % (name.split("(")[0][:90], calls, calls / (ROUNDS + 1), avg / 1e3, lo / 1e3, hi / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--out", metavar="FILE", help="also write the timing report to FILE")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("error_analysis_ab.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = os.path.abspath(args.out) if args.out else None
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                        # evaluate() writes its `confusion` file into the working directory
        try:
            if args.profile:
                profile(device)
                return 0
            return timing(device, out)
        finally:
            os.chdir(ROOT)


if __name__ == "__main__":
    sys.exit(main())
