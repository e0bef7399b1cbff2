#!/usr/bin/env python
"""--data openloris (50 x 50) and core50 (128 x 128): what a step and an evaluate forward cost on the engine, beside the oracle's torch
statements on the same GPU (a same-node comparator: a baseline, not a target), the engine's workspace at the default sizes, and the
float loader kernel beside the uint8 one (profiles/datasets_steps.txt).

  python scripts/datasets_steps.py [--out FILE]        # timing: ER + random retrieval + reservoir, 10 stream + 10 memory rows per step
                                                       # (a task of STEPS batches through train_learner, loader included), and one
                                                       # eval-mode forward of the default --test_batch (128); per leg the median of
                                                       # REPEATS repeats with their max / min; host clock around a synchronised window
  rocprofv3 --kernel-trace --stats -d OUT -o p -- python scripts/datasets_steps.py --profile-loader
                                                       # 300 calls of each loader kernel at 32 x 32, 10 rows: nothing timed by the host
  python scripts/datasets_steps.py --summarise OUT     # the two kernels' times from the database

Nothing is asserted: the script reports what it measures."""
import argparse
import ctypes as C
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

REPEATS, STEPS, CMP_STEPS, MEM = 7, 40, 10, 200
SHAPES = {"openloris": (50, 69), "core50": (128, 50)}


def seed_host(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def build(data, device):
    import ocl_amd  # noqa: F401
    from ocl_amd import name_match
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    params = bench.make_params(dict(agent="ER", data=data, batch=10, eps_mem_batch=10, mem_size=MEM))
    seed_host(0)
    model = setup_architecture(params).to(device)
    opt = setup_opt("SGD", model, params.learning_rate, params.weight_decay)
    agent = name_match.agents["ER"](model, opt, params)
    return params, model, agent


def workspace_bytes(model):
    """ws_bytes the engine asks of ocl_net_bind for this model's description (no device needed)."""
    from ocl_amd import ffi
    L, h, desc = ffi.lib(), ffi.vp(0), model._engine_desc()
    ffi.check(L.ocl_net_create(C.byref(desc), C.byref(h)), "net_create")
    ws = L.ocl_net_workspace_bytes(h)
    L.ocl_net_destroy(h)
    return desc, ws


def stats(v):
    return "median %.3f  min %.3f  max %.3f  max/min %.3f   repeats %s" % (statistics.median(v), min(v), max(v), max(v) / min(v),
                                                                            " ".join("%.3f" % t for t in v))


def engine_legs(data, device):
    hw, ncls = SHAPES[data]
    params, model, agent = build(data, device)
    x, y = bench.synth_u8(STEPS * 10, hw, ncls, 1)
    xm, ym = bench.synth_u8(MEM, hw, ncls, 2)
    agent.buffer.update(torch.from_numpy(xm).permute(0, 3, 1, 2).float().div(255).to(device), torch.from_numpy(ym).to(device), y_host=ym)
    start = None
    step_ms = []
    for r in range(REPEATS + 1):      # (the first repeat warms every shape up and is dropped)
        if start is None:
            model._ensure_bound()
            start = model.flat_params().clone()
        with torch.no_grad():
            model.flat_params().copy_(start)
        seed_host(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.train_learner(x, y)
        torch.cuda.synchronize()
        step_ms.append((time.perf_counter() - t0) / STEPS * 1e3)
    xe = torch.rand(params.test_batch, 3, hw, hw, device=device)
    model.eval()
    ev_ms = []
    with torch.no_grad():
        for r in range(REPEATS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                model.forward(xe)
            torch.cuda.synchronize()
            ev_ms.append((time.perf_counter() - t0) / 5 * 1e3)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return step_ms[1:], ev_ms[1:], sd, model._desc.max_batch


def comparator_legs(data, device, sd):
    """The oracle's statements (oracle/ocl_oracle.py: OracleNet, er_step) with every tensor on the GPU: stock ROCm eager."""
    from oracle import ocl_oracle as O
    hw, ncls = SHAPES[data]
    x, y = bench.synth_u8(CMP_STEPS * 10, hw, ncls, 1)
    xs, ys = O.to_tensor(x).to(device), torch.from_numpy(y).to(device)
    xm, ym = bench.synth_u8(MEM, hw, ncls, 2)
    step_ms = []
    for r in range(REPEATS + 1):
        state = O.OrderedDict((k, v.clone().requires_grad_(v.is_floating_point() and "running" not in k)) for k, v in sd.items())
        names = [k for k in state if state[k].requires_grad]
        buf = O.OracleBuffer(MEM, (3, hw, hw))
        buf.img, buf.label = O.to_tensor(xm).to(device), torch.from_numpy(ym).to(device)
        buf.current_index = buf.n_seen_so_far = MEM
        seed_host(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(CMP_STEPS):
            O.er_step(state, names, buf, xs[i * 10:(i + 1) * 10], ys[i * 10:(i + 1) * 10], dict(eps_mem_batch=10, lr=0.1), "random")
        torch.cuda.synchronize()
        step_ms.append((time.perf_counter() - t0) / CMP_STEPS * 1e3)
    net = O.OracleNet(O.OrderedDict((k, v.clone()) for k, v in sd.items()), head=None, training=False)
    xe = torch.rand(128, 3, hw, hw, device=device)
    ev_ms = []
    with torch.no_grad():
        for r in range(REPEATS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                net.forward(xe)
            torch.cuda.synchronize()
            ev_ms.append((time.perf_counter() - t0) / 5 * 1e3)
    return step_ms[1:], ev_ms[1:]


def timing(device, out):
    lines = ["datasets_steps: %s, torch %s; ER + random retrieval + reservoir, 10 stream + 10 memory rows per step, mem_size %d (full), SGD lr 0.1;"
             % (torch.cuda.get_device_name(device), torch.__version__, MEM),
             "engine: %d steps per repeat through train_learner (loader included); comparator: the oracle's torch statements on the same GPU, %d steps per"
             % (STEPS, CMP_STEPS),
             "repeat (a same-node baseline, not a target); evaluate forward: one eval-mode pass of 128 images; %d repeats after one warm-up repeat" % REPEATS]
    for data in ("openloris", "core50"):
        hw, _ = SHAPES[data]
        e_step, e_ev, sd, mb = engine_legs(data, device)
        torch.cuda.empty_cache()
        c_step, c_ev = comparator_legs(data, device, sd)
        torch.cuda.empty_cache()
        lines.append("%s (%d x %d)" % (data, hw, hw))
        lines.append("  step      engine      ms  %s" % stats(e_step))
        lines.append("  step      comparator  ms  %s" % stats(c_step))
        lines.append("  evaluate  engine      ms  %s" % stats(e_ev))
        lines.append("  evaluate  comparator  ms  %s" % stats(c_ev))
        lines.append("  engine / comparator: step %.3f, evaluate forward %.3f" % (statistics.median(e_step) / statistics.median(c_step),
                                                                               statistics.median(e_ev) / statistics.median(c_ev)))
    lines += workspace_lines()
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


def workspace_lines():
    import ocl_amd  # noqa: F401
    from ocl_amd.setup_elements import setup_architecture
    lines = ["workspace the engine asks for at the defaults (ws_bytes of ocl_net_bind; n_slots 2 + the scratch slot):"]
    for data in ("openloris", "core50"):
        desc, ws = workspace_bytes(setup_architecture(bench.make_params(dict(agent="ER", data=data))))
        lines.append("  %-10s max_batch %3d: %d bytes (%.2f GiB)" % (data, desc.max_batch, ws, ws / 2.0 ** 30))
    return lines


LOADER_CALLS = 300


def profile_loader(device):
    import ocl_amd  # noqa: F401
    from ocl_amd import ops
    rng = np.random.default_rng(0)
    u8_host = torch.from_numpy(rng.integers(0, 256, (500, 32, 32, 3), dtype=np.uint8))
    u8, f32 = u8_host.to(device), (u8_host.float() / 255).to(device)     # (the same images: IEEE division on the host, as in the u8 kernel)
    for i in range(LOADER_CALLS):
        idx = torch.from_numpy(rng.integers(0, 500, 10)).to(device)
        a = ops.gather_u8_images(u8, idx)
        b = ops.gather_f32_images(f32, idx)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    print("profiled: %d calls of each loader kernel, 10 rows of 32 x 32 x 3" % LOADER_CALLS)


def summarise(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if len(dbs) != 1:
        raise SystemExit("expected one rocprofv3 database under %s, found %d" % (directory, len(dbs)))
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    print("loader kernels, 10 rows of 32 x 32 x 3 per call (rocprofv3 --kernel-trace --stats, one run, %d calls each):" % LOADER_CALLS)
    t = {}
    for name, cnt, avg, lo, hi in rows:
        for tag in ("gather_u8_hwc_f32_chw", "gather_f32_hwc_f32_chw_kernel"):
            if name.startswith(tag + "("):
                t[tag] = avg
                print("  %-32s %4d calls  avg %7.1f ns  min %6d  max %6d" % (tag, cnt, avg, lo, hi))
    if len(t) == 2:
        f, u = t["gather_f32_hwc_f32_chw_kernel"], t["gather_u8_hwc_f32_chw"]
        print("  bytes moved per call: f32 %d read + %d written, u8 %d read + %d written; the f32 kernel takes %.2f of the u8 kernel's time"
              % (10 * 12288, 10 * 12288, 10 * 3072, 10 * 12288, f / u))
        print("  (its bound is the row bytes moved: %d bytes in %.1f ns is %.1f GB/s -- at 10 rows both kernels are a launch's latency, not a bandwidth)"
              % (20 * 12288, f, 20 * 12288 / f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-loader", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--workspace", action="store_true", help="only the workspace sizes (needs no GPU)")
    ap.add_argument("--out", metavar="FILE", help="also write the timing report to FILE")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return 0
    if args.workspace:
        print("\n".join(workspace_lines()))
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("datasets_steps.py measures on an MI355X; no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.profile_loader:
        profile_loader(device)
        return 0
    return timing(device, args.out)


if __name__ == "__main__":
    sys.exit(main())
