#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/gdumb.npz from the REAL reference agent (agents/gdumb.py) on the
case `gdumb_c10` of tests/gdumb_ref.py, and from the reference's own greedy_balancing_update on the label sequences of
gdumb_ref.BALANCER_CASES.

The reference runs twice (determinism at one thread); the restatement tests/gdumb_ref.py::GdumbOracle runs over the same stream and
every recorded array must be bit-equal to the reference's, otherwise nothing is written.  Per task: acc, the memory in train_mem's order
(labels, image row sums), the per-class counts and the digest_state rows.  Per balancer case and batch: the counts and the per-class
contents, sample numbers standing for images.

    python scripts/make_gdumb_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import case_params, make_stream, seed_all          # noqa: E402
import gdumb_ref                                                      # noqa: E402

NAME = "gdumb_c10"


def reference_memory(agent):
    """The reference agent's memory in train_mem's order."""
    mem_x, mem_y = [], []
    for c in agent.mem_img.keys():
        mem_x += agent.mem_img[c]
        mem_y += [c] * agent.mem_c[c]
    return mem_x, mem_y


def run_reference_case(cfg):
    """The reference agent through the case's tasks (train_learner + evaluate): per-task records."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(**case_params(cfg), **gdumb_ref.gdumb_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    tasks, tests = make_stream(cfg)
    with R.quiet():
        test_loaders = setup_test_loader(tests, params)
    recs = []
    for x, y in tasks:
        with R.quiet():
            agent.train_learner(x, y)
            acc = agent.evaluate(test_loaders)
        mem_x, mem_y = reference_memory(agent)
        recs.append(gdumb_ref.record(acc, mem_y, torch.stack(mem_x), agent.mem_c, agent.model.state_dict()))
    return recs


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    cfg = gdumb_ref.GDUMB_CASE
    ref, ref2 = run_reference_case(cfg), run_reference_case(cfg)
    mine, ag = gdumb_ref.run_oracle_case(cfg)
    out = {}
    for t, (a, b, c) in enumerate(zip(ref, ref2, mine)):
        for k in gdumb_ref.GOLDEN_KEYS:
            assert np.array_equal(a[k], b[k]), "the reference is not deterministic: task %d %s" % (t, k)
            assert np.array_equal(a[k], c[k]), "GdumbOracle != reference: task %d %s" % (t, k)
            out["%s_t%d_%s" % (NAME, t, k)] = a[k]
    out[NAME + "_ntasks"] = np.int64(len(ref))
    out[NAME + "_total_norm"] = np.array([e["total_norm"] for e in ag.log], dtype=np.float64)
    out[NAME + "_clipped"] = np.array([e["clipped"] for e in ag.log], dtype=np.int64)
    from ocl_amd.gdumb_memory import GreedyBalancer
    for name, mem_size, seed, batches in gdumb_ref.BALANCER_CASES:
        want = gdumb_ref.run_reference_balancer(mem_size, seed, batches)
        got, _ = gdumb_ref.run_balancer_case(GreedyBalancer, mem_size, seed, batches)
        for b, (w, g) in enumerate(zip(want, got)):
            for k in ("counts", "items", "labels"):
                assert np.array_equal(w[k], g[k]), "GreedyBalancer != reference: %s batch %d %s" % (name, b, k)
                out["bal_%s_b%d_%s" % (name, b, k)] = w[k]
    ratios = np.array([e["ratio"] for e in ag.log])
    print("%s: %d memory steps, %d clip, min |total/clip - 1| %.4f, norms %.3f .. %.3f, acc %s" % (
        NAME, len(ag.log), sum(e["clipped"] for e in ag.log), np.abs(ratios - 1).min(), ratios.min() * cfg["clip"], ratios.max() * cfg["clip"],
        [np.round(r["acc"], 3).tolist() for r in ref]))
    path = os.path.join(ROOT, "tests", "golden", "gdumb.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
