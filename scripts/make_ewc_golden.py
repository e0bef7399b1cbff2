#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/ewc.npz from the REAL reference agent (agents/ewc_pp.py) on the
cases `ewc_c10` and `ewc_loops` (epoch 2, the running Fisher's schedule counted across the epochs) of tests/ewc_ref.py.

The reference runs twice (determinism at one thread); the restatement tests/ewc_ref.py::EwcOracle runs over the same stream and every
recorded array must be bit-equal to the reference's, otherwise nothing is written.  Per task: acc, the digest_state rows of the model
and of the four EWC++ dictionaries (running, temporary and normalised Fisher, previous parameters), and [min, max] of the running
Fisher; per iteration the cross-entropy and the penalty sum, which the reference does not keep: they are the restatement's, written
only once it has reproduced the reference bit for bit.  ewc_loops also keeps num_batches_tracked and, per task, the iterations at
which the reference called update_running_fisher (counted by its optimiser steps).  Only recorded results go into the file.

    python scripts/make_ewc_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import make_stream, seed_all                        # noqa: E402
import ewc_ref                                                        # noqa: E402

CASES = (("ewc_c10", ewc_ref.EWC_CASE, ewc_ref.GOLDEN_KEYS), ("ewc_loops", ewc_ref.EWC_LOOPS_CASE, ewc_ref.LOOPS_KEYS))


def run_reference_case(cfg, tasks_only=None):
    """The reference agent through the case's tasks (train_learner + evaluate): per-task records, and the agent."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(**ewc_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    tasks, tests = make_stream(cfg)
    with R.quiet():
        test_loaders = setup_test_loader(tests, params)
    recs = []
    # when the reference updates its running Fisher: the number of optimiser steps of the task made before the call
    seen = dict(steps=0, ema_at=[])
    inner_step, inner_ema = opt.step, agent.update_running_fisher

    def step(*a, **k):
        seen["steps"] += 1
        return inner_step(*a, **k)

    def update_running_fisher(*a, **k):
        seen["ema_at"].append(seen["steps"])
        return inner_ema(*a, **k)

    opt.step, agent.update_running_fisher = step, update_running_fisher
    for x, y in tasks[:tasks_only]:
        seen.update(steps=0, ema_at=[])
        with R.quiet():
            agent.train_learner(x, y)
            acc = agent.evaluate(test_loaders)
        recs.append(ewc_ref.record(acc, model.state_dict(), agent.running_fisher, agent.tmp_fisher, agent.normalized_fisher, agent.prev_params,
                                   ema_at=seen["ema_at"]))
    return recs, agent


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    out = {}
    for name, cfg, keys in CASES:
        (ref, _), (ref2, _) = run_reference_case(cfg), run_reference_case(cfg)
        mine, ag = ewc_ref.run_oracle_case(cfg)
        for t, (a, b, c) in enumerate(zip(ref, ref2, mine)):
            for k in ewc_ref.LOOPS_KEYS:        # (every key is compared; `keys` are written)
                assert np.array_equal(a[k], b[k]), "the reference is not deterministic: %s task %d %s" % (name, t, k)
                assert np.array_equal(a[k], c[k]), "EwcOracle != reference: %s task %d %s" % (name, t, k)
                if k in keys:
                    out["%s_t%d_%s" % (name, t, k)] = a[k]
        out[name + "_ntasks"] = np.int64(len(ref))
        out[name + "_ce"] = np.array([e["ce"] for e in ag.log])
        out[name + "_penalty"] = np.array([e["penalty"] for e in ag.log])
        print("%s: %d iterations, ce %s" % (name, len(ag.log), np.round(out[name + "_ce"], 3).tolist()))
        print("penalty %s" % np.round(out[name + "_penalty"], 4).tolist())
        print("running Fisher updated at %s; [min, max] per task %s, |w| %s, acc %s" % (
            [r["ema_at"].tolist() for r in ref], [r["minmax"].tolist() for r in ref],
            [float(np.sqrt((r["state"][:, 1] ** 2).sum())) for r in ref], [np.round(r["acc"], 3).tolist() for r in ref]))
    path = os.path.join(ROOT, "tests", "golden", "ewc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
