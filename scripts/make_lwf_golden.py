#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/lwf.npz from the REAL reference agent (agents/lwf.py) on the case
`lwf_c10` of tests/lwf_ref.py.

The reference runs twice (determinism at one thread); the restatement tests/lwf_ref.py::LwfOracle runs over the same stream and every
recorded array must be bit-equal to the reference's, otherwise nothing is written.  Per task: acc, the digest_state rows of the model,
and loss_new / loss_old of the task's first two iterations -- what the agent's own criterion and kd_manager.get_kd_loss returned, read
by wrapping the two bound methods of the running agent.  Only recorded results go into the file.

    python scripts/make_lwf_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import make_stream, seed_all                        # noqa: E402
import lwf_ref                                                        # noqa: E402

NAME = "lwf_c10"


def run_reference_case(cfg, tasks_only=None):
    """The reference agent through the case's tasks (train_learner + evaluate): per-task records, the per-iteration losses, the agent."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(**lwf_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    log = []
    inner_kd, inner_ce = agent.kd_manager.get_kd_loss, agent.criterion

    def get_kd_loss(logits, x):
        out = inner_kd(logits, x)
        log.append(dict(loss_old=float(out.detach()) if torch.is_tensor(out) else float(out)))
        return out

    def criterion(logits, labels):
        out = inner_ce(logits, labels)
        log[-1]["loss_new"] = float(out.detach())
        return out

    agent.kd_manager.get_kd_loss, agent.criterion = get_kd_loss, criterion
    tasks, tests = make_stream(cfg)
    with R.quiet():
        test_loaders = setup_test_loader(tests, params)
    recs = []
    for x, y in tasks[:tasks_only]:
        with R.quiet():
            agent.train_learner(x, y)
            acc = agent.evaluate(test_loaders)
        recs.append(lwf_ref.record(acc, model.state_dict()))
    return recs, log, agent


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    cfg = lwf_ref.LWF_CASE
    steps = len(cfg["tasks"][0]) * cfg["n_train"] // 10
    (ref, log, _), (ref2, log2, _) = run_reference_case(cfg), run_reference_case(cfg)
    mine, ag = lwf_ref.run_oracle_case(cfg)
    out = {}
    for t, (a, b, c) in enumerate(zip(ref, ref2, mine)):
        for k in lwf_ref.GOLDEN_KEYS:
            assert np.array_equal(a[k], b[k]), "the reference is not deterministic: task %d %s" % (t, k)
            assert np.array_equal(a[k], c[k]), "LwfOracle != reference: task %d %s" % (t, k)
            out["%s_t%d_%s" % (NAME, t, k)] = a[k]
    losses, losses2, losses_mine = (lwf_ref.recorded_losses(lg, steps) for lg in (log, log2, ag.log))
    assert len(log) == len(log2) == len(ag.log) == steps * len(ref)
    assert np.array_equal(losses, losses2), "the reference's losses are not deterministic"
    assert np.array_equal(losses, losses_mine), "LwfOracle's losses != the reference's"
    assert all(a["loss_new"] == b["loss_new"] and a["loss_old"] == b["loss_old"] for a, b in zip(log, ag.log)), "a later iteration's losses differ"
    out[NAME + "_ntasks"] = np.int64(len(ref))
    out[NAME + "_steps_per_task"] = np.int64(steps)
    out[NAME + "_losses"] = losses
    print("%s: %d iterations; loss_new %s" % (NAME, len(log), np.round([e["loss_new"] for e in log], 3).tolist()))
    print("loss_old %s" % np.round([e["loss_old"] for e in log], 3).tolist())
    print("|w| %s, acc %s" % ([float(np.sqrt((r["state"][:, 1] ** 2).sum())) for r in ref], [np.round(r["acc"], 3).tolist() for r in ref]))
    path = os.path.join(ROOT, "tests", "golden", "lwf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
