#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/agem.npz from the REAL reference agent (agents/agem.py) on the
cases `agem_c10` and `agem_loops` (epoch 2, mem_iters 2) of tests/agem_ref.py.

The reference runs twice (determinism at one thread); the restatement tests/agem_ref.py::agem_step runs over the same stream and every
recorded array must be bit-equal to the reference's, otherwise nothing is written.  Per task: acc, buf_label, buf_rowsum, counters
and the digest_state rows -- what oracle/make_golden.py records for its step cases; agem_loops also num_batches_tracked (nbt).

    python scripts/make_agem_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import case_params, make_stream, seed_all          # noqa: E402
import agem_ref                                                       # noqa: E402

CASES = (("agem_c10", agem_ref.AGEM_CASE, agem_ref.GOLDEN_KEYS), ("agem_loops", agem_ref.AGEM_LOOPS_CASE, agem_ref.LOOPS_KEYS))


def run_reference_case(cfg, tasks_only=None):
    """The reference agent through the case's tasks (train_learner + evaluate): per-task records."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(**case_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    tasks, tests = make_stream(cfg)
    with R.quiet():
        test_loaders = setup_test_loader(tests, params)
    recs = []
    for x, y in tasks[:tasks_only]:
        with R.quiet():
            agent.train_learner(x, y)
            acc = agent.evaluate(test_loaders)
        recs.append(agem_ref.record(acc, agent.buffer.buffer_label.numpy(), agent.buffer.buffer_img, agent.buffer.current_index,
                                    agent.buffer.n_seen_so_far, model.state_dict()))
    return recs


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    out = {}
    for name, cfg, keys in CASES:
        ref, ref2 = run_reference_case(cfg), run_reference_case(cfg)
        mine, ag = agem_ref.run_oracle_case(cfg)
        for t, (a, b, c) in enumerate(zip(ref, ref2, mine)):
            for k in keys:
                assert np.array_equal(a[k], b[k]), "the reference is not deterministic: %s task %d %s" % (name, t, k)
                assert np.array_equal(a[k], c[k]), "agem_step != reference: %s task %d %s" % (name, t, k)
                out["%s_t%d_%s" % (name, t, k)] = a[k]
        out[name + "_ntasks"] = np.int64(len(ref))
        steps = ag.log if cfg.get("mem_iters", 1) == 1 else [dict(cos=c, projected=p) for e in ag.log for c, p in zip(e["cos"], e["projected"])]
        seen = [e for e in steps if e["cos"] is not None]
        print("%s: %d steps, %d see memory, %d project, min |cos| %.4f, acc %s" % (
            name, len(steps), len(seen), sum(e["projected"] for e in seen), min(abs(e["cos"]) for e in seen),
            [np.round(r["acc"], 3).tolist() for r in ref]))
    path = os.path.join(ROOT, "tests", "golden", "agem.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
