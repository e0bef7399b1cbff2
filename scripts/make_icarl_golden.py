#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/icarl.npz from the REAL reference agent (agents/icarl.py) on the
case ICARL_CASE of tests/icarl_ref.py.

The reference runs twice (determinism at one thread); the restatement tests/icarl_ref.py::IcarlOracle runs over the same stream and every
recorded array must be bit-equal to the reference's, otherwise nothing is written.  Per task: acc and the digest_state rows of the model;
over the run: the loss of each task's first two iterations (what the agent's own binary_cross_entropy_with_logits call returned, summed
and averaged as the agent does) and the slot indices of every retrieval, read by wrapping the two names `F` and `random_retrieve` of the
running agent's module.  The losses of all iterations and the shapes the BCE saw are compared as well.  Only recorded results go into
the file.

    python scripts/make_icarl_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import make_stream, seed_all                        # noqa: E402
import icarl_ref                                                      # noqa: E402

NAME = "icarl_c10"


def run_reference_case(cfg, tasks_only=None):
    """The reference agent through the case's tasks (train_learner + evaluate): per-task records, the per-iteration log, the agent."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(**icarl_ref.ref_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    mod = sys.modules[type(agent).__module__]
    log, pending = [], {}
    inner_F, inner_retrieve = mod.F, mod.random_retrieve

    def bce(input, target, **kw):
        out = inner_F.binary_cross_entropy_with_logits(input, target, **kw)
        log.append(dict(loss=float(out.detach().sum(dim=1).mean()), rows=int(input.size(0)), n_cls=int(input.size(1)),
                        teacher=agent.prev_model is not None, indices=pending.pop("indices", None), excl=pending.pop("excl", None)))
        return out

    def random_retrieve(buffer, num_retrieve, excl_indices=None):
        x, y, indices = inner_retrieve(buffer, num_retrieve, excl_indices=excl_indices, return_indices=True)
        pending["indices"], pending["excl"] = indices.numpy().copy(), list(excl_indices)
        return x, y

    mod.F = SimpleNamespace(binary_cross_entropy_with_logits=bce)
    mod.random_retrieve = random_retrieve
    try:
        tasks, tests = make_stream(cfg)
        with R.quiet():
            test_loaders = setup_test_loader(tests, params)
        recs = []
        for x, y in tasks[:tasks_only]:
            with R.quiet():
                agent.train_learner(x, y)
                acc = agent.evaluate(test_loaders)
            recs.append(icarl_ref.record(acc, model.state_dict()))
    finally:
        mod.F, mod.random_retrieve = inner_F, inner_retrieve
    return recs, log, agent


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    cfg = icarl_ref.ICARL_CASE
    batch = 10
    steps = len(cfg["tasks"][0]) * cfg["n_train"] // batch
    (ref, log, _), (ref2, log2, _) = run_reference_case(cfg), run_reference_case(cfg)
    mine, ag = icarl_ref.run_oracle_case(cfg)
    out = {}
    for t, (a, b, c) in enumerate(zip(ref, ref2, mine)):
        for k in icarl_ref.GOLDEN_KEYS:
            assert np.array_equal(a[k], b[k]), "the reference is not deterministic: task %d %s" % (t, k)
            assert np.array_equal(a[k], c[k]), "IcarlOracle != reference: task %d %s" % (t, k)
            out["%s_t%d_%s" % (NAME, t, k)] = a[k]
    assert len(log) == len(log2) == len(ag.log) == steps * len(ref)
    for k, (a, b, c) in enumerate(zip(log, log2, ag.log)):
        for key in ("loss", "rows", "n_cls", "teacher", "excl"):
            assert a[key] == b[key], "the reference is not deterministic: iteration %d %s" % (k, key)
            assert a[key] == c[key], "IcarlOracle != reference: iteration %d %s: %s, %s" % (k, key, a[key], c[key])
        assert (a["indices"] is None) == (b["indices"] is None) == (c["indices"] is None) == (not a["teacher"])
        if a["indices"] is not None:
            assert np.array_equal(a["indices"], b["indices"]) and np.array_equal(a["indices"], c["indices"]), "retrieval of iteration %d" % k
            assert not set(a["indices"].tolist()) & set(a["excl"]), "iteration %d retrieved an excluded slot" % k
    losses = icarl_ref.recorded_losses([e["loss"] for e in log], steps)
    retrievals = icarl_ref.retrieval_table([e["indices"] for e in log if e["indices"] is not None], batch)
    n_excl = np.array([len(e["excl"]) for e in log if e["indices"] is not None], dtype=np.int64)
    assert (n_excl > 0).any(), "the case holds no retrieval with a non-empty exclusion list"
    assert [(e["rows"], e["n_cls"]) for e in log] == [(batch, 2)] * steps + [(2 * batch, 4)] * steps + [(2 * batch, 6)] * steps
    out[NAME + "_ntasks"] = np.int64(len(ref))
    out[NAME + "_steps_per_task"] = np.int64(steps)
    out[NAME + "_losses"] = losses
    out[NAME + "_retrievals"] = retrievals
    out[NAME + "_n_excluded"] = n_excl
    print("%s: %d iterations; loss %s" % (NAME, len(log), np.round([e["loss"] for e in log], 3).tolist()))
    print("retrievals %s, excluded slots per retrieval %s" % (retrievals.shape, n_excl.tolist()))
    print("|w| %s, acc %s" % ([float(np.sqrt((r["state"][:, 1] ** 2).sum())) for r in ref], [np.round(r["acc"], 3).tolist() for r in ref]))
    path = os.path.join(ROOT, "tests", "golden", "icarl.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
