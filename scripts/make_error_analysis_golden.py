#!/usr/bin/env python3
"""Build container only (reference tree present): records tests/golden/error_analysis.npz from the REAL reference ER agent on the CPU, run
with params.error_analysis on the case EA_CASE of tests/error_analysis_ref.py (test batches of 16, so every loader ends on a partial batch).

Per evaluate call e (one after each task), under the keys e<e>_*: every test batch's logits and labels in the order the loaders produced
them (concatenated; `tasks` and `batch_sizes` say where each batch starts and which loader it came from), old_labels, new_labels_zombie and
class_task_map at that moment, the last layer's weight and bias, and every output of the branch: the (no, nn, oo, on) tuple, the two class
scores, the four norms, acc_array and the two lists the reference pickled into its `confusion` file.  The logits are read by wrapping the
running model's forward, the labels by iterating recording stand-ins of the loaders; only recorded data goes into the file.

The reference runs twice (determinism at one thread).  No recorded row may have an exact tie between its two largest logits: with that,
the arg-max of the same float32 inputs is exact whatever computes it.

    python scripts/make_error_analysis_golden.py
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import ref_import as R                                    # noqa: E402
from oracle.synth import make_stream, seed_all, case_params           # noqa: E402
import error_analysis_ref as E                                        # noqa: E402


class RecordingLoader(object):
    """Iterates a loader and keeps the labels of every batch it yielded."""

    def __init__(self, inner, task, log):
        self.inner, self.task, self.log = inner, task, log

    def __iter__(self):
        for x, y in self.inner:
            self.log.append((self.task, y.numpy().copy()))
            yield x, y


def run_reference_case(cfg, test_batch=E.EA_TEST_BATCH):
    """The reference agent through the case's tasks (train_learner + evaluate with error_analysis): one record per evaluate call."""
    R.activate()
    from continuum.data_utils import setup_test_loader
    params = R.default_params(error_analysis=True, test_batch=test_batch, **case_params(cfg))
    seed_all(cfg["seed"])
    model, opt, agent = R.build_agent(params)
    tasks, tests = make_stream(cfg)
    with R.quiet():
        loaders = setup_test_loader(tests, params)
    seen_y, seen_logits = [], []
    inner_forward = model.forward
    recording = [False]

    def forward(x):
        out = inner_forward(x)
        if recording[0]:
            seen_logits.append(out.detach().numpy().copy())
        return out

    model.forward = forward
    recs = []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                       # the reference writes its `confusion` file into the working directory
        try:
            for x, y in tasks:
                with R.quiet():
                    agent.train_learner(x, y)
                    del seen_y[:], seen_logits[:]
                    recording[0] = True
                    acc = agent.evaluate([RecordingLoader(l, t, seen_y) for t, l in enumerate(loaders)])
                    recording[0] = False
                with open("confusion", "rb") as fp:
                    confusion = pickle.load(fp)
                assert len(seen_y) == len(seen_logits) and all(len(y_) == len(l_) for (_, y_), l_ in zip(seen_y, seen_logits))
                logits = np.concatenate(seen_logits)
                assert logits.dtype == np.float32 and not E.top2_tie(logits).any(), "a recorded row has an exact tie between its two largest logits"
                recs.append(dict(
                    logits=logits, labels=np.concatenate([y_ for _, y_ in seen_y]).astype(np.int64),
                    tasks=np.array([t for t, _ in seen_y], dtype=np.int64), batch_sizes=np.array([len(y_) for _, y_ in seen_y], dtype=np.int64),
                    old_labels=np.array(agent.old_labels, dtype=np.int64), new_labels_zombie=np.array(agent.new_labels_zombie, dtype=np.int64),
                    class_task_map=np.array(sorted(agent.class_task_map.items()), dtype=np.int64).reshape(-1, 2), task_seen=np.int64(agent.task_seen),
                    weight=model.linear.weight.detach().numpy().copy(), bias=model.linear.bias.detach().numpy().copy(),
                    error=np.array(agent.error_list[-1], dtype=np.int64), new_class_score=np.float64(agent.new_class_score[-1]),
                    old_class_score=np.float64(agent.old_class_score[-1]), fc_norm_new=np.float64(agent.fc_norm_new[-1]),
                    fc_norm_old=np.float64(agent.fc_norm_old[-1]), bias_norm_new=np.float64(agent.bias_norm_new[-1]),
                    bias_norm_old=np.float64(agent.bias_norm_old[-1]), acc=np.asarray(acc, dtype=np.float64),
                    confusion=np.array(confusion, dtype=np.int64)))
        finally:
            os.chdir(cwd)
            model.forward = inner_forward
    return recs


def main():
    assert R.available(), "reference tree not found"
    torch.set_num_threads(1)
    a, b = run_reference_case(E.EA_CASE), run_reference_case(E.EA_CASE)
    out = dict(n_evaluates=np.int64(len(a)), n_loaders=np.int64(len(E.EA_CASE["tasks"])))
    for e, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert np.array_equal(ra[k], rb[k], equal_nan=ra[k].dtype.kind == "f"), "the reference is not deterministic: evaluate %d %s" % (e, k)
            out["e%d_%s" % (e, k)] = ra[k]
        print("evaluate %d: (no, nn, oo, on) %s  new / old score %.6f / %.6f  norms %s  acc %s  batches %s"
              % (e, tuple(ra["error"].tolist()), ra["new_class_score"], ra["old_class_score"],
                 [float(ra[k]) for k in ("fc_norm_new", "fc_norm_old", "bias_norm_new", "bias_norm_old")], np.round(ra["acc"], 3).tolist(),
                 ra["batch_sizes"].tolist()))
    path = os.path.join(ROOT, "tests", "golden", "error_analysis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
