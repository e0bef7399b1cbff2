"""Regenerates tests/golden/datasets.npz from the REAL reference (needs the reference tree; see oracle/ref_import.py):
for --data core50 / openloris, what utils/setup_elements.setup_architecture builds under torch seed 11 -- the state_dict keys, the
tensor shapes, which entries are parameters, and a (sum, L2 norm, first element) digest of every floating tensor.

    python scripts/make_datasets_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import as R  # noqa: E402
from oracle.synth import digest_state  # noqa: E402

CASES = [("er_core50", "ER", "core50"), ("er_openloris", "ER", "openloris"), ("scr_openloris", "SCR", "openloris"),
         ("scr_core50", "SCR", "core50")]
SEED = 11


def main():
    R.activate()
    from utils.setup_elements import setup_architecture
    out = {}
    for name, agent, data in CASES:
        torch.manual_seed(SEED)
        with R.quiet():
            m = setup_architecture(R.default_params(agent=agent, data=data, head="mlp"))
        sd = m.state_dict()
        params = set(k for k, _ in m.named_parameters())
        out[name + "_keys"] = np.array(list(sd.keys()))
        out[name + "_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
        out[name + "_is_param"] = np.array([k in params for k in sd], dtype=np.bool_)
        out[name + "_digest"] = digest_state(sd)
        out[name + "_draw_after"] = torch.rand(4).numpy()   # the next draws of the generator: same number of draws consumed
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "datasets.npz"), **out)
    print("datasets ok")


if __name__ == "__main__":
    main()
