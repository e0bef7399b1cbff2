"""CPU: the case table of the workspace-poison tests (tests/ws_poison_cases.py, run by tests/test_gpu_ws_poison.py and, for the C ABI, by
tests/test_gpu_netcheck.py) says what it claims.

* every operation kind of tests/pass_order_cases.py is claimed by a poison case, so a pass kind added there cannot stay uncovered;
* the fill patterns are 0xFFFFFFFF (NaN, UINT_MAX), 0x7F800000 (+inf) and 0x45800000 (4096.0) and read back as such;
* the passes the table is meant to hold are in it: every probe, the frozen tape at n = 1 and 10, the eval plan buckets, the two odd inputs;
* the GPU files run the whole table, unsliced and without a skip."""
import os
import re

import numpy as np

import pass_order_cases as PC
import ws_poison_cases as WC
from conftest import ROOT


def test_every_pass_order_operation_kind_is_claimed_by_a_poison_case():
    kinds = WC.pass_order_kinds()
    assert {"F", "B", "FZ", "BZ", "I1", "I2", "I2p", "I3", "I4", "I5", "G0", "Z", "DROP", "B!"} <= kinds
    assert kinds - WC.claimed() == set(), "operation kinds of pass_order_cases that no poison case runs"
    # a "seq" case claims exactly what its sequence holds; a direct case only intruder kinds (it runs the pass without the tape around it)
    for c in WC.CASES:
        if c["kind"] == "seq":
            assert set(c["claims"]) == set(op[0] for op in c["seq"]), c["id"]
            PC.check_sequence(c["seq"], c["n_slots"], PC.PROBES[c["model"]])
        else:
            assert set(c["claims"]) <= {"I1", "I2", "I3", "I4", "I5"}, c["id"]


def test_the_fill_patterns_are_the_three_of_the_law():
    assert WC.PATTERNS == {"nan": 0xFFFFFFFF, "inf": 0x7F800000, "f4096": 0x45800000}
    as_float = {k: np.array(v, dtype=np.uint32).view(np.float32) for k, v in WC.PATTERNS.items()}
    assert np.isnan(as_float["nan"]) and np.isposinf(as_float["inf"]) and as_float["f4096"] == np.float32(4096.0)
    assert np.array(WC.PATTERNS["nan"], dtype=np.uint32).view(np.int32) == -1


def test_the_table_holds_the_passes_it_is_meant_to():
    ids = WC.IDS
    assert len(set(ids)) == len(ids)
    by_kind = {}
    for c in WC.CASES:
        assert c["model"] in WC.MODELS
        by_kind.setdefault(c["kind"], []).append(c)
    probes = {(c["model"], c["seq"][0][2]) for c in by_kind["seq"] if [op[0] for op in c["seq"]] == ["F", "B"]}
    assert probes == {(m, p) for m in PC.PROBES for p in PC.PROBES[m]}
    assert {c["seq"][0][2] for c in by_kind["seq"] if [op[0] for op in c["seq"]] == ["FZ", "BZ"]} == {1, 10}
    assert {c["n"] for c in by_kind["features"] if c["model"] == "er_c100"} == {1, 3, 5, 12, 17, 33}
    # ... which are one pass per plan bucket (net.hip: eval-mode plans in buckets of 4 up to 16 images, of 16 above)
    assert sorted((n + 3) // 4 * 4 if n <= 16 else (n + 15) // 16 * 16 for n in WC.EVAL_BUCKETS) == [4, 4, 8, 12, 32, 48]
    assert {c["train"] for c in by_kind["with_params"]} == {True, False}
    assert len(by_kind["stats_only"]) == 1 and len(by_kind["no_grad"]) == 1 and len(by_kind["same_weights"]) == 1 and by_kind["taped"]
    assert any(c["seq"] == PC.find("er_c100-o1-all")["seq"] for c in by_kind["seq"])
    assert any("G0" in c["claims"] for c in by_kind["seq"]) and any(c["id"].endswith("-acc") for c in by_kind["seq"])
    # the odd shapes, on the engines tests/test_gpu_datasets.py builds
    assert WC.MODELS["er_loris"][3:] == (50, 8) and WC.MODELS["er_core50"][3:] == (128, 4)
    odd = {(c["model"], c["kind"], c["n"]) for c in WC.CASES if c["model"] not in PC.MODELS}
    assert odd == {("er_loris", "train", 3), ("er_loris", "features", 1), ("er_core50", "train", 2)}
    for c in WC.CASES:
        assert c["kind"] == "seq" or c["n"] <= WC.MODELS[c["model"]][4]
    # the C ABI matrix
    assert WC.NETCHECK_MODES == [{}, {"OCL_WGRAD_Q": "0"}, {"OCL_WGRAD_MULTI": "0"}, {"OCL_DY_KEEP": "0"}, {"OCL_BN_CHAN": "0"},
                                 {"OCL_SINGLE_STREAM": "1"}, {"OCL_GRAPH": "1"}]
    assert WC.NETCHECK_CASES == [(20, 2, 32, 0), (6, 2, 84, 1), (9, 3, 32, 1)] and WC.NETCHECK_DEFAULT_ONLY == [(220, 2, 32, 1)]
    # passes of more than two BatchNorm groups: the backward's reduce + apply arena (tests/test_gpu_ws_poison.py, off_bsums)
    assert {(c["model"], c["n"], c["groups"]) for c in by_kind["taped"]} >= {("scr_c100", 9, 3), ("er_c100", 12, 4)}


def test_the_gpu_files_run_the_whole_table():
    text = open(os.path.join(ROOT, "tests", "test_gpu_ws_poison.py")).read()
    assert text.count('@pytest.mark.parametrize("cid", WC.IDS)') == 3
    assert '@pytest.mark.parametrize("pattern", sorted(WC.PATTERNS))' in text
    assert "pytestmark = pytest.mark.gpu" in text
    assert not re.search(r"skip|xfail", text)
    net = open(os.path.join(ROOT, "tests", "test_gpu_netcheck.py")).read()
    assert "WC.NETCHECK_MODES" in net and "WC.NETCHECK_CASES" in net and "WC.NETCHECK_DEFAULT_ONLY" in net and "NETCHECK_WS_FILL" in net
    tool = open(os.path.join(ROOT, "online-continual-learning_amd", "csrc", "netcheck.cpp")).read()
    assert 'getenv("NETCHECK_WS_FILL")' in tool and tool.index("NETCHECK_WS_FILL\"))") < tool.index("OK(ocl_net_bind(")
