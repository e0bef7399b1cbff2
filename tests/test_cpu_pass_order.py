"""CPU: the case table of the pass-ordering tests (tests/pass_order_cases.py, run by tests/test_gpu_pass_order.py) says what it claims.

* every probe pass -- the abandoned train tapes of intruder I7 included -- is a row of test_gpu_net.CASES, so its isolated result is
  held to the oracle by test_train_forward_backward_vs_oracle;
* every sequence is well formed: each taped forward is consumed once or abandoned explicitly, no backward meets a slot that the round
  robin has handed to a later forward, live tapes never exceed the case's n_slots (and the checker itself refuses sequences that are not);
* the probes labelled single-stream / two-stream fall on the right side of kTwoStreamMinBatch x 1024 input pixels (the constant is
  read from csrc/net.hip) and of ocl_test_head_side_min_batch;
* the table holds the orderings it is meant to hold, and the GPU file runs every case of it, unsliced."""
import os
import re

import pytest

import pass_order_cases as PC
from conftest import ROOT
import ocl_amd  # noqa: F401
from ocl_amd import ffi

NET_HIP = os.path.join(ROOT, "online-continual-learning_amd", "csrc", "net.hip")


def test_every_probe_is_a_case_of_test_gpu_net():
    import test_gpu_net as TN
    assert set(PC.PROBES) == set(PC.MODELS) == set(PC.ROLES)
    for model, probes in PC.PROBES.items():
        assert len(probes) >= 2
        for name in probes:
            assert PC.case_probe(model, name) in TN.CASES, (model, name)
        a, b, big = PC.ROLES[model]
        assert a in probes and big in probes and (b is None or b in probes) and len({a, b, big}) == 3
    used = {(c["model"], op[2]) for c in PC.CASES for op in c["seq"] if op[0] == "F"}
    assert used == {(m, p) for m in PC.PROBES for p in PC.PROBES[m]}, "a probe no sequence runs, or a pass that is no probe"


def test_every_sequence_is_well_formed():
    ids = [c["id"] for c in PC.CASES]
    assert len(set(ids)) == len(ids)
    for c in PC.CASES:
        peak = PC.check_sequence(c["seq"], c["n_slots"], PC.PROBES[c["model"]])
        assert 1 <= peak <= c["n_slots"], c["id"]
        assert any(op[0] == "B" for op in c["seq"]), c["id"]
        # intruders own no live tape at the end: the last operation is a probe's backward
        assert c["seq"][-1][0] == "B", c["id"]
    assert PC.check_sequence(PC.replay_sequence(), PC.REPLAY_SLOTS, PC.PROBES[PC.REPLAY_MODEL]) == 2


@pytest.mark.parametrize("seq,n_slots", [
    ([("F", "A", "a10")], 2),                                                               # neither consumed nor abandoned
    ([("F", "A", "a10"), ("B", "A"), ("B", "A")], 2),                                       # consumed twice
    ([("F", "A", "a10"), ("DROP", "A"), ("B", "A")], 2),                                    # backward through an abandoned tape
    ([("F", "A", "a10"), ("FZ", "z", 1), ("DROP", "z"), ("F", "i", "a3"), ("DROP", "i"), ("B", "A")], 2),   # slot taken by the round robin
    ([("F", "A", "a10"), ("F", "B", "a3"), ("F", "C", "a100"), ("B", "C"), ("B", "B"), ("B", "A")], 2),     # three live tapes, two slots
    ([("F", "A", "a10"), ("BZ", "A")], 2),                                                  # a train tape is no frozen tape
    ([("F", "A", "nope"), ("B", "A")], 2),                                                  # unknown probe
    ([("F", "A", "a10"), ("B!", "A"), ("B", "A")], 2),                                      # B! needs a consumed tape
])
def test_the_checker_refuses_malformed_sequences(seq, n_slots):
    with pytest.raises(AssertionError):
        PC.check_sequence(seq, n_slots, PC.PROBES["er_c100"])


def test_stream_regimes_fall_on_the_labelled_side_of_the_thresholds():
    text = open(NET_HIP).read()
    found = re.findall(r"static const int kTwoStreamMinBatch = (\d+);", text)
    assert len(found) == 1
    two_min_pixels = int(found[0]) * 1024
    lib = ffi.lib()
    defaults = "OCL_SIDE_EXTRA_MIN" not in os.environ and os.environ.get("OCL_SINGLE_STREAM") != "1"
    for model, probes in PC.PROBES.items():
        hw = PC.MODELS[model][3]
        regimes = set()
        for name, (n, groups, regime, head_side) in probes.items():
            assert n % groups == 0 and n <= PC.MODELS[model][4]
            assert regime == ("two" if n * hw * hw >= two_min_pixels else "single"), (model, name)
            regimes.add(regime)
            if defaults:
                side_min = lib.ocl_test_head_side_min_batch(hw)
                assert side_min > 0 and head_side == (regime == "two" and n >= side_min), (model, name, side_min)
        assert regimes == {"single", "two"}, model
        a, b, big = PC.ROLES[model]
        assert probes[a][2] == "single" and probes[big][2] == "two" and (b is None or probes[b][2] == "single")
    # the head's dW on the side stream, and a two-stream backward that keeps it on the caller's: both are met
    sides = {p[3] for probes in PC.PROBES.values() for p in probes.values() if p[2] == "two"}
    assert sides == {True, False}
    # I1: plans of 12 and of 48 images (net.hip: eval-mode plans in buckets of 4 up to 16 images, of 16 above)
    plan = [(n + 3) // 4 * 4 if n <= 16 else (n + 15) // 16 * 16 for n in PC.I1_SIZES]
    assert plan == [12, 48]
    assert "N <= 16 ? (N + 3) / 4 * 4 : (N + 15) / 16 * 16" in text


def test_the_table_holds_the_orderings_it_is_meant_to():
    first = next(iter(PC.MODELS))
    by = {}
    for c in PC.CASES:
        by.setdefault((c["model"], c["ordering"]), []).append(c)
    for model in PC.MODELS:
        orderings = {o for (m, o) in by if m == model}
        assert orderings == (set(range(1, 9)) if model == first else {1, 2, 4}), (model, orderings)
        # 1: every intruder once, then all in a row
        names = set(PC.intruders(model))
        assert len(names) == 12 and {l for c in by[(model, 1)] for l in c["labels"]} == names | {"all"}
        row = [c for c in by[(model, 1)] if c["labels"] == ("all",)][0]
        for ops in PC.intruders(model).values():
            assert all(op in row["seq"] for op in ops)
        for c in by[(model, 1)]:
            assert c["seq"][0][0] == "F" and c["seq"][-1] == ("B", c["seq"][0][1]) and sum(op[0] == "B" for op in c["seq"]) == 1
        # 2: both orders, with and without zero_grad between the backwards
        variants = set()
        for c in by[(model, 2)]:
            kinds = [op[0] for op in c["seq"]]
            assert kinds[:2] == ["F", "F"] and c["seq"][0][2] != c["seq"][1][2]
            variants.add((tuple(op[1] for op in c["seq"] if op[0] == "B"), "Z" in kinds))
        assert variants == {(("A", "B"), True), (("A", "B"), False), (("B", "A"), True), (("B", "A"), False)}
        # 4: F(large) F(small) B(large) I1 ... B(small), nothing between the large backward and I1
        (c,) = by[(model, 4)]
        _, small, big = PC.ROLES[model][0], PC.ROLES[model][0], PC.ROLES[model][2]
        assert c["seq"][:4] == [("F", "A", big), ("F", "B", small), ("B", "A"), ("I1", PC.I1_SIZES[0])] and c["seq"][-1] == ("B", "B")
    # 3: three slots, three live tapes, consumed neither in issue order nor in its reverse
    for c in by[(first, 3)]:
        issued = [op[1] for op in c["seq"] if op[0] == "F"]
        consumed = [op[1] for op in c["seq"] if op[0] == "B"]
        assert c["n_slots"] == 3 and len(issued) == 3 and sorted(consumed) == sorted(issued)
        assert consumed != issued and consumed != issued[::-1]
        assert [op[0] for op in c["seq"][:3]] == ["F", "F", "F"]
    # 5: two slots, the same probe three times, I1 and I2 between the rounds
    (c,) = by[(first, 5)]
    assert c["n_slots"] == 2 and len({op[2] for op in c["seq"] if op[0] == "F"}) == 1 and sum(op[0] == "F" for op in c["seq"]) == 3
    assert sum(op[0] == "I1" for op in c["seq"]) == 2 and sum(op[0] == "I2" for op in c["seq"]) == 2 and sum(op[0] == "Z" for op in c["seq"]) == 2
    # 6: the engine's first pass is I1, I2, I6 or the probe itself
    assert sorted(c["seq"][0][0] for c in by[(first, 6)]) == ["F", "FZ", "I1", "I2"]
    # 7: the gradient is preset between a backward and the probe's backward
    for c in by[(first, 7)]:
        kinds = [op[0] for op in c["seq"]]
        assert kinds.index("B") < kinds.index("G0") and kinds[-2:] == ["G0", "B"]
    assert {c["seq"][2][2] for c in by[(first, 7)]} == set(PC.PROBES[first])
    # 8: retain_graph on the first backward, the refused one right behind it, then more passes
    (c,) = by[(first, 8)]
    i = c["seq"].index(("B!", "A"))
    assert c["seq"][i - 1] == ("B", "A", "retain") and any(op[0] == "F" for op in c["seq"][i + 1:])
    # default mode: ordering 1 with I2 and ordering 2, one case each per model
    assert len(PC.DEFAULT_MODE) == 2 * len(PC.MODELS)
    for model in PC.MODELS:
        mine = [PC.find(cid) for cid in PC.DEFAULT_MODE if PC.find(cid)["model"] == model]
        assert sorted(c["ordering"] for c in mine) == [1, 2] and [c for c in mine if c["ordering"] == 1][0]["labels"] == ("I2",)
    # replay: the first model's single-stream probes only, three rounds, I2 between a forward and its backward, two live tapes
    seq = PC.replay_sequence()
    assert PC.REPLAY_MODEL == first and {PC.PROBES[first][op[2]][2] for op in seq if op[0] == "F"} == {"single"}
    assert sum(op[0] == "I2" for op in seq) == 3 and sum(op[0] == "B" for op in seq) == 9


def test_the_gpu_file_runs_the_whole_table():
    text = open(os.path.join(ROOT, "tests", "test_gpu_pass_order.py")).read()
    assert '@pytest.mark.parametrize("cid", [c["id"] for c in PC.CASES])' in text
    assert '@pytest.mark.parametrize("cid", PC.DEFAULT_MODE)' in text
    assert "pytestmark = pytest.mark.gpu" in text
    assert not re.search(r"skip|xfail", text)
