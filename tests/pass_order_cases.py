"""Case table of the pass-ordering tests (tests/test_gpu_pass_order.py runs it on the GPU, tests/test_cpu_pass_order.py checks it
without one): which passes meet on one engine, in which order, and with how many tape slots.

A sequence is a list of operations on ONE engine:

    ("F", tape, probe)          taped train-mode forward of a probe pass (a member of test_gpu_net.CASES); updates the running statistics
    ("B", tape)                 its backward (("B", tape, "retain"): with retain_graph=True)
    ("B!", tape)                a second backward through a consumed tape: must raise RuntimeError and change nothing
    ("FZ", tape, n)             frozen-BatchNorm tape: model.eval(), forward under autograd (intruder I6)
    ("BZ", tape)                its backward
    ("DROP", tape)              the tape is abandoned: no backward will follow
    ("Z",)                      zero_grad: the next backward overwrites
    ("G0",)                     the flat gradient is overwritten in place with a seeded random array
    ("I1", n)                   eval-mode feature pass under no_grad (features_batched)
    ("I2", n) / ("I3", n)       forward_with_params(x, 1.05 * flat_params) in train / eval mode: the arena holds another array's packs
    ("I2p", n)                  the same train-mode pass through the C ABI with OCL_FWD_PACK_ALL: the data-gradient packs are the other array's too
    ("I4", n)                   forward_stats_only: updates the running statistics
    ("I5", n)                   train-mode forward under no_grad (scratch slot): updates the running statistics

Whether a backward overwrites or accumulates follows from the sequence (a "Z" or the start of the engine's life in front of it: overwrite),
so one runner checks both laws: overwrite -> the isolated result, accumulate -> float32(existing) + float32(isolated), bit for bit.

Through resnet.py a pass on another parameter array writes the forward layouts only, which lie beside the data-gradient packs in the arena:
after I1, I2 and I3 the backward re-packs (pack_src / pack_have say so) but would read the same bytes without.  I2p is the call that makes
the backward's `repack` branch carry weight: after it the packs the backward reads are those of the other array.

Tape slots are handed out round robin, whether the tapes in between are still alive or not: a tape survives n_slots - 1 later taped
forwards.  `check_sequence` holds every case to that (and to the weaker statement that live tapes never exceed n_slots)."""

# model key -> (agent, data, head, input height = width, max_batch of every engine of the model)
MODELS = {
    "er_c100": ("ER", "cifar100", None, 32, 100),
    "scr_c100": ("SCR", "cifar100", "mlp", 32, 64),
    "er_mini": ("ER", "mini_imagenet", None, 84, 64),
}

# model key -> probe name -> (images, BatchNorm groups, stream regime of the backward, head dW / side-stream forward)
PROBES = {
    "er_c100": {"a10": (10, 1, "single", False), "a3": (3, 1, "single", False), "a100": (100, 1, "two", True)},
    "scr_c100": {"s14": (14, 2, "single", False), "s36": (36, 2, "single", False), "s50": (50, 2, "two", False)},
    "er_mini": {"m6": (6, 1, "single", False), "m20": (20, 2, "two", True)},
}

# (small probe A, another small probe B, two-stream probe) per model
ROLES = {"er_c100": ("a10", "a3", "a100"), "scr_c100": ("s14", "s36", "s50"), "er_mini": ("m6", None, "m20")}

I1_SIZES = (12, 33)        # plans of 12 and of 48 images (eval-mode plans are bucketed to 16 images above 16)
I2_N, I4_N, I5_N = 7, 10, 5
I6_SIZES = (1, 10)


def case_probe(model, probe):
    """The probe as a row of test_gpu_net.CASES."""
    agent, data, head, _, _ = MODELS[model]
    n, groups, _, _ = PROBES[model][probe]
    return (agent, data, head, n, groups)


def intruders(model):
    """name -> operations of one intruder; each owns no live tape when it is over."""
    a, b, big = ROLES[model]
    other = b or big        # I7: a second train tape of another probe size, abandoned
    out = {}
    for n in I1_SIZES:
        out["I1n%d" % n] = [("I1", n)]
    out["I2"] = [("I2", I2_N)]
    out["I3"] = [("I3", I2_N)]
    out["I4"] = [("I4", I4_N)]
    out["I5"] = [("I5", I5_N)]
    for n in I6_SIZES:
        out["I6n%d_abandoned" % n] = [("FZ", "z%da" % n, n), ("DROP", "z%da" % n)]
        # (its gradient goes into a gradient that is zeroed afterwards)
        out["I6n%d_backprop" % n] = [("FZ", "z%db" % n, n), ("BZ", "z%db" % n), ("Z",)]
    out["I7"] = [("F", "i7", other), ("DROP", "i7")]
    out["I2p"] = [("I2p", I2_N)]      # (last: in the row of all intruders no taped forward re-packs behind it)
    return out


def _n_slots(seq):
    """Smallest n_slots the sequence is well formed with (round-robin slots)."""
    need, pos, k = 1, {}, 0
    for op in seq:
        if op[0] in ("F", "FZ"):
            pos[op[1]] = k
            k += 1
        elif op[0] in ("B", "BZ"):
            need = max(need, k - pos[op[1]])
    return max(need, 2)


def _case(cid, model, ordering, seq, n_slots=None, labels=()):
    return dict(id=cid, model=model, ordering=ordering, seq=list(seq), n_slots=n_slots or _n_slots(seq), labels=tuple(labels))


def _build():
    cases = []
    for model in MODELS:
        a, b, big = ROLES[model]
        second = b or big
        intr = intruders(model)
        # 1. F(A) . one intruder . B(A), then all intruders in a row
        for name, ops in intr.items():
            cases.append(_case("%s-o1-%s" % (model, name), model, 1, [("F", "A", a)] + ops + [("B", "A")], labels=(name,)))
        row = [op for ops in intr.values() for op in ops]
        cases.append(_case("%s-o1-all" % model, model, 1, [("F", "A", a)] + row + [("B", "A")], labels=("all",)))
        # 2. two live tapes, both orders, with and without zero_grad between the backwards (the second backward: bsums_dirty)
        for order, (x, y) in (("ab", ("A", "B")), ("ba", ("B", "A"))):
            for z in (True, False):
                seq = [("F", "A", a), ("F", "B", second), ("B", x)] + ([("Z",)] if z else []) + [("B", y)]
                cases.append(_case("%s-o2-%s-%s" % (model, order, "zero" if z else "acc"), model, 2, seq, labels=("two_tapes", "zero" if z else "acc")))
        # 4. two-stream backward, an eval feature pass issued as soon as it returns on the host, then the small tape's backward
        small = a
        seq = [("F", "A", big), ("F", "B", small), ("B", "A"), ("I1", I1_SIZES[0]), ("I1", I1_SIZES[1]), ("B", "B")]
        cases.append(_case("%s-o4-%s" % (model, big), model, 4, seq, labels=("two_stream", "acc")))
    model = "er_c100"
    a, b, big = ROLES[model]
    # 3. three live tapes consumed in an order that is neither issue order nor its reverse
    for z in (True, False):
        zz = [("Z",)] if z else []
        seq = [("F", "A", a), ("F", "B", b), ("F", "C", big), ("B", "B")] + zz + [("B", "C")] + zz + [("B", "A")]
        cases.append(_case("%s-o3-bca-%s" % (model, "zero" if z else "acc"), model, 3, seq, n_slots=3, labels=("zero" if z else "acc",)))
    # 5. rotation: the same probe three times with I1 and I2 between the rounds; two tape slots, each met first and again
    seq = []
    for r in range(3):
        seq += ([("Z",), ("I1", I1_SIZES[0]), ("I2", I2_N)] if r else []) + [("F", "R%d" % r, a), ("B", "R%d" % r)]
    cases.append(_case("%s-o5-rotation" % model, model, 5, seq, n_slots=2))
    # 6. first-pass branches: pack_need_bwd is still 0 at the engine's first forward
    first = {"I1": [("I1", I1_SIZES[0])], "I2": [("I2", I2_N)], "I6": [("FZ", "z", I6_SIZES[1]), ("BZ", "z"), ("Z",)]}
    for name, ops in first.items():
        cases.append(_case("%s-o6-first-%s" % (model, name), model, 6, ops + [("F", "A", a), ("B", "A")], labels=(name,)))
    cases.append(_case("%s-o6-first-probe" % model, model, 6, [("F", "A", a), ("B", "A"), ("Z",), ("F", "A2", a), ("B", "A2")]))
    # 7. accumulation into a preset gradient
    for p in (a, b, big):
        other = b if p == a else a
        cases.append(_case("%s-o7-preset-%s" % (model, p), model, 7, [("F", "B", other), ("B", "B"), ("F", "A", p), ("G0",), ("B", "A")], labels=("acc",)))
    # 8. a consumed tape: the second backward is an error return; the gradient stays, the engine serves the next pass
    seq = [("F", "A", a), ("B", "A", "retain"), ("B!", "A"), ("F", "A2", b), ("B", "A2"), ("Z",), ("F", "A3", a), ("B", "A3")]
    cases.append(_case("%s-o8-consumed" % model, model, 8, seq))
    return cases


CASES = _build()

# deterministic mode off: ordering 1 with I2 and ordering 2 (zero_grad between the backwards), one case each per model
DEFAULT_MODE = ["%s-o1-I2" % m for m in MODELS] + ["%s-o2-ba-zero" % m for m in MODELS]

# launch-sequence replay: ordering 1 with I2 and ordering 2 on the first model's single-stream probes, three rounds on one engine
REPLAY_MODEL = "er_c100"
REPLAY_SLOTS = 3      # three taped forwards per round: every tape meets the same slot in every round, so its replay key comes back


def replay_sequence():
    a, b, _ = ROLES[REPLAY_MODEL]
    seq = []
    for r in range(3):
        seq += [("F", "A%d" % r, a), ("I2", I2_N), ("B", "A%d" % r), ("Z",),
                ("F", "B%d" % r, a), ("F", "C%d" % r, b), ("B", "B%d" % r), ("B", "C%d" % r), ("Z",)]
    return seq


def find(cid):
    hit = [c for c in CASES if c["id"] == cid]
    assert len(hit) == 1, cid
    return hit[0]


def check_sequence(seq, n_slots, probes):
    """Well-formedness: every tape is forwarded once, then consumed once or abandoned explicitly (a "B!" follows a consumed tape);
    no backward meets a slot that a later taped forward has taken (round robin over n_slots); live tapes never exceed n_slots.
    Returns the largest number of live tapes."""
    issued, state, live, peak = {}, {}, 0, 0
    k = 0
    for op in seq:
        kind = op[0]
        if kind in ("F", "FZ"):
            tape = op[1]
            assert tape not in state, "tape %s forwarded twice" % tape
            if kind == "F":
                assert op[2] in probes, "unknown probe %s" % (op[2],)
            issued[tape], state[tape] = k, "live:" + kind
            k += 1
            live += 1
            peak = max(peak, live)
        elif kind in ("B", "BZ"):
            tape = op[1]
            assert state.get(tape) == "live:" + ("F" if kind == "B" else "FZ"), "backward through %s, which is %s" % (tape, state.get(tape))
            assert k - issued[tape] <= n_slots, "tape %s was overwritten: %d taped forwards since, %d slots" % (tape, k - issued[tape] - 1, n_slots)
            state[tape] = "consumed"
            live -= 1
        elif kind == "B!":
            assert state.get(op[1]) == "consumed", "B! needs a consumed tape"
            assert k - issued[op[1]] <= n_slots, "the error must be the engine's (tape consumed), not the slot bookkeeping's"
        elif kind == "DROP":
            assert state.get(op[1], "").startswith("live"), "DROP of %s, which is %s" % (op[1], state.get(op[1]))
            state[op[1]] = "abandoned"
            live -= 1
        else:
            assert kind in ("Z", "G0", "I1", "I2", "I2p", "I3", "I4", "I5"), "unknown operation %s" % (op,)
    left = [t for t, s in state.items() if s.startswith("live")]
    assert not left, "tapes neither consumed nor abandoned: %s" % left
    assert peak <= n_slots, "%d live tapes, %d slots" % (peak, n_slots)
    return peak
