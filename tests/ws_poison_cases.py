"""Case table of the workspace-poison tests (tests/test_gpu_ws_poison.py runs it on the GPU, tests/test_cpu_ws_poison.py checks it without
one): which passes an engine runs as the FIRST passes of its life, over a workspace that holds one of PATTERNS in every 32-bit word.

The law: no stored result of a pass -- output, features, flat gradient, running statistics, num_batches_tracked -- depends on a byte that
neither this pass nor bind-time initialisation wrote.  The reference of every case is the same pass on an engine whose workspace was zeroed.

Two forms of case:

    kind "seq"      a sequence of tests/pass_order_cases.py operations: run by test_gpu_pass_order.execute, held to the isolated results by
                    test_gpu_pass_order.verify (which then come from zero-filled engines);
    any other kind  a pass whose result `execute` throws away (features, the forward_with_params output ...) or that it has no operation
                    for (forward_views_taped, a same_weights() block, the 50 x 50 and 128 x 128 inputs): run by test_gpu_ws_poison.run_direct,
                    every array it returns compared with the zero-filled engine's.

`claims` names the pass_order_cases operation kinds a case exercises on poisoned memory; test_cpu_ws_poison.py holds their union to every
kind that occurs in pass_order_cases.CASES, so a pass kind added there cannot stay without a poison case."""
import pass_order_cases as PC

# name -> 32-bit word
PATTERNS = {
    "nan": 0xFFFFFFFF,       # a NaN; -1 / UINT_MAX for anything read as an integer (an arrival counter)
    "inf": 0x7F800000,       # +inf: times a zero weight it is a NaN, added to anything it stays visible
    "f4096": 0x45800000,     # 4096.0, the slack value of the layer tests: finite, so it shows only accumulation onto unwritten memory
}

# pass_order_cases.MODELS and the two inputs whose lattice is odd at every level (50 -> 25 -> 13 -> 7) or has the longest rows (128),
# with the engines tests/test_gpu_datasets.py builds for them
MODELS = dict(PC.MODELS)
MODELS["er_loris"] = ("ER", "openloris", None, 50, 8)
MODELS["er_core50"] = ("ER", "core50", None, 128, 4)

EVAL_BUCKETS = (1, 3, 5, 12, 17, 33)      # eval plans are made for 4, 4, 8, 12, 32 and 48 images (net.hip: Nplan)
FROZEN_N = PC.I6_SIZES


def _seq(cid, model, seq, n_slots=2):
    claims = tuple(sorted(set(op[0] for op in seq)))
    return dict(id=cid, model=model, kind="seq", seq=list(seq), n_slots=n_slots, claims=claims)


def _direct(cid, model, kind, claims=(), **kw):
    return dict(id=cid, model=model, kind=kind, n_slots=2, claims=tuple(claims), **kw)


def _build():
    cases = []
    # every probe, forward then backward
    for model, probes in PC.PROBES.items():
        for probe in probes:
            cases.append(_seq("%s-probe-%s" % (model, probe), model, [("F", "A", probe), ("B", "A")]))
    # the frozen-BatchNorm tape and its backward
    for n in FROZEN_N:
        cases.append(_seq("er_c100-frozen-n%d" % n, "er_c100", [("FZ", "z", n), ("BZ", "z")]))
    # eval feature passes at every plan bucket
    for n in EVAL_BUCKETS:
        cases.append(_direct("er_c100-features-n%d" % n, "er_c100", "features", claims=("I1",), n=n))
    cases.append(_direct("scr_c100-features-n5", "scr_c100", "features", claims=("I1",), n=5))
    cases.append(_direct("er_c100-with-params-train", "er_c100", "with_params", claims=("I2",), n=PC.I2_N, train=True))
    cases.append(_direct("er_c100-with-params-eval", "er_c100", "with_params", claims=("I3",), n=PC.I2_N, train=False))
    cases.append(_direct("er_c100-stats-only", "er_c100", "stats_only", claims=("I4",), n=PC.I4_N))
    cases.append(_direct("er_c100-train-no-grad", "er_c100", "no_grad", claims=("I5",), n=PC.I5_N))
    cases.append(_direct("scr_c100-views-taped", "scr_c100", "taped", n=14, groups=2))
    cases.append(_direct("er_c100-views-taped", "er_c100", "taped", n=20, groups=2))
    # three and four BatchNorm groups: every BatchNorm backward is the reduce + apply pair, whose sums lie in the front part of off_bsums
    # (barena_off) -- cells no default-mode pass of one or two groups accumulates into
    cases.append(_direct("scr_c100-views-taped-g3", "scr_c100", "taped", n=9, groups=3))
    cases.append(_direct("er_c100-views-taped-g4", "er_c100", "taped", n=12, groups=4))
    cases.append(_direct("er_c100-same-weights", "er_c100", "same_weights", n=12))
    # a second, accumulating backward (two live tapes: the second backward clears the statistics arena itself), a preset gradient,
    # a refused backward -- and the row of all intruders, once
    for cid in ("er_c100-o2-ab-acc", "er_c100-o7-preset-a10", "er_c100-o8-consumed", "er_c100-o1-all"):
        c = PC.find(cid)
        cases.append(_seq(cid, c["model"], c["seq"], c["n_slots"]))
    # the odd shapes: the smallest batches that reach the planner forms tests/datasets_cases.py lists at these sizes
    cases.append(_direct("er_loris-train-n3", "er_loris", "train", n=3, groups=1))
    cases.append(_direct("er_loris-eval-n1", "er_loris", "features", n=1))
    cases.append(_direct("er_core50-train-n2", "er_core50", "train", n=2, groups=1))
    return cases


CASES = _build()
IDS = [c["id"] for c in CASES]


def find(cid):
    hit = [c for c in CASES if c["id"] == cid]
    assert len(hit) == 1, cid
    return hit[0]


def claimed():
    out = set()
    for c in CASES:
        out.update(c["claims"])
    return out


def pass_order_kinds():
    """Every operation kind that occurs in a sequence of pass_order_cases (the replay sequence included)."""
    kinds = set(op[0] for c in PC.CASES for op in c["seq"])
    kinds.update(op[0] for op in PC.replay_sequence())
    return kinds


# C ABI (csrc/netcheck, NETCHECK_WS_FILL): run-time modes and passes; the 220-view pass runs in the default mode only
NETCHECK_MODES = [{}, {"OCL_WGRAD_Q": "0"}, {"OCL_WGRAD_MULTI": "0"}, {"OCL_DY_KEEP": "0"}, {"OCL_BN_CHAN": "0"}, {"OCL_SINGLE_STREAM": "1"},
                  {"OCL_GRAPH": "1"}]
NETCHECK_CASES = [(20, 2, 32, 0), (6, 2, 84, 1), (9, 3, 32, 1)]
NETCHECK_DEFAULT_ONLY = [(220, 2, 32, 1)]
