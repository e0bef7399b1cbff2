"""CPU: the parity suite of the glue kernels and the head chain (tests/test_gpu_aux.py) covers what csrc/conv_aux.hip and the two
BatchNorm helpers of csrc/bn.hip can do.

* every __global__ kernel of conv_aux.hip, and bn_fold_kernel / bn_apply_saved_kernel, is claimed by a case of tests/aux_cases.py;
* every REQUIRED_KEYS entry is claimed, case names are unique, and the GPU file parametrizes every case of the table, unsliced;
* each "above the cap" case launches more work than the launcher's capped grid covers in one stride -- the cap (workgroups x work items per
  workgroup) is parsed from the launcher in the source, not restated here -- and the avgpool cases reach the backward's y-grid of 2 and its cap;
* ocl_net_backward and ocl_test_head call the same head-backward function, and the header documents no debug stop net.hip does not implement;
* the hooks' host-only halves (table export, side-stream threshold, argument checks) answer without a GPU."""
import ctypes as C
import os
import re

import pytest

import aux_cases as AC
from conftest import ROOT
import ocl_amd  # noqa: F401
from ocl_amd import ffi

CSRC = os.path.join(ROOT, "online-continual-learning_amd", "csrc")
KERNEL_RE = r"__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?(\w+)\s*\("


def src(name):
    return open(os.path.join(CSRC, name)).read()


def body_of(text, signature):
    """The text of the function whose definition starts with `signature`, braces balanced."""
    i = text.index(signature)
    j = text.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        if depth == 0:
            return text[i:k + 1]
        k += 1


def launcher_cap(name):
    """(max workgroups in x, work items one workgroup covers per stride) of a grid-stride launcher, from its source."""
    text = src("bn.hip") if name == "launch_bn_apply_saved" else src("conv_aux.hip")
    body = body_of(text, "int %s(" % name)
    caps = [int(v) for v in re.findall(r"std::min(?:<int64_t>)?\((\d+),", body)]
    assert len(caps) == 1, (name, caps)
    block = [int(v) for v in re.findall(r"dim3\((\d+)\), 0, s", body)]
    assert len(block) == 1, (name, block)
    return caps[0], block[0]


def test_every_kernel_is_claimed():
    kernels = set(re.findall(KERNEL_RE, src("conv_aux.hip")))
    assert len(kernels) == 10, sorted(kernels)
    claimed = {k for cases in AC.CASES.values() for c in cases for k in c["kernels"]}
    assert kernels - claimed == set(AC.EXEMPT_KERNELS), sorted(kernels - claimed)
    bn = set(re.findall(KERNEL_RE, src("bn.hip")))
    assert set(AC.BN_KERNELS) <= bn, sorted(bn)
    assert set(AC.BN_KERNELS) <= claimed
    assert claimed <= kernels | set(AC.BN_KERNELS), sorted(claimed - kernels)
    assert set(AC.OPS) == set(AC.CASES)
    # a layout case reaches the kernel its segment count selects (one segment: the plain kernel, launch_nchw3_to_nhwc4_segments)
    assert "if (sg.n == 1) return launch_nchw3_to_nhwc4(" in src("conv_aux.hip")
    for c in AC.LAYOUT:
        assert c["kernels"] == (AC.PLAIN if len(c["ns"]) == 1 else AC.SEG), c["name"]
        assert 1 <= len(c["ns"]) <= 8 and min(c["ns"]) >= 1


def test_every_required_key_is_claimed_and_names_are_unique():
    for op, cases in AC.CASES.items():
        names = [c["name"] for c in cases]
        assert len(names) == len(set(names)), op
    seeds = [c["seed"] for cases in AC.CASES.values() for c in cases]
    assert len(seeds) == len(set(seeds))
    keys = set(AC.all_keys())
    missing = [k for k in AC.REQUIRED_KEYS if k not in keys]          # exact: "layout:1_segment" is not claimed by "layout:1_segment_84"
    assert not missing, missing
    assert len(AC.REQUIRED_KEYS) == len(set(AC.REQUIRED_KEYS))
    # the data keys are claimed by the cases whose sizes can hold such data
    for c in AC.L2NORM:
        assert ("l2norm:zero_row" in c["also"]) == (c["n"] >= 7), c["name"]
    for c in AC.HEAD:
        assert ("head:zero_feat_row" in c["also"]) == (c["kind"] in (2, 3) and (c["n"] == "side" or c["n"] >= 2)), c["name"]
        assert ("head:dead_h1_columns" in c["also"]) == (c["kind"] == 1), c["name"]


def test_the_gpu_file_runs_every_case():
    txt = open(os.path.join(ROOT, "tests", "test_gpu_aux.py")).read()
    for op in AC.CASES:
        assert re.search(r'@case_of\("%s"\)' % op, txt), "no test of tests/test_gpu_aux.py is parametrized over the %s cases" % op
    assert re.search(r"def case_of\(op\):\n    return pytest\.mark\.parametrize\(\"name\", AC\.ids\(op\)\)", txt)
    assert "pytest.mark.skip" not in txt and "xfail" not in txt


def test_cases_above_the_cap_exceed_the_cap_of_the_source():
    capped = [c for cases in AC.CASES.values() for c in cases if "cap" in c]
    launchers = {c["cap"][0] for c in capped}
    assert launchers == {"launch_nchw3_to_nhwc4", "launch_nchw3_to_nhwc4_segments", "launch_relu_bwd", "launch_fill", "launch_bn_apply_saved"}
    for c in capped:
        name, work = c["cap"]
        groups, block = launcher_cap(name)
        per_group = block
        if name == "launch_bn_apply_saved":   # its grid is sized in units of 1024 (4 per thread) and strides by 256
            per_group = int(re.search(r"\(units \+ (\d+)\) / (\d+)\)", body_of(src("bn.hip"), "int launch_bn_apply_saved(")).group(2))
        assert work > groups * per_group, "%s: %d work items do not exceed the cap %d x %d of %s" % (c["name"], work, groups, per_group, name)
        assert work <= 2 * groups * per_group + 4096, "%s: larger than the cap needs" % c["name"]
    # the work counts the cases state are the ones their sizes give
    for c in AC.LAYOUT:
        if "cap" in c:
            assert c["cap"][1] == sum(c["ns"]) * c["hw"] ** 2
    for c in AC.RELU_BWD + AC.FILL:
        if "cap" in c:
            assert c["cap"][1] == c["n"]
    for c in AC.BN_APPLY:
        if "cap" in c:
            assert c["cap"][1] == c["m"] * (c["c"] // 4)
    # cases below the cap exist for every capped launcher as well
    assert any("cap" not in c for c in AC.RELU_BWD) and any("cap" not in c for c in AC.BN_APPLY)


def test_avgpool_cases_reach_both_y_grids_of_the_backward():
    body = body_of(src("conv_aux.hip"), "int launch_avgpool_bwd(")
    m = re.search(r"std::max\(1, std::min\((\d+), cdiv\(H \* W \* C, (\d+)\)\)\)", body)
    assert m, body
    cap, per = int(m.group(1)), int(m.group(2))
    rows = set()
    for c in AC.AVGPOOL:
        want = max(1, min(cap, -(-c["h"] * c["w"] * c["c"] // per)))
        assert want == c["ygrid"], c["name"]
        rows.add((want, -(-c["h"] * c["w"] * c["c"] // per) > cap))
    assert (2, False) in rows and (cap, True) in rows, rows
    assert any(c["h"] % 4 for c in AC.AVGPOOL) and any(c["n"] > 1 for c in AC.AVGPOOL)


def test_backward_and_hook_share_one_head_backward():
    net = src("net.hip")
    assert len(re.findall(r"\n(?:static )?int head_backward\(", net)) == 1
    for fn in ("int ocl_net_backward(", "int ocl_test_head("):
        body = body_of(net, fn)
        assert len(re.findall(r"\bhead_backward\(", body)) == 1, fn
        for launcher in ("launch_l2norm_bwd", "launch_relu_bwd", "launch_colsum", "launch_fill"):
            assert launcher not in body, "%s launches %s itself" % (fn, launcher)
    assert "head_forward(" in body_of(net, "int ocl_test_head(")
    # the thresholds are read, not restated: each constant is defined once and the hook's file holds no second number for it
    assert len(re.findall(r"kTwoStreamMinBatch\s*=", net)) == 1 and len(re.findall(r"kSideExtraMinBatch\s*=", net)) == 1
    header = open(os.path.join(ROOT, "include", "ocl_hip.h")).read()
    assert "990" not in header


def test_hooks_answer_on_the_host():
    lib = ffi.lib()
    for hw in (32, 84):
        sizes = (ffi.i64 * 2)()
        table = (ffi.i64 * (9 * 32))()
        n = lib.ocl_test_pack_all(hw, 20, 3, None, None, None, 0, None, 0, table, 32, sizes, None)
        assert n == 20, lib.ocl_last_error()
        rows = [tuple(table[9 * l: 9 * l + 9]) for l in range(n)]
        assert rows[0][3:6] == (20, 3, 9) and rows[0][2] == -1 and rows[0][6] == 4          # the stem: no data-gradient pack, Cin padded to 4
        assert sum(1 for r in rows if r[5] == 1) == 3                                      # three projection shortcuts
        assert all(r[1] >= 0 and (r[2] >= 0 or r[4] == 3) for r in rows)
        ends = sorted([(r[1], r[1] + r[5] * r[6] * r[7]) for r in rows] + [(r[2], r[2] + r[5] * r[3] * r[8]) for r in rows if r[2] >= 0])
        assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= sizes[1], "packs overlap or leave the arena"
        net = C.c_void_p()
        d = ffi.NetDesc(hw, hw, 20, 10, 0, 0, 1, 1)
        assert lib.ocl_net_create(C.byref(d), C.byref(net)) == 0
        assert sizes[0] == lib.ocl_net_param_count(net)
        lib.ocl_net_destroy(net)
    assert lib.ocl_test_pack_all(32, 20, 0, None, None, None, 0, None, 0, None, 0, None, None) < 0
    assert lib.ocl_test_pack_all(32, 20, 3, None, None, None, 5, None, 0, None, 0, None, None) < 0
    if "OCL_SIDE_EXTRA_MIN" not in os.environ and os.environ.get("OCL_SINGLE_STREAM") != "1":
        n32, n84 = lib.ocl_test_head_side_min_batch(32), lib.ocl_test_head_side_min_batch(84)
        assert 1 < n84 < n32 and (n84 - 1) * 84 * 84 < n32 * 1024 <= n84 * 84 * 84, (n32, n84)
    assert lib.ocl_test_aux(0, None, None) < 0
    assert lib.ocl_test_head(None, None) < 0
