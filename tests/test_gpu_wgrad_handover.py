"""GPU: the hand-over schedule of the large-pass backward changes WHEN the weight gradients are issued and on which stream, never what they
compute.  One training pass of `csrc/netcheck` (a consumer of the C-ABI alone, OCL_DETERMINISTIC=1) per setting, every setting a process
of its own (the switches are read once per process); every gradient, output and running statistic is compared bit for bit with the
default's.

  128 images in two groups: the smallest pass that takes the coarse hand-over (three layers per event pair);
  192 images in two groups: the smallest pass at which layer 1 plans the 4x4x1 weight-gradient form (192 * 1024 pixels = 6 * 128 * 256);
   48 images: the two-stream threshold, below the coarse path -- the settings do nothing there.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "online-continual-learning_amd", "csrc")
NETCHECK = os.path.join(CSRC, "netcheck")


def _run(cfg, mode, path, env):
    if not os.path.exists(NETCHECK):
        subprocess.run(["make", "-C", CSRC, "netcheck"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([NETCHECK] + [str(v) for v in cfg] + [mode, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OCL_DETERMINISTIC="1", **env))
    return r.returncode, r.stdout + r.stderr


# (images, BatchNorm groups, input size, head)
SIZES = [(128, 2, 32, 1), (192, 2, 32, 1), (48, 2, 32, 1)]
SETTINGS = [{"OCL_WGRAD_FLUSH_TAIL": "0"}, {"OCL_WGRAD_FLUSH_TAIL": "21"}, {"OCL_WGRAD_FLUSH": "1"}, {"OCL_SINGLE_STREAM": "1"}]
_refs = {}


@pytest.fixture(scope="module")
def ref_of(tmp_path_factory):
    """The default schedule's result per pass size: written once, compared by every setting."""
    def get(cfg):
        if cfg not in _refs:
            path = str(tmp_path_factory.mktemp("handover") / ("ref_n%d.bin" % cfg[0]))
            rc, out = _run(cfg, "write", path, {})
            assert rc == 0, out
            _refs[cfg] = path
        return _refs[cfg]
    return get


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: "_".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("cfg", SIZES, ids=lambda c: "n%d_g%d_hw%d_head%d" % c)
def test_hand_over_schedule_is_bit_identical_to_the_default(cfg, env, ref_of):
    rc, out = _run(cfg, "compare", ref_of(cfg), env)
    assert rc == 0, out
    m = re.search(r"(\d+) of (\d+) tensors differ in some bit", out)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) >= 60, out
