"""CPU: the misaligned- and overlapping-pointer refusals of ocl_ewc_fisher_ema / ocl_ewc_fisher_normalize under test ids that do not
change from one process to the next.

tests/test_cpu_ewc.py::test_ema_and_normalize_refuse_bad_arguments_without_a_device writes the pointer VALUE of each such case into its
test id (`_ema-r=140141234762292`): the value is the address of a ctypes buffer, which the operating system places elsewhere in every
process, so those twelve ids never occur twice and a run cannot be compared with another one by id.  The same twelve cases are stated
here by their offset from that buffer (`_ema-r=A+4`); the callers and the buffer are that module's own."""
import pytest

import test_cpu_ewc as E

MB = E.MB
CASES = [
    ("_ema", "r", 4, "A+4"), ("_ema", "t", MB + 8, "A+MB+8"),                                       # misaligned
    ("_ema", "t", 0, "A"), ("_ema", "t", 48, "A+48"), ("_ema", "r", MB - 16, "A+MB-16"),            # overlapping: on it, inside it, ending inside it
    ("_normalize", "r", 4, "A+4"), ("_normalize", "f", MB + 8, "A+MB+8"), ("_normalize", "ws", 5 * MB + 2, "A+5*MB+2"),
    ("_normalize", "f", 0, "A"), ("_normalize", "f", 48, "A+48"), ("_normalize", "ws", 32, "A+32"), ("_normalize", "mm", 16, "A+16"),
]


@pytest.mark.parametrize("call,key,offset", [c[:3] for c in CASES], ids=["%s-%s=%s" % (c[0], c[1], c[3]) for c in CASES])
def test_ema_and_normalize_refuse_misplaced_pointers_without_a_device(call, key, offset):
    rc, msg = getattr(E, call)(**{key: E.A + offset})
    assert rc == E.OCL_ERR_ARG, (rc, msg)
    assert msg.startswith("ewc:"), msg
    assert ("aligned" in msg) or ("overlap" in msg), msg
