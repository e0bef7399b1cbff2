"""The two yardsticks of the kernel parity suites against float64 (tests/test_gpu_small_ops.py, tests/test_gpu_aux.py), and their report rows.

* check_derived: a bound derived from the operation (sums of products: 1.01 * K * 2^-24 * sum|terms|, K the number of fp32-accumulated terms);
* check_vs_torch32: the same formula evaluated by plain torch-CPU fp32 on the same inputs has error e_ref against float64 (max over the tensor);
  the kernel's must be <= max(4 * e_ref, 4 ulp of the largest |reference| element).
Each appends (case, tensor, kernel error, e_ref or '-', bound, error / bound) to the caller's report list before it asserts; for a per-element
bound the row is the element with the largest error / bound."""
import numpy as np

U = 2.0 ** -24


def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 2.0 ** -149


def record(report, case, tensor, err, e_ref, bound):
    report.append((case, tensor, err, "-" if e_ref is None else "%.4g" % e_ref, bound, err / bound if bound else (0.0 if err == 0 else float("inf"))))


def check_vs_torch32(report, case, tensor, got, ref64, ref32, cap=None):
    """Transcendental kernels: error <= max(4 * e_ref, 4 ulp of the largest |reference| element)."""
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    assert np.isfinite(got).all(), "%s %s: non-finite output" % (case, tensor)
    err = float(np.abs(got - ref64).max())
    e_ref = float(np.abs(ref32 - ref64).max())
    bound = max(4 * e_ref, 4 * ulp32(np.abs(ref64).max()))
    if cap is not None:
        bound = min(bound, cap)
    record(report, case, tensor, err, e_ref, bound)
    print("%s %s: kernel error %.4g, torch fp32 error %.4g, bound %.4g" % (case, tensor, err, e_ref, bound))
    assert err <= bound, "%s %s: error %.4g against float64 exceeds %.4g (torch fp32: %.4g)" % (case, tensor, err, bound, e_ref)


def check_derived(report, case, tensor, got, ref64, bound):
    got, ref64, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref64, bound))
    assert np.isfinite(got).all(), "%s %s: non-finite output" % (case, tensor)
    err = np.abs(got - ref64)
    bound = np.broadcast_to(bound, err.shape)
    # the reported element is the one closest to (or farthest past) its bound: the largest err / bound; an element whose bound is 0 must be exact
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    e, b = float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])
    record(report, case, tensor, e, None, b)
    print("%s %s: element closest to its bound: error %.4g, bound %.4g" % (case, tensor, e, b))
    assert (err <= bound).all(), "%s %s: error %.4g exceeds the derived bound %.4g" % (case, tensor, e, b)
