"""CPU: the designed batch-norm inputs (tests/bn_rows_inputs.py) do what they
are designed for.  float64 is the reference.  On the offset columns (mean
exactly 4096 + k/256 in fp32, variance about 21) the two textbook fp32 schemes
-- one-pass E[x^2] - E[x]^2 and a sequential Welford -- both miss the project's
parity cap 1e-4 * max(1, |ref|) in y, so the GPU test that runs the kernels on
these columns (tests/test_gpu_bn_rows.py) has teeth; the scheme the kernels
use (fp64 sums of the widened x and x * x, combined in block order, rounded
once) meets it with room."""
import numpy as np
import pytest

import bn_rows_inputs as bi

CAP = 1e-4
ROWS, COLS = 4096, 8


def _y(x, mean, var, gamma, beta, eps=1e-5, slope=0.2):
    """The apply pass as the kernels run it: fp32, centred first."""
    f = np.float32
    invstd = (1.0 / np.sqrt(var.astype(np.float64) + eps)).astype(f)
    v = (x - mean.astype(f)) * (gamma * invstd) + beta
    return np.where(v > 0, v, v * f(slope)).astype(f)


def _naive_fp32(x):
    s1 = np.add.accumulate(x, axis=0, dtype=np.float32)[-1]
    s2 = np.add.accumulate(x * x, axis=0, dtype=np.float32)[-1]
    n = np.float32(x.shape[0])
    mean = s1 / n
    return mean, np.maximum(s2 / n - mean * mean, np.float32(0))


def _welford_fp32(x):
    f = np.float32
    mean = np.zeros(x.shape[1], f)
    m2 = np.zeros(x.shape[1], f)
    for i in range(x.shape[0]):
        d = x[i] - mean
        mean = mean + d / f(i + 1)
        m2 = m2 + d * (x[i] - mean)
    return mean, m2 / f(x.shape[0])


def _blocked_fp64(x, block=512):
    """fp64 sums of x and x * x per row block, the blocks added in order."""
    xd = x.astype(np.float64)
    s1 = np.zeros(x.shape[1])
    s2 = np.zeros(x.shape[1])
    for r in range(0, x.shape[0], block):
        s1 += xd[r:r + block].sum(0)
        s2 += (xd[r:r + block] ** 2).sum(0)
    mean = s1 / x.shape[0]
    return mean, np.maximum(s2 / x.shape[0] - mean * mean, 0.0)


def _err(y, ref):
    return float(np.abs(y.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("rows", [2, 5, ROWS, ROWS + 3])
def test_designed_columns_have_their_exact_means(rows):
    x = bi.designed_table(rows, COLS, seed=rows)
    assert x.dtype == np.float32
    mean = x.astype(np.float64).mean(0)
    for j in range(COLS):
        col = x[:, j].astype(np.float64)
        if bi.kind(j) == "offset":
            assert mean[j] == bi.offset_mean(j) and np.float32(mean[j]) == mean[j]
            assert np.array_equal(np.sort(col - mean[j]), np.sort(mean[j] - col))  # symmetric about the mean
        elif bi.kind(j) == "constant":
            assert col.min() == col.max()
        elif bi.kind(j) == "at_mean":
            assert mean[j] == bi.AT_MEAN and (col == bi.AT_MEAN).any()
    g, b = bi.params(COLS)
    assert all(b[j] == 0 for j in range(COLS) if bi.kind(j) == "at_mean")


def test_at_mean_rows_give_an_exact_zero():
    x = bi.designed_table(ROWS, COLS, seed=1)
    g, b = bi.params(COLS)
    ref, mean, var = bi.reference(x, g, b)
    j = 2
    at = x[:, j] == bi.AT_MEAN
    assert 0.1 < at.mean() < 0.5 and (ref[at, j] == 0).all() and (ref[~at, j] != 0).all()


def test_textbook_fp32_schemes_miss_the_cap_and_the_kernels_scheme_meets_it():
    x = bi.designed_table(ROWS, COLS, seed=2)
    g, b = bi.params(COLS)
    ref, mean, var = bi.reference(x, g, b)
    offs = [j for j in range(COLS) if bi.kind(j) == "offset"]
    assert 20.0 < var[offs].min() and var[offs].max() < 23.0
    for name, scheme in (("one-pass fp32", _naive_fp32), ("Welford fp32", _welford_fp32)):
        m, v = scheme(x)
        e_var = float(np.abs(v[offs].astype(np.float64) - var[offs]).max())
        e_y = _err(_y(x, m, v, g, b)[:, offs], ref[:, offs])
        print(f"{name}: max|var - fp64| {e_var:.3e}, y {e_y:.3e} of max(1, |ref|)")
        assert e_y > CAP, f"{name} meets the cap on the offset columns: the designed input has no teeth"
    m, v = _blocked_fp64(x)
    e_y = _err(_y(x, m, v, g, b), ref)
    print(f"blocked fp64 sums: max|var - fp64| {float(np.abs(v - var).max()):.3e}, y {e_y:.3e}")
    assert float(np.abs(v - var).max()) < 1e-8 and e_y < CAP / 100
