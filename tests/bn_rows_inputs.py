"""Designed inputs for the batch-norm-over-rows kernels (grl_bn_rows_*).

designed_table(rows, cols, seed) -> float32 [rows, cols]; column j is of kind
KINDS[j % 4]:

  offset    values 4096 + k/256 +- d, the d's multiples of 1/256 in [-8, 8]
            laid out in +-pairs (an odd row count adds one d = 0), in shuffled
            row order: every value is exact in fp32 (ulp 2^-11 there), the mean
            is EXACTLY 4096 + k/256 (k = the column index), the variance about
            64/3.  sum(x^2) ~ 1.7e7 per row: a one-pass fp32 E[x^2] - E[x]^2
            loses the variance entirely, a sequential fp32 Welford drifts.
  constant  one value: variance exactly 0, invstd = 1/sqrt(eps), y = beta.
  at_mean   small integers symmetric about 3 with about a quarter of the rows
            EXACTLY 3 = the mean: with beta = 0 those give y == 0, where the
            LeakyReLU gradient takes the negative slope (torch's x > 0 rule).
  normal    N(m, s^2) with m, s varying by column.

params(cols, seed) -> gamma, beta (float32 [cols]); beta is 0 in at_mean columns.
"""
import numpy as np

KINDS = ("offset", "constant", "at_mean", "normal")
AT_MEAN = 3.0


def kind(j: int) -> str:
    return KINDS[j % 4]


def offset_mean(j: int) -> float:
    return 4096.0 + j / 256.0


def designed_table(rows: int, cols: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = np.empty((rows, cols), dtype=np.float64)
    half = rows // 2
    for j in range(cols):
        k = kind(j)
        if k == "offset":
            d = rng.integers(-2048, 2049, size=half) / 256.0
            col = np.concatenate([d, -d, np.zeros(rows - 2 * half)]) + offset_mean(j)
            x[:, j] = rng.permutation(col)
        elif k == "constant":
            x[:, j] = 1.5 + (j // 4) * 0.25
        elif k == "at_mean":
            d = rng.integers(1, 6, size=half).astype(np.float64)
            d[rng.random(half) < 0.25] = 0.0
            d[:1] = 0.0  # at least one pair sits on the mean (2 rows: both)
            col = np.concatenate([d, -d, np.zeros(rows - 2 * half)]) + AT_MEAN
            x[:, j] = rng.permutation(col)
        else:
            x[:, j] = rng.normal(rng.uniform(-2, 2), rng.uniform(0.1, 3.0), size=rows)
    out = x.astype(np.float32)
    exact = [j for j in range(cols) if kind(j) != "normal"]
    assert np.array_equal(out[:, exact].astype(np.float64), x[:, exact])  # designed values are fp32 numbers
    return out


def params(cols: int, seed: int = 0):
    rng = np.random.default_rng(seed + 1000)
    gamma = rng.uniform(0.5, 1.5, cols).astype(np.float32) * np.where(rng.random(cols) < 0.3, -1, 1).astype(np.float32)
    beta = rng.normal(0, 0.5, cols).astype(np.float32)
    for j in range(cols):
        if kind(j) == "at_mean":
            beta[j] = 0.0
    return gamma, beta


def reference(x, gamma, beta, eps=1e-5, slope=0.2):
    """float64 numpy statement of the forward: (y, mean, biased variance)."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    v = (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return np.where(v > 0, v, v * slope), mean, var
