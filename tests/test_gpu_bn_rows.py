"""GPU: batch norm over rows + LeakyReLU (grl.ops.batchnorm_rows over
grl_bn_rows_fwd_train / _fwd_eval / _bwd) against torch's float64 batch_norm +
leaky_relu autograd (with an exact mean: torch_chain) on the designed tables of tests/bn_rows_inputs.py: an
offset column (mean exactly 4096 + k/256, where one-pass fp32 formulas and an
fp32 Welford miss the cap: tests/test_bn_rows_design.py), a constant column, a
column with rows exactly at the mean and beta = 0 (y == 0: the gradient takes
the slope) and normal columns.

Cap: max|d| <= 1e-4 * max(1, |ref|), the project's parity rule
(tests/test_gpu_model.py).  Each test prints the measured error and the error
of torch's own fp32 chain on the same inputs.

Shapes: the listed ones, and one on each side of every boundary of the
kernels' geometry (csrc/bn_rows.hip): column lanes 8/16/32/64 switch above 32,
64, 128 columns, a second column tile starts above 256; a row block holds
16 rows per row lane (512 rows at <= 32 columns, 64 rows from 129 columns on),
and above 1024 blocks the blocks grow instead (65536 rows at 256 columns)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_rows_inputs as bi
from grl import GrlError
from grl.ops import batchnorm_rows, batchnorm_rows_bwd, batchnorm_rows_fwd_eval, batchnorm_rows_fwd_train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
EPS, MOM = 1e-5, 0.1

SHAPES = [(2, 1), (3, 4), (5, 6), (257, 260), (1023, 32), (1024, 32), (1025, 32), (4099, 256), (300, 1028),
          # row-block boundaries: one / two blocks, and the block cap
          (512, 32), (513, 32), (64, 256), (65, 256), (65536, 256), (65537, 256),
          # column-lane and column-tile boundaries
          (37, 33), (37, 64), (37, 65), (37, 128), (37, 129), (37, 257)]


def err(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def check(got, ref, what, notes):
    e = err(got, ref)
    notes.append(f"{what} {e:.2e}")
    assert e <= TOL, f"{what}: max|d| {e:.3e} of max(1, |ref|) > {TOL:.0e}"


def inputs(rows, cols, seed=0, with_params=True):
    x = torch.from_numpy(bi.designed_table(rows, cols, seed)).to(DEV)
    g, b = bi.params(cols, seed)
    rng = np.random.default_rng(seed + 7)
    dy = torch.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32)).to(DEV)
    rm = torch.from_numpy(rng.standard_normal(cols).astype(np.float32)).to(DEV)
    rv = torch.from_numpy(rng.uniform(0.5, 2.0, cols).astype(np.float32)).to(DEV)
    if not with_params:
        return x, None, None, dy, rm, rv
    return x, torch.from_numpy(g).to(DEV), torch.from_numpy(b).to(DEV), dy, rm, rv


def torch_chain(x, w, b, dy, rm, rv, slope, dtype, composed=False):
    """torch's batch_norm + leaky_relu and their autograd in `dtype`: y, running stats, dx, dgamma, dbeta.

    composed (the float64 reference): the batch norm written out in torch ops -- mean = sum / n, the biased
    variance about it, autograd through both -- instead of F.batch_norm.  F.batch_norm's float64 statistics are a
    Welford merge (on the device and on the host): on a designed column, whose sum is exact in float64, it leaves
    the mean +-1e-16 off, a row AT the mean then has a pre-activation of +-1e-16 instead of 0, and that noise's
    sign picks the LeakyReLU gradient (1 or the slope) at random.  sum / n is exact there, the pre-activation is
    exactly 0 and the gradient is the slope by torch's own leaky_relu rule: the reference is defined where the
    at_mean column tests it.  compare() checks that the two float64 chains are one function wherever F.batch_norm
    is well defined: y and the running statistics everywhere, the gradients in every column but the at_mean ones."""
    c = lambda t: None if t is None else t.detach().to(dtype).clone()  # noqa: E731
    xr, wr, br, rmr, rvr = c(x).requires_grad_(True), c(w), c(b), c(rm), c(rv)
    for t in (wr, br):
        if t is not None:
            t.requires_grad_(True)
    if composed:
        n = xr.shape[0]
        mean = xr.sum(0) / n
        var = ((xr - mean) ** 2).sum(0) / n
        v = (xr - mean) / torch.sqrt(var + EPS)
        v = v if wr is None else v * wr
        v = v if br is None else v + br
        with torch.no_grad():
            rmr.mul_(1 - MOM).add_(MOM * mean)
            rvr.mul_(1 - MOM).add_(MOM * var * (n / (n - 1)))
    else:
        v = F.batch_norm(xr, rmr, rvr, wr, br, True, MOM, EPS)
    y = F.leaky_relu(v, slope)
    y.backward(c(dy))
    return y.detach(), rmr, rvr, xr.grad, None if wr is None else wr.grad, None if br is None else br.grad


def ours(x, w, b, dy, rm, rv, slope):
    xr = x.detach().requires_grad_(True)  # (no clone: a column slice keeps its layout)
    wr = None if w is None else w.detach().clone().requires_grad_(True)
    br = None if b is None else b.detach().clone().requires_grad_(True)
    rmr, rvr = rm.clone(), rv.clone()
    y = batchnorm_rows(xr, wr, br, rmr, rvr, True, MOM, EPS, slope)
    y.backward(dy)
    return y.detach(), rmr, rvr, xr.grad, None if wr is None else wr.grad, None if br is None else br.grad


NAMES = ("y", "running_mean", "running_var", "dx", "dgamma", "dbeta")


def compare(x, w, b, dy, rm, rv, slope, tag):
    got = ours(x, w, b, dy, rm, rv, slope)
    ref = torch_chain(x, w, b, dy, rm, rv, slope, torch.float64, composed=True)
    f32 = torch_chain(x, w, b, dy, rm, rv, slope, torch.float32)
    # the composed float64 reference is torch's float64 batch_norm + leaky_relu autograd (see torch_chain)
    f64 = torch_chain(x, w, b, dy, rm, rv, slope, torch.float64)
    well_defined = torch.tensor([bi.kind(j) != "at_mean" for j in range(x.shape[1])], device=DEV)
    for n, r, t in zip(NAMES, ref, f64):
        if r is not None:
            sel = (Ellipsis, well_defined) if n in ("dx", "dgamma", "dbeta") else Ellipsis
            assert err(t[sel], r[sel]) <= 1e-10, f"the two float64 references differ in {n}"
    if x.shape[1] > 2 and (b is None or float(b[2]) == 0):  # ... and exact where the design needs it to be
        at = x[:, 2] == bi.AT_MEAN
        assert at.any() and bool((ref[0][at, 2] == 0).all())
    notes, theirs = [], []
    try:
        for n, a, r, t in zip(NAMES, got, ref, f32):
            if r is None:
                assert a is None
                continue
            theirs.append(f"{n} {err(t, r):.2e}")
            check(a, r, n, notes)
    finally:
        print(f"\n{tag}: ours {', '.join(notes)} | torch fp32 {', '.join(theirs)}")
    return got


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_matches_float64_torch(rows, cols):
    compare(*inputs(rows, cols, seed=rows + cols), 0.2, f"{rows}x{cols}")


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
@pytest.mark.parametrize("with_params", [True, False])
def test_slopes_and_missing_affine(slope, with_params):
    x, w, b, dy, rm, rv = inputs(1025, 36, seed=3, with_params=with_params)
    y = compare(x, w, b, dy, rm, rv, slope, f"slope {slope} affine {with_params}")[0]
    if with_params:  # the at_mean column (beta = 0): rows at the mean give an exact zero
        at = x[:, 2] == bi.AT_MEAN
        assert at.any() and bool((y[at, 2] == 0).all())


@pytest.mark.parametrize("col0,width", [(4, 264), (1, 264), (1, 261), (3, 300)])
def test_column_slices_of_a_wider_table(col0, width):
    """ldx > cols: a slice at an aligned column (the float4 form) and at column 1 / an odd stride (the scalar form)."""
    rows, cols = 257, 256
    x, w, b, dy, rm, rv = inputs(rows, cols, seed=col0)
    wide = torch.full((rows, width), float("nan"), device=DEV)
    xs = wide[:, col0:col0 + cols]
    xs.copy_(x)
    got = compare(xs, w, b, dy, rm, rv, 0.2, f"slice at {col0} of {width}")
    base = ours(x, w, b, dy, rm, rv, 0.2)
    for n, a, c in zip(NAMES, got, base):  # the same bits whatever the layout and the form
        assert torch.equal(a, c), n


def test_two_runs_and_both_forms_give_the_same_bits():
    rows, cols = 4099, 260
    x, w, b, dy, rm, rv = inputs(rows, cols, seed=9)
    one, two = ours(x, w, b, dy, rm, rv, 0.2), ours(x, w, b, dy, rm, rv, 0.2)
    for n, a, c in zip(NAMES, one, two):
        assert torch.equal(a, c), f"run to run: {n}"
    # the scalar form: the same table one float off the 16-B grid, and the gradient likewise
    off = torch.empty(rows * cols + 1, device=DEV)[1:].view(rows, cols)
    off.copy_(x)
    doff = torch.empty(rows * cols + 1, device=DEV)[1:].view(rows, cols)
    doff.copy_(dy)
    assert off.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    y_v, m_v, s_v = batchnorm_rows_fwd_train(x, w, b, None, None, MOM, EPS, 0.2)
    y_s, m_s, s_s = batchnorm_rows_fwd_train(off, w, b, None, None, MOM, EPS, 0.2)
    assert torch.equal(y_v, y_s) and torch.equal(m_v, m_s) and torch.equal(s_v, s_s)
    assert torch.equal(y_v, one[0])
    g_v = batchnorm_rows_bwd(dy, y_v, x, w, m_v, s_v, 0.2)
    g_s = batchnorm_rows_bwd(doff, y_s, off, w, m_s, s_s, 0.2)
    for n, a, c in zip(("dx", "dgamma", "dbeta"), g_v, g_s):
        assert torch.equal(a, c), f"float4 against scalar: {n}"
    # dx may alias dy
    d2 = dy.clone()
    g_i = batchnorm_rows_bwd(d2, y_v, x, w, m_v, s_v, 0.2, out=d2)
    assert g_i[0].data_ptr() == d2.data_ptr() and all(torch.equal(a, c) for a, c in zip(g_i, g_v))


@pytest.mark.parametrize("rows,cols", [(1, 5), (2, 1), (1025, 32), (300, 1028), (4099, 256)])
def test_eval_matches_float64_and_runs_in_place(rows, cols):
    x, w, b, _, rm, rv = inputs(rows, cols, seed=5)
    rm = rm + x.mean(0)  # running statistics near the data's, so y is of order one
    with torch.no_grad():
        y = batchnorm_rows(x, w, b, rm, rv, False, MOM, EPS, 0.2)
    d = torch.float64
    ref = F.leaky_relu(F.batch_norm(x.to(d), rm.to(d), rv.to(d), w.to(d), b.to(d), False, 0.0, EPS), 0.2)
    f32 = F.leaky_relu(F.batch_norm(x, rm, rv, w, b, False, 0.0, EPS), 0.2)
    print(f"\neval {rows}x{cols}: ours {err(y, ref):.2e} | torch fp32 {err(f32, ref):.2e}")
    assert err(y, ref) <= TOL
    xi = x.clone()
    out = batchnorm_rows_fwd_eval(xi, w, b, rm, rv, EPS, 0.2, out=xi)
    assert out.data_ptr() == xi.data_ptr() and torch.equal(xi, y)
    off = torch.empty(rows * cols + 1, device=DEV)[1:].view(rows, cols).copy_(x)  # the scalar form, in place
    batchnorm_rows_fwd_eval(off, w, b, rm, rv, EPS, 0.2, out=off)
    assert torch.equal(off, y)
    # with gradients enabled the inference form is torch's (documented as not hot) and differentiable
    xr = x.clone().requires_grad_(True)
    yt = batchnorm_rows(xr, w, b, rm, rv, False, MOM, EPS, 0.2)
    assert yt.requires_grad and err(yt.detach(), ref) <= TOL


def test_leading_axes_are_rows():
    """(B, N, C) is B * N rows, as the reference's permute -> BatchNorm1d -> permute sees it."""
    x, w, b, dy, rm, rv = inputs(6 * 41, 32, seed=2)
    x3 = x.view(6, 41, 32).clone().requires_grad_(True)
    rm3, rv3 = rm.clone(), rv.clone()
    y3 = batchnorm_rows(x3, w, b, rm3, rv3, True, MOM, EPS, 0.2)
    bn = torch.nn.BatchNorm1d(32, eps=EPS, momentum=MOM).to(DEV).double()
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    ref = F.leaky_relu(bn(x3.detach().double().permute(0, 2, 1)).permute(0, 2, 1), 0.2)
    assert y3.shape == (6, 41, 32) and err(y3.detach(), ref) <= TOL
    assert err(rm3, bn.running_mean) <= TOL and err(rv3, bn.running_var) <= TOL


def test_refusals():
    x = torch.randn(8, 16, device=DEV)
    with pytest.raises(GrlError, match="bfloat16"):
        batchnorm_rows(x.to(torch.bfloat16), None, None, None, None, True)
    with pytest.raises(GrlError, match="more than one value per channel"):
        batchnorm_rows(x[:1], None, None, None, None, True)
    with pytest.raises(GrlError, match="weight"):
        batchnorm_rows(x, torch.ones(15, device=DEV), None, None, None, True)
    with pytest.raises(GrlError, match="ROCm device tensor"):
        batchnorm_rows(x.cpu(), None, None, None, None, True)


def test_rows_past_two_to_the_31_elements():
    """Element offsets past 2^31: the last rows of a [2^23 + 5, 256] table (8.6 GB) in the training forward and
    in the in-place inference pass."""
    rows, cols = (1 << 23) + 5, 256
    x = torch.empty(rows, cols, device=DEV)
    assert x.numel() > 1 << 31
    x.normal_(1.0, 2.0)
    tail = slice(rows - 300, rows)
    x[tail] += 3.0
    w, b = torch.full((cols,), 1.25, device=DEV), torch.full((cols,), -0.5, device=DEV)
    y, mean, invstd = batchnorm_rows_fwd_train(x, w, b, None, None, MOM, EPS, 0.2)
    m64 = x.sum(0, dtype=torch.float64) / rows
    sq = torch.zeros(cols, dtype=torch.float64, device=DEV)
    for r in range(0, rows, 1 << 20):  # the variance in float64 without a float64 copy of the table
        sq += ((x[r:r + (1 << 20)].double() - m64) ** 2).sum(0)
    v64 = sq / rows
    assert err(mean, m64) <= TOL and err(invstd, 1.0 / torch.sqrt(v64 + EPS)) <= TOL
    ref = F.leaky_relu((x[tail].double() - m64) / torch.sqrt(v64 + EPS) * 1.25 - 0.5, 0.2)
    assert err(y[tail], ref) <= TOL
    del y
    rm, rv = m64.float(), v64.float()
    batchnorm_rows_fwd_eval(x, w, b, rm, rv, EPS, 0.2, out=x)
    assert err(x[tail], ref) <= TOL
