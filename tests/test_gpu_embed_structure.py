"""GPU: the bag-linear kernels of csrc/embed.hip on DESIGNED inputs.

tests/test_gpu_embed.py feeds them bag-of-characters rows (11 nonzeros) and
fully dense blocks; here the inputs are tests/embed_patterns.py's, whose
censuses tests/test_embed_patterns.py asserts on the CPU: forward rows that
fill the 512-entry list exactly, overflow it by one entry, once and many
times, sit on the 1536-column scan-round boundary, are all zero between dense
rows or hold -0.0; weight-gradient lists of exactly 0, 1, 15, 16, 17, 31, 32,
33, 47, 48, 49 and 4096 entries with runs that end on or span a 16-entry
batch, in whole and partial chunks, with the db column opening or closing a
column block.

Two checks each.  EXACT data: V holds small integers, the other operand
multiples of 2^-6 (2^-4 for the 70,000-row gradient) of magnitude at most 4,
so every partial sum is exact in fp32 (the test asserts the precondition:
sum |terms| in units of the last fractional bit stays below 2^24) and the
result must EQUAL float64's -- a dropped, doubled or misplaced list entry
cannot hide.  REAL data: the forward within the worst-case bound of an n-term
fmaf chain plus the bias add, (n + 1) 2^-24 (sum |v w| + |b|) with n the
row's nonzero count; the gradient within this project's 1e-5 sum |terms| and
run to run bitwise."""
import functools

import numpy as np
import pytest
import torch

import embed_patterns as ep
from grl.ops import bag_linear, bag_linear_bwd_weight, bag_linear_forward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

FWD_C = [1, 64, 65, 256, 257, 512]
DW_CASES = [(3100, 303), (1537, 304), (70_000, 47)]  # tests/test_embed_patterns.py takes their census
DW_C = [1, 256, 257, 512]


def _dyadic(rng, shape, frac_bits=6):
    """Random multiples of 2^-frac_bits in [-4, 4]."""
    return (rng.integers(-4 << frac_bits, (4 << frac_bits) + 1, shape) / float(1 << frac_bits)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _forward_rows(K, exact):
    V, rows = ep.forward_rows(K, K, exact)
    V.setflags(write=False)
    return V, rows


def _strided(V, pad=5):
    """V as a column slice of a wider, sentinel-filled tensor (ldv > K)."""
    M, K = V.shape
    wide = torch.full((M, K + pad), 9.0, device=DEV)
    wide[:, :K] = torch.from_numpy(np.array(V)).to(DEV)
    return wide[:, :K]


def _forward_operands(K, C, bias, exact):
    rng = np.random.default_rng(K + C)
    if exact:
        Wt, b = _dyadic(rng, (K, C)), _dyadic(rng, C)
    else:
        Wt, b = (rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    return Wt, (b if bias else None)


def _forward_ref(V, Wt, b, relu):
    """float64 result and the sum of |terms| per element."""
    V64, W64 = V.astype(np.float64), Wt.astype(np.float64)
    ref = V64 @ W64 + (0.0 if b is None else b.astype(np.float64))
    mag = np.abs(V64) @ np.abs(W64) + (0.0 if b is None else np.abs(b.astype(np.float64)))
    return (np.maximum(ref, 0.0) if relu else ref), mag


def _forward_run(V, Wt, b, relu):
    Vd, Wd = _strided(V), torch.from_numpy(Wt).to(DEV)
    bd = None if b is None else torch.from_numpy(b).to(DEV)
    assert Vd.stride(0) > Vd.shape[1]
    out = bag_linear_forward(Vd, Wd, bd, relu)
    assert torch.equal(out, bag_linear_forward(Vd.contiguous(), Wd, bd, relu)), "ldv > K and ldv == K differ"
    assert torch.equal(out, bag_linear(Vd, Wd.t().contiguous(), bd, relu)), "bag_linear and bag_linear_forward differ"
    return out.cpu().numpy()


@pytest.mark.parametrize("relu,bias", [(True, True), (False, False)])
@pytest.mark.parametrize("C", FWD_C)
@pytest.mark.parametrize("K", ep.FWD_K)
def test_forward_exact_data_equals_float64(K, C, relu, bias):
    V, rows = _forward_rows(K, True)
    Wt, b = _forward_operands(K, C, bias, True)
    ref, mag = _forward_ref(V, Wt, b, relu)
    assert mag.max() * 64 < 2 ** 24  # every partial sum is exact in fp32
    out = _forward_run(V, Wt, b, relu)
    bad = np.nonzero((out != ref).any(1))[0]
    names = [n for n, i in rows.items() if i in set(bad.tolist())]
    assert bad.size == 0, f"rows {names} differ from float64, max|d| = {np.abs(out - ref).max()}"


@pytest.mark.parametrize("relu,bias", [(True, True), (False, False)])
@pytest.mark.parametrize("C", FWD_C)
@pytest.mark.parametrize("K", ep.FWD_K)
def test_forward_real_data_within_the_fmaf_chain_bound(K, C, relu, bias):
    V, rows = _forward_rows(K, False)
    Wt, b = _forward_operands(K, C, bias, False)
    ref, mag = _forward_ref(V, Wt, b, relu)
    n = np.count_nonzero(V, axis=1)[:, None]  # -0.0 is not counted: the kernel skips it
    bound = (n + 1) * 2.0 ** -24 * mag
    err = np.abs(_forward_run(V, Wt, b, relu).astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (f"row {worst[0]} column {worst[1]}: error {err[worst]:.3e} over the bound "
                                  f"{bound[worst]:.3e}")


def test_forward_rows_that_share_a_wave():
    """More rows than the launch has waves (at most 16 four-wave workgroups a
    CU), so a wave walks row m, then m + waves, then m + 2 waves with one list:
    a dense row, an all-zero row and a dense row again, and a row that leaves
    the list one entry after an overflow before a one-entry row.  Exact data."""
    K, C = 1537, 64
    waves = torch.cuda.get_device_properties(DEV).multi_processor_count * 16 * 4
    M = 2 * waves + 8
    src, rows = _forward_rows(K, True)
    V = torch.zeros(M, K, device=DEV)
    place = {}
    for lane, names in ((0, ("dense_a", "zero_mid", "dense_b")), (5, ("n513", "n1", "full512")),
                        (7, ("full512_last", "n0", "n1025"))):
        for i, name in enumerate(names):
            place[lane + i * waves] = rows[name]
    at = torch.tensor(sorted(place), device=DEV)
    V[at] = torch.from_numpy(np.array(src[[place[r] for r in sorted(place)]])).to(DEV)
    Wt, b = _forward_operands(K, C, True, True)
    Wd, bd = torch.from_numpy(Wt).to(DEV), torch.from_numpy(b).to(DEV)
    out = bag_linear_forward(V, Wd, bd, True)
    ref = torch.relu(bd.double()).float().expand(M, C).clone()
    ref[at] = torch.relu(V[at].double() @ Wd.double() + bd.double()).float()
    assert torch.equal(out, ref), f"{int((out != ref).any(1).sum())} rows differ"


# ------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=2)
def _dw_matrix(M, K, exact):
    V = ep.dw_matrix(M, K, M + K, exact)
    return _strided(V) if K == 304 else torch.from_numpy(V).to(DEV)  # one case reads V with ldv > K


def _dw_ref(V, g, relu_out):
    """float64 dWt, db and the sum of |terms| per element."""
    gd = g.double()
    if relu_out is not None:
        gd = torch.where(relu_out > 0, gd, torch.zeros((), dtype=gd.dtype, device=gd.device))
    Vd = V.double()
    return Vd.T @ gd, gd.sum(0), Vd.abs().T @ gd.abs(), gd.abs().sum(0)


def _dw_params():
    return [(M, K, C) for M, K in DW_CASES for C in (DW_C if M < 65536 else [256])]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,K,C", _dw_params())
def test_weight_gradient_exact_data_equals_float64(M, K, C, relu):
    V = _dw_matrix(M, K, True)
    assert (K == 304) == (V.stride(0) > K)
    frac = 6 if M < 65536 else 4
    rng = np.random.default_rng(M + C)
    g = torch.from_numpy(_dyadic(rng, (M, C), frac)).to(DEV)
    relu_out = torch.from_numpy(_dyadic(rng, (M, C), frac)).to(DEV) if relu else None  # zeros and negatives mask
    rW, rb, aW, ab = _dw_ref(V, g, relu_out)
    assert float(max(aW.max(), ab.max())) * (1 << frac) < 2 ** 24  # every partial sum is exact in fp32
    dWt, db = bag_linear_bwd_weight(V, g, relu_out, True)
    bad = (dWt.double() != rW).any(1).nonzero().flatten().tolist()
    assert not bad, f"dWt rows (columns of V) {bad[:20]} differ from float64"
    assert torch.equal(db.double(), rb), "db differs from float64"
    dWt2, none = bag_linear_bwd_weight(V, g, relu_out, False)
    assert none is None and torch.equal(dWt, dWt2), "dWt without db differs"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,K,C", _dw_params())
def test_weight_gradient_real_data_within_bound_and_deterministic(M, K, C, relu):
    V = _dw_matrix(M, K, False)
    gen = torch.Generator(device=DEV).manual_seed(M + C)
    g = torch.randn(M, C, generator=gen, device=DEV)
    relu_out = torch.relu(torch.randn(M, C, generator=gen, device=DEV)) if relu else None
    rW, rb, aW, ab = _dw_ref(V, g, relu_out)
    dWt, db = bag_linear_bwd_weight(V, g, relu_out, True)
    assert float(((dWt.double() - rW).abs() - 1e-5 * aW).max()) <= 1e-30
    assert float(((db.double() - rb).abs() - 1e-5 * ab).max()) <= 1e-30
    dWt2, db2 = bag_linear_bwd_weight(V, g, relu_out, True)
    assert torch.equal(dWt, dWt2) and torch.equal(db, db2), "not bitwise run to run"
    dWt3, none = bag_linear_bwd_weight(V, g, relu_out, False)
    assert none is None and torch.equal(dWt, dWt3), "dWt without db differs"
