"""CPU: a rounding design for the typed SpMM with bf16 on both sides
(grl_typed_spmm_fwd_bf16_to_bf16, grl_typed_spmm_bwd_bf16), proved here to hit
what it claims; tests/test_gpu_spmm_bf16_io.py runs it on the GPU.

The kernels keep fp32 accumulators and round once, to nearest even, at the
store.  A random table almost never produces an fp32 sum that lies exactly
between two bf16 values, so a store that truncated, rounded half up, or
rounded twice would pass a random test.  design() builds a small typed graph
(N = 64, L = 3, F = 16; every table entry is a bf16 value) whose oracle fp32
sums are, up to sign and a power-of-two column scale,
    1 + 2^-8              a tie, even lower neighbour        -> 0x3F80
    (1 + 2^-7) + 2^-8     a tie, odd lower neighbour         -> 0x3F82
    1 + 2^-8 + 2^-20      just above a tie                   -> 0x3F81
    1 + 2^-8 - 2^-20      just below a tie                   -> 0x3F80
Every partial sum is exact in fp32, so the classes hold in any summation
order -- whole rows, or chunk partials added by the fixup: row 0 is a hub of
90 entries, heavy at the split (64, 24) of the GPU test, where its ties are
rounded by the fixup kernel.  The backward runs on the transposed graph with
dZ's first typed segment = the table, so column r of the backward sums what
row r's first segment sums forward (row 5: its self term plus one entry).
"""
import numpy as np
import torch

import graph_patterns as gp
from oracle import c_oracle

N, L, F, HAS_SELF = 64, 3, 16, True
S = L + 1
SPLIT = (64, 24)
A, E, B, C, D = 60, 61, 62, 63, 59  # value nodes: 1, 2^-7, 2^-8, 2^-20, -2^-20 (times the column's sign and scale)
TIE_EVEN, TIE_ODD, ABOVE, BELOW = [A, B], [A, E, B], [A, B, C], [A, B, D]
CLASSES = ("tie_even", "tie_odd", "above", "below")
HUB, SELF_ROW = 0, 5


def design():
    """The design's host arrays: the forward graph P (rowptr, colidx), its
    transpose PT (rowptr_t, colidx_t), the table X [N, F] and the backward
    gradient dZ [N, S * F] -- fp32 arrays of bf16 values."""
    rows = {r: {} for r in range(N)}
    fill = list(range(6, 6 + 28))  # nodes whose table rows are zero
    rows[HUB] = {0: TIE_EVEN + fill, 1: TIE_ODD + fill[:27], 2: ABOVE + fill[:27]}
    rows[1] = {0: TIE_EVEN, 1: BELOW, 2: TIE_ODD}
    rows[2] = {0: TIE_ODD, 2: TIE_EVEN}
    rows[3] = {0: ABOVE, 1: TIE_EVEN}
    rows[4] = {0: BELOW}
    rows[SELF_ROW] = {0: [B]}
    rng = np.random.default_rng(23)
    for r in range(6, N):  # a thin base over the zero rows, so that the other rows and columns are not empty
        rows[r] = {int(rng.integers(L)): rng.choice(np.arange(6, 59), size=3, replace=False).tolist()}
    segs = [np.sort(np.asarray(rows[r].get(t, []), dtype=np.int32)) for r in range(N) for t in range(L)]
    rowptr = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int32)
    colidx = np.concatenate(segs).astype(np.int32)
    assert rowptr[L] - rowptr[0] == 90 > SPLIT[0]
    col = np.array([(-1.0) ** j * 2.0 ** (j // 2) for j in range(F)], dtype=np.float32)  # sign and scale of column j
    X = np.zeros((N, F), dtype=np.float32)
    for node, v in ((A, 1.0), (E, 2.0 ** -7), (B, 2.0 ** -8), (C, 2.0 ** -20), (D, -2.0 ** -20)):
        X[node] = np.float32(v) * col
    dZ = np.zeros((N, S, F), dtype=np.float32)
    dZ[:, 1] = X                # the first typed segment carries the table
    dZ[SELF_ROW, 0] = X[A]      # and row 5's self term the 1 that its one entry, 2^-8, is added to
    for a in (X, dZ):
        assert np.array_equal(torch.from_numpy(a).to(torch.bfloat16).float().numpy(), a)  # bf16 values
    rowptr_t, colidx_t = gp.transpose_host(rowptr, colidx, L, N)
    return {"rowptr": rowptr, "colidx": colidx, "rowptr_t": rowptr_t, "colidx_t": colidx_t, "X": X,
            "dZ": dZ.reshape(N, S * F)}


def oracle(d, split=None):
    """(Z of P over X, dX of PT over dZ) in fp32, by the CPU oracle."""
    Z = c_oracle.spmm_fwd(d["rowptr"], d["colidx"], d["X"], L, HAS_SELF, split=split)
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(d["rowptr_t"], d["colidx_t"], L, N, HAS_SELF, None)
    dX = c_oracle.spmm_bwd(colptr, zrow, eid, d["dZ"], L, F, N, HAS_SELF, cvals, split=split)
    return Z, dX


def classes(a):
    """name -> boolean mask over the fp32 array a, by the mantissa below bf16's
    (sign and exponent free): the four sums of the module docstring."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    low, odd, top = u & 0xFFFF, (u >> 16) & 1 == 1, (u >> 17) & 0x3F  # top: the mantissa bits above bf16's last
    plain = (top == 0) & (a != 0)
    return {"tie_even": plain & (low == 0x8000) & ~odd, "tie_odd": plain & (low == 0x8000) & odd,
            "above": plain & (low == 0x8008) & ~odd, "below": plain & (low == 0x7FF8) & ~odd}


def rne(a):
    """bf16 bits of the fp32 array a, rounded to nearest even by torch on the CPU."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_the_five_bit_patterns():
    v = np.array([1 + 2.0 ** -8, (1 + 2.0 ** -7) + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20],
                 dtype=np.float32)
    assert rne(v).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80]
    assert rne(-v).tolist() == [0xBF80, 0xBF82, 0xBF81, 0xBF80]
    c = classes(v)
    assert [int(np.nonzero(c[k])[0][0]) for k in CLASSES] == [0, 1, 2, 3]


def test_every_class_occurs_forward_and_backward_with_both_signs():
    d = design()
    for split in (None, SPLIT):
        Z, dX = oracle(d, split)
        Z3 = Z.reshape(N, S, F)
        for what, a in (("forward", Z3[:, 1:]), ("backward", dX)):
            c = classes(a)
            for k in CLASSES:
                assert (c[k] & (a > 0)).any() and (c[k] & (a < 0)).any(), f"{what}: class {k} missing (split={split})"
        # the hub's sums are ties: rounded by the fixup when the split is forced
        assert classes(Z3[HUB, 1])["tie_even"].all() and classes(Z3[HUB, 2])["tie_odd"].all()
        assert classes(Z3[HUB, 3])["above"].all() and classes(dX[HUB])["tie_even"].all()
        assert classes(dX[SELF_ROW])["tie_even"].all()  # self term + one entry
        assert np.array_equal(dX[:5], Z3[:5, 1])  # a backward column sums what the forward row's first segment sums
    whole, chunked = oracle(d, None), oracle(d, SPLIT)
    assert all(np.array_equal(a, b) for a, b in zip(whole, chunked))  # exact sums: any order


def test_the_split_makes_the_hub_heavy_on_both_sides():
    d = design()
    assert d["rowptr"][L] - d["rowptr"][0] > SPLIT[0]
    colptr = c_oracle.csr_to_csc(d["rowptr_t"], d["colidx_t"], L, N, HAS_SELF, None)[0]
    assert colptr[HUB + 1] - colptr[HUB] > SPLIT[0]
    assert (np.diff(d["rowptr"][::L])[1:] <= SPLIT[0]).all() and (np.diff(colptr)[1:] <= SPLIT[0]).all()


def test_truncation_and_round_half_up_would_each_show():
    d = design()
    for a in oracle(d):
        u = np.ascontiguousarray(a).view(np.uint32)
        want = rne(a)
        trunc = (u >> 16).astype(np.uint16)
        half_up = ((u + 0x8000) >> 16).astype(np.uint16)
        assert (trunc != want).any() and (half_up != want).any()
        c = classes(a)
        assert (trunc != want)[c["tie_odd"] | c["above"]].all() and (half_up != want)[c["tie_even"]].all()
        assert (trunc == want)[c["tie_even"] | c["below"]].all() and (half_up == want)[c["tie_odd"]].all()
