"""GPU: the one-kernel GraphConv (graphconv_ws_body.inc in all its forms, and
the phase-alternating fg_ws = 0 kernel) on DESIGNED graphs.

Every other GPU test of this kernel walks uniform random graphs; here the
graph is tests/graph_patterns.py's: empty groups and tiles, a lone row behind
or before seven empty ones, list totals of exactly 64 / 128, a row end on a
fetch boundary, a 2048-entry list, and DropEdge draws that empty whole fetch
blocks or everything (tests/test_graph_patterns.py proves on the CPU that
each of these occurs).  Each shape runs on P and on its transpose, so every
row pattern also reaches the typed transpose the data-gradient kernel walks.
The shapes are the smallest that still take the one kernel (2 N C K >= 1.6e10),
and every case first checks by the entry's workspace query WHICH path runs.
After each group of one-kernel calls grl.check() turns a starved ring
(GRL_E_TIMEOUT, NaN outputs) into a failure naming the entry point."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import graph_patterns as gp
import grl
from grl import DropEdge, TypedGraph, _lib
from grl.ops import (graph_conv, graph_conv_bwd_data, graph_conv_fwd_train, graph_conv_infer, linear_bwd_weight,
                     linear_fwd, typed_aggregate)
from oracle import c_oracle
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A

# name: N, L, has_self, F, C
SHAPES = {
    "S1": (17_473, 6, True, 256, 256),   # 8 gather + 4 MFMA waves, one group per wave; N % 64 = 1
    "S1b": (17_529, 6, True, 256, 256),  # N % 64 = 57, N % 8 = 1
    "S2": (17_473, 6, True, 256, 512),   # 4 + 8 waves, two groups per gather wave
    "S3": (17_473, 6, True, 512, 256),   # two virtual segments: every list is walked twice
    "S4": (17_473, 7, False, 256, 256),  # the rowptr window full (8 * 7 + 1 lanes), no self term
}
DROPS = {"none": None, **{k: DropEdge(*v) for k, v in gp.VARIANTS.items()}, "vals": None}
assert sorted({(v[0], v[1]) for v in SHAPES.values()}) == sorted(gp.SHAPES_NL)  # the census covers every (N, L)
GRID = [("S1", v) for v in DROPS] + [(s, v) for s in ("S1b", "S2", "S3", "S4") for v in ("none", "drop03")]
GRID_BF16 = [("S1", v) for v in DROPS] + [("S2", v) for v in ("none", "drop03")]
SIDES = ["P", "PT"]


class Case:
    """One shape's host arrays and device operands on one side (P or its transpose), read-only."""

    def __init__(self, shape, side):
        self.N, self.L, self.has_self, self.F, self.C = N, L, hs, F, C = SHAPES[shape]
        rp, ci, _ = gp.pattern_graph(N, L, gp.SEED)
        if side == "PT":
            rp, ci = gp.transpose_host(rp, ci, L, N)
        self.rowptr, self.colidx = rp, ci
        self.S = L + (1 if hs else 0)
        self.K = K = self.S * F
        rng = np.random.default_rng(N + F + C)
        self.X = rng.standard_normal((N, F)).astype(np.float32)
        self.W = (rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32)
        self.b = rng.standard_normal(C).astype(np.float32)
        self.G = rng.standard_normal((N, C)).astype(np.float32)
        # edge values in (0.1, 2) with a few exact zeros: X is finite, so skipping a zero-weight entry and
        # adding it are the same bits
        self.vals = rng.uniform(0.1, 2.0, len(ci)).astype(np.float32)
        self.vals[rng.choice(len(ci), 40, replace=False)] = 0.0
        self.vals[rp[(gp.placements(N)["P3"][0] * 8) * L] + 63] = 0.0  # and one on a fetch block's last lane
        self.Xt, self.Wt, self.bt, self.Gt = (torch.from_numpy(a).to(DEV) for a in (self.X, self.W, self.b, self.G))

    def graph(self, variant, rowptr=None, colidx=None):
        vals = self.vals if variant == "vals" else None
        g = TypedGraph.from_csr_host(self.rowptr if rowptr is None else rowptr,
                                     self.colidx if colidx is None else colidx, self.L, DEV, has_self=self.has_self,
                                     vals=vals)
        return g.with_dropedge(DROPS[variant])

    def odrop(self, variant):
        de = DROPS[variant]
        return None if de is None else c_oracle.drop(de.p, de.seed, de.call, de.drop_self)

    def ovals(self, variant):
        return self.vals if variant == "vals" else None


@functools.lru_cache(maxsize=2)
def _case(shape, side):
    return Case(shape, side)


@functools.lru_cache(maxsize=1)
def _forward_oracle(shape, side, variant):
    """(Z, pre, scale): the CPU oracle's aggregation (fp32, one fmaf per kept
    entry in CSR order) and float64 Z W + b with the sum of |terms|."""
    c = _case(shape, side)
    Z = c_oracle.spmm_fwd(c.rowptr, c.colidx, c.X, c.L, c.has_self, vals=c.ovals(variant), d=c.odrop(variant))
    Z64, W64, b64 = Z.astype(np.float64), c.W.astype(np.float64), c.b.astype(np.float64)
    return Z, Z64 @ W64 + b64, np.abs(Z64) @ np.abs(W64) + np.abs(b64)


def _fwd_query(X, g, W, C, out=None, Z=None):
    csr = g.csr_c(X.shape[1])
    a = [ctypes.byref(csr), X.data_ptr(), X.stride(0), X.shape[1], W.data_ptr(), C]
    if Z is not None:
        return _lib.lib().grl_graphconv_fwd_train_bf16_z16_workspace_query(*a, out.data_ptr(), out.stride(0),
                                                                          Z.data_ptr())
    if out is not None:
        return _lib.lib().grl_graphconv_fwd_bf16_to_bf16_workspace_query(*a, out.data_ptr(), out.stride(0))
    name = "grl_graphconv_fwd_bf16_workspace_query" if X.dtype == BF16 else "grl_graphconv_fwd_workspace_query"
    return getattr(_lib.lib(), name)(*a)


def _one_kernel(ws, rows, K, C, zbytes=4):
    """W's planes (and the status word), far below Z: the one kernel runs."""
    return ws < 3 * (256 if C <= 256 else 512) * K * 2 + 4096 < rows * K * zbytes


def _bits(t):
    return t.view(torch.int16)


def _relu_of(variant):
    return variant not in ("none", "all_spare_self")


# ------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID)
def test_forward_is_the_two_op_chain_and_the_oracle(shape, variant, side, grl_option):
    """(a) graph_conv_infer on both kernels (fg_ws 1 / 0): one kernel by the
    workspace query, bitwise linear_fwd(typed_aggregate(X)), within
    1e-5 (|Z| |W| + |b|) + 1e-6 of float64 Z W + b on the oracle's Z.
    (b) graph_conv_fwd_train: Z bitwise the CPU oracle's, element for element
    (the gather role against one fmaf per kept entry), out bitwise (a)'s."""
    c = _case(shape, side)
    g = c.graph(variant)
    relu = _relu_of(variant)
    Z, pre, scale = _forward_oracle(shape, side, variant)
    assert g.split_stats()["csr"]["heavy_segments"] == 0
    two_op = linear_fwd(typed_aggregate(c.Xt, g), c.Wt, c.bt, relu)
    want = np.maximum(pre, 0.0) if relu else pre
    outs = []
    for fg_ws in (1, 0):
        grl_option("fg_ws", fg_ws)
        assert _one_kernel(_fwd_query(c.Xt, g, c.Wt, c.C), c.N, c.K, c.C), (fg_ws, "two kernels would run")
        out = graph_conv_infer(c.Xt, g, c.Wt, c.bt, relu)
        grl.check()
        assert torch.equal(out, two_op), f"fg_ws={fg_ws}: not the two-op bits"
        err = np.abs(out.cpu().numpy() - want)
        assert np.all(err <= 1e-5 * scale + 1e-6), (fg_ws, float((err / (1e-5 * scale + 1e-6)).max()))
        outs.append(out)
    grl_option("fg_ws", 1)
    if variant == "all_self":  # every weight is 0: out is relu(b)
        assert torch.equal(outs[0], torch.relu(c.bt).expand(c.N, c.C))
    out_t, Z_t = graph_conv_fwd_train(c.Xt, g, c.Wt, c.bt, relu)
    grl.check()
    Zg = Z_t.cpu().numpy()
    bad = np.argwhere(Zg != Z)
    assert bad.size == 0, f"Z differs from the oracle at {len(bad)} elements, first (row, col) {bad[0].tolist()}"
    assert torch.equal(out_t, outs[0])


# ------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID_BF16)
def test_bf16_forms_keep_their_contracts(shape, variant, side):
    """(c) bf16 X: out and Z bitwise the fp32 entry on X.float(); bf16 out
    into a column slice of a sentinel table: the fp32 out rounded to nearest
    even, sentinels untouched; bf16 Z: the fp32 Z rounded to nearest even, out
    unchanged.  Each on the one kernel by its own workspace query."""
    c = _case(shape, side)
    g = c.graph(variant)
    relu = _relu_of(variant)
    N, K, C = c.N, c.K, c.C
    Xb = c.Xt.to(BF16)
    out_f, Z_f = graph_conv_fwd_train(Xb.float(), g, c.Wt, c.bt, relu)
    assert _one_kernel(_fwd_query(Xb, g, c.Wt, C), N, K, C)
    assert torch.equal(graph_conv_infer(Xb, g, c.Wt, c.bt, relu), out_f)
    out_b, Z_b = graph_conv_fwd_train(Xb, g, c.Wt, c.bt, relu)
    grl.check()
    assert torch.equal(out_b, out_f) and torch.equal(Z_b, Z_f)
    del out_b, Z_b
    want_out, want_z = _bits(out_f.to(BF16)), _bits(Z_f.to(BF16))
    del Z_f

    def table():
        t = torch.full((N, C + 128), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
        return t, t[:, 64:64 + C]

    def untouched(t):
        return bool((_bits(t[:, :64]) == SENTINEL).all()) and bool((_bits(t[:, 64 + C:]) == SENTINEL).all())

    t, out = table()
    assert _one_kernel(_fwd_query(Xb, g, c.Wt, C, out), N, K, C)
    assert graph_conv_infer(Xb, g, c.Wt, c.bt, relu, out=out) is out
    grl.check()
    assert torch.equal(_bits(out), want_out) and untouched(t)
    t, out = table()
    _, Z32 = graph_conv_fwd_train(Xb, g, c.Wt, c.bt, relu, out=out)
    grl.check()
    assert torch.equal(_bits(out), want_out) and untouched(t) and torch.equal(_bits(Z32.to(BF16)), want_z)
    del Z32
    t, out = table()
    buf = torch.full(((N + 1) * K,), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    Z16 = buf[:N * K].view(N, K)
    assert _one_kernel(_fwd_query(Xb, g, c.Wt, C, out, Z16), N, K, C, zbytes=2)
    graph_conv_fwd_train(Xb, g, c.Wt, c.bt, relu, out=out, Z=Z16)
    grl.check()
    assert torch.equal(_bits(Z16), want_z) and bool((_bits(buf[N * K:]) == SENTINEL).all())
    assert torch.equal(_bits(out), want_out) and untouched(t)


# ------------------------------------------------------------------ (d) + (e)
def _segsum64(rp, ci, w, G64):
    """float64 sum_e w_e G[ci_e] per CSR segment -> [segments, C]."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (torch calls its sparse CSR support beta)
        A = torch.sparse_csr_tensor(torch.from_numpy(np.asarray(rp, dtype=np.int64)),
                                    torch.from_numpy(np.asarray(ci, dtype=np.int64)),
                                    torch.from_numpy(np.asarray(w, dtype=np.float64)),
                                    size=(len(rp) - 1, G64.shape[0]))
        return (A @ torch.from_numpy(G64)).numpy()  # (a CPU product, float64 throughout)


def _weights(c, variant):
    """(w, wself): every entry's and every row's self loop's weight under the
    variant, as the kernels form them (fp32 value times fp32 scale)."""
    nnz = len(c.colidx)
    w = c.vals.copy() if variant == "vals" else np.ones(nnz, dtype=np.float32)
    wself = np.ones(c.N, dtype=np.float32)
    de = DROPS[variant]
    if de is not None:
        _, _, scale = ohash.dropedge_params(de.p)
        w = np.where(ohash.dropedge_keep(de.p, de.seed, de.call, np.arange(nnz, dtype=np.uint64)), w * scale,
                     np.float32(0)).astype(np.float32)
        if de.drop_self:
            keep = ohash.dropedge_keep(de.p, de.seed, de.call, np.arange(nnz, nnz + c.N, dtype=np.uint64))
            wself = np.where(keep, scale, np.float32(0)).astype(np.float32)
    return w, wself


@functools.lru_cache(maxsize=1)
def _backward_oracle(shape, side, variant):
    """float64 restatement of the data gradient (as test_gpu_graphconv_random_shapes):
    dZ = G W^T in float64, then the oracle's transposed gather; sX the same on
    |G|, |W|.  And A_drop^T G per segment in float64 with its sum of |terms|."""
    c = _case(shape, side)
    d = c.odrop(variant)
    G64, W64 = c.G.astype(np.float64), c.W.astype(np.float64)
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(c.rowptr, c.colidx, c.L, c.N, c.has_self, c.ovals(variant))
    sb = int(c.rowptr[-1])
    dX = c_oracle.spmm_bwd(colptr, zrow, eid, (G64 @ W64.T).astype(np.float32), c.L, c.F, c.N, c.has_self, cvals, d=d,
                           self_base=sb).astype(np.float64)
    sX = c_oracle.spmm_bwd(colptr, zrow, eid, (np.abs(G64) @ np.abs(W64.T)).astype(np.float32), c.L, c.F, c.N,
                           c.has_self, cvals, d=d, self_base=sb)
    rpt, cit, eidt = gp.transpose_host(c.rowptr, c.colidx, c.L, c.N, return_eid=True)
    w, wself = _weights(c, variant)
    wt = w[eidt].astype(np.float64)
    agg = _segsum64(rpt, cit, wt, G64).reshape(c.N, c.L * c.C)
    sagg = _segsum64(rpt, cit, np.abs(wt), np.abs(G64)).reshape(c.N, c.L * c.C)
    if c.has_self:
        agg = np.concatenate([wself[:, None].astype(np.float64) * G64, agg], axis=1)
        sagg = np.concatenate([wself[:, None].astype(np.float64) * np.abs(G64), sagg], axis=1)
    return dX, sX, agg, sagg, (rpt, cit)


def _bwd_bf16_query(G, g, W, F, dX):
    gt, _ = g.typed_transpose()
    csr = gt.with_dropedge(g.dropedge).csr_c(G.shape[1])
    return _lib.lib().grl_graphconv_bwd_data_bf16_workspace_query(
        ctypes.byref(csr), G.data_ptr(), G.stride(0), G.shape[1], W.data_ptr(), min(F, 512), dX.data_ptr(),
        dX.stride(0))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID)
def test_data_gradient_one_kernel(shape, variant, side):
    """(d) graph_conv_bwd_data with the aggregate: not None (the one kernel
    over the typed transpose ran), deterministic, dX within 2e-5 sX + 1e-6 of
    the float64 restatement, G_agg within 1e-5 of the sum of |terms| of
    float64 A_drop^T G -- and, without DropEdge and values, bitwise the CPU
    oracle's aggregation over transpose_host(P): the typed transpose keeps
    forward-CSR order (a stable radix sort), so the fmaf chains are the same.
    (e) bf16 G and dX: the bits of the fp32 dX on G.float(), rounded to
    nearest even."""
    c = _case(shape, side)
    g = c.graph(variant)
    dX64, sX, agg, sagg, (rpt, cit) = _backward_oracle(shape, side, variant)
    res = graph_conv_bwd_data(c.Gt, g, c.Wt, c.F, want_aggregate=True)
    assert res is not None, "the shape should take the one-kernel data gradient"
    dX, G_agg, _ = res
    again = graph_conv_bwd_data(c.Gt, g, c.Wt, c.F, want_aggregate=True)
    grl.check()
    assert torch.equal(again[0], dX) and torch.equal(again[1], G_agg)
    del again
    err = np.abs(dX.cpu().numpy() - dX64)
    assert np.all(err <= 2e-5 * sX + 1e-6), float((err / (2e-5 * sX + 1e-6)).max())
    Ga = G_agg.cpu().numpy()
    err = np.abs(Ga - agg)
    assert np.all(err <= 1e-5 * sagg), float((err / (1e-5 * sagg + 1e-30)).max())
    if variant == "none":
        ref = c_oracle.spmm_fwd(rpt, cit, c.G, c.L, c.has_self)
        bad = np.argwhere(Ga != ref)
        assert bad.size == 0, f"G_agg differs from the oracle at {len(bad)} elements, first {bad[0].tolist()}"
    del G_agg, Ga
    # (e)
    Gb = c.Gt.to(BF16)
    want = graph_conv_bwd_data(Gb.float(), g, c.Wt, c.F)
    assert want is not None
    out = torch.empty(c.N, c.F, dtype=BF16, device=DEV)
    planes = c.S * c.C * (256 if c.F <= 256 else 512) * 3 * 2 + 256
    assert _bwd_bf16_query(Gb, g, c.Wt, c.F, out) == planes  # the one kernel runs
    got = graph_conv_bwd_data(Gb, g, c.Wt, c.F, out=out)
    grl.check()
    assert got is out and torch.equal(_bits(out), _bits(want.to(BF16)))


# ------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("variant", list(DROPS))
def test_layer_through_autograd(variant, side, grl_option):
    """(f) graph_conv(relu=True) forward + backward on S1 with
    graphconv_fused_bwd 1 / 0: out, dW, db bitwise between the settings, dX
    within 2e-5 sX + 1e-6 of the float64 restatement through the layer's own
    ReLU mask.  With recompute=True: out and dX bitwise the saved-Z runs'; dW
    and db bitwise too where Z is re-aggregated (fused_bwd 0), and -- where
    the data-gradient kernel's aggregate gives dW_s = X^T G_s, the same
    products in another order -- within 1e-5 of the sums of |terms|
    (test_recompute_takes_weight_gradient_from_the_aggregate's contract)."""
    c = _case("S1", side)
    g = c.graph(variant)
    res = {}
    for rc in (False, True):
        for fb in (1, 0):
            grl_option("graphconv_fused_bwd", fb)
            X, W, b = (t.clone().requires_grad_(True) for t in (c.Xt, c.Wt, c.bt))
            out = graph_conv(X, g, W, b, relu=True, recompute=rc)
            (out * c.Gt).sum().backward()
            grl.check()
            res[rc, fb] = (out.detach(), X.grad, W.grad, b.grad)
    grl_option("graphconv_fused_bwd", 1)
    out, dX1, dW, db = res[False, 1]
    assert torch.equal(out, graph_conv_infer(c.Xt, g, c.Wt, c.bt, True))
    for a, r in zip((out, dW, db), (res[False, 0][0], res[False, 0][2], res[False, 0][3])):
        assert torch.equal(a, r)
    assert torch.equal(dX1, graph_conv_bwd_data(c.Gt, g, c.Wt, c.F, out))  # the one-kernel dX is what ran
    # float64 restatement through the ReLU mask of the layer's own output
    d = c.odrop(variant)
    gz = c.G.astype(np.float64) * (out.cpu().numpy() > 0)
    W64 = c.W.astype(np.float64)
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(c.rowptr, c.colidx, c.L, c.N, c.has_self, c.ovals(variant))
    sb = int(c.rowptr[-1])
    dX64 = c_oracle.spmm_bwd(colptr, zrow, eid, (gz @ W64.T).astype(np.float32), c.L, c.F, c.N, c.has_self, cvals,
                             d=d, self_base=sb).astype(np.float64)
    sX = c_oracle.spmm_bwd(colptr, zrow, eid, (np.abs(gz) @ np.abs(W64.T)).astype(np.float32), c.L, c.F, c.N,
                           c.has_self, cvals, d=d, self_base=sb)
    for key in ((False, 1), (False, 0)):
        err = np.abs(res[key][1].cpu().numpy() - dX64)
        assert np.all(err <= 2e-5 * sX + 1e-6), (key, float((err / (2e-5 * sX + 1e-6)).max()))
    # recompute=True
    for fb in (1, 0):
        assert torch.equal(res[True, fb][0], out) and torch.equal(res[True, fb][1], res[False, fb][1]), fb
    assert torch.equal(res[True, 0][2], dW) and torch.equal(res[True, 0][3], db)
    ge = torch.where(out > 0, c.Gt, torch.zeros((), device=DEV))
    bound_w, _ = linear_bwd_weight(typed_aggregate(c.Xt, g).abs(), ge.abs(), None, False)
    assert bool(((res[True, 1][2] - dW).abs() <= 1e-5 * bound_w + 1e-6).all())
    assert bool(((res[True, 1][3] - db).abs() <= 1e-5 * ge.abs().sum(0) + 1e-6).all())


# ------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("variant", ["none", "drop03", "high_p", "vals"])
def test_row_views_cut_inside_patterned_groups(variant, side):
    """(g) g.rows_view(r0, r1) with r0 / r1 inside a P3, a P5 and a P2 group
    (not multiples of 8, so every group of the view straddles two of the
    whole graph's): the view runs the one kernel (rows_view carries the whole
    graph's row count as path_rows) and is bitwise the whole graph's rows."""
    c = _case("S1", side)
    g = c.graph(variant)
    at = gp.placements(c.N)
    assert at["P3"][0] == 0 and at["P2"][-1] == c.N // 8 - 1
    cuts = [(3, c.N), (at["P5"][0] * 8 + 3, c.N), (5, c.N - 1 - 3)]
    Z = typed_aggregate(c.Xt, g)
    whole = graph_conv_infer(c.Xt, g, c.Wt, c.bt, True)
    for r0, r1 in cuts:
        v = g.rows_view(r0, r1)
        assert r0 % 8 and v.num_rows == r1 - r0 and v.self_row0 == r0
        assert _one_kernel(_fwd_query(c.Xt, v, c.Wt, c.C), r1 - r0, c.K, c.C)
        part = graph_conv_infer(c.Xt, v, c.Wt, c.bt, True)
        grl.check()
        assert torch.equal(part, whole[r0:r1]), (r0, r1)
        assert torch.equal(typed_aggregate(c.Xt, v), Z[r0:r1]), (r0, r1)
        out_t, Z_t = graph_conv_fwd_train(c.Xt, v, c.Wt, c.bt, True)
        grl.check()
        assert torch.equal(out_t, whole[r0:r1]) and torch.equal(Z_t, Z[r0:r1]), (r0, r1)


# ------------------------------------------------------------------------ (h)
def test_both_sides_of_the_heavy_threshold():
    """(h) One more edge on a 2048-edge row makes it heavy: the split plan
    reports it, the workspace query asks for Z (two kernels), graph_conv_infer
    is still the two-op bits, and the data gradient over a graph whose
    TRANSPOSE has the heavy row returns None.  P itself has no heavy row."""
    c = _case("S1", "P")
    N, L, K, C = c.N, c.L, c.K, c.C
    g = c.graph("none")
    assert g.split_stats() == {"csr": {"heavy_segments": 0, "chunks": 0}, "csc": {"heavy_segments": 0, "chunks": 0}}
    assert _one_kernel(_fwd_query(c.Xt, g, c.Wt, C), N, K, C)
    row = gp.placements(N)["P5_rows"][3]
    rp, ci = gp.add_edge(c.rowptr, c.colidx, L, N, row, (3 + 1) % L)
    assert np.diff(rp).reshape(N, L)[row].sum() == 2049
    gh = c.graph("none", rp, ci)
    assert gh.split_stats()["csr"]["heavy_segments"] >= 1
    assert _fwd_query(c.Xt, gh, c.Wt, C) >= N * K * 4
    out = graph_conv_infer(c.Xt, gh, c.Wt, c.bt, True)
    grl.check()
    assert torch.equal(out, linear_fwd(typed_aggregate(c.Xt, gh), c.Wt, c.bt, True))
    Z = c_oracle.spmm_fwd(rp, ci, c.X, L, True, split=(gh.split_threshold, gh.split_chunk)).astype(np.float64)
    W64 = c.W.astype(np.float64)
    scale = np.abs(Z) @ np.abs(W64) + np.abs(c.b)
    assert np.all(np.abs(out.cpu().numpy() - np.maximum(Z @ W64 + c.b, 0.0)) <= 1e-5 * scale + 1e-6)
    # the transposed graph: no heavy row of its own (the forward takes one kernel), a heavy row in ITS transpose
    rpt, cit = gp.transpose_host(rp, ci, L, N)
    gt = c.graph("none", rpt, cit)
    assert gt.split_stats()["csr"]["heavy_segments"] == 0
    assert _one_kernel(_fwd_query(c.Xt, gt, c.Wt, C), N, K, C)
    assert graph_conv_bwd_data(c.Gt, gt, c.Wt, c.F) is None
    g_pt = c.graph("none", *gp.transpose_host(c.rowptr, c.colidx, L, N))  # (without the extra edge: one kernel)
    assert graph_conv_bwd_data(c.Gt, g_pt, c.Wt, c.F) is not None
    grl.check()
