"""GPU: the split-bf16 ("x6") GEMM, GraphConv and attention kernels on inputs
where ONE plane-product sum decides each output element (x6_isolate.py,
DESIGN.md §4.2): one operand is one-hot along the reduction index, so an
element is a single a * b of full-mantissa fp32 values and is held to
2^-22 |a b| of the float64 product -- a bound from the numpy model and the
analysis (test_x6_isolate.py), 16 times below what one dropped, duplicated
or misplaced low-order plane product costs (2^-16 of the term).  The
tolerances of the other GPU tests average such an error away over K."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grl.ops
import x6_isolate as xi
from grl import TypedGraph, _lib
from grl.ops import (graph_conv_bwd_data, graph_conv_fwd_train, graph_conv_infer, linear_bwd_data, linear_bwd_weight,
                     linear_fwd_ex, node_attention_backward, node_attention_forward, x6_rows_ok)
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _full(shape, gen):
    """randn * 2^randint(-8, 9) on the device: full-mantissa fp32 values."""
    scale = torch.pow(2.0, torch.randint(-8, 9, shape, device=DEV, generator=gen).float())
    v = torch.randn(shape, device=DEV, generator=gen) * scale
    return torch.where(v == 0, torch.full_like(v, 1 + 2.0 ** -23), v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(got, a, b, bound=xi.BARE, what="", scale=None):
    """x6_isolate.check_bound for device tensors: got within bound * |a b| (or
    bound * scale) of the float64 a * b (b None: of a), the product gathered
    and formed on the device; returns the worst ratio to the bound."""
    ref = (a.double() * b.double() if b is not None else a.double()).cpu().numpy()
    return xi.check_bound(got.cpu().numpy(), ref, ref if scale is None else scale.double().cpu().numpy(), bound, what)


def _differs_from_fp32(x6_result, fp32_call, grl_option, what):
    """Pins that the split-bf16 kernel ran: the same call with gemm_x6 = 0 (the
    fp32-MFMA GEMM, whose single products are correctly rounded) gives other
    bits.  A quiet fall-back to it would meet every bound here."""
    grl_option("gemm_x6", 0)
    other = fp32_call()
    grl_option("gemm_x6", 1)
    assert not torch.equal(other, x6_result), f"{what}: the fp32 GEMM's bits -- the x6 kernel did not run"


def _pin_rows(K, C):
    """The smallest path_rows at which a 4-row [., K] x [K, C] product takes the x6 GEMM."""
    lo, hi = 4, 1 << 40
    path = _lib.lib().grl_linear_fwd_path
    assert path(4, K, C, hi) == 1, (K, C)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if path(4, K, C, mid) == 1 else (mid + 1, hi)
    assert path(4, K, C, lo) == 1 and path(4, K, C, lo - 1) == 0
    return lo


def _slices(n, K, width):
    """k(i) = 37 i mod K for i < n in consecutive slices of `width`: together
    the slices visit every one of the K positions (37 is coprime to K)."""
    full = xi.sweep(-(-max(n, K) // width) * width, K, 0)
    return [full[i:i + width] for i in range(0, -(-K // width) * width, width)]


# ---- GEMM: linear.hip --------------------------------------------------------
GEMM_SHAPES = [(300, 16, 8), (300, 48, 200), (517, 1792, 256), (260, 3584, 520)]


@pytest.mark.parametrize("variant", ["w_one_hot", "w_one_hot_strided_z", "z_one_hot"])
@pytest.mark.parametrize("w_layout", [0, 1])
@pytest.mark.parametrize("M,K,C", GEMM_SHAPES)
def test_gemm_forward_single_products(M, K, C, w_layout, variant, grl_option):
    """gemm_x6_kernel through grl_linear_fwd_ex (both W layouts: both plane
    splits of W), no bias, no ReLU; path_rows pins the x6 path for a small M.
    w_one_hot: W has one non-zero per column and Z is dense, so out[m, c] =
    Z[m, k(c)] W[k(c), c] exercises Z's in-kernel split at every (m, k) over
    the runs; z_one_hot: Z has one non-zero per row and W is dense, out[m, c]
    = Z[m, k(m)] W[k(m), c], every (k, c) of W's planes."""
    grl_option("gemm_x6", 1)
    rows = _pin_rows(K, C)
    assert x6_rows_ok(M, C, K, rows) and not x6_rows_ok(M, C, K, rows - 1)
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    rng = np.random.default_rng(M + K + C)
    worst = 0.0
    if variant == "z_one_hot":
        W = _full((K, C), gen)
        Wk = W.t().contiguous() if w_layout else W
        m = torch.arange(M, device=DEV)
        for k_of_m in _slices(M, K, M):
            k = _dev(k_of_m)
            Z = _dev(xi.one_hot_rows(rng, M, K, k_of_m))
            out = linear_fwd_ex(Z, Wk, w_layout, None, False, rows)
            worst = max(worst, _check(out, Z[m, k][:, None], W[k], what=f"out, Z one-hot at 37 m + {int(k_of_m[0])}"))
    else:
        wide = torch.zeros(M, K + 24, device=DEV)
        Z = wide[:, 8:8 + K] if variant.endswith("strided_z") else wide[:, :K].contiguous()
        Z.copy_(_full((M, K), gen))
        assert Z.stride(0) == (K + 24 if variant.endswith("strided_z") else K)
        c = torch.arange(C, device=DEV)
        for k_of_c in _slices(C, K, C):
            k = _dev(k_of_c)
            W = _dev(xi.one_hot_cols(rng, K, C, k_of_c))
            Wk = W.t().contiguous() if w_layout else W
            out = linear_fwd_ex(Z, Wk, w_layout, None, False, rows)
            what = f"out, W one-hot at 37 c + {int(k_of_c[0])}"
            worst = max(worst, _check(out, Z[:, k], W[k, c][None, :], what=what))
    _differs_from_fp32(out, lambda: linear_fwd_ex(Z, Wk, w_layout, None, False, 0), grl_option, "forward")
    print(f"gemm_x6 fwd ({M}, {K}, {C}) layout {w_layout} {variant}: worst error {worst:.3f} x 2^-22 |a b|")


BWD_SHAPE = (17_443, 1792, 256)  # just above the x6 size floor; M is 3 past a multiple of 16


@pytest.mark.parametrize("variant", ["w_one_hot", "g_one_hot"])
def test_gemm_data_gradient_single_products(variant, grl_option):
    """grl_linear_bwd_data (dZ = g W^T on gemm_x6_kernel, W's planes split
    from its [K][C] layout; the reduction runs over the C columns)."""
    grl_option("gemm_x6", 1)
    M, K, C = BWD_SHAPE
    assert x6_rows_ok(M, K, C) and not x6_rows_ok(M - 8, K, C)  # the [M, C] x [C, K] product that entry runs
    gen = torch.Generator(device=DEV).manual_seed(5)
    if variant == "w_one_hot":  # dZ[m, k] = g[m, c(k)] W[k, c(k)]
        g = _full((M, C), gen)
        c = _dev(xi.sweep(K, C, 3))
        W = torch.zeros(K, C, device=DEV)
        W[torch.arange(K, device=DEV), c] = _full((K,), gen)
        dZ = linear_bwd_data(g, None, W)
        worst = _check(dZ, g[:, c], W[torch.arange(K, device=DEV), c][None, :], what="dZ, W one-hot per row")
    else:  # dZ[m, k] = g[m, c(m)] W[k, c(m)]
        W = _full((K, C), gen)
        c = _dev(xi.sweep(M, C, 1))
        m = torch.arange(M, device=DEV)
        g = torch.zeros(M, C, device=DEV)
        g[m, c] = _full((M,), gen)
        dZ = linear_bwd_data(g, None, W)
        worst = _check(dZ, g[m, c][:, None], W[:, c].t(), what="dZ, g one-hot per row")
    _differs_from_fp32(dZ, lambda: linear_bwd_data(g, None, W), grl_option, "dZ")
    print(f"gemm_x6 dZ {variant}: worst error {worst:.3f} x 2^-22 |a b|")


def _rows_over(n, M):
    """n rows spread evenly over [0, M), the first three moved to the last
    three rows: every 256-row stretch (a split-K slab is at least that long)
    and the final, partial K16 step hold one."""
    r = (np.arange(n, dtype=np.int64) * M) // n
    r[:3] = [M - 1, M - 2, M - 3]
    assert len(np.unique(r)) == n and len(np.unique(r // 256)) == -(-M // 256) and (r >= M // 16 * 16).sum() == 3
    return r


@pytest.mark.parametrize("variant", ["z_one_hot", "g_one_hot"])
def test_gemm_weight_gradient_single_products(variant, grl_option):
    """gemm_x6t_kernel (dW = Z^T g, the reduction over the M rows in split-K
    slabs whose sums add exact zeros here): z_one_hot -- Z has one non-zero
    per column, at row r(k), and g is dense, dW[k, c] = Z[r(k), k] g[r(k), c];
    g_one_hot the mirror image.  db against the float64 column sum."""
    grl_option("gemm_x6", 1)
    M, K, C = BWD_SHAPE
    assert M % 16 == 3 and x6_rows_ok(M, K, C)
    gen = torch.Generator(device=DEV).manual_seed(9)
    if variant == "z_one_hot":
        g = _full((M, C), gen)
        r = _dev(_rows_over(K, M))
        k = torch.arange(K, device=DEV)
        Z = torch.zeros(M, K, device=DEV)
        Z[r, k] = _full((K,), gen)
        dW, db = linear_bwd_weight(Z, g, None, True)
        worst = _check(dW, Z[r, k][:, None], g[r], what="dW, Z one-hot per column")
    else:
        Z = _full((M, K), gen)
        r = _dev(_rows_over(C, M))
        c = torch.arange(C, device=DEV)
        g = torch.zeros(M, C, device=DEV)
        g[r, c] = _full((C,), gen)
        dW, db = linear_bwd_weight(Z, g, None, True)
        worst = _check(dW, Z[r].t(), g[r, c][None, :], what="dW, g one-hot per column")
    # the fp32 column sum, as test_large_tile_gemms_match_fp64 holds it: 1e-5 of sum |terms|
    _check(db, g.double().sum(0), None, 1e-5, "db", scale=g.double().abs().sum(0))
    _differs_from_fp32(dW, lambda: linear_bwd_weight(Z, g, None, False)[0], grl_option, "dW (gemm_x6t_kernel)")
    print(f"gemm_x6t dW {variant}: worst error {worst:.3f} x 2^-22 |a b|")


# ---- GraphConv: graphconv.hip, graphconv_ws_body.inc ---------------------------
def _graph(N, L, deg, seed, K, C):
    rowptr, colidx = ohash.synth_csr(0, L, N, int(N * deg), seed)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, has_self=True)
    g.path_rows = _pin_rows(K, C)  # the x6 GEMM, hence the one-kernel layer, on a small graph
    return g


def _fused_ws(X, g, W, C):
    name = f"grl_graphconv_fwd{'_bf16' if X.dtype == torch.bfloat16 else ''}_workspace_query"
    csr = g.csr_c(X.shape[1])
    return getattr(_lib.lib(), name)(ctypes.byref(csr), X.data_ptr(), X.stride(0), X.shape[1], W.data_ptr(), C)


@pytest.mark.parametrize("form", ["ws", "phases", "bf16_table"])
@pytest.mark.parametrize("N,C", [(300, 256), (129, 256), (300, 512)])
def test_graphconv_forward_single_products(N, C, form, grl_option):
    """The one-kernel GraphConv forwards (warp-specialized, phase-alternating
    fg_ws = 0, and on a bf16 feature table; C = 512: the 8-MFMA-wave form):
    with W one-hot per column over all (L + 1) F rows, out[n, c] =
    Z[n, k(c)] W[k(c), c] for the Z that graph_conv_fwd_train writes (bitwise
    the oracle's aggregation, test_gpu_graphconv.py) -- every segment and
    column residue over the runs; and with W a single dense row k0,
    out[n, c] = Z[n, k0] W[k0, c]."""
    L, F = 6, 256
    K = (L + 1) * F
    grl_option("fg_ws", 0 if form == "phases" else 1)
    g = _graph(N, L, 9.0, N + C, K, C)
    gen = torch.Generator(device=DEV).manual_seed(N + C)
    rng = np.random.default_rng(N + C)
    X = _full((N, F), gen)
    if form == "bf16_table":
        X = X.to(torch.bfloat16)
    c = torch.arange(C, device=DEV)
    worst = 0.0
    Z = None
    hot = [("cols", k_of_c) for k_of_c in _slices(C, K, C)] + [("row", k0) for k0 in (0, 255 + 37, 3 * F + 129, K - 1)]
    for kind, where in hot:
        if kind == "cols":
            k = _dev(where)
            W = _dev(xi.one_hot_cols(rng, K, C, where))
        else:
            W = torch.zeros(K, C, device=DEV)
            W[where] = _full((C,), gen)
            k = torch.full((C,), where, device=DEV)
        assert _fused_ws(X, g, W, C) == K * (256 if C <= 256 else 512) * 6 + 256  # W's planes only: the one kernel
        out = graph_conv_infer(X, g, W, None, False)
        out_t, Zt = graph_conv_fwd_train(X, g, W, None, False)
        assert torch.equal(out_t, out) and (Z is None or torch.equal(Zt, Z))
        Z = Zt
        worst = max(worst, _check(out, Z[:, k], W[k, c][None, :], what=f"out, W one-hot ({kind} {int(k[0])})"))
    assert bool((Z != 0).any(0).all())  # every column of Z carries values
    print(f"graphconv fwd N={N} C={C} {form}: worst error {worst:.3f} x 2^-22 |a b|")


def test_graphconv_data_gradient_few_products():
    """grl_graphconv_bwd_data (the one-kernel layer over the typed transpose)
    with G one-hot per row on a sparse graph: dX[m, f] = sum over the few
    non-zeros j = (s, c) of the aggregate G_agg[m, :] (written by the same
    kernel; sums of single values) of G_agg[m, j] W[s F + f, c].  A row with
    n non-zeros is held to (4 + 6 (n - 1)) 2^-24 of sum |terms|: 2^-22 for
    one product; each further product's six additions round at the
    accumulator's magnitude (2^-24 sum |terms| each)."""
    N, L, F, C = 20_011, 6, 256, 256
    S = L + 1
    g = TypedGraph.synthetic(N, 1.0, L, seed=4, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(N)
    W = _full((S * F, C), gen)
    n = torch.arange(N, device=DEV)
    G = torch.zeros(N, C, device=DEV)
    G[n, _dev(xi.sweep(N, C, 2))] = _full((N,), gen)
    res = graph_conv_bwd_data(G, g, W, F, want_aggregate=True)
    assert res is not None, "shape should take the one-kernel path"
    dX, G_agg, _ = res
    rows, j = G_agg.nonzero(as_tuple=True)
    per_row = torch.bincount(rows, minlength=N)
    assert int(per_row.min()) >= 1 and float((per_row <= 2).double().mean()) > 0.5
    s, c = j // C, j % C
    terms = G_agg[rows, j].double()[:, None] * W.view(S, F, C)[s, :, c].double()  # [nnz, F]
    ref = torch.zeros(N, F, device=DEV, dtype=torch.float64).index_add_(0, rows, terms)
    scale = torch.zeros(N, F, device=DEV, dtype=torch.float64).index_add_(0, rows, terms.abs())
    units = (4 + 6 * (per_row - 1)).double()[:, None]
    worst = _check(dX, ref, None, 2.0 ** -24, "dX", scale=units * scale)
    single = per_row == 1
    w1 = _check(dX[single], ref[single], None, xi.BARE, "dX, rows of one product", scale=scale[single])
    print(f"graphconv dX: worst error {worst:.3f} x the bound; rows of one product {w1:.3f} x 2^-22 |a b| "
          f"({int(single.sum())} rows)")


# ---- attention: attention.hip --------------------------------------------------
# (B, N, dk, dv, T) -> what the library's rules select for it (attention.hip: launch_attn, the plane staging of
# grl_node_attention_fwd_rows / _bwd_rows, the workspace sizes), as test_attention_regimes pins it:
#   x6_bwd  the split-bf16 backward kernels (dk <= 32 and dv in (96, 128]; else the fp32-MFMA backward, whatever
#           the forward runs)
#   planes  operands split once per call into LDS-DMA planes (>= 4096 rows, with a workspace)
#   fused   dQ folded into the dK pass (planes and dk <= 16): attn_bwd_kq16_kernel / attn_bwd_kq_x6_kernel, and
#           dH on attn_bwd_h16_kernel (16x16x32); otherwise attn_bwd_q_x6_kernel + attn_bwd_kv_x6_kernel
ATTN_REGIMES = {
    (2, 864, 4, 128, 24): dict(x6_bwd=True, planes=False, fused=False),  # in-kernel split, DKP = 16
    (8, 864, 16, 128, 24): dict(x6_bwd=True, planes=True, fused=True),  # planes, the 16x16x32 backward kernels
    (1, 2048, 16, 100, 36): dict(x6_bwd=True, planes=False, fused=False),  # key splits + combine, zero-padded dv
    (4, 1100, 32, 32, 26): dict(x6_bwd=False, planes=True, fused=False),  # the forward's 32-wide planes, DKP = 32;
    # its backward is the fp32-MFMA one (dv <= 96)
    (4, 1100, 32, 128, 26): dict(x6_bwd=True, planes=True, fused=False),  # the DKP = 32 x6 backward (two K chunks
    # of planes): attn_bwd_q_x6_kernel<32>, attn_bwd_kv_x6_kernel<32> on 256-key workgroups, query-split grid
    (4, 1100, 16, 128, 26): dict(x6_bwd=True, planes=True, fused=True),  # the 16x16x32 kernels on a split grid
}
ATTN_SHAPES = list(ATTN_REGIMES)
ATTN_FORMS = {"x6": {}, "x6-no-workspace": {}, "pipe0": {"attn_pipe": 0}, "wg4": {"attn_fwd8": 0, "attn_dh8": 0},
              "dh16_0": {"attn_dh16": 0}, "kq16_0": {"attn_kq16": 0}, "fused_dq0": {"attn_fused_dq": 0},
              "f32": {"attn_x6": 0}}


@functools.lru_cache(maxsize=None)
def _few_hot(B, N, dk, dv, T):
    """One fixture per batch (its own key and query permutations; the curve
    coordinates at a rotating offset inside dk), stacked on the device."""
    fxs = [xi.few_hot(N, dk, dv, seed=100 * N + b, T=T, offset=(5 * b) % (dk - 3)) for b in range(B)]
    dev = {name: torch.from_numpy(np.stack([getattr(f, name) for f in fxs])).to(DEV)
           for name in ("Q", "K", "H", "V", "dout")}
    dev["gamma"] = torch.from_numpy(fxs[0].gamma).to(DEV)
    for f in fxs:
        f.gamma = fxs[0].gamma
    return fxs, dev


@pytest.mark.parametrize("form", sorted(ATTN_FORMS))
@pytest.mark.parametrize("B,N,dk,dv,T", ATTN_SHAPES)
def test_attention_few_hot(B, N, dk, dv, T, form, monkeypatch, grl_option):
    """The few-hot fixture (x6_isolate.few_hot) through every kernel form the
    path options select, forward and backward.  Forward: onorm == H[k*]
    bitwise on hard rows (2^-23 on the fp32-MFMA control), p_r H[r] / l on
    soft-pair rows within 2^-21, out, rmax, rsum (x6_isolate.assert_forward).
    Backward: every row of dH, dK and the hard rows of dQ one scalar times
    dO / Q / K within 2^-21 (2^-20 where two queries meet), and every gradient
    and probability loosely against float64 (x6_isolate.assert_backward: why
    the backward's probabilities cannot be held tighter at these scores).
    Which kernels a shape runs: ATTN_REGIMES, pinned by
    test_attention_regimes.  Every option runs at every shape; one that
    selects nothing there (attn_dh16 without planes, any backward option at
    dv = 32) reruns the same kernels."""
    for name, value in ATTN_FORMS[form].items():
        grl_option(name, value)
    if form == "x6-no-workspace":
        monkeypatch.setattr(grl.ops, "_attn_workspace", lambda *a, **k: (None, 0))
    fxs, t = _few_hot(B, N, dk, dv, T)
    out, onorm, rmax, rsum = node_attention_forward(t["Q"], t["K"], t["H"], t["V"], t["gamma"], stats=True)
    dQ, dK, dH = node_attention_backward(t["Q"], t["K"], t["H"], t["gamma"], onorm, rmax, rsum, t["dout"])
    dO = t["dout"] * t["gamma"]  # as node_attention_backward forms it
    host = [a.cpu().numpy() for a in (out, onorm, rmax, rsum, dO, dQ, dK, dH)]
    worst = {}
    for b, f in enumerate(fxs):
        o, on, rm, rs, do, dq, dk_, dh = (a[b] for a in host)
        w = xi.assert_forward(f, on, o, rm, rs, bitwise_onorm=form != "f32", what=f"{form} batch {b}")
        w.update(xi.assert_backward(f, do, dq, dk_, dh, what=f"{form} batch {b}"))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    print(f"attention ({B}, {N}, {dk}, {dv}) {form}: worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("B,N,dk,dv,T", ATTN_SHAPES)
def test_attention_regimes(B, N, dk, dv, T, grl_option):
    """Which backward kernels a shape of test_attention_few_hot runs, pinned
    by what only they do -- the path options do not say which kernel ran, and
    the fp32-MFMA backward would meet every bound: the backward on the same
    saved stats gives other bits with attn_x6 = 0 exactly where the x6
    backward runs; the dQ slabs are in the backward workspace, and
    attn_fused_dq / attn_kq16 / attn_dh16 = 0 change bits, exactly where the
    fused 16x16x32 kernels run."""
    want = ATTN_REGIMES[(B, N, dk, dv, T)]
    lib = _lib.lib()
    ws = lib.grl_node_attention_workspace_size(B, N, dk, dv)
    bws = lib.grl_node_attention_bwd_workspace_size(B, N, dk, dv)
    assert (B * N >= 4096) == want["planes"] and (bws > ws) == want["fused"]
    _, t = _few_hot(B, N, dk, dv, T)
    _, onorm, rmax, rsum = node_attention_forward(t["Q"], t["K"], t["H"], t["V"], t["gamma"], stats=True)

    def backward(**options):
        for name, value in options.items():
            grl_option(name, value)
        res = node_attention_backward(t["Q"], t["K"], t["H"], t["gamma"], onorm, rmax, rsum, t["dout"])
        for name in options:
            grl_option(name, 1)
        return res

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    ref = backward()
    assert same(ref, backward())  # deterministic, so a difference below is another kernel
    assert same(ref, backward(attn_x6=0)) == (not want["x6_bwd"])
    assert same(ref, backward(attn_fused_dq=0)) == (not want["fused"])
    assert same(ref, backward(attn_kq16=0)) == (not want["fused"])
    assert torch.equal(ref[2], backward(attn_dh16=0)[2]) == (not want["fused"])
