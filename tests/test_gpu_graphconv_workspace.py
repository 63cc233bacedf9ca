"""GPU: the GraphConv entries keep to the workspace they ask for.

The forward entries take their pointers from one description of the two-kernel
chain's workspace (graphconv.hip: fwd_chain_layout: an fp32 Z, the linear's
fp32 output, the linear's own workspace), the one their queries answer from.
Here every wrapper runs once on a workspace torch allocated, and once on one of
exactly the bytes asked for, filled with 0xFF bytes (NaN as fp32 and as bf16)
and followed by 4096 guard bytes of 0xA5.  The outputs must be the same bits and
the guard unchanged: a region read before it is written, two regions that
overlap, or a store past the total breaks one of the two.

Shapes: N = 20011, 6 types and self loops, F = C = 256 -- just above the x6
GEMM's flop floor, one kernel; the same with the graphconv_fused option 0, the
chain on the x6 linear (and, for the fp32 inference entry, in row chunks under a
bounded workspace); N = 300, F = 64, C = 32, the chain on the small fp32 linear
with its own workspace size.  DropEdge 0.3 on the one-kernel and the small
forward cases and on the bf16 data gradient.  The data gradient has no path
below the floor, so it runs at the large shape only."""
import pytest
import torch

from grl import DropEdge, TypedGraph, ops
from grl.ops import graph_conv_bwd_data, graph_conv_fwd_train, graph_conv_infer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
GUARD = 4096
L = 6
# mode -> (N, F, C, graphconv_fused, DropEdge)
MODES = {"one_kernel": (20_011, 256, 256, 1, DropEdge(0.3, 3, 2, True)),
         "chain_x6": (20_011, 256, 256, 0, None),
         "chain_small": (300, 64, 32, 1, DropEdge(0.3, 5, 1, True))}
_cache = {}


def _case(N, F, C):
    """(graph, X, W, b, g) for a shape, made once: the tests only read them."""
    if (N, F, C) not in _cache:
        graph = TypedGraph.synthetic(N, 16.0, L, seed=N % 7, device=DEV)
        gen = torch.Generator(device=DEV).manual_seed(N + F)
        K = graph.segments * F
        _cache[N, F, C] = (graph, torch.randn(N, F, device=DEV, generator=gen),
                           torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5,
                           torch.randn(C, device=DEV, generator=gen), torch.randn(N, C, device=DEV, generator=gen))
    return _cache[N, F, C]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _same_under_a_guarded_workspace(monkeypatch, run):
    """run() -> a tuple of tensors: once as it is, once with every workspace exact, NaN-filled and guarded."""
    want = run()
    made = []

    def guarded(nbytes, device):
        if not nbytes:
            return None
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[:nbytes] = 0xFF
        buf[nbytes:] = 0xA5
        made.append((buf, nbytes))
        return buf[:nbytes]

    monkeypatch.setattr(ops, "_workspace", guarded)
    got = run()
    torch.cuda.synchronize()
    assert made, "the call asked for no workspace"
    for buf, nbytes in made:
        assert bool((buf[nbytes:] == 0xA5).all()), f"a store past the {nbytes} bytes asked for"
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
    return made


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("operands", ["fp32", "bf16", "bf16_to_bf16"])
def test_infer_keeps_to_its_workspace(mode, operands, monkeypatch, grl_option):
    N, F, C, fused, de = MODES[mode]
    grl_option("graphconv_fused", fused)
    graph, X, W, b, _ = _case(N, F, C)
    graph = graph.with_dropedge(de)
    Xo = X if operands == "fp32" else X.to(BF16)

    def run():
        out = torch.empty(N, C, dtype=BF16, device=DEV) if operands == "bf16_to_bf16" else None
        return (graph_conv_infer(Xo, graph, W, b, True, out=out),)

    made = _same_under_a_guarded_workspace(monkeypatch, run)
    K = graph.segments * F
    assert (made[0][1] < N * K * 2) == (mode == "one_kernel")  # W's planes alone, or Z whole in the workspace


def test_infer_in_row_chunks_keeps_to_its_workspace(monkeypatch, grl_option):
    N, F, C, _, _ = MODES["chain_x6"]
    grl_option("graphconv_fused", 0)
    graph, X, W, b, _ = _case(N, F, C)
    graph = graph.with_dropedge(DropEdge(0.3, 2, 0, True))
    K = graph.segments * F
    bound = 3 * ((C + 255) // 256 * 256) * K * 2 + 256 + 256 + 8704 * K * 4  # W's planes and 8704 rows of Z: 3 chunks
    whole = graph_conv_infer(X, graph, W, b, True)
    made = _same_under_a_guarded_workspace(
        monkeypatch, lambda: (graph_conv_infer(X, graph, W, b, True, max_workspace_bytes=bound),))
    assert made[0][1] == bound < N * K * 4
    assert torch.equal(whole, graph_conv_infer(X, graph, W, b, True, max_workspace_bytes=bound))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("operands", ["fp32", "bf16", "bf16_to_bf16", "z16"])
def test_fwd_train_keeps_to_its_workspace(mode, operands, monkeypatch, grl_option):
    N, F, C, fused, de = MODES[mode]
    grl_option("graphconv_fused", fused)
    graph, X, W, b, _ = _case(N, F, C)
    graph = graph.with_dropedge(de)
    Xo = X if operands == "fp32" else X.to(BF16)

    def run():
        out = torch.empty(N, C, dtype=BF16, device=DEV) if operands in ("bf16_to_bf16", "z16") else None
        return graph_conv_fwd_train(Xo, graph, W, b, True, out=out, z_dtype=BF16 if operands == "z16" else None)

    _same_under_a_guarded_workspace(monkeypatch, run)


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_bwd_data_keeps_to_its_workspace(operands, monkeypatch):
    N, F, C, _, _ = MODES["one_kernel"]
    graph, _, W, _, g = _case(N, F, C)
    graph = graph.with_dropedge(DropEdge(0.3, 4, 1, True) if operands == "bf16" else None)
    go = g if operands == "fp32" else g.to(BF16)

    def run():
        res = graph_conv_bwd_data(go, graph, W, F, want_aggregate=True)
        assert res is not None, "outside the one-kernel path"
        return res[:2]  # dX, G_agg

    _same_under_a_guarded_workspace(monkeypatch, run)
