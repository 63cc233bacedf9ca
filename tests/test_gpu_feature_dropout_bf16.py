"""The bf16 feature dropout (grl_feature_dropout_bf16 through
grl.ops.feature_dropout_apply / feature_dropout) and the scaled bf16 ReLU mask
pass (grl_relu_grad_bf16_scaled) on the GPU.

The dropout is compared on bits against the fp32 entry on the widened input,
rounded once (.to(bfloat16) rounds to nearest even): every load form (16 B, 8 B
and 2 B a lane), column slices beside sentinels, in place, and a slice that is
only 2 B-aligned.  The mask pass is compared on bits against its statement in
torch and against grl_relu_grad on the widened result."""
import ctypes

import pytest
import torch

from grl import DropEdge, _lib
from grl.graph import current_stream_handle
from grl.ops import _relu_grad_bf16, feature_dropout, feature_dropout_apply, relu_grad, relu_grad_bf16_scaled

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern
SEED, CALL = 77, (1 << 48) + 3
SHAPES = [(1, 1), (3, 4), (5, 8), (7, 12), (2, 264), (33, 250)]  # (5, 8), (2, 264): 16 B; (3, 4), (7, 12): 8 B; else 2 B
BIG_ROW0 = 1 << 33  # row0 * cols > 2^32 at every width


def _bits(t):
    return t.view(torch.int16)


def _sentinel_table(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


def _values(rows, cols):
    """bf16 values whose products with 1/0.7 need rounding (random mantissas),
    with -0, +0 and subnormals of both signs among them."""
    gen = torch.Generator(device=DEV).manual_seed(rows * 1000 + cols)
    x = (torch.randn(rows, cols, device=DEV, generator=gen) * 3).to(BF16)
    flat = _bits(x).view(-1)
    special = torch.tensor([-0x8000, 0x0000, 0x0001, 0x007F, -0x8000 + 3, 0x0040], dtype=torch.int16, device=DEV)
    n = min(flat.numel() // 2, special.numel())
    flat[1:1 + n] = special[:n]
    return x


def _record(p, seed_tensor):
    if seed_tensor:
        return DropEdge(p, 0, CALL, seed_tensor=torch.tensor([SEED], dtype=torch.int64, device=DEV))
    return DropEdge(p, SEED, CALL)


def _want(x, de, row0):
    """The contract: the fp32 entry on the widened x, rounded once."""
    return feature_dropout_apply(x.float().contiguous(), de, row0).to(BF16)


@pytest.mark.parametrize("p", [0.3, 0.5, 1.0, 0.0])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bits_are_the_fp32_entrys_rounded_once(rows, cols, p):
    x = _values(rows, cols)
    for row0 in (0, BIG_ROW0):
        want = _want(x, _record(p, False), row0)
        for seed_tensor in (False, True):
            de = _record(p, seed_tensor)
            got = feature_dropout_apply(x, de, row0)
            assert got.dtype == BF16 and got.shape == x.shape and got.is_contiguous()
            assert torch.equal(_bits(got), _bits(want)), (row0, seed_tensor)
        # column slices of wider tables as x and out, sentinels on both sides
        xw, ow = _sentinel_table(rows, cols + 16), _sentinel_table(rows, cols + 24)
        xw[:, 8:8 + cols] = x
        out = feature_dropout_apply(xw[:, 8:8 + cols], de, row0, out=ow[:, 16:16 + cols])
        assert out.data_ptr() == ow[:, 16:16 + cols].data_ptr()
        assert torch.equal(_bits(ow[:, 16:16 + cols]), _bits(want))
        assert bool((_bits(ow[:, :16]) == SENTINEL).all()) and bool((_bits(ow[:, 16 + cols:]) == SENTINEL).all())
        assert torch.equal(_bits(xw[:, 8:8 + cols]), _bits(x)) and bool((_bits(xw[:, :8]) == SENTINEL).all())
        # in place: out aliasing x
        xi = xw[:, 8:8 + cols]
        feature_dropout_apply(xi, de, row0, out=xi)
        assert torch.equal(_bits(xi), _bits(want))
        assert bool((_bits(xw[:, :8]) == SENTINEL).all()) and bool((_bits(xw[:, 8 + cols:]) == SENTINEL).all())
        # a slice starting at an odd column: only 2 B-aligned, the one-element form, the same bits
        xo, oo = _sentinel_table(rows, cols + 9), _sentinel_table(rows, cols + 9)
        xo[:, 1:1 + cols] = x
        assert xo[:, 1:].data_ptr() % 4 == 2
        feature_dropout_apply(xo[:, 1:1 + cols], de, row0, out=oo[:, 1:1 + cols])
        assert torch.equal(_bits(oo[:, 1:1 + cols]), _bits(want))
        assert bool((_bits(oo[:, :1]) == SENTINEL).all()) and bool((_bits(oo[:, 1 + cols:]) == SENTINEL).all())
    if p == 0.0:  # an inactive record copies the bits
        assert torch.equal(_bits(want), _bits(x))
    if p == 1.0:  # everything dropped: +0
        assert bool((_bits(want) == 0).all())


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("row0", [0, BIG_ROW0])
def test_the_kept_set_is_grl_dropedge_mask_over_the_same_ids(rows, cols, row0):
    p = 0.3
    x = _values(rows, cols)
    de = _record(p, False)
    keep = torch.empty(rows * cols, dtype=torch.uint8, device=DEV)
    dc = de.to_c()
    _lib.call("grl_dropedge_mask", ctypes.byref(dc), row0 * cols, rows * cols, keep.data_ptr(),
              current_stream_handle(DEV))
    keep = keep.view(rows, cols).bool()
    got = feature_dropout_apply(x, de, row0)
    scale = float(dc.scale)
    want = torch.where(keep, (x.float() * scale).to(BF16), torch.zeros((), dtype=BF16, device=DEV))
    assert torch.equal(_bits(got), _bits(want))
    # kept elements keep their sign and never vanish (scale > 1); dropped ones are +0
    assert torch.equal(_bits(got) != 0, keep & (_bits(x) != 0))


def test_autograd_hands_back_the_forward_map_of_a_bf16_gradient():
    rows, cols, row0 = 33, 250, 12
    de = _record(0.5, False)
    x = _values(rows, cols).requires_grad_(True)
    out = feature_dropout(x, de, row0)
    assert out.dtype == BF16
    assert torch.equal(_bits(out.detach()), _bits(_want(x.detach(), de, row0)))
    up = _values(cols, rows).t().contiguous()  # other values
    out.backward(up)
    assert x.grad.dtype == BF16 and x.grad.shape == x.shape
    assert torch.equal(_bits(x.grad), _bits(feature_dropout_apply(up, de, row0)))
    assert torch.equal(_bits(x.grad), _bits(_want(up, de, row0)))
    # a batch of rows [B, N, C] keeps its shape
    x3 = _values(6, 8).view(2, 3, 8)
    assert torch.equal(_bits(feature_dropout(x3, de)), _bits(feature_dropout_apply(x3.view(6, 8), de, 0).view(2, 3, 8)))


def test_dtype_and_layout_errors():
    de = _record(0.5, False)
    x = _values(8, 16)
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x.to(torch.float16), de, 0)
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x.t(), de, 0)  # no unit column stride
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x[:1].expand(8, 16), de, 0)  # rows not apart
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x.view(2, 4, 16), de, 0)
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x, de, 0, out=torch.empty(8, 16, device=DEV))  # an fp32 out
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x, de, 0, out=torch.empty(8, 8, dtype=BF16, device=DEV))
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x, de, 0, out=torch.empty(16, 8, dtype=BF16, device=DEV).t())
    with pytest.raises(_lib.GrlError):
        feature_dropout_apply(x.cpu(), de, 0)


# ---------------------------------------------------------------- the scaled mask pass
@pytest.mark.parametrize("C", [1, 3, 256, 257])
@pytest.mark.parametrize("M", [1, 7, 9, 1000])
def test_scaled_mask_pass(M, C, monkeypatch):
    import grl.ops as ops

    monkeypatch.setattr(ops, "PREMASK_ROWS", 1)  # relu_grad through grl_relu_grad at these row counts
    scale = float(_record(0.3, False).to_c().scale)
    gen = torch.Generator(device=DEV).manual_seed(M * 1000 + C)
    g = torch.randn(M, C, device=DEV, generator=gen).to(BF16)
    out = torch.relu(torch.randn(M, C, device=DEV, generator=gen)).to(BF16)
    _bits(out).view(-1)[::5] = -0x8000  # -0: not > 0
    _bits(g).view(-1)[::3] = -0x8000    # -0 gradients, masked and open
    zero = torch.zeros((), dtype=BF16, device=DEV)
    want16 = torch.where(out > 0, (g.float() * scale).to(BF16), zero)
    want32, _, want_db = relu_grad(want16.float().contiguous(), torch.ones(M, C, device=DEV), True)
    assert torch.equal(want32, want16.float())
    g16, g32, db = relu_grad_bf16_scaled(g, out, scale, True, True)
    assert g16.dtype == BF16 and g32.dtype == torch.float32 and g32.is_contiguous()
    assert torch.equal(_bits(g16), _bits(want16)) and torch.equal(g32, want32) and torch.equal(db, want_db)
    assert bool((_bits(g16)[~(out > 0)] == 0).all())  # masked entries are +0, a masked -0 included
    # each output NULL in turn
    a, b, c = relu_grad_bf16_scaled(g, out, scale, False, True)
    assert c is None and torch.equal(b, want32) and torch.equal(_bits(a), _bits(want16))
    a, b, c = relu_grad_bf16_scaled(g, out, scale, True, False)
    assert b is None and torch.equal(c, want_db) and torch.equal(_bits(a), _bits(want16))
    a, b, c = _relu_grad_bf16(g, out, True, True, want_16=False, scale=scale)
    assert a is None and torch.equal(b, want32) and torch.equal(c, want_db)
    # strided operands beside sentinels
    gw, ow = _sentinel_table(M, C + 8), _sentinel_table(M, 2 * C + 1)
    gw[:, 4:4 + C] = g
    ow[:, C + 1:] = out
    table = _sentinel_table(M, C + 16)
    a, b, c = _relu_grad_bf16(gw[:, 4:4 + C], ow[:, C + 1:], True, True, g_eff16=table[:, 8:8 + C], scale=scale)
    assert torch.equal(_bits(a), _bits(want16)) and torch.equal(b, want32) and torch.equal(c, want_db)
    assert bool((_bits(table[:, :8]) == SENTINEL).all()) and bool((_bits(table[:, 8 + C:]) == SENTINEL).all())
    # g_eff16 aliasing g
    gi = gw[:, 4:4 + C]
    a, b, c = _relu_grad_bf16(gi, ow[:, C + 1:], True, True, g_eff16=gi, scale=scale)
    assert a is gi and torch.equal(_bits(gi), _bits(want16)) and torch.equal(b, want32) and torch.equal(c, want_db)
    assert bool((_bits(gw[:, :4]) == SENTINEL).all()) and bool((_bits(gw[:, 4 + C:]) == SENTINEL).all())
    assert bool((_bits(ow[:, :C + 1]) == SENTINEL).all())
