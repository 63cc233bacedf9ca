"""Autograd ops over the libgrl kernels.

  typed_aggregate(X, graph)   Z = A_drop X           robust_gcn.py:45-47
                              (+ edge_dropout, drop_robust_gcn.py:76,80,85)
  graph_linear(Z, W, b, relu) out = Z W + b [ReLU]    robust_gcn.py:50
                              (+ F.relu, drop_robust_gcn.py:76,80,85)

Both run on the current torch HIP stream; backward regenerates the DropEdge
mask from the graph's (p, seed, call) record, exactly like forward.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call
from .graph import EdgeBlockedGraph, TypedGraph, _require_device, current_stream_handle


def _rows_view(X: torch.Tensor) -> torch.Tensor:
    """2-D row view with unit column stride (no copy when possible)."""
    X2 = X.reshape(-1, X.shape[-1])
    if X2.stride(-1) != 1:
        X2 = X2.contiguous()
    return X2


def _ptr(t):
    """A tensor's address, or None (NULL) for no tensor."""
    return t.data_ptr() if t is not None else None


def _workspace(nbytes: int, device):
    """A workspace of nbytes on `device`; None (NULL) for none."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def _de_ref(graph):
    """The graph's DropEdge record by reference, or None (NULL) without one.
    The reference holds the ctypes struct, which so lives as long as the
    call's argument list."""
    return ctypes.byref(graph.dropedge.to_c()) if graph.dropedge is not None else None


# What the aggregation gathers from: fp32, or bf16 read as stored and widened
# on the fly (grl_typed_spmm_fwd_bf16) -- never through a widened copy.
_TABLE_DTYPES = (torch.float32, torch.bfloat16)


def _bf16_suffix(X2: torch.Tensor, out: torch.Tensor = None) -> str:
    """'_bf16' for a bfloat16 table: the grl_graphconv_fwd*_bf16 entries;
    '_bf16_to_bf16' when `out` is bfloat16 too."""
    if X2.dtype != torch.bfloat16:
        return ""
    return "_bf16_to_bf16" if out is not None and out.dtype == torch.bfloat16 else "_bf16"


def _graphconv_fwd_call(entry: str, csr, X2, F, Wc, bc, relu: bool, out, Z, graph, ws_bytes: int):
    """One grl_graphconv_fwd* call on a new workspace (ldo behind a bfloat16 out, Z behind that when training)."""
    ws = _workspace(ws_bytes, X2.device)
    call(entry, ctypes.byref(csr), X2.data_ptr(), X2.stride(0), F, Wc.data_ptr(), _ptr(bc), Wc.shape[1], int(relu),
         out.data_ptr(), *([out.stride(0)] if out.dtype == torch.bfloat16 else []),
         *([Z.data_ptr()] if Z is not None else []), _de_ref(graph), _ptr(ws), ws_bytes,
         current_stream_handle(X2.device))


def _want_bf16(who: str, out, out_dtype) -> bool:
    """Whether a call's result is bfloat16: by its `out` tensor, or by
    `out_dtype` (None: float32) when it makes a new one."""
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"{who}: out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
    if out is not None and out_dtype is not None and out.dtype != out_dtype:
        raise _lib.GrlError(f"{who}: out is {out.dtype}, out_dtype {out_dtype}")
    return (out.dtype if out is not None else out_dtype) == torch.bfloat16


def _forward_args(who: str, X, graph, W=None, b=None, out=None, Z=None, want_Z: bool = False,
                  z_dtype=torch.float32):
    """The checked operands of a forward over `graph` -- (X2, F, Wc, bc, out,
    Z): the features' 2-D row view and width, the contiguous weights
    [segments * F, C] and bias (None without), out [num_rows, C] (with
    weights) and Z [num_rows, segments * F] (want_Z), each the contiguous
    fp32 tensor given or a new one.  The features may be bfloat16 (the table
    is read as stored); weights and bias are float32.  With bfloat16 features
    `out` may be a bfloat16 [num_rows, C] tensor with unit column stride and
    any row stride (a column-slice view of a wider table), written in place.
    z_dtype = torch.bfloat16 (bfloat16 features only): Z is a contiguous
    bfloat16 tensor instead."""
    _require_device(X, "node features")
    if X.dtype not in _TABLE_DTYPES:
        raise _lib.GrlError(f"{who}: node features must be float32 or bfloat16 (got {X.dtype})")
    if W is not None and (W.dtype != torch.float32 or (b is not None and b.dtype != torch.float32)):
        raise _lib.GrlError(f"{who}: weights and bias must be float32")
    X2 = _rows_view(X)
    if X2.shape[0] != graph.num_cols:
        raise _lib.GrlError(f"features have {X2.shape[0]} rows, graph gathers from {graph.num_cols}")
    F = X2.shape[1]
    K = graph.segments * F
    Wc = W.contiguous() if W is not None else None
    if Wc is not None and Wc.shape[0] != K:
        raise _lib.GrlError(f"weights have {Wc.shape[0]} rows, expected {graph.segments} x {F}")

    if z_dtype == torch.bfloat16 and X.dtype != torch.bfloat16:
        raise _lib.GrlError(f"{who}: a bfloat16 Z needs bfloat16 node features (got {X.dtype}): there is no mixed "
                            "form -- cast the table once")

    def target(t, what, cols, dtype=torch.float32):
        shape = (graph.num_rows, cols)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=X.device)
        if what == "out" and t.dtype == torch.bfloat16:
            if X.dtype != torch.bfloat16:
                raise _lib.GrlError(f"{who}: a bfloat16 out needs bfloat16 node features (got {X.dtype}): there is no "
                                    "fp32-table form with a bf16 output -- cast the table once")
            if tuple(t.shape) != shape or t.stride(1) != 1 or t.stride(0) < cols or t.device != X.device:
                raise _lib.GrlError(f"{who}: a bfloat16 out must be a {shape} tensor on {X.device} with unit column "
                                    "stride and a row stride of at least its width")
            return t
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != X.device:
            name = "float32" if dtype == torch.float32 else "bfloat16"
            raise _lib.GrlError(f"{who}: {what} must be a contiguous {name} {shape} tensor on {X.device}")
        return t

    return (X2, F, Wc, b.contiguous() if b is not None else None,
            target(out, "out", Wc.shape[1]) if Wc is not None else None, target(Z, "Z", K, z_dtype) if want_Z else None)


def spmm_forward(X: torch.Tensor, graph: TypedGraph, out: torch.Tensor = None, out_dtype=None) -> torch.Tensor:
    """Z = A_drop X without autograd bookkeeping, optionally into `out`
    (contiguous [num_rows, segments*F]): the inference / benchmark form.
    X float32 or bfloat16 (read as stored: half the gather bytes, Z bitwise
    the fp32 result on X.float()).  Z is float32 unless `out` is bfloat16 or
    out_dtype = torch.bfloat16 (bfloat16 X only; there is no mixed form): then
    Z is that fp32 result rounded once to nearest even, written as bfloat16
    by the kernel (grl_typed_spmm_fwd_bf16_to_bf16) -- no fp32 Z exists."""
    z16 = _want_bf16("spmm_forward", out, out_dtype)
    if isinstance(graph, EdgeBlockedGraph):
        return _blocked_forward(X, graph, out, torch.bfloat16 if z16 else torch.float32)
    X2, F, _, _, _, Z = _forward_args("spmm_forward", X, graph, Z=out, want_Z=True,
                                      z_dtype=torch.bfloat16 if z16 else torch.float32)
    if X2.dtype == torch.bfloat16:
        call("grl_typed_spmm_fwd_bf16_to_bf16" if z16 else "grl_typed_spmm_fwd_bf16", ctypes.byref(graph.csr_c(F)),
             X2.data_ptr(), X2.stride(0), F, 0, Z.data_ptr(), graph.segments * F, F, _de_ref(graph),
             current_stream_handle(X.device))
        return Z
    call("grl_typed_spmm_fwd", ctypes.byref(graph.csr_c(F)), X2.data_ptr(), X2.stride(0), F, Z.data_ptr(),
         _de_ref(graph), current_stream_handle(X.device))
    return Z


def spmm_forward_slice(X: torch.Tensor, graph: TypedGraph, out: torch.Tensor, col0: int,
                       self_col0: int = 0) -> torch.Tensor:
    """Columns [col0, col0 + F) of Z = A_drop X into `out` (contiguous
    [num_rows, segments * F_total]), where X is that column slice's table
    ([graph.num_cols, F], any row stride) and row n's self term reads X row
    self_col0 + n (grl_typed_spmm_fwd_slice; a bfloat16 table:
    grl_typed_spmm_fwd_bf16, into a bfloat16 `out`
    grl_typed_spmm_fwd_bf16_to_bf16).  Bitwise equal, per element, to the
    whole-width spmm_forward: the pipelined halo exchange of grl.dist
    aggregates one slice while the next is in flight."""
    _require_device(X, "node features")
    if X.dtype not in _TABLE_DTYPES or X.dim() != 2 or X.stride(1) != 1:
        raise _lib.GrlError("slice table must be a 2-D float32 or bfloat16 tensor with unit column stride")
    if X.shape[0] != graph.num_cols:
        raise _lib.GrlError(f"slice table has {X.shape[0]} rows, graph gathers from {graph.num_cols}")
    F = X.shape[1]
    S = graph.segments
    if out.dtype not in _TABLE_DTYPES or not out.is_contiguous() or out.shape[0] != graph.num_rows \
            or out.shape[1] % S or out.device != X.device:
        raise _lib.GrlError(f"out must be a contiguous float32 [{graph.num_rows}, {S} x F_total] tensor "
                            "(bfloat16 for a bfloat16 table)")
    if out.dtype == torch.bfloat16 and X.dtype != torch.bfloat16:
        raise _lib.GrlError(f"a bfloat16 out needs a bfloat16 slice table (got {X.dtype}): there is no mixed form")
    zseg = out.shape[1] // S
    if col0 < 0 or col0 + F > zseg:
        raise _lib.GrlError(f"columns [{col0}, {col0 + F}) outside the {zseg}-column segments")
    entry = "grl_typed_spmm_fwd_slice" if X.dtype == torch.float32 else \
        "grl_typed_spmm_fwd_bf16" + ("_to_bf16" if out.dtype == torch.bfloat16 else "")
    call(entry, ctypes.byref(graph.csr_c(F)), X.data_ptr(), X.stride(0), F, int(self_col0),
         out.data_ptr() + out.element_size() * col0, out.stride(0), zseg, _de_ref(graph),
         current_stream_handle(X.device))
    return out


def _blocked_forward(X: torch.Tensor, graph: EdgeBlockedGraph, out: torch.Tensor = None,
                     dtype=torch.float32) -> torch.Tensor:
    """Z (of `dtype`) of a graph with >= 2^31 edges: one aggregation per row
    block (self rows at the block's first row, Z rows likewise)."""
    X2 = _rows_view(X)
    if X2.shape[0] != graph.num_cols:
        raise _lib.GrlError(f"features have {X2.shape[0]} rows, graph gathers from {graph.num_cols}")
    F = X2.shape[1]
    shape = (graph.num_rows, graph.segments * F)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=X.device)
    elif tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != dtype:
        raise _lib.GrlError(f"out must be a contiguous {dtype} {shape} tensor")
    for blk, r0, r1 in zip(graph.blocks, graph.row_bounds[:-1], graph.row_bounds[1:]):
        spmm_forward_slice(X2, blk, out[r0:r1], 0, self_col0=r0)
    return out


def _blocked_backward(dZ: torch.Tensor, graph: EdgeBlockedGraph, F: int) -> torch.Tensor:
    """dX of a graph with >= 2^31 edges: the blocks' CSCs in block order --
    the first with the self term over every row, the rest continuing each
    column's sum (grl_typed_spmm_bwd_accum)."""
    dZ = dZ.contiguous().float()
    dX = torch.empty(graph.num_cols, F, dtype=torch.float32, device=dZ.device)
    stream = current_stream_handle(dZ.device)
    ldz = graph.segments * F
    for i, (blk, r0) in enumerate(zip(graph.blocks, graph.row_bounds[:-1])):
        csc = blk.csc_c(F)
        if i == 0:
            csc.self_rows = min(graph.num_rows, graph.num_cols)  # every node's self loop, dZ rows from 0
        call("grl_typed_spmm_bwd" if i == 0 else "grl_typed_spmm_bwd_accum", ctypes.byref(csc),
             dZ.data_ptr() + 4 * r0 * ldz, F, dX.data_ptr(), F, _de_ref(blk), stream)
    return dX


def _bwd_out(who: str, out, graph, F, dtype, device):
    """dX [graph.num_cols, F] of `dtype`: the tensor given (unit column
    stride, any row stride) or a new one."""
    if out is None:
        return torch.empty(graph.num_cols, F, dtype=dtype, device=device)
    if tuple(out.shape) != (graph.num_cols, F) or out.dtype != dtype or out.stride(1) != 1 or out.stride(0) < F \
            or out.device != device:
        raise _lib.GrlError(f"{who}: out must be a {dtype} [{graph.num_cols}, {F}] tensor on {device} with unit "
                            "column stride")
    return out


def spmm_backward(dZ: torch.Tensor, graph: TypedGraph, F: int, out: torch.Tensor = None,
                  out_dtype=None) -> torch.Tensor:
    """dX = A_drop^T dZ (grl_typed_spmm_bwd over the cached CSC, same mask),
    optionally into `out` ([graph.num_cols, F], unit column stride).  dX is
    float32 -- a bfloat16 dZ is widened first -- unless `out` is bfloat16 or
    out_dtype = torch.bfloat16: then dZ must be bfloat16 (there is no mixed
    form), is gathered as stored (an expanded or transposed gradient is copied
    once, in bfloat16) and dX is the fp32 result on dZ.float() rounded once to
    nearest even, written as bfloat16 by the kernel (grl_typed_spmm_bwd_bf16):
    no widened dZ and no fp32 dX exist.  An EdgeBlockedGraph gives the same
    bits through its fp32 accumulating chain, rounded at the end."""
    x16 = _want_bf16("spmm_backward", out, out_dtype)
    if x16 and dZ.dtype != torch.bfloat16:
        raise _lib.GrlError(f"spmm_backward: a bfloat16 dX needs a bfloat16 dZ (got {dZ.dtype}): there is no mixed form")
    if isinstance(graph, EdgeBlockedGraph):
        dX = _blocked_backward(dZ, graph, F)
        if out is None:
            return dX.to(torch.bfloat16) if x16 else dX
        return _bwd_out("spmm_backward", out, graph, F, out.dtype, dZ.device).copy_(dX)
    if x16:
        _require_device(dZ, "dZ")
        dZ = dZ.reshape(graph.num_rows, graph.segments * F)
        if not dZ.is_contiguous():
            dZ = dZ.contiguous()
        dX = _bwd_out("spmm_backward", out, graph, F, torch.bfloat16, dZ.device)
        call("grl_typed_spmm_bwd_bf16", ctypes.byref(graph.csc_c(F)), dZ.data_ptr(), F, 0, F, dX.data_ptr(),
             dX.stride(0), _de_ref(graph), current_stream_handle(dZ.device))
        return dX
    dZ = dZ.contiguous().float()
    dX = _bwd_out("spmm_backward", out, graph, F, torch.float32, dZ.device)
    call("grl_typed_spmm_bwd", ctypes.byref(graph.csc_c(F)), dZ.data_ptr(), F, dX.data_ptr(), dX.stride(0),
         _de_ref(graph), current_stream_handle(dZ.device))
    return dX


def spmm_backward_slice(dZ: torch.Tensor, graph: TypedGraph, col0: int, out: torch.Tensor) -> torch.Tensor:
    """Columns [col0, col0 + F) of dX = A_drop^T dZ into `out` ([graph.num_cols,
    F], unit column stride, any row stride), dZ contiguous
    [num_rows, segments * F_total] (grl_typed_spmm_bwd_slice).  dZ and out are
    both float32 or both bfloat16 (grl_typed_spmm_bwd_bf16).  Bitwise equal,
    per element, to spmm_backward: the pipelined backward of grl.dist sends
    one slice's halo-row gradients home while the next slice gathers."""
    if isinstance(graph, EdgeBlockedGraph):
        raise _lib.GrlError("column-slice backward takes a TypedGraph (edge-blocked graphs: spmm_backward)")
    _require_device(dZ, "dZ")
    if dZ.dtype not in _TABLE_DTYPES or not dZ.is_contiguous() or dZ.dim() != 2 or dZ.shape[0] != graph.num_rows \
            or dZ.shape[1] % graph.segments:
        raise _lib.GrlError(f"dZ must be a contiguous float32 [{graph.num_rows}, {graph.segments} x F_total] tensor "
                            "(or bfloat16, with a bfloat16 out)")
    F_total = dZ.shape[1] // graph.segments
    if out.dtype != dZ.dtype:
        raise _lib.GrlError(f"dZ is {dZ.dtype}, out {out.dtype}: there is no mixed form")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != graph.num_cols or out.device != dZ.device:
        raise _lib.GrlError(f"out must be a {dZ.dtype} [{graph.num_cols}, F] tensor with unit column stride")
    F = out.shape[1]
    entry = "grl_typed_spmm_bwd_bf16" if dZ.dtype == torch.bfloat16 else "grl_typed_spmm_bwd_slice"
    call(entry, ctypes.byref(graph.csc_c(F)), dZ.data_ptr(), F_total, int(col0), F,
         out.data_ptr(), out.stride(0), _de_ref(graph), current_stream_handle(dZ.device))
    return out


class _TypedAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X: torch.Tensor, graph: TypedGraph, out_dtype=None) -> torch.Tensor:
        Z = spmm_forward(X, graph, out_dtype=out_dtype)
        ctx.graph = graph
        ctx.xshape = X.shape
        ctx.xdtype = X.dtype
        ctx.z16 = Z.dtype == torch.bfloat16
        return Z

    @staticmethod
    def backward(ctx, dZ: torch.Tensor):
        if ctx.z16:  # bf16 dZ gathered as stored, bf16 dX as the kernel writes it: no fp32 pass on either side
            dX = spmm_backward(dZ, ctx.graph, ctx.xshape[-1], out_dtype=torch.bfloat16)
            return dX.view(ctx.xshape), None, None
        # an fp32 Z, so dZ is fp32: one fp32 transpose pass, rounded once for a bf16 X
        return spmm_backward(dZ, ctx.graph, ctx.xshape[-1]).view(ctx.xshape).to(ctx.xdtype), None, None


def typed_aggregate(X: torch.Tensor, graph: TypedGraph, out_dtype=None) -> torch.Tensor:
    """Z[n, s*F:(s+1)*F]: segment 0 = own row (identity block), segment 1+t =
    sum over type-t neighbours; rows of X = graph.num_cols.  X float32 or
    bfloat16 (unit column stride, any row stride; a column-slice view is read
    in place); Z is fp32 by default, and a bfloat16 X gets a bfloat16
    gradient: the fp32 dX rounded to nearest even.  out_dtype =
    torch.bfloat16 (bfloat16 X only): Z is bfloat16 -- the fp32 Z rounded once
    -- and its bfloat16 gradient goes through grl_typed_spmm_bwd_bf16; X.grad
    is the bfloat16 dX that kernel writes (bitwise the default path's on the
    widened dZ).  Chained aggregations then pass bfloat16 tables both ways."""
    return _TypedAggregate.apply(X, graph, out_dtype)


# Row count from which the backward applies the ReLU mask to g once
# (torch.where, one elementwise pass) instead of inside the GEMM loads, so the
# two backward GEMMs qualify for libgrl's large-tile LDS-DMA path (which
# streams operands straight into LDS and cannot mask on the way).
PREMASK_ROWS = 65536


def relu_grad(g: torch.Tensor, out, want_db: bool = False):
    """(g_eff, mask_for_the_gemm, db): g through ReLU's derivative [out > 0].
    From PREMASK_ROWS rows the mask is applied here, in one pass
    (grl_relu_grad) that also sums db when asked -- bitwise the db
    linear_bwd_weight would give on g_eff; otherwise db is None and the GEMM
    (which then masks on its loads) gives it."""
    if out is None:
        return g, None, None
    if g.shape[0] < PREMASK_ROWS:
        return g, out, None
    _require_device(g, "relu_grad g")
    M, C = g.shape
    if out.shape != g.shape or not out.is_contiguous() or not g.is_contiguous():
        raise _lib.GrlError(f"relu_grad: g {tuple(g.shape)} and the ReLU output {tuple(out.shape)} "
                            "must be contiguous and of one shape")
    g_eff = torch.empty_like(g)
    db = torch.empty(C, dtype=torch.float32, device=g.device) if want_db else None
    ws_bytes = _lib.lib().grl_relu_grad_workspace_size(M, C) if want_db else 0
    ws = _workspace(ws_bytes, g.device)
    call("grl_relu_grad", g.data_ptr(), out.data_ptr(), g_eff.data_ptr(), _ptr(db), M, C, _ptr(ws), ws_bytes,
         current_stream_handle(g.device))
    return g_eff, None, db


def _rows_apart(t: torch.Tensor) -> bool:
    """Whether a 2-D tensor with unit column stride keeps its rows apart: a
    row stride of at least its width (an expanded tensor -- row stride 0, as
    autograd hands out the gradient of a sum over rows -- does not)."""
    return t.shape[0] <= 1 or t.stride(0) >= t.shape[1]


def _ld(t: torch.Tensor) -> int:
    """The row stride handed to libgrl (a single row's stride means nothing: at least the width)."""
    return max(t.stride(0), t.shape[1]) if t.shape[0] <= 1 else t.stride(0)


def relu_grad_bf16(g: torch.Tensor, out: torch.Tensor, want_db: bool = False, want_f32: bool = False):
    """(g_eff16, g_eff32, db) of a bfloat16 output gradient g through the
    ReLU's [out > 0], out the layer's bfloat16 output, in ONE pass over the
    two (grl_relu_grad_bf16): g_eff16 the selected bf16 gradient (a new
    contiguous tensor: the one-kernel data gradient's table), g_eff32 its
    contiguous fp32 copy (want_f32: what the dW GEMM reads) and db (want_db).
    Selection only, nothing is rounded: g_eff32 and db are bitwise relu_grad's
    on g.float(), out.float().  g, out: [M, C] with unit column stride and a
    row stride of at least C."""
    return _relu_grad_bf16(g, out, want_db, want_f32)


def relu_grad_bf16_scaled(g: torch.Tensor, out: torch.Tensor, scale: float, want_db: bool = False,
                          want_f32: bool = False):
    """relu_grad_bf16 with a scale (grl_relu_grad_bf16_scaled): x = out > 0 ?
    RNE_bf16(float(g) * scale) : +0 -- the backward of ReLU then feature
    dropout in one pass when `out` is the DROPPED output (> 0 exactly where the
    element was kept and the ReLU open) and scale the record's 1 / (1 - p).
    (g_eff16, g_eff32, db) as there, over x."""
    return _relu_grad_bf16(g, out, want_db, want_f32, scale=scale)


def _relu_grad_bf16(g, out, want_db, want_f32, g_eff16=None, want_16=True, scale=None):
    """relu_grad_bf16 with the C entry's other forms: `g_eff16` names the
    tensor to write (strided; g itself masks in place), want_16=False skips
    that output and `scale` takes grl_relu_grad_bf16_scaled."""
    _require_device(g, "relu_grad_bf16 g")
    tensors = [g, out] + ([g_eff16] if g_eff16 is not None else [])
    if any(t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape != g.shape or (t.shape[1] > 0 and t.stride(1) != 1)
           or not _rows_apart(t) or t.device != g.device for t in tensors):
        raise _lib.GrlError("relu_grad_bf16: g, the ReLU output and g_eff16 must be 2-D bfloat16 tensors of one "
                            "shape with unit column stride and a row stride of at least their width (an expanded "
                            "tensor: .contiguous() first)")
    M, C = g.shape
    if want_16 and g_eff16 is None:
        g_eff16 = torch.empty(M, C, dtype=torch.bfloat16, device=g.device)
    if not want_16:
        g_eff16 = None
    g_eff32 = torch.empty(M, C, dtype=torch.float32, device=g.device) if want_f32 else None
    db = torch.empty(C, dtype=torch.float32, device=g.device) if want_db else None
    ws_bytes = _lib.lib().grl_relu_grad_workspace_size(M, C) if want_db else 0
    ws = _workspace(ws_bytes, g.device)
    call("grl_relu_grad_bf16" if scale is None else "grl_relu_grad_bf16_scaled", g.data_ptr(), _ld(g), out.data_ptr(),
         _ld(out), _ptr(g_eff16), _ld(g_eff16) if g_eff16 is not None else 0, _ptr(g_eff32), _ptr(db), M, C,
         *([] if scale is None else [float(scale)]), _ptr(ws), ws_bytes, current_stream_handle(g.device))
    return g_eff16, g_eff32, db


def linear_fwd(Z2: torch.Tensor, W: torch.Tensor, b, relu: bool) -> torch.Tensor:
    M, K = Z2.shape
    C = W.shape[1]
    out = torch.empty(M, C, dtype=torch.float32, device=Z2.device)
    ws_bytes = _lib.lib().grl_linear_fwd_workspace_size(M, K, C)
    ws = _workspace(ws_bytes, Z2.device)
    call("grl_linear_fwd", Z2.data_ptr(), Z2.stride(0), W.data_ptr(), _ptr(b), out.data_ptr(), M, K, C, int(relu),
         _ptr(ws), ws_bytes, current_stream_handle(Z2.device))
    return out


def linear_bwd_data(g: torch.Tensor, relu_out, W: torch.Tensor) -> torch.Tensor:
    M, C = g.shape
    K = W.shape[0]
    dZ = torch.empty(M, K, dtype=torch.float32, device=g.device)
    ws_bytes = _lib.lib().grl_linear_bwd_data_workspace_size(M, K, C)
    ws = _workspace(ws_bytes, g.device)
    call("grl_linear_bwd_data", g.data_ptr(), _ptr(relu_out), W.data_ptr(), dZ.data_ptr(), K, M, K, C, _ptr(ws),
         ws_bytes, current_stream_handle(g.device))
    return dZ


def linear_bwd_weight(Z2: torch.Tensor, g: torch.Tensor, relu_out, want_db: bool):
    M, K = Z2.shape
    C = g.shape[1]
    dW = torch.empty(K, C, dtype=torch.float32, device=g.device)
    db = torch.empty(C, dtype=torch.float32, device=g.device) if want_db else None
    ws_bytes = _lib.lib().grl_linear_bwd_weight_workspace_size(M, K, C)
    ws = _workspace(ws_bytes, g.device)
    call("grl_linear_bwd_weight", Z2.data_ptr(), Z2.stride(0), g.data_ptr(), _ptr(relu_out), dW.data_ptr(), _ptr(db),
         M, K, C, _ptr(ws), ws_bytes, current_stream_handle(g.device))
    return dW, db


def _linear_bwd_weight_bf16_run(entry: str, Z: torch.Tensor, g16: torch.Tensor, want_db: bool):
    """The checked operands through a bf16 dW entry: its workspace query (0: None,
    before anything is allocated), dW, db and the workspace, the call.  A
    float32 g (grl_linear_bwd_weight_bf16z) is dense: that entry takes no ldg."""
    M, K = Z.shape
    C = g16.shape[1]
    g_args = (g16.data_ptr(), _ld(g16)) if g16.dtype == torch.bfloat16 else (g16.data_ptr(),)
    ws_bytes = getattr(_lib.lib(), entry + "_workspace_query")(Z.data_ptr(), _ld(Z), *g_args, M, K, C)
    if ws_bytes == 0:
        return None
    dW = torch.empty(K, C, dtype=torch.float32, device=g16.device)
    db = torch.empty(C, dtype=torch.float32, device=g16.device) if want_db else None
    ws = _workspace(ws_bytes, g16.device)
    call(entry, Z.data_ptr(), _ld(Z), *g_args, dW.data_ptr(), _ptr(db), M, K, C, _ptr(ws), ws_bytes,
         current_stream_handle(g16.device))
    return dW, db


def linear_bwd_weight_bf16(Z2: torch.Tensor, g16: torch.Tensor, want_db: bool):
    """(dW, db) = (Z2^T g16, column sums of g16) with the bfloat16 gradient read
    as stored (grl_linear_bwd_weight_bf16g: half the plane products of the
    split-bf16 dW GEMM, no widened copy), bitwise linear_bwd_weight(Z2,
    g16.float(), None, want_db) -- or None where that entry's workspace query is
    0 (below the x6 size floor, g16 off the 8 B grid, the dw_bf16g or gemm_x6
    path option 0, ...); the caller then widens g16.  Nothing is allocated
    before the query.  g16: 2-D bfloat16 with unit column stride and a row
    stride of at least its width (a column slice of a wider table is read in
    place), already through the ReLU's mask; Z2: [M, K] float32, unit column
    stride."""
    _require_device(g16, "linear_bwd_weight_bf16 g")
    if (g16.dtype != torch.bfloat16 or g16.dim() != 2 or (g16.shape[1] > 0 and g16.stride(1) != 1)
            or not _rows_apart(g16)):
        raise _lib.GrlError("linear_bwd_weight_bf16: g must be a 2-D bfloat16 tensor with unit column stride and a row "
                            "stride of at least its width (an expanded tensor: .contiguous() first)")
    if (Z2.dtype != torch.float32 or Z2.dim() != 2 or Z2.shape[0] != g16.shape[0] or Z2.device != g16.device
            or (Z2.shape[1] > 0 and Z2.stride(1) != 1) or not _rows_apart(Z2)):
        raise _lib.GrlError(f"linear_bwd_weight_bf16: Z must be a float32 [{g16.shape[0]}, K] tensor on {g16.device} "
                            "with unit column stride")
    return _linear_bwd_weight_bf16_run("grl_linear_bwd_weight_bf16g", Z2, g16, want_db)


def linear_bwd_weight_bf16z(Z16: torch.Tensor, g16: torch.Tensor, want_db: bool):
    """(dW, db) = (Z16^T g16, column sums of g16) with BOTH operands bfloat16 and
    read as stored (grl_linear_bwd_weight_bf16zg: one plane product of the
    split-bf16 dW GEMM per block, no split and no widened copy), bitwise
    linear_bwd_weight(Z16.float(), g16.float(), None, want_db) -- or None where
    that entry's workspace query is 0 (below the x6 size floor, an operand off
    the 8 B grid, the dw_bf16z or gemm_x6 path option 0, ...); the caller then
    widens Z16.  Nothing is allocated before the query.  Z16 [M, K] and g16
    [M, C]: 2-D bfloat16 with unit column stride and a row stride of at least
    their width (column slices of wider tables are read in place); g16 already
    through the ReLU's mask."""
    _require_device(g16, "linear_bwd_weight_bf16z g")
    for t, what in ((Z16, "Z"), (g16, "g")):
        if (t.dtype != torch.bfloat16 or t.dim() != 2 or (t.shape[1] > 0 and t.stride(1) != 1) or not _rows_apart(t)
                or t.device != g16.device):
            raise _lib.GrlError(f"linear_bwd_weight_bf16z: {what} must be a 2-D bfloat16 tensor on {g16.device} with "
                                "unit column stride and a row stride of at least its width (an expanded tensor: "
                                ".contiguous() first)")
    if Z16.shape[0] != g16.shape[0]:
        raise _lib.GrlError(f"linear_bwd_weight_bf16z: Z has {Z16.shape[0]} rows, g {g16.shape[0]}")
    return _linear_bwd_weight_bf16_run("grl_linear_bwd_weight_bf16zg", Z16, g16, want_db)


def linear_bwd_weight_bf16z_f32g(X16: torch.Tensor, g: torch.Tensor, want_db: bool):
    """(dW, db) = (X16^T g, column sums of g) with the bfloat16 X16 read as
    stored and g float32 (grl_linear_bwd_weight_bf16z: X16 staged as one plane
    of the split-bf16 dW GEMM, three plane products for six, no widened copy),
    bitwise linear_bwd_weight(X16.float(), g, None, want_db) -- or None where
    that entry's workspace query is 0 (below the x6 size floor, X16 off the 8 B
    grid, g off the 16 B grid, the dw_bf16z_f32g or gemm_x6 path option 0,
    ...); the caller then widens X16.  Nothing is allocated before the query.
    X16 [M, K]: 2-D bfloat16 with unit column stride and a row stride of at
    least its width (a column slice of a wider table is read in place); g
    [M, C]: float32, contiguous, already through the ReLU's mask."""
    _require_device(g, "linear_bwd_weight_bf16z_f32g g")
    if not _bf16_rows(X16) or X16.device != g.device:
        raise _lib.GrlError(f"linear_bwd_weight_bf16z_f32g: X must be a 2-D bfloat16 tensor on {g.device} with unit "
                            "column stride and a row stride of at least its width (an expanded tensor: "
                            ".contiguous() first)")
    if g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != X16.shape[0] or not g.is_contiguous():
        raise _lib.GrlError(f"linear_bwd_weight_bf16z_f32g: g must be a contiguous float32 [{X16.shape[0]}, C] tensor")
    return _linear_bwd_weight_bf16_run("grl_linear_bwd_weight_bf16z", X16, g, want_db)


class _GraphLinear(torch.autograd.Function):
    """out = Z W + b [ReLU]; backward on the same MFMA GEMM kernel with the
    ReLU mask fused into the operand loads (no g*mask temporary)."""

    @staticmethod
    def forward(ctx, Z: torch.Tensor, W: torch.Tensor, b, relu: bool, path_rows: int = 0):
        Z2 = _rows_view(Z)
        Wc = W.contiguous()
        bc = b.contiguous() if b is not None else None
        # path_rows > 0: the GEMM path chosen for that many rows (a node-range
        # shard's whole graph), so the shard's rows are the one-GPU layer's bits
        out = linear_fwd_ex(Z2, Wc, 0, bc, relu, path_rows) if path_rows > 0 else linear_fwd(Z2, Wc, bc, relu)
        ctx.relu = relu
        ctx.has_b = b is not None
        ctx.save_for_backward(Z2, Wc, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        Z2, W, out = ctx.saved_tensors
        want_b = ctx.has_b and ctx.needs_input_grad[2]
        g, mask, db_pre = relu_grad(g.contiguous().float(), out if ctx.relu else None, want_b)
        dZ = dW = db = None
        if ctx.needs_input_grad[0]:
            dZ = linear_bwd_data(g, mask, W)
        if ctx.needs_input_grad[1] or (want_b and db_pre is None):
            dW, db = linear_bwd_weight(Z2, g, mask, want_b and db_pre is None)
            if not ctx.needs_input_grad[1]:
                dW = None
        return dZ, dW, db_pre if db_pre is not None else db, None, None


# The widest dX one grl_graphconv_bwd_data call writes (the library's rule,
# grl_graphconv_bwd_data_shape_ok; tests/test_abi.py ties the two): a wider
# dX runs in column blocks, which this constant cuts.
FUSED_MAX_OUT = 512


def x6_rows_ok(M: int, N: int, K: int, path_rows: int = 0) -> bool:
    """Whether an [M, K] x [K, N] product, chosen for max(M, path_rows) rows,
    takes the split-bf16 GEMM (and so a GraphConv the one-kernel forms): the
    library's own answer (grl_linear_fwd_path).  Both GEMM paths' per-element
    arithmetic is independent of M (the fp32 one sums K in fixed chunks), so
    row blocks of one layer match the whole call bitwise when both take the
    same path -- which path_rows (the whole call's rows) guarantees."""
    return _lib.lib().grl_linear_fwd_path(int(M), int(K), int(N), int(path_rows)) != 0


def _bwd_data_eligible(g: torch.Tensor, graph, W: torch.Tensor, F: int, width: int, fresh_g: bool = False) -> bool:
    """Whether the one-kernel data gradient may take g [num_rows, C], W
    [segments * F, C] over `graph` with dX in column blocks at least `width`
    wide: the graphconv_fused_bwd option, a graph that has a typed transpose,
    operands of the layer's shapes, and the library's shape rule
    (grl_graphconv_bwd_data_shape_ok) for the transpose's rows.  Cheap: asked
    before the (cached, once per graph) transpose is built; the workspace
    query on the transpose then decides.  fresh_g (a bf16 g only): what is
    gathered is a new contiguous tensor of g's shape, so g's own strides are
    not looked at."""
    if (_lib.get_option("graphconv_fused_bwd") == 0 or isinstance(graph, EdgeBlockedGraph)
            or not graph.transpose_ok):
        return False
    M, C = g.shape
    # (an fp32 g contiguous; a bf16 g -- the bf16 entry's gradient table -- rows at least C apart)
    if g.dtype == torch.float32:
        g_ok = g.is_contiguous()
    else:
        g_ok = g.dtype == torch.bfloat16 and (fresh_g or (g.stride(1) == 1 and _rows_apart(g)))
    if (graph.num_cols < graph.num_rows or graph.self_rows != graph.num_rows or M != graph.num_rows
            or not g_ok or W.dtype != torch.float32 or tuple(W.shape) != (graph.segments * F, C)):
        return False
    # (a graph without columns -- an empty node-range shard -- launches nothing, so has no shape to refuse)
    return graph.num_cols == 0 or _lib.lib().grl_graphconv_bwd_data_shape_ok(
        graph.num_cols, graph.num_types, int(graph.has_self), C, width) != 0


def graph_conv_bwd_data(g: torch.Tensor, graph: TypedGraph, W: torch.Tensor, F: int, relu_out=None,
                        want_aggregate: bool = False, out: torch.Tensor = None):
    """dX of one GraphConv layer in one kernel (grl_graphconv_bwd_data):
    dX = sum_s (A_drop,s^T g) W_s^T over the graph's typed transpose, for g
    the output gradient ([num_rows, C]; through the ReLU's [relu_out > 0]
    when relu_out is given).  F > 512 (gcn3's 2C-wide input at C = 512) runs
    one call per <= 512-column block of dX (the gather repeats per block; dZ
    still never exists).  None when the shape is outside the one-kernel path (the caller
    then runs dZ = g W^T and the CSC gather).  The graphconv_fused_bwd path
    option 0 disables it.  want_aggregate: return (dX, G_agg, g_eff) with G_agg =
    [A_drop,s^T g_eff]_s ([num_cols, segments * C], written by the same
    kernel) and g_eff the gradient through the ReLU, for dW_s = X^T G_agg_s.
    A bfloat16 g (2-D, unit column stride, any row stride: a column slice of a
    wider table is gathered in place) takes grl_graphconv_bwd_data_bf16: the
    gather reads half the bytes and dX is returned in bfloat16, bitwise the
    fp32 dX on g.float() rounded to nearest even, G_agg (fp32) bitwise that
    call's.  None where that entry's workspace query is 0 (also: the
    graphconv_bwd_bf16 path option 0); the caller then widens g.
    out (a bfloat16 g only): the dX to write, a bfloat16 [num_cols, F] tensor
    with unit column stride and any row stride (a column-slice view is written
    in place, the columns beside it untouched; two column blocks are stored
    straight into it).  An fp32 g with an out, or a bfloat16 g with an fp32
    out, raises GrlError."""
    # A bf16 g through a ReLU: what the kernel gathers is the masked copy made below, a new contiguous
    # tensor, so the query is asked for such a tensor, not for g (whose rows it never reads) -- and before the
    # mask pass, which an ineligible call then does not run.  (An fp32 g: the query on g, as ever; its masked
    # copy is contiguous like the g the rule asks for, and as aligned as any new tensor.)
    plan = _bwd_data_plan(g, graph, W, F, out, fresh_g=relu_out is not None and g.dtype == torch.bfloat16)
    if plan is None:
        return None
    if relu_out is not None:  # (exact on bf16 too: a selection)
        g = torch.where(relu_out > 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
    return _bwd_data_run(plan, g, graph, W, F, want_aggregate)


# What a workspace query is asked for a tensor that does not exist yet: torch's device allocator hands out
# blocks aligned to 512 B, which every alignment rule of the library divides, and a new [R, W] tensor's row
# stride is W.  (_bwd_data_run's launch would refuse, not misread, a tensor that broke this.)
_FRESH_ADDRESS = 512


def _bwd_data_plan(g: torch.Tensor, graph, W: torch.Tensor, F: int, out: torch.Tensor = None, fresh_g: bool = False):
    """What graph_conv_bwd_data launches for these operands -- (csr, eid,
    column bounds, workspace bytes, out) -- or None outside the one-kernel
    path.  No device memory is allocated: the workspace query that decides
    looks at addresses and row strides only, so a dX that _bwd_data_run will
    allocate (out None) is asked as a new tensor, and so is a bf16 g with
    fresh_g -- the caller launches on a new contiguous [num_rows, C] tensor it
    makes once the plan stands (the masked gradient), not on g."""
    if g.dim() != 2:
        raise _lib.GrlError(f"graph_conv_bwd_data: g must be 2-D (got {tuple(g.shape)})")
    bf16 = g.dtype == torch.bfloat16
    rows = graph.num_cols  # dX rows: every column of the graph (a shard's halo rows get partials)
    if out is not None:
        if out.dtype != g.dtype or not bf16:
            raise _lib.GrlError(f"graph_conv_bwd_data: g is {g.dtype} and out {out.dtype}: out= is a bfloat16 dX "
                                "for a bfloat16 g (there is no mixed form; an fp32 g returns a new fp32 dX)")
        if (tuple(out.shape) != (rows, F) or out.device != g.device or (F > 0 and out.stride(1) != 1)
                or not _rows_apart(out)):
            raise _lib.GrlError(f"graph_conv_bwd_data: out must be a bfloat16 {(rows, F)} tensor on {g.device} "
                                "with unit column stride and a row stride of at least F")
    M, C = g.shape
    nblk = -(-F // FUSED_MAX_OUT)
    wblk = (-(-F // nblk) + 3) // 4 * 4 if nblk > 1 else F  # block width, a multiple of 4
    bounds = [(f0, min(F, f0 + wblk)) for f0 in range(0, F, wblk)]
    if nblk > 2 or not _bwd_data_eligible(g, graph, W, F, min(b - a for a, b in bounds),
                                          fresh_g=fresh_g and bf16):  # (at most two blocks)
        return None
    gt, eid = graph.typed_transpose()
    gt = gt.with_dropedge(graph.dropedge)
    csr = gt.csr_c(C)
    if not bf16:
        ws_bytes = _lib.lib().grl_graphconv_bwd_data_workspace_query(ctypes.byref(csr), g.data_ptr(), g.stride(0), C,
                                                                     W.data_ptr(), bounds[0][1])
        return (csr, eid, bounds, ws_bytes, None) if ws_bytes else None
    g_at, ldg = (_FRESH_ADDRESS, C) if fresh_g else (g.data_ptr(), _ld(g))
    dx_at, lddx = (_FRESH_ADDRESS, F) if out is None else (out.data_ptr(), _ld(out))
    sizes = [_lib.lib().grl_graphconv_bwd_data_bf16_workspace_query(
        ctypes.byref(csr), g_at, ldg, C, W.data_ptr(), f1 - f0, dx_at + 2 * f0, lddx) for f0, f1 in bounds]
    return (csr, eid, bounds, max(sizes), out) if min(sizes) else None


def _bwd_data_run(plan, g: torch.Tensor, graph, W: torch.Tensor, F: int, want_aggregate: bool = False):
    """The launches of a _bwd_data_plan for g (the gradient through the ReLU;
    where the plan was asked with fresh_g, the new contiguous tensor)."""
    csr, eid, bounds, ws_bytes, dX = plan
    M, C = g.shape
    S = graph.segments
    bf16 = g.dtype == torch.bfloat16
    rows = graph.num_cols
    if dX is None:
        dX = torch.empty(rows, F, dtype=g.dtype, device=g.device)
    ws = _workspace(ws_bytes, g.device)
    stream = current_stream_handle(g.device)
    G_agg = torch.empty(rows, S * C, dtype=torch.float32, device=g.device) if want_aggregate else None
    for i, (f0, f1) in enumerate(bounds):
        w = f1 - f0
        Wb = W.contiguous() if len(bounds) == 1 else W.reshape(S, F, C)[:, f0:f1, :].reshape(S * w, C).contiguous()
        if bf16:  # strided stores: a column block goes straight into dX[:, f0:f1]
            call("grl_graphconv_bwd_data_bf16", ctypes.byref(csr), eid.data_ptr(), g.data_ptr(), _ld(g), M, C,
                 Wb.data_ptr(), w, dX.data_ptr() + 2 * f0, _ld(dX), _ptr(G_agg) if i == 0 else None,
                 _de_ref(graph), ws.data_ptr(), ws_bytes, stream)
            continue
        out = dX if len(bounds) == 1 else torch.empty(rows, w, dtype=torch.float32, device=g.device)
        call("grl_graphconv_bwd_data", ctypes.byref(csr), eid.data_ptr(), g.data_ptr(), g.stride(0), M, C,
             Wb.data_ptr(), w, out.data_ptr(), _ptr(G_agg) if i == 0 else None, _de_ref(graph), ws.data_ptr(),
             ws_bytes, stream)
        if len(bounds) > 1:
            dX[:, f0:f1] = out
    return (dX, G_agg, g) if want_aggregate else dX


def _transpose_rows_view(gt: TypedGraph, r0: int, r1: int, dropedge) -> TypedGraph:
    """Rows [r0, r1) of the typed transpose as a TypedGraph (rowptr a slice,
    colidx / vals / eid shared), cached on the transpose so its split plan is
    built once per graph, not once per backward."""
    cache = gt._shared.setdefault("row_views", {})
    v = cache.get((r0, r1))
    if v is None:
        L = gt.num_types
        v = TypedGraph(gt.rowptr[r0 * L: r1 * L + 1], gt.colidx, L, vals=gt.vals, has_self=gt.has_self,
                       num_cols=gt.num_cols, edge_id_base=gt.edge_id_base, self_id_base=gt.self_id_base,
                       self_rows=r1 - r0)
        v.split_threshold, v.split_chunk = gt.split_threshold, gt.split_chunk
        cache[(r0, r1)] = v
    return v.with_dropedge(dropedge)


def graph_conv_bwd_data_rows_views(g: torch.Tensor, graph: TypedGraph, W: torch.Tensor, F: int, blocks):
    """The per-block launch data of graph_conv_bwd_data_rows -- [(view, csr,
    workspace bytes) or None for an empty block] -- or None when some block
    is outside the one-kernel path.  No device work beyond the cached
    transpose and split plans: a caller that must decide collectively
    (grl.dist rows_backward) asks this first, agrees, then launches."""
    if g.dtype != torch.float32 or not _bwd_data_eligible(g, graph, W, F, F):  # (row blocks: the fp32 entry only)
        return None
    C = g.shape[1]
    for r0, r1 in blocks:
        if not (r0 == 0 or r0 >= graph.num_rows) or r1 < r0 or r1 > graph.num_cols:
            raise _lib.GrlError(f"row block [{r0}, {r1}) must start at 0 or at/after row {graph.num_rows}")
    gt, eid = graph.typed_transpose()
    Wc = W.contiguous()
    views = []
    for r0, r1 in blocks:
        if r1 == r0:
            views.append(None)
            continue
        v = _transpose_rows_view(gt, r0, r1, graph.dropedge)
        csr = v.csr_c(C)
        ws_bytes = _lib.lib().grl_graphconv_bwd_data_workspace_query(ctypes.byref(csr), g.data_ptr(), g.stride(0),
                                                                     C, Wc.data_ptr(), F)
        if ws_bytes == 0:
            return None
        views.append((v, csr, ws_bytes))
    return views


def graph_conv_bwd_data_rows(g: torch.Tensor, graph: TypedGraph, W: torch.Tensor, F: int, blocks, dX: torch.Tensor,
                             on_block=None, views=None) -> bool:
    """The one-kernel data gradient (graph_conv_bwd_data) computed in row
    blocks of dX, one grl_graphconv_bwd_data call per block [r0, r1) over a
    row-range view of the cached typed transpose, so a caller can act on a
    block (e.g. send a node-range shard's halo rows home) while the next one
    computes.  Every row is the same arithmetic as in the whole-range call
    (rows do not mix in the kernel), so dX is bitwise that call's.  A block
    starting at row 0 carries the self term of rows < graph.num_rows; other
    blocks must lie at or beyond num_rows (a shard's halo rows: no self term).
    g: the output gradient already through the ReLU.  dX: [graph.num_cols, F]
    (written).  on_block(r0, r1) runs after each block's launch.  views:
    graph_conv_bwd_data_rows_views' result for these arguments (else it is
    computed here).  False (and nothing written) when some block is outside
    the one-kernel path; the caller then takes the whole-range path."""
    if views is None:
        views = graph_conv_bwd_data_rows_views(g, graph, W, F, blocks)
    if views is None or tuple(dX.shape) != (graph.num_cols, F) or not dX.is_contiguous():
        return False
    gt, eid = graph.typed_transpose()
    Wc = W.contiguous()
    M, C = g.shape
    stream = current_stream_handle(g.device)
    ws = None
    for (r0, r1), view in zip(blocks, views):
        if view is not None:
            v, csr, ws_bytes = view
            if ws is None or ws.numel() < ws_bytes:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device)
            g_rows = M if r0 == 0 else 0  # the self term: forward rows only
            call("grl_graphconv_bwd_data", ctypes.byref(csr), eid.data_ptr(), g.data_ptr(), g.stride(0),
                 min(g_rows, r1 - r0), C, Wc.data_ptr(), F, dX[r0:r1].data_ptr(), None, _de_ref(graph),
                 ws.data_ptr(), ws_bytes, stream)
        if on_block is not None:
            on_block(r0, r1)
    return True


class _GraphConv(torch.autograd.Function):
    """One GraphConv layer, X -> Z = A_drop X -> out = Z W + b [ReLU]
    (robust_gcn.py:45-51), as one autograd node: the same kernels and
    results as typed_aggregate + graph_linear.  X float32 or bfloat16 (the
    bf16-table forward entries; the backward is the fp32 layer's on the fp32
    Z and output gradient, dX rounded once to X's dtype -- and with a bf16
    output gradient too, where grl_graphconv_bwd_data_bf16 applies, the data
    gradient gathers that gradient as stored and writes the bf16 dX itself,
    the same bits with no widened copy: _backward_bf16).  fdrop (with a ReLU
    and a bf16 output): the feature dropout that follows the layer, applied
    in place to the output in the forward and as one scaled mask pass over the
    saved dropped output in the backward (graph_conv).  (Running dW on a second HIP
    stream beside dZ / the transposed gather was measured and bought nothing:
    39-41 ms per C3 layer either way, each kernel already fills the chip.)"""

    @staticmethod
    def forward(ctx, X: torch.Tensor, graph: TypedGraph, W: torch.Tensor, b, relu: bool, recompute: bool,
                out_bf16: bool = False, fdrop=None, row0: int = 0, z_bf16: bool = False):
        Wc = W.contiguous()
        bc = b.contiguous() if b is not None else None
        # out_bf16 (a bf16 X on a TypedGraph: graph_conv checks): the layer's epilogue writes bf16
        out = torch.empty(graph.num_rows, Wc.shape[1], dtype=torch.bfloat16, device=X.device) if out_bf16 else None
        if isinstance(graph, EdgeBlockedGraph):
            Z = spmm_forward(X, graph)
            out = linear_fwd(Z, Wc, bc, relu)
        elif recompute:  # Z is not kept: the one-kernel inference form (Z stays on chip)
            Z = None
            out = graph_conv_infer(X, graph, Wc, bc, relu, out=out)
        else:  # one kernel that also writes Z where it applies (grl_graphconv_fwd_train)
            # z_bf16 (out_bf16 on a TypedGraph: graph_conv checks): the saved Z holds bf16 too, half the bytes
            out, Z = graph_conv_fwd_train(X, graph, Wc, bc, relu, out=out,
                                          z_dtype=torch.bfloat16 if z_bf16 else None)
        ctx.graph, ctx.relu, ctx.has_b, ctx.xshape, ctx.xdtype = graph, relu, b is not None, X.shape, X.dtype
        ctx.recompute = recompute
        ctx.z16 = Z is not None and Z.dtype == torch.bfloat16  # (never with recompute: X is what is kept)
        # fdrop (relu and out_bf16: graph_conv checks): the feature dropout in place on the fresh bf16 output, which
        # is then the one tensor returned and saved -- > 0 exactly where kept and open, so the backward needs the
        # record's scale alone (grl_relu_grad_bf16_scaled), no hash and no pre-dropout copy
        ctx.fscale = None
        if fdrop is not None:
            feature_dropout_apply(out, fdrop, row0, out=out)
            ctx.fscale = float(fdrop.to_c().scale)
        # recompute: keep X (F wide) instead of Z ((L+1)F wide); the backward
        # regenerates Z with the same DropEdge record, so it is the same bits
        ctx.save_for_backward(X if recompute else Z, Wc, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        Z, W, out = ctx.saved_tensors
        want_w = ctx.needs_input_grad[2]
        want_b = ctx.has_b and ctx.needs_input_grad[3]
        if (g.dtype == torch.bfloat16 and ctx.xdtype == torch.bfloat16 and ctx.needs_input_grad[0]
                and not isinstance(ctx.graph, EdgeBlockedGraph)):
            res = _GraphConv._backward_bf16(ctx, g, Z, W, out, want_w, want_b)
            if res is not None:
                return res
        if ctx.z16:  # a bf16 saved Z on the widened path: widened once, exactly; the fp32 layer's backward on it
            Z = Z.float()
        if ctx.fscale is not None:
            # the fused dropout where the bf16 data gradient does not apply: the masked, scaled bf16 gradient
            # first (one pass over g and the dropped output), then the widened path on it -- whose own mask
            # [out > 0] selects what is already selected
            g2 = g.reshape(-1, g.shape[-1])
            if not (g2.stride(1) == 1 and _rows_apart(g2)):
                g2 = g2.contiguous()
            g = _relu_grad_bf16(g2, out, False, False, scale=ctx.fscale)[0]
        # a bf16 out hands back a bf16 g: the fp32 layer's backward on g.float(), the ReLU mask from the bf16
        # out ([out > 0] survives the rounding); both widened to fp32 here
        g, mask, db_pre = relu_grad(g.contiguous().float(), out.float() if ctx.relu else None, want_b)
        if ctx.recompute and ctx.needs_input_grad[0] and want_w and ctx.xdtype == torch.float32:
            # X was kept, not Z: the one-kernel data gradient also writes G_s = A_drop,s^T g and
            # dW_s = Z_s^T g = X^T G_s -- no re-aggregation of Z (same products, another order).
            # (X^T G_s is an fp32 GEMM: a bf16 X re-aggregates Z below instead of being widened.)
            res = graph_conv_bwd_data(g, ctx.graph, W, ctx.xshape[-1], mask, want_aggregate=True)
            if res is not None:
                dX, G_agg, g_eff = res
                X2 = _rows_view(Z)
                S, F, C = ctx.graph.segments, X2.shape[1], g.shape[1]
                dWt, _ = linear_bwd_weight(X2, G_agg, None, False)  # [F, S*C]
                del G_agg
                dW = dWt.view(F, S, C).transpose(0, 1).reshape(S * F, C)
                db = (db_pre if db_pre is not None else g_eff.sum(0)) if want_b else None
                return dX.view(ctx.xshape), None, dW, db, None, None, None, None, None, None
        if ctx.recompute and (want_w or (want_b and db_pre is None)):
            Z = spmm_forward(Z, ctx.graph)
        dW = db = dX = None
        if ctx.needs_input_grad[0]:
            F = ctx.xshape[-1]
            dX = graph_conv_bwd_data(g, ctx.graph, W, F, mask)  # one kernel, no dZ (large graphs)
            if dX is None:
                dZ = linear_bwd_data(g, mask, W)
                dX = spmm_backward(dZ, ctx.graph, F)
                del dZ
            dX = dX.view(ctx.xshape).to(ctx.xdtype)  # a bf16 X: the fp32 dX rounded once
        if want_w or (want_b and db_pre is None):
            dW, db = linear_bwd_weight(Z, g, mask, want_b and db_pre is None)
        if db_pre is not None:
            db = db_pre
        return dX, None, dW if want_w else None, db, None, None, None, None, None, None

    @staticmethod
    def _backward_bf16(ctx, g: torch.Tensor, Z, W: torch.Tensor, out, want_w: bool, want_b: bool):
        """The backward of a bf16 X under a bf16 output gradient where
        grl_graphconv_bwd_data_bf16 applies (else None, and backward runs the
        widened path): the data gradient gathers the bf16 gradient as stored and
        writes the bf16 dX, so g.float(), out.float() and an fp32 [N, F] dX
        never exist.  From PREMASK_ROWS rows one grl_relu_grad_bf16 pass makes
        the masked bf16 gradient, db, and -- only when dW wants it -- the fp32
        g_eff the dW GEMM reads.  Where grl_linear_bwd_weight_bf16g applies
        (linear_bwd_weight_bf16; from PREMASK_ROWS rows, or without a ReLU) dW
        reads the masked bf16 gradient too, and no fp32 [N, C] tensor is made
        at all.  Every gradient is bitwise the widened path's."""
        graph, F = ctx.graph, ctx.xshape[-1]
        g2 = g.reshape(-1, g.shape[-1])
        M, C = g2.shape
        relu = ctx.relu
        premask = relu and M >= PREMASK_ROWS
        # With a ReLU the kernel gathers the masked gradient, a new contiguous tensor made once the plan
        # stands; without one it gathers g as handed over, unless autograd handed over an expanded gradient
        # (row stride 0: the gradient of a sum over nodes) or one without unit column stride, which is copied.
        as_is = not relu and g2.stride(1) == 1 and _rows_apart(g2)
        plan = _bwd_data_plan(g2, graph, W, F, fresh_g=not as_is)
        if plan is None:
            return None
        if not (g2.stride(1) == 1 and _rows_apart(g2)):
            g2 = g2.contiguous()
        # dW from the masked bf16 gradient the dX kernel gathers (grl_linear_bwd_weight_bf16g), where the widened
        # path's dW is the split-bf16 GEMM on an unmasked operand -- its bits, then, with no fp32 copy of g.  Not
        # below PREMASK_ROWS with a ReLU: there the widened path's GEMM masks on its loads in the fp32-MFMA
        # kernel, other bits.  Asked before the mask pass (which then skips its fp32 output) for the tensors as
        # they will be: the masked gradient and a recomputed Z are new contiguous tensors.
        # A bf16 saved Z (ctx.z16): the bf16zg query is asked where the bf16g query is, and where it answers, dW is
        # ONE plane product on the two tables as stored (linear_bwd_weight_bf16z); where it does not, Z is widened
        # once (exactly) and the code below runs on it as on an fp32 saved Z.
        gemm = want_w or (want_b and not premask)
        dw16 = dwz = False
        if gemm and (premask or not relu):
            K = graph.segments * F
            g_at, ldg = (_FRESH_ADDRESS, C) if premask else (g2.data_ptr(), _ld(g2))
            if ctx.z16:
                dwz = _lib.lib().grl_linear_bwd_weight_bf16zg_workspace_query(Z.data_ptr(), _ld(Z), g_at, ldg, M, K,
                                                                              C) != 0
            if not dwz:
                z_at, ldz = (_FRESH_ADDRESS, K) if ctx.recompute or ctx.z16 else (Z.data_ptr(), _ld(Z))
                dw16 = _lib.lib().grl_linear_bwd_weight_bf16g_workspace_query(z_at, ldz, g_at, ldg, M, K, C) != 0
        g32 = mask = db_pre = None
        if premask:
            g16, g32, db_pre = _relu_grad_bf16(g2, out, want_b, want_w and not (dw16 or dwz), scale=ctx.fscale)
        elif ctx.fscale is not None:
            # the fused dropout below PREMASK_ROWS: the scaled pass still makes the gradient (masked by the dropped
            # output, scaled, rounded once) and its fp32 copy for the dW GEMM, which keeps masking on its loads
            # with the dropped output -- it selects the same values as the unfused chain's, so the same bits
            g16, g32, _ = _relu_grad_bf16(g2, out, False, gemm, scale=ctx.fscale)
        else:
            g16 = torch.where(out > 0, g2, torch.zeros((), dtype=g2.dtype, device=g.device)) if relu else g2
        dX = _bwd_data_run(plan, g16, graph, W, F).view(ctx.xshape)
        if not (dw16 or dwz):
            del g16
        dW = db = None
        if gemm:
            if ctx.recompute:
                Z = spmm_forward(Z, graph)
            res = None
            if dwz:
                res = linear_bwd_weight_bf16z(Z, g16, want_b and db_pre is None)
            if ctx.z16 and res is None:
                Z = Z.float()
            if dwz:
                if res is None:  # (the tensors are not as asked for: both widened, the same values)
                    g32 = g16.float().contiguous()
                del g16
            elif dw16:
                res = linear_bwd_weight_bf16(Z, g16, want_b and db_pre is None)
                if res is None:  # (the tensors are not as asked for: the masked gradient widened, the same values)
                    g32 = g16.float().contiguous()
                del g16
            elif not premask:  # the dW GEMM reads fp32 (and masks on its loads below PREMASK_ROWS)
                g32 = g2.float().contiguous() if ctx.fscale is None else g32
                mask = out.float() if relu else None
            dW, db = res if res is not None else linear_bwd_weight(Z, g32, mask, want_b and db_pre is None)
        if db_pre is not None:
            db = db_pre
        return dX, None, dW if want_w else None, db, None, None, None, None, None, None


def graph_conv_fwd_train(X: torch.Tensor, graph: TypedGraph, W: torch.Tensor, b=None, relu: bool = False,
                         out: torch.Tensor = None, Z: torch.Tensor = None, z_dtype=None):
    """(out, Z) of one GraphConv layer through grl_graphconv_fwd_train: the
    one-kernel path writes Z as a by-product (for the backward's dW); the
    result is bitwise spmm_forward then linear_fwd.  out / Z: contiguous
    [num_rows, C] / [num_rows, segments * F] fp32 tensors to write (e.g. the
    row block of a streamed layer).  X float32, or bfloat16 read as stored
    (grl_graphconv_fwd_train_bf16): out and Z bitwise the call's on X.float().
    With a bfloat16 X, out may be bfloat16 (_forward_args; a column-slice view
    is written in place, grl_graphconv_fwd_train_bf16_to_bf16): the fp32 out
    rounded to nearest even in the kernel's epilogue, Z fp32 as before.
    z_dtype=torch.bfloat16, or a bfloat16 Z passed in (a bfloat16 X and a
    bfloat16 out only; Z contiguous [num_rows, segments * F]): Z holds bf16 as
    well (grl_graphconv_fwd_train_bf16_z16), bitwise the fp32 Z rounded to
    nearest even -- half the bytes kept for the backward, which
    linear_bwd_weight_bf16z reads as stored; out is bitwise the fp32-Z call's."""
    who = "graph_conv_fwd_train"
    if z_dtype not in (None, torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"{who}: z_dtype must be None, float32 or bfloat16 (got {z_dtype})")
    if z_dtype == torch.bfloat16 or (Z is not None and Z.dtype == torch.bfloat16):
        if z_dtype == torch.float32:
            raise _lib.GrlError(f"{who}: z_dtype=float32 with a bfloat16 Z")
        return _graph_conv_fwd_train_z16(who, X, graph, W, b, relu, out, Z)
    X2, F, Wc, bc, out, Z = _forward_args(who, X, graph, W, b, out, Z, want_Z=True)
    K, C = Wc.shape
    csr = graph.csr_c(F)
    ws_bytes = _lib.lib().grl_linear_fwd_ex_workspace_size(graph.num_rows, K, C, graph.path_rows)
    if out.dtype == torch.bfloat16:
        full = _lib.lib().grl_graphconv_fwd_bf16_to_bf16_workspace_query(
            ctypes.byref(csr), X2.data_ptr(), X2.stride(0), F, Wc.data_ptr(), C, out.data_ptr(), out.stride(0))
        if full >= graph.num_rows * K * 4 or Z.data_ptr() % 16:  # two kernels: the linear's fp32 [num_rows, C]
            ws_bytes += (graph.num_rows * C * 4 + 255) // 256 * 256
    _graphconv_fwd_call("grl_graphconv_fwd_train" + _bf16_suffix(X2, out), csr, X2, F, Wc, bc, relu, out, Z, graph,
                        ws_bytes)
    return out, Z


def _graph_conv_fwd_train_z16(who: str, X, graph, W, b, relu: bool, out, Z):
    """graph_conv_fwd_train with a bfloat16 Z (grl_graphconv_fwd_train_bf16_z16):
    a bfloat16 X and a bfloat16 out (given, or a new contiguous one) on a
    TypedGraph; Z the contiguous bfloat16 [num_rows, segments * F] tensor given
    or a new one.  The workspace is the entry's own query: W's planes for the
    one kernel, else the fp32 Z scratch, the linear's fp32 output and its
    workspace."""
    if isinstance(graph, EdgeBlockedGraph):
        raise _lib.GrlError(f"{who}: a bfloat16 Z needs a TypedGraph (an EdgeBlockedGraph aggregates by blocks, in fp32)")
    if X.dtype != torch.bfloat16:
        raise _lib.GrlError(f"{who}: a bfloat16 Z needs bfloat16 node features (got {X.dtype}): there is no fp32-table "
                            "form with a bf16 Z -- cast the table once")
    if out is not None and out.dtype != torch.bfloat16:
        raise _lib.GrlError(f"{who}: a bfloat16 Z needs a bfloat16 out (got {out.dtype}): the fp32-output entries keep "
                            "an fp32 Z, whose gradient is fp32 too")
    if out is None:
        out = torch.empty(graph.num_rows, W.shape[1], dtype=torch.bfloat16, device=X.device)
    X2, F, Wc, bc, out, _ = _forward_args(who, X, graph, W, b, out)
    K, C = Wc.shape
    if Z is None:
        Z = torch.empty(graph.num_rows, K, dtype=torch.bfloat16, device=X.device)
    elif (tuple(Z.shape) != (graph.num_rows, K) or Z.dtype != torch.bfloat16 or not Z.is_contiguous()
          or Z.device != X.device):
        raise _lib.GrlError(f"{who}: Z must be a contiguous bfloat16 {(graph.num_rows, K)} tensor on {X.device}")
    csr = graph.csr_c(F)
    ws_bytes = _lib.lib().grl_graphconv_fwd_train_bf16_z16_workspace_query(
        ctypes.byref(csr), X2.data_ptr(), X2.stride(0), F, Wc.data_ptr(), C, out.data_ptr(), out.stride(0),
        Z.data_ptr())
    _graphconv_fwd_call("grl_graphconv_fwd_train_bf16_z16", csr, X2, F, Wc, bc, relu, out, Z, graph, ws_bytes)
    return out, Z


def graph_conv_infer(X: torch.Tensor, graph: TypedGraph, W: torch.Tensor, b=None, relu: bool = False,
                     max_workspace_bytes: int = None, out: torch.Tensor = None) -> torch.Tensor:
    """GraphConv forward for inference through one grl_graphconv_fwd call
    (aggregation + linear [+ReLU]).  On large graphs this is one fused kernel
    and Z never reaches HBM; otherwise Z lives only in the call's workspace
    and max_workspace_bytes bounds it (the call then works in row chunks,
    bitwise equal to the whole-graph result).  out: a contiguous
    [num_rows, C] float32 tensor to write (e.g. a row block of a halo table).
    X float32, or bfloat16 read as stored (grl_graphconv_fwd_bf16: out bitwise
    the call's on X.float(); one kernel where X is 8 B-aligned with a row
    stride that is a multiple of 4, else Z whole in the workspace -- the bf16
    entry has no row-chunked form, so a max_workspace_bytes below that raises).
    With a bfloat16 X, out may be bfloat16 with any row stride, e.g. a column
    slice of the next layer's table (grl_graphconv_fwd_bf16_to_bf16): bitwise
    the fp32 out rounded to nearest even, written by the kernel's epilogue --
    one kernel where, besides, out is 4 B-aligned with an even row stride."""
    X2, F, Wc, bc, out, _ = _forward_args("graph_conv_infer", X, graph, W, b, out)
    C = Wc.shape[1]
    csr = graph.csr_c(F)
    sfx = _bf16_suffix(X2, out)
    out_args = [out.data_ptr(), out.stride(0)] if out.dtype == torch.bfloat16 else []
    # the fused one-kernel path needs only W's planes; else Z whole (the bf16-out rule also looks at out's rows)
    query = getattr(_lib.lib(), f"grl_graphconv_fwd{sfx}_workspace_query")
    full = query(ctypes.byref(csr), X2.data_ptr(), X2.stride(0), F, Wc.data_ptr(), C, *out_args)
    ws_bytes = full if max_workspace_bytes is None else min(full, int(max_workspace_bytes))
    _graphconv_fwd_call("grl_graphconv_fwd" + sfx, csr, X2, F, Wc, bc, relu, out, None, graph, ws_bytes)
    return out


# Z bytes above which a training GraphConv keeps X and recomputes Z in the
# backward instead of holding Z between the passes (recompute=None): at C5
# scale (2^23 nodes, d=512) Z is 120 GB per layer, X 17 GB.  (The one-kernel
# backward's transient G_agg is Z-sized when C == F: recompute bounds the
# memory held between the passes, not the backward's peak -- graph_conv.)
RECOMPUTE_Z_BYTES = 8 << 30


def graph_conv(X: torch.Tensor, graph: TypedGraph, W: torch.Tensor, b=None, relu: bool = False,
               recompute: bool = None, out_dtype=None, fdrop=None, row0: int = 0, z_dtype=None) -> torch.Tensor:
    """GraphConv forward (aggregation + linear [+ReLU]) as one autograd node;
    X: [num_cols, F] (or [B, N, F] for a batch graph).  When no gradient is
    wanted (eval, torch.no_grad) it is one grl_graphconv_fwd call instead:
    the same kernels, so the same bits.
    recompute: True keeps X instead of Z between the passes ((L+1)x less
    saved memory); None decides by Z's size (RECOMPUTE_Z_BYTES).  Where the
    one-kernel data gradient applies (grl_graphconv_bwd_data), the backward
    takes dW_s = X^T G_s from the aggregate G_s = A_drop,s^T g it writes:
    out and dX are bitwise the saved-Z path's, dW / db the same products
    summed in another order (fp32 rounding level).  Elsewhere Z is
    re-aggregated (one more SpMM pass) and every gradient is bitwise the
    saved-Z path's.  Peak memory in the G_s form: the transient G_agg
    [num_cols, (L+1) C] of the backward is Z-sized when C == F, so recompute
    lowers the memory held BETWEEN the passes, not the backward's peak.
    A bfloat16 X (fp32 W, b) is the same one autograd node on the bf16-table
    entries (grl_graphconv_fwd_bf16, _fwd_train_bf16: the one-kernel layer
    gathering half the bytes; no widened copy of X is made).  out is bitwise
    the layer's on X.float(); the backward is that layer's on the fp32 Z and
    output gradient, so dW and db are those of its saved-Z path and X.grad is
    its dX rounded once to bfloat16.  With recompute=True the bf16 X is what
    is kept, and the backward re-aggregates Z from it (the bf16 SpMM, the
    same bits): it does not take the dW_s = X^T G_s form, which needs an
    fp32 X, so dW and db stay bitwise the saved-Z path's.
    out_dtype=torch.bfloat16 (a bfloat16 X on a TypedGraph only; None and
    torch.float32: the fp32 output as ever): a new contiguous bfloat16 tensor
    written by the kernel's epilogue (grl_graphconv_fwd[_train]_bf16_to_bf16),
    bitwise the fp32 output rounded to nearest even, from the same one
    autograd node.  Autograd then hands the node a bfloat16 output gradient.
    Where the one-kernel data gradient takes it as stored
    (grl_graphconv_bwd_data_bf16: a nonzero workspace query, the
    graphconv_bwd_bf16 path option on) the backward gathers the bf16 gradient
    rows -- half the bytes -- and writes the bf16 X.grad from the kernel's
    epilogue; from PREMASK_ROWS rows one pass (grl_relu_grad_bf16) applies the
    ReLU mask of the bfloat16 output and sums db, and dW reads the masked
    bfloat16 gradient as stored (grl_linear_bwd_weight_bf16g: a nonzero
    workspace query, the dw_bf16g path option on; elsewhere the pass also makes
    the fp32 gradient the dW GEMM reads).  No g.float(), out.float() or fp32
    [N, F] dX exists there.  Elsewhere the backward is the fp32 layer's on
    g.float() with the ReLU mask taken from the bfloat16 output, dX rounded
    once as above.  X.grad, dW and db are the same bits either way.
    recompute=True keeps the bf16 X and re-aggregates Z, as above.
    fdrop (a DropEdge record, as FeatureDropout.record() returns; row0 the
    global row of the first output row): the feature dropout that follows the
    layer, feature_dropout(out, fdrop, row0).  With relu=True and
    out_dtype=torch.bfloat16 it is fused into the node: the forward runs
    grl_feature_dropout_bf16 IN PLACE on the layer's fresh bfloat16 output and
    returns and saves that one tensor (no pre-dropout copy is kept), and the
    backward makes the masked, scaled bfloat16 gradient in one
    grl_relu_grad_bf16_scaled pass at every row count (the dropped output is
    > 0 exactly where the element was kept and the ReLU open, so one selection
    is both masks and no hash is drawn); below PREMASK_ROWS the dW GEMM stays
    the one that masks on its loads, reading that gradient widened with the
    dropped output as its mask.  out, X.grad, dW and db are bitwise those of
    the unfused chain feature_dropout(graph_conv(...), fdrop, row0).  With
    gradients disabled it is graph_conv_infer followed by the in-place pass.
    In every other combination (an fp32 output, no ReLU, an EdgeBlockedGraph)
    fdrop is applied as a separate feature_dropout after the node.
    z_dtype=torch.bfloat16 (with out_dtype=torch.bfloat16 on a TypedGraph only;
    None and torch.float32: the fp32 Z as ever): the Z kept between the passes
    holds bf16 (grl_graphconv_fwd_train_bf16_z16: the fp32 Z rounded to nearest
    even as it is written), half the bytes -- the saved-activation precision
    of mixed-precision training.  out, X.grad and db are bitwise those of
    z_dtype=None (the multiply consumes the unrounded Z, and neither the data
    gradient nor db reads Z); dW alone sees the rounded Z: where
    grl_linear_bwd_weight_bf16zg applies (from PREMASK_ROWS rows or without a
    ReLU; a nonzero workspace query, the dw_bf16z path option on) it is one
    plane product on the two bf16 tables as stored, elsewhere Z is widened once
    and the backward above runs on it -- the same dW bits either way where a
    split-bf16 kernel runs.  recompute=None counts the bytes Z would take, 2 an
    element; with recompute=True z_dtype has no effect (X is what is kept, and
    the backward re-aggregates an fp32 Z).  Ignored when no gradient is wanted."""
    if X.dtype not in _TABLE_DTYPES:
        raise _lib.GrlError(f"graph_conv: node features must be float32 or bfloat16 (got {X.dtype})")
    if W.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise _lib.GrlError("graph_conv: weights and bias must be float32")
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"graph_conv: out_dtype must be None, float32 or bfloat16 (got {out_dtype})")
    out_bf16 = out_dtype == torch.bfloat16
    if out_bf16 and (X.dtype != torch.bfloat16 or isinstance(graph, EdgeBlockedGraph)):
        raise _lib.GrlError(f"graph_conv: out_dtype=bfloat16 needs bfloat16 node features on a TypedGraph (got "
                            f"{X.dtype}): there is no fp32-table form with a bf16 output -- cast the table once")
    if z_dtype not in (None, torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"graph_conv: z_dtype must be None, float32 or bfloat16 (got {z_dtype})")
    z_bf16 = z_dtype == torch.bfloat16
    if z_bf16 and not out_bf16:
        raise _lib.GrlError("graph_conv: z_dtype=bfloat16 needs out_dtype=bfloat16 (bfloat16 node features on a "
                            "TypedGraph): the fp32-output layer keeps an fp32 Z")
    fused = fdrop is not None and relu and out_bf16
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (X, W, b))):
        if isinstance(graph, EdgeBlockedGraph):  # one int32 CSR per call: aggregate by blocks, then the linear
            out = linear_fwd(spmm_forward(X, graph), W.contiguous(), b.contiguous() if b is not None else None, relu)
        else:
            out = torch.empty(graph.num_rows, W.shape[1], dtype=torch.bfloat16, device=X.device) if out_bf16 else None
            out = graph_conv_infer(X, graph, W, b, relu, out=out)
        if fused:
            return feature_dropout_apply(out, fdrop, int(row0), out=out)
        return out if fdrop is None else feature_dropout(out, fdrop, row0)
    if recompute is None:
        recompute = graph.num_rows * graph.segments * X.shape[-1] * (2 if z_bf16 else 4) > RECOMPUTE_Z_BYTES
    out = _GraphConv.apply(X, graph, W, b, relu, bool(recompute), out_bf16, fdrop if fused else None, int(row0),
                           z_bf16)
    return out if fused or fdrop is None else feature_dropout(out, fdrop, row0)


def graph_linear(Z: torch.Tensor, W: torch.Tensor, b=None, relu: bool = False, path_rows: int = 0) -> torch.Tensor:
    """out = Z W + b (optionally ReLU) on MFMA; Z rows x (L+1)F.  path_rows:
    the row count the GEMM path is chosen for (0: Z's own rows; a node-range
    shard passes the whole graph's, as graph_conv does through
    GrlTypedCsr.path_rows)."""
    _require_device(Z, "aggregated features")
    return _GraphLinear.apply(Z, W, b, relu, int(path_rows))


# -------------------------------------------------------- feature dropout
def _bf16_rows(t: torch.Tensor) -> bool:
    """A 2-D bfloat16 tensor with unit column stride and its rows apart (a
    column-slice view of a wider table included)."""
    return (t.dtype == torch.bfloat16 and t.dim() == 2 and (t.shape[1] == 0 or t.stride(1) == 1) and _rows_apart(t))


def feature_dropout_apply(x2: torch.Tensor, de, row0: int, out: torch.Tensor = None) -> torch.Tensor:
    """out = x2 * keep * 1/(1-p) for the element ids (row0 + r) * cols + c
    (grl_feature_dropout); x2 a 2-D fp32 row view.  Or a 2-D bfloat16 tensor
    with unit column stride and its rows apart, read as stored
    (grl_feature_dropout_bf16: bitwise the fp32 result on x2.float(), rounded
    once to nearest even; no widened copy): `out` is then a bfloat16 tensor of
    the same kind and shape, x2 itself included (the pass runs in place)."""
    _require_device(x2, "dropout input")
    if x2.dtype == torch.bfloat16:
        if out is None:
            out = torch.empty(x2.shape, dtype=torch.bfloat16, device=x2.device)
        if not _bf16_rows(x2) or not _bf16_rows(out) or out.shape != x2.shape or out.device != x2.device:
            raise _lib.GrlError("feature_dropout: a bfloat16 input and out must be 2-D bfloat16 tensors of one shape on "
                                "one device with unit column stride and a row stride of at least their width")
        dc = de.to_c()
        call("grl_feature_dropout_bf16", x2.data_ptr(), _ld(x2), out.data_ptr(), _ld(out), x2.shape[0], x2.shape[1],
             int(row0), ctypes.byref(dc), current_stream_handle(x2.device))
        return out
    if x2.dtype != torch.float32 or x2.dim() != 2 or x2.stride(1) != 1:
        raise _lib.GrlError("feature_dropout: a 2-D float32 (or bfloat16) tensor with unit column stride")
    if out is None:
        out = torch.empty(x2.shape, dtype=torch.float32, device=x2.device)
    dc = de.to_c()
    call("grl_feature_dropout", x2.data_ptr(), x2.stride(0), out.data_ptr(), out.stride(0), x2.shape[0], x2.shape[1],
         int(row0), ctypes.byref(dc), current_stream_handle(x2.device))
    return out


class _FeatureDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, de, row0: int):
        ctx.de, ctx.row0 = de, row0
        return feature_dropout_apply(x2, de, row0)

    @staticmethod
    def backward(ctx, g):
        # (a bfloat16 gradient goes through the bf16 entry as stored: the same map, no widened copy)
        return feature_dropout_apply(_rows_view(g.contiguous()), ctx.de, ctx.row0), None, None


def feature_dropout(x: torch.Tensor, de, row0: int = 0) -> torch.Tensor:
    """nn.Dropout(p) over node-feature rows with the mask of element (global
    row, column) a counter hash under the DropEdge record `de` (its p, seed
    / seed tensor and call id): drop_robust_gcn.py:64,77,81,86,100.  row0:
    the global row of x's first row (a node-range shard's row_begin), so a
    shard's rows get the one-GPU model's mask.  x float32, or bfloat16 read
    as stored (feature_dropout_apply): the result and the gradient are then
    bfloat16, each the fp32 map's value rounded once."""
    lead = x.shape[:-1]
    x2 = _rows_view(x)
    return _FeatureDropout.apply(x2, de, int(row0)).view(*lead, x.shape[-1])


# ------------------------------------------- batch norm over rows + LeakyReLU
def _bn_rows_table(t: torch.Tensor, what: str, like: torch.Tensor = None) -> None:
    if (t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 0 and t.stride(1) != 1) or not _rows_apart(t)
            or (like is not None and (t.shape != like.shape or t.device != like.device))):
        raise _lib.GrlError(f"batchnorm_rows: {what} must be a 2-D float32 tensor with unit column stride and a row "
                            f"stride of at least its width (got {t.dtype}, {tuple(t.shape)}, strides {t.stride()})")


def _bn_rows_vector(t, what: str, cols: int, device) -> None:
    if t is not None and (t.dtype != torch.float32 or t.shape != (cols,) or not t.is_contiguous()
                          or t.device != device):
        raise _lib.GrlError(f"batchnorm_rows: {what} must be a contiguous float32 [{cols}] tensor on {device}")


def batchnorm_rows_fwd_train(x2, weight, bias, running_mean, running_var, momentum, eps, slope, out=None):
    """(y, save_mean, save_invstd) of grl_bn_rows_fwd_train on a 2-D fp32 row
    view x2 (a column slice of a wider table included); the running buffers
    (None: none) are updated in place."""
    _require_device(x2, "batchnorm_rows input")
    _bn_rows_table(x2, "x")
    rows, cols = x2.shape
    for t, what in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        _bn_rows_vector(t, what, cols, x2.device)
    y = torch.empty(rows, cols, dtype=torch.float32, device=x2.device) if out is None else out
    _bn_rows_table(y, "out", x2)
    mean = torch.empty(cols, dtype=torch.float32, device=x2.device)
    invstd = torch.empty(cols, dtype=torch.float32, device=x2.device)
    ws_bytes = _lib.lib().grl_bn_rows_workspace_size(rows, cols)
    ws = _workspace(ws_bytes, x2.device)
    call("grl_bn_rows_fwd_train", x2.data_ptr(), _ld(x2), rows, cols, _ptr(weight), _ptr(bias), float(eps),
         float(slope), float(momentum), _ptr(running_mean), _ptr(running_var), y.data_ptr(), _ld(y), mean.data_ptr(),
         invstd.data_ptr(), _ptr(ws), ws_bytes, current_stream_handle(x2.device))
    return y, mean, invstd


def batchnorm_rows_fwd_eval(x2, weight, bias, running_mean, running_var, eps, slope, out=None):
    """y of grl_bn_rows_fwd_eval on a 2-D fp32 row view; out may be x2 itself
    (the pass runs in place)."""
    _require_device(x2, "batchnorm_rows input")
    _bn_rows_table(x2, "x")
    rows, cols = x2.shape
    if running_mean is None or running_var is None:
        raise _lib.GrlError("batchnorm_rows: the inference form needs running_mean and running_var")
    for t, what in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        _bn_rows_vector(t, what, cols, x2.device)
    y = torch.empty(rows, cols, dtype=torch.float32, device=x2.device) if out is None else out
    _bn_rows_table(y, "out", x2)
    call("grl_bn_rows_fwd_eval", x2.data_ptr(), _ld(x2), rows, cols, _ptr(weight), _ptr(bias), running_mean.data_ptr(),
         running_var.data_ptr(), float(eps), float(slope), y.data_ptr(), _ld(y), current_stream_handle(x2.device))
    return y


def batchnorm_rows_bwd(dy2, y2, x2, weight, mean, invstd, slope, want_weight=True, want_bias=True, out=None):
    """(dx, dweight, dbias) of grl_bn_rows_bwd; out may be dy2 itself."""
    _require_device(dy2, "batchnorm_rows gradient")
    _bn_rows_table(x2, "x")
    _bn_rows_table(y2, "y", x2)
    _bn_rows_table(dy2, "the output gradient", x2)
    rows, cols = x2.shape
    dx = torch.empty(rows, cols, dtype=torch.float32, device=x2.device) if out is None else out
    _bn_rows_table(dx, "out", x2)
    dw = torch.empty(cols, dtype=torch.float32, device=x2.device) if want_weight else None
    db = torch.empty(cols, dtype=torch.float32, device=x2.device) if want_bias else None
    ws_bytes = _lib.lib().grl_bn_rows_workspace_size(rows, cols)
    ws = _workspace(ws_bytes, x2.device)
    call("grl_bn_rows_bwd", dy2.data_ptr(), _ld(dy2), y2.data_ptr(), _ld(y2), x2.data_ptr(), _ld(x2), rows, cols,
         _ptr(weight), mean.data_ptr(), invstd.data_ptr(), float(slope), dx.data_ptr(), _ld(dx), _ptr(dw), _ptr(db),
         _ptr(ws), ws_bytes, current_stream_handle(x2.device))
    return dx, dw, db


class _BatchNormRows(torch.autograd.Function):
    """Training-mode batch norm over rows + LeakyReLU as one node: saves x, y,
    save_mean, save_invstd; the backward is one grl_bn_rows_bwd call."""

    @staticmethod
    def forward(ctx, x2, weight, bias, running_mean, running_var, momentum: float, eps: float, slope: float):
        y, mean, invstd = batchnorm_rows_fwd_train(x2, weight, bias, running_mean, running_var, momentum, eps, slope)
        ctx.save_for_backward(x2, y, mean, invstd, weight)
        ctx.slope = slope
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, y, mean, invstd, weight = ctx.saved_tensors
        dy2 = dy if dy.dim() == 2 and dy.stride(1) == 1 and _rows_apart(dy) else dy.contiguous()
        want_w = weight is not None and ctx.needs_input_grad[1]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        dx, dw, db = batchnorm_rows_bwd(dy2, y, x2, weight, mean, invstd, ctx.slope, want_w, want_b)
        return dx if ctx.needs_input_grad[0] else None, dw, db, None, None, None, None, None


def batchnorm_rows(x: torch.Tensor, weight, bias, running_mean, running_var, training: bool, momentum: float = 0.1,
                   eps: float = 1e-5, negative_slope: float = 0.2) -> torch.Tensor:
    """leaky_relu(batch_norm(x), negative_slope) with the channels on x's LAST
    axis and the statistics over all other axes: the reference's
    x.permute(0, 2, 1) -> nn.BatchNorm1d -> permute back -> F.leaky_relu
    (deep_rp_robust_gcn.py:39-45, 57-63) without the transposed copies.
    x [..., C] float32 on the device (bfloat16 is refused); weight / bias [C]
    or None (1 / 0); running_mean / running_var [C] or None.

    training (or no running statistics): batch statistics, accumulated in
    fp64 (grl_bn_rows_fwd_train), the running buffers updated in place, one
    autograd node whose backward is one grl_bn_rows_bwd call.  Results are the
    same bits run to run and on every device.  At least two rows.
    Inference with gradients disabled: one pass (grl_bn_rows_fwd_eval).
    Inference with gradients enabled is not a hot path: torch's F.batch_norm +
    F.leaky_relu on the 2-D view, differentiable through torch."""
    _require_device(x, "batchnorm_rows input")
    if x.dtype != torch.float32:
        raise _lib.GrlError(f"batchnorm_rows: a float32 input (got {x.dtype}); bfloat16 tables are not supported")
    if x.dim() < 1:
        raise _lib.GrlError("batchnorm_rows: x must have a channel axis")
    lead, C = x.shape[:-1], x.shape[-1]
    x2 = _rows_view(x)
    if x2.shape[0] > 1 and not _rows_apart(x2):
        x2 = x2.contiguous()
    if training or running_mean is None or running_var is None:
        if x2.shape[0] == 1:
            raise _lib.GrlError("batchnorm_rows: training needs more than one value per channel (got 1 row)")
        y = _BatchNormRows.apply(x2, weight, bias, running_mean, running_var, float(momentum), float(eps),
                                 float(negative_slope))
    elif not torch.is_grad_enabled():
        y = batchnorm_rows_fwd_eval(x2, weight, bias, running_mean, running_var, eps, negative_slope)
    else:
        y = torch.nn.functional.leaky_relu(
            torch.nn.functional.batch_norm(x2, running_mean, running_var, weight, bias, False, 0.0, eps),
            negative_slope)
    return y.view(*lead, C)


# ------------------------------------------------------- row-local linears
def linear_fwd_ex(X2: torch.Tensor, W: torch.Tensor, w_layout: int, b, relu: bool, path_rows: int = 0,
                  out: torch.Tensor = None) -> torch.Tensor:
    """out = X2 W (+ b) [ReLU] through grl_linear_fwd_ex; W [K, C]
    (w_layout 0) or [C, K] (1, nn.Linear.weight); the path chosen for
    max(M, path_rows) rows."""
    M, K = X2.shape
    C = W.shape[1] if w_layout == 0 else W.shape[0]
    if out is None:
        out = torch.empty(M, C, dtype=torch.float32, device=X2.device)
    ws_bytes = _lib.lib().grl_linear_fwd_ex_workspace_size(M, K, C, int(path_rows))
    ws = _workspace(ws_bytes, X2.device)
    call("grl_linear_fwd_ex", X2.data_ptr(), X2.stride(0), W.data_ptr(), int(w_layout), _ptr(b), out.data_ptr(), M, K,
         C, int(relu), int(path_rows), _ptr(ws), ws_bytes, current_stream_handle(X2.device))
    return out


def linear_fwd_bf16x(X16: torch.Tensor, W: torch.Tensor, w_layout: int, b, relu: bool, path_rows: int = 0):
    """out = X16 W (+ b) [ReLU] with the bfloat16 X read as stored
    (grl_linear_fwd_bf16x: X DMA'd into one LDS plane of the split-bf16 GEMM,
    three plane products for six, no widened copy), bitwise
    linear_fwd_ex(X16.float(), W, w_layout, b, relu, path_rows) -- or None
    where that entry's workspace query is 0 (below the x6 size floor, X16 off
    the 16 B grid or its row stride off the 8-element grid, the linear_bf16x or
    gemm_x6 path option 0, ...); the caller then widens X16.  Nothing is
    allocated before the query.  X16: 2-D bfloat16 with unit column stride and
    a row stride of at least its width (a column slice of a wider table is
    read in place); W float32, [K, C] (w_layout 0) or [C, K] (1), contiguous."""
    _require_device(X16, "linear_fwd_bf16x X")
    if not _bf16_rows(X16):
        raise _lib.GrlError("linear_fwd_bf16x: X must be a 2-D bfloat16 tensor with unit column stride and a row "
                            "stride of at least its width (an expanded tensor: .contiguous() first)")
    M, K = X16.shape
    if (W.dtype != torch.float32 or W.dim() != 2 or not W.is_contiguous() or W.device != X16.device
            or W.shape[1 if w_layout else 0] != K):
        raise _lib.GrlError(f"linear_fwd_bf16x: W must be a contiguous float32 [{K}, C] (w_layout 0) or [C, {K}] "
                            f"(w_layout 1) tensor on {X16.device}")
    C = W.shape[0] if w_layout else W.shape[1]
    ws_bytes = _lib.lib().grl_linear_fwd_bf16x_workspace_query(X16.data_ptr(), _ld(X16), W.data_ptr(), M, K, C,
                                                               int(path_rows))
    if ws_bytes == 0:
        return None
    out = torch.empty(M, C, dtype=torch.float32, device=X16.device)
    ws = _workspace(ws_bytes, X16.device)
    call("grl_linear_fwd_bf16x", X16.data_ptr(), _ld(X16), W.data_ptr(), int(w_layout), _ptr(b), out.data_ptr(), M, K,
         C, int(relu), int(path_rows), _ptr(ws), ws_bytes, current_stream_handle(X16.device))
    return out


def linear_fwd_to_bf16(X2: torch.Tensor, W: torch.Tensor, w_layout: int, b, relu: bool, path_rows: int = 0,
                       out: torch.Tensor = None):
    """out = X2 W (+ b) [ReLU] stored as bfloat16 rows by the GEMM's epilogue
    (grl_linear_fwd_to_bf16: each fp32 value rounded once to nearest even, no
    fp32 [M, C] table, no cast pass), bitwise linear_fwd_ex(X2, W, w_layout, b,
    relu, path_rows).to(torch.bfloat16) -- or None where that entry's workspace
    query is 0 (off grl_linear_fwd_ex's x6 path, out off the 4 B grid or with an
    odd row stride, the linear_out_bf16 or gemm_x6 path option 0, ...); the
    caller then runs linear_fwd_ex and casts.  Nothing is allocated before the
    query.  X2: 2-D float32 with unit column stride; W
    float32, [K, C] (w_layout 0) or [C, K] (1), contiguous; out: a bfloat16
    [M, C] tensor with unit column stride and a row stride of at least C (a
    column slice of a wider bfloat16 table is written in place), made if None."""
    _require_device(X2, "linear_fwd_to_bf16 X")
    if (X2.dtype != torch.float32 or X2.dim() != 2 or (X2.shape[1] > 0 and X2.stride(1) != 1)
            or not _rows_apart(X2)):
        raise _lib.GrlError("linear_fwd_to_bf16: X must be a 2-D float32 tensor with unit column stride and a row "
                            "stride of at least its width")
    M, K = X2.shape
    if (W.dtype != torch.float32 or W.dim() != 2 or not W.is_contiguous() or W.device != X2.device
            or W.shape[1 if w_layout else 0] != K):
        raise _lib.GrlError(f"linear_fwd_to_bf16: W must be a contiguous float32 [{K}, C] (w_layout 0) or [C, {K}] "
                            f"(w_layout 1) tensor on {X2.device}")
    C = W.shape[0] if w_layout else W.shape[1]
    if out is not None and (not _bf16_rows(out) or out.shape != (M, C) or out.device != X2.device):
        raise _lib.GrlError(f"linear_fwd_to_bf16: out must be a bfloat16 [{M}, {C}] tensor on {X2.device} with unit "
                            "column stride and a row stride of at least its width")
    # (an out still to be made is asked about as what it will be: rows C apart on an allocation's 256 B grid)
    out_ptr, ldo = (out.data_ptr(), _ld(out)) if out is not None else (256, C)
    ws_bytes = _lib.lib().grl_linear_fwd_to_bf16_workspace_query(X2.data_ptr(), _ld(X2), W.data_ptr(), out_ptr, ldo,
                                                                 M, K, C, int(path_rows))
    if ws_bytes == 0:
        return None
    if out is None:
        out = torch.empty(M, C, dtype=torch.bfloat16, device=X2.device)
    ws = _workspace(ws_bytes, X2.device)
    call("grl_linear_fwd_to_bf16", X2.data_ptr(), _ld(X2), W.data_ptr(), int(w_layout), _ptr(b), out.data_ptr(),
         _ld(out), M, K, C, int(relu), int(path_rows), _ptr(ws), ws_bytes, current_stream_handle(X2.device))
    return out


class _RowLinear(torch.autograd.Function):
    """nn.Linear (+ ReLU) on the libgrl GEMM: out = X W^T + b.  Every output
    row is the same fp32 operations whatever the row count (both GEMM paths
    are M-invariant and path_rows pins the choice), so a node-range shard's
    rows are bitwise the one-GPU model's.
    A bfloat16 X2 (W stays float32) is the node of X2.float() followed by this
    one, bit for bit: where linear_fwd_bf16x applies the forward reads X2 as
    stored and saves it (no widened copy); elsewhere X2 is widened first.  The
    backward of a saved bfloat16 X2 reads it as stored for dW
    (linear_bwd_weight_bf16z_f32g) and has the data-gradient GEMM store the
    bfloat16 dX itself (linear_fwd_to_bf16: the fp32 dX rounded once, as
    autograd does through .float()): no fp32 [M, K] table in either direction.
    Where one of the two returns None (below the x6 floor, its path option 0)
    that half runs the widened way -- X2.float() for dW, the fp32 GEMM and a
    cast for dX -- with the same bits."""

    @staticmethod
    def forward(ctx, X2, W, b, relu: bool, path_rows: int):
        C = W.shape[0]
        pad = -C % 4  # an output width off the float4 grid (the classifier's 53) runs padded with zero rows of W
        Wc = W.contiguous() if not pad else torch.nn.functional.pad(W, (0, 0, 0, pad))
        bc = None if b is None else (b.contiguous() if not pad else torch.nn.functional.pad(b, (0, pad)))
        ctx.x16 = X2.dtype == torch.bfloat16
        out = linear_fwd_bf16x(X2, Wc, 1, bc, relu, path_rows) if ctx.x16 else None
        if out is None:
            if ctx.x16:
                X2 = X2.float()
            out = linear_fwd_ex(X2, Wc, 1, bc, relu, path_rows)
        ctx.relu, ctx.path_rows, ctx.C = relu, path_rows, C
        ctx.save_for_backward(X2, Wc, out if relu else None)
        return out if not pad else out[:, :C].contiguous()

    @staticmethod
    def backward(ctx, g):
        X2, W, out = ctx.saved_tensors
        g = g.contiguous().float()
        C, Cp = ctx.C, W.shape[0]
        if Cp != C:
            g = torch.nn.functional.pad(g, (0, Cp - C))
        if ctx.relu:
            g = torch.where(out > 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
        dX = dW = db = None
        if ctx.needs_input_grad[0]:  # g [M, C] x W [C, K]
            if ctx.x16:  # the gradient of X.float(): the fp32 dX rounded once, by the GEMM's epilogue where it applies
                dX = linear_fwd_to_bf16(g, W, 0, None, False, ctx.path_rows)
            if dX is None:
                dX = linear_fwd_ex(g, W, 0, None, False, ctx.path_rows)
                if ctx.x16:
                    dX = dX.to(torch.bfloat16)
        want_b = ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            # X^T g [K, C]; an X2 saved as bfloat16 is read as stored where that entry applies, else widened for the
            # fp32 dW entry (a transient, freed with this frame)
            res = linear_bwd_weight_bf16z_f32g(X2, g, want_b) if X2.dtype == torch.bfloat16 else None
            dWt, db = res if res is not None else linear_bwd_weight(X2.float(), g, None, want_b)
            dW = dWt.t()[:C] if ctx.needs_input_grad[1] else None
            db = db[:C] if db is not None else None
        return dX, dW, db, None, None


def row_linear(X: torch.Tensor, W: torch.Tensor, b=None, relu: bool = False, path_rows: int = 0) -> torch.Tensor:
    """nn.Linear(K, C) [+ ReLU] over the rows of X [..., K] (W [C, K], b [C])
    on the libgrl GEMM (grl_linear_fwd_ex): the row-local linears of
    GraphCNNDropEdge (drop_robust_gcn.py:36-58, robust_gcn.py:81-83).
    path_rows: the row count the GEMM path is chosen for (a node-range
    shard passes the whole graph's).  X float32, or bfloat16 read as stored
    where linear_fwd_bf16x applies (and widened where not): the result and
    every gradient are bitwise row_linear(X.float(), ...)'s, the gradient of X
    bfloat16 (_RowLinear).  The backward of a bfloat16 X reads it as stored for
    dW and has the GEMM store the bfloat16 dX where
    linear_bwd_weight_bf16z_f32g and linear_fwd_to_bf16 apply: no fp32 copy of
    X or of its gradient."""
    _require_device(X, "linear input")
    if X.dtype not in (torch.float32, torch.bfloat16) or W.dtype != torch.float32:
        raise _lib.GrlError("row_linear: a float32 or bfloat16 input and a float32 weight required")
    lead = X.shape[:-1]
    X2 = _rows_view(X)
    if X2.dtype == torch.bfloat16 and not _rows_apart(X2):  # an expanded tensor (row stride 0)
        X2 = X2.contiguous()
    # path_rows >= M: the M-invariant kernels only (never grl_linear_fwd's unpinned large-M tile)
    out = _RowLinear.apply(X2, W, b, relu, int(max(path_rows, X2.shape[0])))
    return out.view(*lead, W.shape[0])


# ---------------------------------------------------------------- attention
def _attn_check(Q, K, H, V, gamma):
    """Shapes and dtypes.  V and gamma are float32; K and H are both float32 or
    both bfloat16 (tables stored as bf16); Q is float32 or bfloat16."""
    for t, what in ((Q, "queries"), (K, "keys"), (H, "values"), (V, "residual"), (gamma, "gamma")):
        _require_device(t, what)
    for t, what in ((V, "residual"), (gamma, "gamma")):
        if t.dtype != torch.float32:
            raise _lib.GrlError(f"attention {what} must be float32 (got {t.dtype})")
    if Q.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"attention queries must be float32 or bfloat16 (got {Q.dtype})")
    if K.dtype != H.dtype or K.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.GrlError(f"attention keys and values must both be float32 or both bfloat16 (got {K.dtype}, "
                            f"{H.dtype})")
    if Q.dim() != 3 or K.shape != Q.shape or H.dim() != 3 or H.shape[:2] != Q.shape[:2] or V.shape != H.shape \
            or gamma.shape != (H.shape[2],):
        raise _lib.GrlError(f"attention shapes: Q {tuple(Q.shape)}, K {tuple(K.shape)}, H {tuple(H.shape)}, "
                            f"V {tuple(V.shape)}, gamma {tuple(gamma.shape)}")


def _attn_workspace(B, N, dk, dv, device, backward: bool = False):
    """bf16 planes of the attention operands, split once per call, and the
    backward's partials (grl.h)."""
    lib = _lib.lib()
    n = (lib.grl_node_attention_bwd_workspace_size if backward else lib.grl_node_attention_workspace_size)(B, N, dk, dv)
    if not n:
        return None, 0
    try:
        return torch.empty(n, dtype=torch.uint8, device=device), n
    except torch.cuda.OutOfMemoryError:
        if not backward:
            raise
        # the backward's dQ slabs (N^2 / 4 bytes at dk <= 16) do not fit: the smaller
        # workspace runs the separate dQ kernel instead (grl.h)
        n = lib.grl_node_attention_workspace_size(B, N, dk, dv)
        return (torch.empty(n, dtype=torch.uint8, device=device), n) if n else (None, 0)


# Value columns per kernel call: the kernels hold one query's output row in
# registers (dv <= 256; 128 when dk > 32, where the fp32 kernels also carry
# 64-wide Q/K rows).  Wider values run as column blocks of one softmax: each
# block recomputes S = Q K^T (same bits, so the same P), and the backward's
# dS = P o (dP - D) is linear in the per-block dP_b and D_b, so dQ and dK are
# the block sums (robust_gcn.py:78-96 for any input_dim up to 512).
def _dv_blocks(dk: int, dv: int):
    width = 256 if dk <= 32 else 128
    n = -(-dv // width)
    step = -(-dv // n)
    step = -(-step // 32) * 32
    return [(c0, min(dv, c0 + step)) for c0 in range(0, dv, step)]


def node_attention_forward(Q, K, H, V, gamma, stats: bool = False, q_range=None):
    """out = gamma * softmax(Q K^T) H + V (robust_gcn.py:90-96), fused.
    stats=True also returns (o_norm, row_max, row_sum) for the backward.
    q_range=(q0, q1): only those query rows are computed (the other rows of
    the outputs are zeros) -- a node-range shard's queries against every key
    (grl_node_attention_fwd_rows).
    K and H may both be bfloat16 (tables stored as bf16): where
    grl_node_attention_fwd_bf16kv_path allows, the kernel stages them as they
    lie (grl_node_attention_fwd_bf16kv_rows); elsewhere they are widened and
    the fp32 call runs.  A bfloat16 Q is widened."""
    _attn_check(Q, K, H, V, gamma)
    Q, K, H, V, gamma = (t.contiguous() for t in (Q.float(), K, H, V, gamma))
    B, N, dk = Q.shape
    dv = H.shape[2]
    q0, q1 = (0, N) if q_range is None else (int(q_range[0]), int(q_range[1]))
    blocks = _dv_blocks(dk, dv)
    if len(blocks) > 1:
        parts = [node_attention_forward(Q, K, H[..., a:b].contiguous(), V[..., a:b].contiguous(),
                                        gamma[a:b].contiguous(), stats=stats, q_range=q_range) for a, b in blocks]
        if not stats:
            return torch.cat(parts, -1)
        out = torch.cat([p[0] for p in parts], -1)
        onorm = torch.cat([p[1] for p in parts], -1)
        return out, onorm, parts[0][2], parts[0][3]
    alloc = torch.empty_like if q_range is None else torch.zeros_like  # ranged: rows outside stay defined
    out = alloc(V)
    onorm = alloc(V) if stats else None
    rmax = alloc(V[..., 0]) if stats else None
    rsum = (torch.ones_like(V[..., 0]) if q_range is not None else torch.empty_like(V[..., 0])) if stats else None
    lib = _lib.lib()
    if K.dtype == torch.bfloat16 and lib.grl_node_attention_fwd_bf16kv_path(B, N, dk, dv) \
            and K.data_ptr() % 16 == 0 and H.data_ptr() % 16 == 0:
        n = lib.grl_node_attention_fwd_bf16kv_workspace_size(B, N, dk, dv)  # the key split's partials only
        ws = torch.empty(n, dtype=torch.uint8, device=V.device) if n else None
        call("grl_node_attention_fwd_bf16kv_rows", Q.data_ptr(), K.data_ptr(), H.data_ptr(), V.data_ptr(),
             gamma.data_ptr(), out.data_ptr(), _ptr(onorm), _ptr(rmax), _ptr(rsum), B, N, dk, dv, q0, q1, _ptr(ws), n,
             current_stream_handle(V.device))
        return (out, onorm, rmax, rsum) if stats else out
    if K.dtype == torch.bfloat16:  # no bf16 form of this call: the fp32 entry on the widened tables
        K, H = K.float(), H.float()
    ws, ws_bytes = _attn_workspace(B, N, dk, dv, V.device)
    call("grl_node_attention_fwd_rows", Q.data_ptr(), K.data_ptr(), H.data_ptr(), V.data_ptr(), gamma.data_ptr(),
         out.data_ptr(), _ptr(onorm), _ptr(rmax), _ptr(rsum), B, N, dk, dv, q0, q1, _ptr(ws), ws_bytes,
         current_stream_handle(V.device))
    return (out, onorm, rmax, rsum) if stats else out


def node_attention_backward(Q, K, H, gamma, onorm, rmax, rsum, dout, q_range=None):
    """(dQ, dK, dH) of out = gamma * softmax(Q K^T) H + V for the output
    gradient dout, from the forward's stats (grl_node_attention_bwd).
    q_range=(q0, q1): only those queries -- dQ of the range (other rows
    zero), dK / dH of every key from the range's queries alone (partials).
    float32 Q, K, H and stats only (the kernels read and write fp32; a caller
    holding bf16 tables widens them, as _NodeAttention does)."""
    for t, what in ((Q, "queries"), (K, "keys"), (H, "values"), (gamma, "gamma"), (onorm, "o_norm"),
                    (rmax, "row_max"), (rsum, "row_sum")):
        if t.dtype != torch.float32:
            raise _lib.GrlError(f"attention backward: {what} must be float32 (got {t.dtype})")
    dout = dout.contiguous().float()
    B, N, dk = Q.shape
    dv = H.shape[2]
    q0, q1 = (0, N) if q_range is None else (int(q_range[0]), int(q_range[1]))
    dO = dout * gamma
    dQ = dK = None
    dHs = []
    for a, b in _dv_blocks(dk, dv):  # one block unless dv exceeds a call's width
        dO_b = dO[..., a:b].contiguous()
        D = (dO_b * onorm[..., a:b]).sum(-1).contiguous()
        dQ_b = torch.empty_like(Q) if q_range is None else torch.zeros_like(Q)
        dK_b = torch.empty_like(K)
        dH_b = torch.empty(B, N, b - a, dtype=H.dtype, device=H.device)
        H_b = H[..., a:b].contiguous()
        ws, ws_bytes = _attn_workspace(B, N, dk, b - a, Q.device, backward=True)
        call("grl_node_attention_bwd_rows", Q.data_ptr(), K.data_ptr(), H_b.data_ptr(), dO_b.data_ptr(),
             rmax.data_ptr(), rsum.data_ptr(), D.data_ptr(), dQ_b.data_ptr(), dK_b.data_ptr(), dH_b.data_ptr(),
             B, N, dk, b - a, q0, q1, _ptr(ws), ws_bytes,
             current_stream_handle(Q.device))
        dQ = dQ_b if dQ is None else dQ + dQ_b
        dK = dK_b if dK is None else dK + dK_b
        dHs.append(dH_b)
    dH = dHs[0] if len(dHs) == 1 else torch.cat(dHs, -1)
    return dQ, dK, dH


class _NodeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, H, V, gamma):
        out, onorm, rmax, rsum = node_attention_forward(Q, K, H, V, gamma, stats=True)
        ctx.save_for_backward(Q.contiguous(), K.contiguous(), H.contiguous(), gamma, onorm, rmax, rsum)
        return out

    @staticmethod
    def backward(ctx, dout):
        Q, K, H, gamma, onorm, rmax, rsum = ctx.saved_tensors
        dout = dout.contiguous().float()
        # bf16 K / H (saved as they came): widened once for the fp32 backward, whose saved
        # o_norm / row_max / row_sum are the bf16 forward's by its contract (grl.h); a
        # gradient follows its input's dtype
        dQ, dK, dH = node_attention_backward(Q.float(), K.float(), H.float(), gamma, onorm, rmax, rsum, dout)
        dgamma = (dout * onorm).sum((0, 1))
        return dQ.to(Q.dtype), dK.to(K.dtype), dH.to(H.dtype), dout, dgamma


def node_self_attention(Q: torch.Tensor, K: torch.Tensor, H: torch.Tensor, V: torch.Tensor,
                        gamma: torch.Tensor) -> torch.Tensor:
    """Autograd op: gamma * softmax_rows(Q K^T) H + V on the fused kernels
    (grl_node_attention_fwd / _bwd); never materialises the N x N scores."""
    return _NodeAttention.apply(Q, K, H, V, gamma)


# ------------------------------------------------------ bag-of-chars linear
def bag_linear_forward(V2: torch.Tensor, Wt: torch.Tensor, b, relu: bool) -> torch.Tensor:
    """relu?(V2 @ Wt + b) gathering only the nonzero rows of Wt per row of V2."""
    M, K = V2.shape
    C = Wt.shape[1]
    out = torch.empty(M, C, dtype=torch.float32, device=V2.device)
    call("grl_bag_linear_fwd", V2.data_ptr(), V2.stride(0), M, K, Wt.data_ptr(), C, _ptr(b), int(relu),
         out.data_ptr(), current_stream_handle(V2.device))
    return out


# emb1's weight gradient on the sparse kernel from this many rows on (A/B at
# K = 4369, C = 256, ~7 + 4 nonzeros per row, profiles/r02_probe_bag_dw.json:
# M = 4096 dense GEMM 0.16 vs sparse 0.25 ms; 20k 0.59 vs 0.47; 100k 2.71 vs 1.51)
BAG_DW_SPARSE_ROWS = 16384


def bag_linear_bwd_weight(V2: torch.Tensor, g: torch.Tensor, relu_out, want_db: bool):
    """(dWt [K, C], db [C] or None) = V2^T g', 1^T g' with g' = g [out > 0],
    reading a row of g' only for V2's nonzeros (grl_bag_linear_bwd_weight)."""
    M, K = V2.shape
    C = g.shape[1]
    dWt = torch.empty(K, C, dtype=torch.float32, device=g.device)
    db = torch.empty(C, dtype=torch.float32, device=g.device) if want_db else None
    ws_bytes = _lib.lib().grl_bag_linear_bwd_weight_workspace_size(M, K, C)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=g.device)
    call("grl_bag_linear_bwd_weight", V2.data_ptr(), V2.stride(0), g.data_ptr(), _ptr(relu_out), dWt.data_ptr(),
         _ptr(db), M, K, C, ws.data_ptr(), ws_bytes, current_stream_handle(g.device))
    return dWt, db


class _BagLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, V2, W, b, relu: bool):
        Wt = W.t().contiguous()
        out = bag_linear_forward(V2, Wt, b, relu)
        ctx.relu = relu
        ctx.has_b = b is not None
        ctx.save_for_backward(V2, Wt, out)
        return out

    @staticmethod
    def backward(ctx, g):
        V2, Wt, out = ctx.saved_tensors
        g, relu_out, _ = relu_grad(g.contiguous().float(), out if ctx.relu else None)
        dV = linear_bwd_data(g, relu_out, Wt) if ctx.needs_input_grad[0] else None
        if V2.shape[0] >= BAG_DW_SPARSE_ROWS:  # large M: only V's nonzeros read a row of g
            dWt, db = bag_linear_bwd_weight(V2, g, relu_out, ctx.has_b)
        else:  # few rows: the split-K MFMA GEMM is faster (tools/probe_bag_dw.py)
            dWt, db = linear_bwd_weight(V2, g, relu_out, ctx.has_b)
        return dV, dWt.t(), db, None


def bag_linear(V: torch.Tensor, W: torch.Tensor, b, relu: bool = False) -> torch.Tensor:
    """nn.Linear(K, C) (+ReLU) for sparse inputs such as emb1's bag-of-chars
    rows: V [..., K], W [C, K] (nn.Linear.weight), b [C] or None."""
    _require_device(V, "bag-of-chars input")
    if V.dtype != torch.float32 or W.dtype != torch.float32:
        raise _lib.GrlError("bag_linear: float32 input and weight required")
    lead = V.shape[:-1]
    V2 = V.reshape(-1, V.shape[-1])
    if V2.stride(-1) != 1:
        V2 = V2.contiguous()
    return _BagLinear.apply(V2, W, b, relu).view(*lead, W.shape[0])
