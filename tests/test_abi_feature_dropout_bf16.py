"""CPU-only: the bf16 feature dropout (grl_feature_dropout_bf16) and the
scaled bf16 ReLU mask pass (grl_relu_grad_bf16_scaled): exported, declared in
include/grl.h and bound; their host-side argument errors are GRL_E_INVALID
without a device (no pointer is dereferenced, no device work is issued); and
a numpy statement of why the scaled pass needs no hash: with the DROPPED ReLU
output as its mask, where(drop(out) > 0, RNE(g * scale), 0) is bitwise
where(out > 0, RNE(g * keep * scale), 0), the backward of the unfused chain."""
import os
import re

import numpy as np
import pytest

from grl import _lib
from oracle import hash as ohash

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
DROP, SCALED = "grl_feature_dropout_bf16", "grl_relu_grad_bf16_scaled"


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


@pytest.mark.parametrize("name", [DROP, SCALED])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures_follow_their_siblings():
    assert _lib.SIGNATURES[DROP] == _lib.SIGNATURES["grl_feature_dropout"]
    res, args = _lib.SIGNATURES[SCALED]
    tres, targs = _lib.SIGNATURES["grl_relu_grad_bf16"]
    assert res == tres and len(args) == len(targs) + 1
    scale_at = [i for i, a in enumerate(args) if a is _lib.ctypes.c_float]
    assert len(scale_at) == 1
    assert list(args[:scale_at[0]]) + list(args[scale_at[0] + 1:]) == list(targs)


def test_feature_dropout_bf16_host_checks():
    fn = getattr(_lib.lib(), DROP)
    err = _lib.lib().grl_last_error
    # nothing to do: OK before any pointer is looked at
    assert fn(None, 8, None, 8, 0, 8, 0, None, None) == _lib.GRL_OK
    assert fn(None, 0, None, 0, 5, 0, 0, None, None) == _lib.GRL_OK
    # negative sizes
    assert fn(0x1000, 8, 0x2000, 8, -1, 8, 0, None, None) == _lib.GRL_E_INVALID and DROP.encode() in err()
    assert fn(0x1000, 8, 0x2000, 8, 5, -8, 0, None, None) == _lib.GRL_E_INVALID
    assert fn(0x1000, 8, 0x2000, 8, 5, 8, -1, None, None) == _lib.GRL_E_INVALID
    # strides below cols (also with no rows: refused before the early return)
    assert fn(0x1000, 6, 0x2000, 8, 5, 8, 0, None, None) == _lib.GRL_E_INVALID and b"strides" in err()
    assert fn(0x1000, 8, 0x2000, 6, 5, 8, 0, None, None) == _lib.GRL_E_INVALID
    assert fn(0x1000, 6, 0x2000, 8, 0, 8, 0, None, None) == _lib.GRL_E_INVALID
    # NULL with work to do
    assert fn(None, 8, 0x2000, 8, 5, 8, 0, None, None) == _lib.GRL_E_INVALID and b"NULL pointer" in err()
    assert fn(0x1000, 8, None, 8, 5, 8, 0, None, None) == _lib.GRL_E_INVALID
    # an odd address for a 2-byte type
    assert fn(0x1001, 8, 0x2000, 8, 5, 8, 0, None, None) == _lib.GRL_E_INVALID and b"2-B aligned" in err()
    assert fn(0x1000, 8, 0x2001, 8, 5, 8, 0, None, None) == _lib.GRL_E_INVALID


def test_relu_grad_bf16_scaled_host_checks():
    fn = getattr(_lib.lib(), SCALED)
    s = 2.0
    assert fn(None, 8, None, 8, None, 8, None, None, 0, 8, s, None, 0, None) == _lib.GRL_OK
    assert fn(None, 0, None, 0, None, 0, None, None, 5, 0, s, None, 0, None) == _lib.GRL_OK
    assert fn(None, 8, None, 8, None, 8, None, None, -1, 8, s, None, 0, None) == _lib.GRL_E_INVALID
    assert SCALED.encode() in _lib.lib().grl_last_error()
    assert fn(None, 8, 0x2000, 8, None, 8, None, None, 5, 8, s, None, 0, None) == _lib.GRL_E_INVALID  # NULL g
    assert b"NULL pointer" in _lib.lib().grl_last_error()
    assert fn(0x1000, 6, 0x2000, 8, None, 0, None, None, 5, 8, s, None, 0, None) == _lib.GRL_E_INVALID  # ldg < C
    assert fn(0x1000, 8, 0x2000, 6, None, 0, None, None, 5, 8, s, None, 0, None) == _lib.GRL_E_INVALID  # ldo < C
    assert fn(0x1000, 8, 0x2000, 8, 0x3000, 6, None, None, 5, 8, s, None, 0, None) == _lib.GRL_E_INVALID  # lde < C
    assert fn(0x1001, 8, 0x2000, 8, None, 0, None, None, 5, 8, s, None, 0, None) == _lib.GRL_E_INVALID  # odd address
    need = _lib.lib().grl_relu_grad_workspace_size(5, 8)
    assert fn(0x1000, 8, 0x2000, 8, None, 0, None, 0x5000, 5, 8, s, 0x6000, need - 1, None) == _lib.GRL_E_WORKSPACE
    assert fn(0x1000, 8, 0x2000, 8, None, 0, None, 0x5000, 5, 8, s, None, 0, None) == _lib.GRL_E_WORKSPACE


# ---- the scaled pass's argument, in numpy on bf16 bits -------------------------------------------------
def widen(h):
    return (h.astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne(f):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


@pytest.mark.parametrize("p", [0.3, 0.5, 1.0])
def test_the_dropped_output_is_both_masks(p):
    rng = np.random.default_rng(int(p * 10))
    n = 1 << 16
    # a ReLU output: random bf16 >= 0 (subnormals and large values included), exact zeros and -0
    out = rng.integers(0x0001, 0x7F00, n).astype(np.uint16)
    out[rng.random(n) < 0.3] = 0x0000
    out[rng.random(n) < 0.05] = 0x8000
    out[:64] = np.arange(1, 65, dtype=np.uint16)  # the smallest subnormals
    g = rne(rng.standard_normal(n).astype(np.float32))
    g[rng.random(n) < 0.05] = 0x8000
    g[rng.random(n) < 0.05] = 0x0000
    _, _, scale = ohash.dropedge_params(p)
    keep = ohash.dropedge_keep(p, 17, (1 << 48) + 3, np.arange(n, dtype=np.uint64) + np.uint64(5 << 32))
    assert p == 1.0 or (0.2 < keep.mean() < 0.8)
    zero = np.uint16(0)

    def drop(h):  # grl_feature_dropout_bf16: kept RNE(x * scale), dropped the fp32 entry's 0.0f
        return np.where(keep, rne(widen(h) * scale), zero)

    out_drop = drop(out)
    fused = np.where(widen(out_drop) > 0, rne(widen(g) * scale), zero)  # grl_relu_grad_bf16_scaled on the dropped out
    unfused = np.where(widen(out) > 0, drop(g), zero)                   # dropout's backward, then the ReLU's
    assert np.array_equal(fused, unfused)
    # (what it rests on: the dropped output is > 0 exactly where kept and open)
    assert np.array_equal(widen(out_drop) > 0, keep & (widen(out) > 0))
    assert (fused != 0).any() or p == 1.0
