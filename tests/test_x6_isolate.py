"""CPU: the proof that the plane-isolating GPU tests (test_gpu_x6_planes.py)
can fail.  The numpy model of one split-bf16 product (x6_isolate.six_product)
meets the per-element bound 2^-22; every single-product mutation -- a plane
product dropped, duplicated or swapped -- breaks it on at least half of the
elements; and the few-hot attention fixture has the rows it is designed to
have, agrees with a dense float64 attention, meets its own bounds in an fp32
restatement and misses them when a low-order product is dropped.  No kernel
runs here."""
import numpy as np
import pytest
import torch

import x6_isolate as xi
from test_x6_split import _values

PAIRS = 1 << 20


def _pairs(seed):
    rng = np.random.default_rng(seed)
    return xi.full_values(rng, PAIRS), xi.full_values(rng, PAIRS)


def test_model_meets_the_bare_bound_on_random_pairs():
    a, b = _pairs(0)
    worst = xi.check_products(xi.six_product(a, b), a, b, xi.BARE, "six products")
    print(f"worst error {worst * 4:.3f} * 2^-24 |a b|")
    assert worst * 4 <= 1.7  # the measured 1.58 * 2^-24: well inside the analytic 3.1 * 2^-24


def test_model_meets_the_bare_bound_on_adversarial_values():
    """test_x6_split's values (binade edges, 1 + 2^-23, 1 - 2^-24, the largest
    and smallest magnitudes the split is exact for) against full-mantissa
    partners in [1, 2), both ways round."""
    rng = np.random.default_rng(1)
    a = _values(rng, 100_000, lo=-60, hi=60)
    b = (1.0 + rng.random(a.size)).astype(np.float32) * np.where(rng.random(a.size) < 0.5, -1, 1).astype(np.float32)
    xi.check_products(xi.six_product(a, b), a, b, xi.BARE, "adversarial a")
    xi.check_products(xi.six_product(b, a), b, a, xi.BARE, "adversarial b")


def _without(prod):
    return tuple(p for p in xi.ORDER if p != prod)


MUTATIONS = {f"drop_{i}{j}": _without((i, j)) for i, j in xi.ORDER}
MUTATIONS["11_for_02"] = tuple((1, 1) if p == (0, 2) else p for p in xi.ORDER)
MUTATIONS["20_for_02"] = tuple((2, 0) if p == (0, 2) else p for p in xi.ORDER)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_every_single_product_mutation_breaks_the_bound(name):
    a, b = _pairs(2)
    share = xi.violating_share(xi.six_product(a, b, MUTATIONS[name]), a, b, xi.BARE)
    print(f"{name}: {share:.2%} of elements beyond 2^-22")
    assert share >= 0.5
    with pytest.raises(AssertionError, match="beyond"):
        xi.check_products(xi.six_product(a, b, MUTATIONS[name]), a, b, xi.BARE, name)


def test_sweep_visits_every_residue():
    for K in (16, 48, 1792, 3584, 7 * 256):
        for s in (0, 5):
            k = xi.sweep(max(K, 64), K, s)
            assert len(np.unique(k[:K])) == K and len(np.unique(k[:64] % 64)) == min(64, K)
    rng = np.random.default_rng(0)
    W = xi.one_hot_cols(rng, 48, 200, xi.sweep(200, 48, 3))
    assert ((W != 0).sum(0) == 1).all() and (W != 0).any(1).all()
    # every value has non-zero low planes
    v = W[W != 0]
    assert all(np.count_nonzero(p) > 0.95 * v.size for p in xi.split3(v))


# ---- the few-hot attention fixture -----------------------------------------
@pytest.fixture(scope="module")
def fx():
    return xi.few_hot(864, 4, 32, seed=3)


def _dense64(fx):
    """Plain dense float64 softmax attention, forward and backward (torch)."""
    Q, K, H, V, g = (torch.from_numpy(a).double().requires_grad_(True) for a in (fx.Q, fx.K, fx.H, fx.V, fx.gamma))
    S = Q @ K.T
    P = torch.softmax(S, -1)
    onorm = P @ H
    out = g * onorm + V
    out.backward(torch.from_numpy(fx.dout).double())
    return S.detach().numpy(), P.detach().numpy(), onorm.detach().numpy(), out.detach().numpy(), \
        [t.grad.numpy() for t in (Q, K, H)]


def test_fixture_rows_are_as_designed(fx):
    S, P, onorm, out, _ = _dense64(fx)
    q = np.arange(fx.N)
    hard, soft = fx.kind == 0, fx.kind == 1
    assert hard.sum() == 288 and soft.sum() == 576 and np.abs(S).max() > 1.5e5
    # the float64 softmax has one (hard) or two (soft pair) probabilities that fp32 can hold; the rest underflow
    live = P > 2.0 ** -150
    assert np.array_equal(live.sum(1), 1 + soft)
    assert live[q, fx.kstar].all() and live[q[soft], fx.runner[soft]].all()
    p_r = P[q[soft], fx.runner[soft]] / P[q[soft], fx.kstar[soft]]
    assert p_r.min() > 0.55 and p_r.max() < 0.9 and p_r.max() - p_r.min() > 0.2
    # every key is the target of one query (hard) or two (soft-pair winners and runners-up)
    n_w = np.bincount(fx.kstar, minlength=fx.N) + np.bincount(fx.runner[soft], minlength=fx.N)
    assert set(np.unique(n_w)) == {1, 2} and (n_w[fx.kstar[hard]] == 1).all()
    # winners and runners-up on every slot of a 32-key block, in both orders, in the same and in other blocks
    assert len(np.unique(fx.kstar % 32)) == 32 and len(np.unique(fx.runner[soft] % 32)) == 32
    before = fx.runner[soft] < fx.kstar[soft]
    same = fx.runner[soft] // 32 == fx.kstar[soft] // 32
    assert before.any() and (~before).any() and same.any() and (before & ~same).any() and (~before & ~same).any()
    # soft-pair winners carry no value, runners-up one value column, over every column
    assert not fx.H[fx.kstar[soft]].any() and ((fx.H[fx.runner[soft]] != 0).sum(1) == 1).all()
    assert len(np.unique(fx.hcol[fx.runner[soft]])) == fx.dv


def test_fixture_expectations_match_dense_float64(fx):
    _, _, onorm, out, _ = _dense64(fx)
    e_on, e_out, e_rmax, e_rsum, _ = xi.forward_expect(fx)
    # (float64 scores of 2e5 are exact to ~4e-11, hence rtol; the dense softmax keeps the e^-141 and smaller
    # weights that fp32 flushes to 0: far below atol)
    np.testing.assert_allclose(e_on, onorm, rtol=1e-9, atol=1e-50)
    np.testing.assert_allclose(e_out, out, rtol=1e-9, atol=1e-50)
    S = _dense64(fx)[0]
    np.testing.assert_allclose(e_rmax, S.max(1), rtol=1e-14)
    np.testing.assert_allclose(e_rsum, np.exp(S - S.max(1, keepdims=True)).sum(1), rtol=1e-9)


@pytest.mark.parametrize("dk,offset,N,T", [(4, 0, 864, 24), (16, 7, 864, 24), (32, 28, 1100, 26)])
def test_fp32_restatement_meets_every_forward_bound(dk, offset, N, T):
    f = xi.few_hot(N, dk, 32, seed=dk, T=T, offset=offset)
    worst = xi.assert_forward(f, *xi.forward_restated(f), what="restated")
    print({k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("where", ["s_order", "ph_order"])
@pytest.mark.parametrize("drop", [(2, 0), (1, 1), (0, 2)])
def test_restatement_with_a_dropped_product_fails(fx, where, drop):
    res = xi.forward_restated(fx, **{where: _without(drop)})
    with pytest.raises(AssertionError):
        xi.assert_forward(fx, *res, what="mutated")


def test_backward_expectations_match_dense_float64(fx):
    grads = _dense64(fx)[4]
    exp = xi.backward_expect(fx)
    for name, g in zip(("dQ", "dK", "dH"), grads):
        val, scale = exp[name]
        # hard rows' dQ / dK are 0 up to the float64 rounding of dP - D: compare on the terms' scale
        assert np.all(np.abs(val - g) <= 1e-9 * scale + 1e-50), name
    hard = fx.kind == 0
    assert np.all(np.abs(grads[0][hard]) <= 1e-9 * exp["dQ"][1][hard] + 1e-50)


def test_fp32_restatement_meets_every_backward_bound(fx):
    onorm, _, rmax, rsum = xi.forward_restated(fx)
    worst = xi.assert_backward(fx, *xi.backward_restated(fx, onorm, rmax, rsum), what="restated")
    print({k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("where,drop", [("s_order", (2, 0)), ("s_order", (1, 1)), ("s_order", (0, 2)),
                                        ("ph_order", (1, 1)), ("ph_order", (0, 2)), ("ph_order", (0, 1)),
                                        ("sk_order", (1, 1)), ("sk_order", (0, 2)), ("sk_order", (0, 1))])
def test_backward_restatement_with_a_dropped_product_fails(fx, where, drop):
    """A low-order product dropped in the backward's S (the probabilities
    leave their loose band), or one that carries a low plane of the vector
    operand in p.dO (dH) or in dS.K / dS.Q (dQ, dK)."""
    onorm, _, rmax, rsum = xi.forward_restated(fx)
    res = xi.backward_restated(fx, onorm, rmax, rsum, **{where: _without(drop)})
    with pytest.raises(AssertionError):
        xi.assert_backward(fx, *res, what="mutated")


def test_proportional_check_is_blind_to_a_scaled_row(fx):
    """What the backward's proportionality check cannot see, stated as a test:
    the scalar operand's own a_2 b_0 dropped scales the row by 1 - 2^-16."""
    onorm, _, rmax, rsum = xi.forward_restated(fx)
    res = xi.backward_restated(fx, onorm, rmax, rsum, ph_order=_without((2, 0)), sk_order=_without((2, 0)))
    xi.assert_backward(fx, *res, what="a2 b0 dropped")
