"""Inputs that isolate single plane products of the split-bf16 ("x6") scheme
(DESIGN.md §4.2), in numpy, for the CPU proof (test_x6_isolate.py) and the
GPU tests (test_gpu_x6_planes.py).  No GPU import.

The existing tolerances average a wrong low-order product (worth 2^-16 of its
term) away over the K terms of a dot product.  Here every output element's dot
product has exactly one non-zero term: one operand is one-hot along the
reduction index, every other term is x * 0 with all planes zero, and adds an
exact 0 to the accumulator.  The element is then one six-product sum a * b of
two full-mantissa fp32 numbers, checked against the float64 product.

Bounds (conditions from this model and the analysis, not from the kernels):
three dropped products (2^-24 + 2^-24 + 2^-32 of |a b|) plus five fp32
roundings of partial sums no larger than the result, the last at 2^-24: about
3.1 * 2^-24 analytically; the model measures 1.58 * 2^-24 on 2^20 pairs.
BARE = 2^-22 leaves room for an accumulator that truncates.  One dropped or
duplicated low-order product breaks 2^-22 on more than 85 % of random pairs."""
import numpy as np

ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))  # x6_mfma's order: small terms first
BARE = 2.0 ** -22  # one six-product sum against the float64 product
EXTRA = 2.0 ** -21  # ... followed by a few more fp32 operations (each counted where it is used)


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even) -> fp32, as v_cvt_pk_bf16_f32."""
    u = np.asarray(x).astype(np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def split3(v: np.ndarray):
    v = np.asarray(v).astype(np.float32)
    v0 = bf16_rne(v)
    r1 = (v - v0).astype(np.float32)
    v1 = bf16_rne(r1)
    r2 = (r1 - v1).astype(np.float32)
    v2 = bf16_rne(r2)
    return v0, v1, v2


def six_product(a, b, order=ORDER, acc=None):
    """a * b as the kernels form it: the plane products a_i b_j of `order`
    (each exact in fp32: two 8-bit significands), added one by one to an fp32
    accumulator.  `order` lets a caller drop, duplicate or swap products."""
    ap, bp = split3(a), split3(b)
    acc = np.zeros(np.broadcast(ap[0], bp[0]).shape, np.float32) if acc is None else acc.astype(np.float32)
    for i, j in order:
        acc = (acc + (ap[i] * bp[j]).astype(np.float32)).astype(np.float32)
    return acc


# ---- one-hot operands ------------------------------------------------------
def full_values(rng, shape) -> np.ndarray:
    """randn * 2^randint(-8, 9): full 24-bit significands (all three planes
    non-zero), 17 binades; zeros (probability ~0) are replaced by 1 + 2^-23."""
    v = rng.standard_normal(shape).astype(np.float32) * np.float32(2.0) ** rng.integers(-8, 9, shape).astype(np.float32)
    v = v.astype(np.float32)
    v[v == 0] = np.float32(1 + 2.0 ** -23)
    return v


def sweep(n: int, K: int, s: int, step: int = 37) -> np.ndarray:
    """k(c) = (step c + s) mod K for c < n: with step odd and coprime to K the
    positions visit every residue of K (and of 64, when n >= 64), so every lane
    and k-slot of a fragment and of a staged block meets non-zero low planes."""
    assert np.gcd(step, K) == 1 or K == 1, (step, K)
    return (step * np.arange(n, dtype=np.int64) + s) % K


def one_hot_cols(rng, K: int, C: int, k_of_c: np.ndarray) -> np.ndarray:
    """[K, C] with one non-zero per column c, at row k_of_c[c]."""
    W = np.zeros((K, C), np.float32)
    W[k_of_c, np.arange(C)] = full_values(rng, C)
    return W


def one_hot_rows(rng, M: int, K: int, k_of_m: np.ndarray) -> np.ndarray:
    """[M, K] with one non-zero per row m, at column k_of_m[m]."""
    Z = np.zeros((M, K), np.float32)
    Z[np.arange(M), k_of_m] = full_values(rng, M)
    return Z


def worst_ratio(got, ref, scale, bound) -> float:
    """max |got - ref| / (bound * scale) in float64 (0 where both vanish)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    lim = bound * np.abs(np.asarray(scale, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / lim)
    return float(r.max()) if r.size else 0.0


def check_bound(got, ref, scale, bound, what="") -> float:
    """Every element of `got` within bound * |scale| of the float64 `ref`; no
    element is excluded.  On failure: the violating share and the worst ratio.
    Returns the worst ratio error / (bound * scale)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    bad = np.abs(got - ref) > bound * np.abs(np.asarray(scale, np.float64))
    worst = worst_ratio(got, ref, scale, bound)
    assert not bad.any(), (f"{what}: {bad.mean():.2%} of {bad.size} elements beyond 2^{np.log2(np.max(bound)):.0f} of "
                           f"their scale, worst {worst:.3g} x the bound, first at {tuple(np.argwhere(bad)[0])}")
    return worst


def check_products(got, a, b, bound=BARE, what="") -> float:
    """got[...] == a[...] * b[...] (a single x6 product each) within
    bound * |a b| of the float64 product, per element."""
    ref = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return check_bound(got, ref, ref, bound, what)


def violating_share(got, a, b, bound=BARE) -> float:
    ref = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) > bound * np.abs(ref)).mean())


# ---- the few-hot attention fixture -------------------------------------------
# Keys on a product of moment curves, K[k] = s (t1, -t1^2/2, t2, -t2^2/2), and
# queries Q[q] = s (u1, 1, u2, 1): S[q, k] = s^2 (|u|^2 - |t_k - u|^2) / 2.  The
# key at the query's own point wins by s^2/2 = 160 natural units per unit of
# squared distance: e^-160 underflows to exactly 0 in fp32, so a query on a
# grid point sees a softmax with one non-zero probability (a hard row), or two
# when a runner-up key sits eps away along t1 (a soft-pair row).
GAIN = 160.0  # s^2 / 2


class FewHot:
    """One batch of the fixture (numpy; fp32 inputs, float64 expectations).

    Q, K [N, dk]; H, V, dout [N, dv]; gamma [dv]; kind [N] (0 hard, 1
    soft pair); kstar [N] the key at the query's point; runner [N] the
    runner-up key or -1.  Hard keys have one query each; H[winner] = 0 on
    soft-pair rows and H[runner] is one-hot along dv (column hcol[runner])."""

    def scores64(self, q, k):
        """float64 scores of the fp32 inputs, gathered: S[q[i], k[i]]."""
        return np.einsum("id,id->i", self.Q[q].astype(np.float64), self.K[k].astype(np.float64))

    def score_scale(self, q, k):
        return np.einsum("id,id->i", np.abs(self.Q[q].astype(np.float64)), np.abs(self.K[k].astype(np.float64)))


def few_hot(N: int, dk: int, dv: int, seed: int, T: int = 24, offset: int = 0, permute: bool = True) -> FewHot:
    """T x T grid points with a key each; every other point (checkerboard) also
    gets a runner-up key eps away along t1, eps per key so that
    P_r = e^(-160 eps^2) spreads over (0.58, 0.85): 3 T^2 / 2 keys.  Keys
    beyond that ("fillers") lie on a strip off the grid (t1 >= T + 4).  One
    query per grid point and per filler key, and the remaining T^2 / 2 queries
    repeat the soft-pair points: N queries like keys, every hard key the
    target of exactly one query, every soft-pair winner and runner-up of
    exactly two with the same Q row (hence the same probabilities).  The four
    curve coordinates sit at columns offset .. offset + 3 of dk, zeros
    elsewhere.  permute: keys and queries in a random order, so that winners
    and runners-up fall on every slot of a 32-key block, in both orders."""
    assert dk >= 4 and 0 <= offset <= dk - 4 and T % 2 == 0 and N >= 3 * T * T // 2
    rng = np.random.default_rng(seed)
    fx = FewHot()
    s = np.sqrt(2 * GAIN)
    gi, gj = (a.ravel() for a in np.meshgrid(np.arange(T), np.arange(T), indexing="ij"))
    G = T * T
    soft_pt = np.flatnonzero((gi + gj) % 2 == 0)  # these points get a runner-up
    n_soft = len(soft_pt)
    p_target = rng.uniform(0.58, 0.85, n_soft)
    eps = np.sqrt(-np.log(p_target) / GAIN)
    n_fill = N - G - n_soft
    fi, fj = T + 4 + np.arange(n_fill) // T, np.arange(n_fill) % T
    # key ids: grid points, runners-up, fillers
    t1 = np.concatenate([gi.astype(np.float64), gi[soft_pt] + eps, fi.astype(np.float64)])
    t2 = np.concatenate([gj, gj[soft_pt], fj]).astype(np.float64)
    # query ids: grid points, fillers, the soft-pair points again; tgt = the key at the query's point
    tgt = np.concatenate([np.arange(G), G + n_soft + np.arange(n_fill), soft_pt])
    u1, u2 = t1[tgt], t2[tgt]
    kperm = rng.permutation(N) if permute else np.arange(N)  # key id -> row of K
    qperm = rng.permutation(N) if permute else np.arange(N)
    K = np.zeros((N, dk), np.float32)
    Q = np.zeros((N, dk), np.float32)
    K[kperm[:, None], offset + np.arange(4)] = np.stack([s * t1, -s * t1 * t1 / 2, s * t2, -s * t2 * t2 / 2], 1)
    Q[qperm[:, None], offset + np.arange(4)] = np.stack([s * u1, s * np.ones(N), s * u2, s * np.ones(N)], 1)
    runner_of_key = np.full(N, -1, np.int64)
    runner_of_key[soft_pt] = G + np.arange(n_soft)
    has_r = runner_of_key[tgt] >= 0
    kind = np.zeros(N, np.int64)
    kstar = np.zeros(N, np.int64)
    runner = np.full(N, -1, np.int64)
    kstar[qperm] = kperm[tgt]
    runner[qperm[has_r]] = kperm[runner_of_key[tgt][has_r]]
    kind[qperm] = has_r.astype(np.int64)
    H = full_values(rng, (N, dv))
    H[kperm[soft_pt]] = 0.0  # soft-pair winners
    hcol = np.full(N, -1, np.int64)
    rk = kperm[G:G + n_soft]  # runners-up: one-hot along dv, the column sweeping every residue
    hcol[rk] = sweep(n_soft, dv, seed % dv, step=37 if dv % 37 else 41)
    H[rk] = 0.0
    H[rk, hcol[rk]] = full_values(rng, n_soft)
    fx.Q, fx.K, fx.H = Q, K, H
    fx.V = rng.standard_normal((N, dv)).astype(np.float32)
    fx.gamma = full_values(rng, dv)
    fx.dout = full_values(rng, (N, dv))
    fx.kind, fx.kstar, fx.runner, fx.hcol = kind, kstar, runner, hcol
    fx.N, fx.dk, fx.dv, fx.T = N, dk, dv, T
    return fx


def forward_expect(fx: FewHot, p_r=None):
    """float64 (onorm, out, rmax, rsum, p_r) of the fixture, closed form over
    the one or two live keys of each row.  p_r [N]: the runner-up's weight
    relative to the row maximum to use on soft-pair rows (recovered from the
    kernel under test as rsum - 1); default: the float64 softmax's."""
    q = np.arange(fx.N)
    soft = fx.kind == 1
    r = np.where(soft, fx.runner, fx.kstar)
    s_w, s_r = fx.scores64(q, fx.kstar), fx.scores64(q, r)
    if p_r is None:
        p_r = np.where(soft, np.exp(s_r - s_w), 0.0)
    p_r = np.where(soft, np.asarray(p_r, np.float64), 0.0)
    rsum = 1.0 + p_r
    H64 = fx.H.astype(np.float64)
    onorm = (H64[fx.kstar] + p_r[:, None] * np.where(soft[:, None], H64[r], 0.0)) / rsum[:, None]
    out = fx.gamma.astype(np.float64) * onorm + fx.V.astype(np.float64)
    return onorm, out, np.maximum(s_w, s_r), rsum, p_r


def forward_restated(fx: FewHot, s_order=ORDER, ph_order=ORDER):
    """The x6 forward on the fixture's live keys, restated in fp32 numpy:
    base-2 scores (Q scaled by log2(e) before its split, the six products per
    coordinate in one accumulator), p = 2^(s - m), l = 1 + p_r, P.H by the six
    products, one multiply by 1 / l; out = gamma * onorm + V.  Returns
    (onorm, out, rmax, rsum) as fp32.  s_order / ph_order: the products of the
    score and of P.H (to drop one)."""
    f32 = np.float32
    q = np.arange(fx.N)
    soft = fx.kind == 1
    r = np.where(soft, fx.runner, fx.kstar)
    Q2 = (fx.Q * f32(1.44269504088896341)).astype(f32)

    def score(k):
        acc = np.zeros(fx.N, f32)
        for d in range(fx.dk):
            acc = six_product(Q2[q, d], fx.K[k, d], s_order, acc)
        return acc

    s_w, s_r = score(fx.kstar), score(r)
    m = np.maximum(s_w, s_r)
    p_w = np.exp2((s_w - m).astype(f32)).astype(f32)
    p_r = np.where(soft, np.exp2((s_r - m).astype(f32)), 0).astype(f32)
    l = (p_w + p_r).astype(f32)
    acc = six_product(p_w[:, None], fx.H[fx.kstar], ph_order)
    acc = six_product(p_r[:, None], fx.H[r], ph_order, acc)
    onorm = (acc * (f32(1.0) / l)[:, None]).astype(f32)
    out = ((fx.gamma * onorm).astype(f32) + fx.V).astype(f32)
    return onorm, out, (m * f32(0.69314718055994531)).astype(f32), l


def assert_forward(fx: FewHot, onorm, out, rmax, rsum, bitwise_onorm=True, what=""):
    """What a forward on the fixture must satisfy; returns the worst ratio to
    the bound per output.  Rounding counts, in units of 2^-24 relative:
      onorm, soft-pair rows (EXTRA = 8 units): p_r recovered as rsum - 1 is
        exact to 2^-24 absolute, <= 2 units of a p_r in (0.5, 1); the product
        p_r H 1.58 (or one rounding of acc * alpha when the runner-up came
        first); 1 / l <= 2 (a 1-ulp reciprocal); the multiply by it 1.
      out: the above times gamma, plus the multiply and the add, each half an
        ulp of its result: 2^-23 (|gamma onorm| + |V|).
      rmax against the float64 score (2^-20 = 16 units of sum |q_d k_d|): the
        log2(e) scale of q 1.5 (rounding and the constant's own error), each
        of the <= 4 live products 1.58 and the sum of their roundings <= 3,
        the ln 2 scale back 1.5, the fp32 store of a float64 reference 1:
        about 9, rounded up to the next power of two."""
    onorm, out, rmax, rsum = (np.asarray(a) for a in (onorm, out, rmax, rsum))
    hard, soft = fx.kind == 0, fx.kind == 1
    q = np.arange(fx.N)
    worst = {}
    _, _, e_rmax, e_rsum, e_p = forward_expect(fx)
    assert np.array_equal(rsum[hard], np.ones(hard.sum(), np.float32)), f"{what}: rsum != 1 on hard rows"
    # loose on purpose: a correct fp32 score of magnitude 2e5 is off by ~0.06 natural units; a dropped low-order
    # product in S moves it by |S| 2^-17 ~ 2 units, which flips the winner or pushes p_r out of (0.5, 1)
    worst["rsum"] = check_bound(rsum[soft], e_rsum[soft], e_rsum[soft], 0.25, f"{what} rsum")
    p_r = rsum.astype(np.float64) - 1.0
    assert np.all((p_r[soft] > 0.5) & (p_r[soft] < 1.0)), f"{what}: p_r outside (0.5, 1)"
    r_live = np.where(soft, fx.runner, fx.kstar)
    scale = np.maximum(fx.score_scale(q, fx.kstar), fx.score_scale(q, r_live))
    worst["rmax"] = check_bound(rmax, e_rmax, scale, 2.0 ** -20, f"{what} rmax")
    on_ref, out_ref, _, _, _ = forward_expect(fx, p_r)
    H_star = fx.H[fx.kstar]
    if bitwise_onorm:  # 1.0 * (h2 + h1 + h0) small-first is exact: h1 + h2 = H - h0 is representable
        assert np.array_equal(onorm[hard].view(np.uint32), H_star[hard].view(np.uint32)), \
            f"{what}: onorm != H[k*] bitwise on {np.mean(onorm[hard] != H_star[hard]):.2%} of hard-row elements"
        worst["onorm_hard"] = 0.0
    else:
        worst["onorm_hard"] = check_bound(onorm[hard], on_ref[hard], on_ref[hard], 2.0 ** -23, f"{what} onorm hard")
    worst["onorm_soft"] = check_bound(onorm[soft], on_ref[soft], on_ref[soft], EXTRA, f"{what} onorm soft")
    g_on = np.abs(fx.gamma.astype(np.float64) * on_ref)
    lim = 2.0 ** -23 * (g_on + np.abs(fx.V.astype(np.float64)))
    lim[soft] += EXTRA * g_on[soft]
    if not bitwise_onorm:
        lim[hard] += 2.0 ** -23 * g_on[hard]
    worst["out"] = check_bound(out, out_ref, lim, 1.0, f"{what} out")
    return worst


# ---- the backward on the fixture ---------------------------------------------
# The backward recomputes P = 2^(s - lse2) from fp32 scores of magnitude 2e5,
# whose ulp is 2^-6 and more: any fp32 kernel's P is then right to a few per
# cent only (|S| 2^-23), and no P-dependent gradient can meet a per-product
# bound against float64.  What stays exact is the structure: every row of dH,
# dK and (on hard rows) dQ is ONE scalar -- a probability or a dS, whatever
# its value -- times a known vector, a single six-product sum per element:
#   dH[k, :] = p (sum of dO[q, :] over the one or two queries with that p)
#   dK[k, :] = (sum of dS) Q[q, :]      dQ[q, :] = dS K[k*, :]  (hard rows)
#   dQ[q, d] = (dS_r + dS_w) K[w, d]  (soft-pair rows, where K[r, d] == K[w, d])
# The scalar is recovered from the kernel's own row (the median ratio) and
# checked only loosely; the row must then be proportional to the vector within
# the bound.  Seen: a wrong low plane of the vector operand (dO, Q, K through
# LDS, DMA and transposed reads) and any product a_i b_j with j >= 1 dropped,
# duplicated or swapped (j: the vector operand's plane).  Not seen: an error
# that scales the whole row, such as the scalar operand's own a_2 b_0 dropped.
def live_pairs(fx: FewHot):
    """(q, k) of every probability that is not exactly 0."""
    q = np.arange(fx.N)
    soft = fx.kind == 1
    return np.concatenate([q, q[soft]]), np.concatenate([fx.kstar, fx.runner[soft]])


def backward_expect(fx: FewHot):
    """float64 closed form over the live pairs: {name: (value, sum |terms|)}
    for dQ, dK, dH, and p [pairs] / the pairs themselves under "pairs"."""
    qs, ks = live_pairs(fx)
    onorm, _, rmax, rsum, _ = forward_expect(fx)
    Q, K, H = (a.astype(np.float64) for a in (fx.Q, fx.K, fx.H))
    p = np.exp(fx.scores64(qs, ks) - rmax[qs]) / rsum[qs]
    dO = fx.dout.astype(np.float64) * fx.gamma.astype(np.float64)
    D, Dabs = (dO * onorm).sum(1), np.abs(dO * onorm).sum(1)
    dP = np.einsum("if,if->i", dO[qs], H[ks])
    dPabs = np.einsum("if,if->i", np.abs(dO[qs]), np.abs(H[ks]))
    dS, dSabs = p * (dP - D[qs]), p * (dPabs + Dabs[qs])
    res = {"pairs": (qs, ks, p, dSabs)}
    for name, rows, w, wabs, vec in (("dQ", qs, dS, dSabs, K[ks]), ("dK", ks, dS, dSabs, Q[qs]),
                                     ("dH", ks, p, p, dO[qs])):
        val, scale = np.zeros((fx.N, vec.shape[1])), np.zeros((fx.N, vec.shape[1]))
        np.add.at(val, rows, w[:, None] * vec)
        np.add.at(scale, rows, wabs[:, None] * np.abs(vec))
        res[name] = (val, scale)
    return res


def check_proportional(got, base, bound, terms=None, what=""):
    """Each row of `got` is c * (row of base) for one scalar c per row, within
    bound * |c base| per element -- or within bound * terms where `terms`
    [rows, cols] is given and not NaN (sums whose terms may cancel).  c: the
    median of got / base over the row's non-zero base elements (0 for a row
    without any).  A zero base element demands an exact zero.  Returns (the
    worst ratio to the bound, c)."""
    got, base = np.asarray(got, np.float64), np.asarray(base, np.float64)
    some = (base != 0).any(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(base != 0, got / base, np.nan)
    ratio[~some] = 0.0
    c = np.nanmedian(ratio, 1)
    ref = c[:, None] * base
    scale = np.abs(ref) if terms is None else np.where(np.isnan(terms), np.abs(ref), terms)
    return check_bound(got, ref, scale, bound, what), c


def assert_backward(fx: FewHot, dO, dQ, dK, dH, what=""):
    """What a backward on the fixture must satisfy (see above); dO: the fp32
    gamma * dout the kernels were given.  Returns the worst ratios.  Rounding
    counts, in units of 2^-24 relative to the row's terms:
      one query per key (2^-21 = 8 units): the element's product 1.58, the
        recovered scalar (another element's product) 1.58.
      two queries per key (soft-pair winners and runners-up, 2^-20 = 16
        units): two products 3.2, the second one's six additions each rounding
        at the first one's magnitude 6, the recovered scalar 1.58.  Their
        terms may cancel, so the bound is on sum |terms|, the scalars' sizes
        from the float64 closed form times the loose 1.25.
    Loose checks (0.25 of sum |terms|): every gradient against the float64
    closed form, and the probabilities recovered from dH against the float64
    softmax; a dropped low-order product in the backward's S moves p by e^2."""
    dO, dQ, dK, dH = (np.asarray(a, np.float64) for a in (dO, dQ, dK, dH))
    exp = backward_expect(fx)
    qs, ks, p, dSabs = exp["pairs"]
    worst = {}
    for name, got in (("dQ", dQ), ("dK", dK), ("dH", dH)):
        worst[name + "_loose"] = check_bound(got, exp[name][0], exp[name][1], 0.25, f"{what} {name} vs float64")
    n_q = np.bincount(ks, minlength=fx.N)  # live queries per key: 1, or 2 sharing one Q row
    assert n_q.min() >= 1 and n_q.max() <= 2
    two = (n_q == 2)[:, None]
    bound = np.where(two, 2.0 ** -20, 2.0 ** -21)
    # dH[k, :] = p * sum_q dO[q, :]
    base, babs = np.zeros_like(dH), np.zeros_like(dH)
    np.add.at(base, ks, dO[qs])
    np.add.at(babs, ks, np.abs(dO[qs]))
    p_key = np.zeros(fx.N)
    p_key[ks] = p
    terms = np.where(two, 1.25 * p_key[:, None] * babs, np.nan)
    worst["dH"], c = check_proportional(dH, base, bound, terms, f"{what} dH")
    worst["p_bwd"] = check_bound(c, p_key, p_key, 0.25, f"{what} probabilities recovered from dH")
    # dK[k, :] = (sum_q dS[q, k]) * Q[q, :]
    q_of_key = np.zeros(fx.N, np.int64)
    q_of_key[ks] = qs
    dS_terms = np.zeros(fx.N)
    np.add.at(dS_terms, ks, dSabs)
    Qk = fx.Q[q_of_key].astype(np.float64)
    terms = np.where(two, 1.25 * dS_terms[:, None] * np.abs(Qk), np.nan)
    worst["dK"], _ = check_proportional(dK, Qk, bound, terms, f"{what} dK")
    # dQ[q, :] = dS * K[k*, :] on hard rows
    hard = (fx.kind == 0)[:, None]
    worst["dQ_hard"], _ = check_proportional(np.where(hard, dQ, 0.0), fx.K[fx.kstar], 2.0 ** -21, None,
                                             f"{what} dQ hard rows")
    # soft-pair rows: dQ[q, :] = dS_r K[r, :] + dS_w K[w, :], and the two keys share their t2 coordinates (and the
    # zero padding): there dQ[q, d] = (dS_r + dS_w) K[w, d], two products in one accumulator
    soft = fx.kind == 1
    r = np.where(soft, fx.runner, fx.kstar)
    shared = soft[:, None] & (fx.K[r] == fx.K[fx.kstar])
    dS_q = np.zeros(fx.N)
    np.add.at(dS_q, qs, dSabs)
    Kw = np.where(shared, fx.K[fx.kstar], 0.0).astype(np.float64)
    terms = 1.25 * dS_q[:, None] * np.abs(Kw)
    worst["dQ_soft"], _ = check_proportional(np.where(shared, dQ, 0.0), Kw, 2.0 ** -20, terms,
                                             f"{what} dQ soft-pair rows, shared coordinates")
    return worst


def backward_restated(fx: FewHot, onorm, rmax, rsum, s_order=ORDER, ph_order=ORDER, sk_order=ORDER):
    """The x6 backward on the live pairs in fp32 numpy: base-2 scores,
    lse2 = rmax log2(e) + log2(rsum), p = 2^(s - lse2), dP by the six
    products, dS = p (dP - D), and dQ / dK / dH by the six products of each
    live pair, one accumulator per output row (winner first).  s_order /
    ph_order / sk_order: the products of S, of p.dO and of dS.K / dS.Q.
    Returns (dO, dQ, dK, dH) as fp32."""
    f32 = np.float32
    qs, ks = live_pairs(fx)  # winners' pairs, then runners-up's
    dO = (fx.dout * fx.gamma).astype(f32)
    D = (dO * onorm).astype(f32).sum(1, dtype=f32)
    Q2 = (fx.Q * f32(1.44269504088896341)).astype(f32)
    s = np.zeros(len(qs), f32)
    for d in range(fx.dk):
        s = six_product(Q2[qs, d], fx.K[ks, d], s_order, s)
    lse2 = (rmax.astype(np.float64) * 1.44269504088896341 + np.log2(rsum.astype(np.float64))).astype(f32)
    p = np.exp2((s - lse2[qs]).astype(f32)).astype(f32)
    dP = np.zeros(len(qs), f32)
    for f in range(fx.dv):
        dP = six_product(dO[qs, f], fx.H[ks, f], ORDER, dP)
    dS = (p * (dP - D[qs]).astype(f32)).astype(f32)
    outs = []
    for rows, w, vec, o in ((qs, dS, fx.K[ks], sk_order), (ks, dS, fx.Q[qs], sk_order), (ks, p, dO[qs], ph_order)):
        acc = np.zeros((fx.N, vec.shape[1]), f32)
        first = np.zeros(len(rows), bool)
        first[np.unique(rows, return_index=True)[1]] = True  # each row's first pair, then its second
        for sel in (first, ~first):
            acc[rows[sel]] = six_product(w[sel, None], vec[sel], o, acc[rows[sel]])
        outs.append(acc)
    return (dO, *outs)
