"""[b_0] and [p] of a CQ lookup from per-table-row bucket sums ("b's commitments by table row").

b = 1 / (f + beta) takes one value per table row looked up and beta^-1 on the blinding rows, so the two n-term MSMs over
b's coefficients are MSMs of N + 1 terms over sums of per-row bases.  Checked here with the Python oracle alone, against
`msm(b0, b0_g1_bound)` and `msm(b0, g)` as oracle/cq_prover.py:402,406 compute them, in both forms:

  * with the row bases U_i = w^-i g_lagrange[i], V_i = w^-i B_i (B = g_to_lagrange of b0_g1_bound padded with the identity)
    and the fixed points C^U, C^V that carry the "- b(0)" of b_0 = (b - b(0)) / X;
  * with the shifted bases the library builds (cq.hpp: b_row_bases), g_to_lagrange of (identity, g[0 .. n-1)) and of
    (identity, b0_g1_bound): coefficient 0 of b meets the identity, so no b(0) term is left.
"""
import pytest

from oracle import bn254 as B
from oracle.bn254 import JAC_ID, R_MOD, batch_to_affine, fr_random, inv_mod, jac_add, jac_mul, jac_neg, jac_to_affine, to_jac
from oracle.kzg import ParamsKZG, g_to_lagrange
from oracle.poly import EvaluationDomain, best_multiexp

P = R_MOD


def _sum(points):
    acc = JAC_ID
    for p in points:
        acc = jac_add(acc, to_jac(p))
    return acc


def _lincomb(scalars, jacs):
    acc = JAC_ID
    for s, p in zip(scalars, jacs):
        acc = jac_add(acc, jac_mul(p, s))
    return acc


@pytest.mark.parametrize("k", [5, 6, 7])
def test_b0_and_p_from_bucket_sums(k):
    rng = B.Xoshiro256ss(100 + k)
    n, bf, N = 1 << k, 5, 8
    u = n - (bf + 1)
    params = ParamsKZG(k, fr_random(rng))
    tau = fr_random(rng)
    bound = batch_to_affine([jac_mul(to_jac(g), tau) for g in params.g[1:]])  # any n - 1 points
    dom = EvaluationDomain(4, k)

    table = [fr_random(rng) for _ in range(N)]
    # repeated rows (row 0 of the table takes most of them, as a padded witness does), table row 5 unused
    rows = [0 if i % 3 else (1, 2, 3, 4, 6, 7)[(i // 3) % 6] for i in range(u)]
    assert 5 not in rows and len(set(rows)) == N - 1
    m = [rows.count(j) for j in range(N)]
    beta = fr_random(rng)
    beta_inv = inv_mod(beta, P)
    f = [table[j] for j in rows]
    b = [inv_mod((fi + beta) % P, P) for fi in f] + [beta_inv] * (bf + 1)  # cq_prover.py:397-399
    b_poly = dom.lagrange_to_coeff(b)  # (a copy: ifft itself works in place, cq_prover.py:400)
    b0 = b_poly[1:]
    want_p = jac_to_affine(best_multiexp(b0, bound))          # cq_prover.py:402
    want_b0 = jac_to_affine(best_multiexp(b0 + [0], params.g))  # cq_prover.py:406

    a = [inv_mod((table[j] + beta) % P, P) if m[j] else 0 for j in range(N)]  # a'_j; empty buckets are skipped
    bucket = rows + [N] * (bf + 1)  # the blinding rows name the extra bucket
    scal = a + [beta_inv]

    def bucket_sums(bases):
        return [_sum(bases[i] for i in range(n) if bucket[i] == j) for j in range(N + 1)]

    # ---- U, V, C^U, C^V and the "- b(0) C" term ------------------------------------------------------------------
    w_inv = [pow(dom.omega_inv, i, P) for i in range(n)]
    U = batch_to_affine([jac_mul(to_jac(params.g_lagrange[i]), w_inv[i]) for i in range(n)])
    Bl = g_to_lagrange(list(bound) + [None], k)
    V = batch_to_affine([jac_mul(to_jac(Bl[i]), w_inv[i]) for i in range(n)])
    b_at_zero = (sum(m[j] * a[j] for j in range(N)) + (bf + 1) * beta_inv) % P * inv_mod(n, P) % P
    assert b_at_zero == b_poly[0]
    for bases, want in ((U, want_b0), (V, want_p)):
        S = bucket_sums(bases)
        assert S[5] == JAC_ID
        got = jac_add(_lincomb(scal, S), jac_neg(jac_mul(_sum(bases), b_at_zero)))
        assert jac_to_affine(got) == want

    # ---- the shifted bases: no b(0) term ------------------------------------------------------------------------------
    for src, want in ((params.g[: n - 1], want_b0), (bound, want_p)):
        bases = g_to_lagrange([None] + list(src), k)
        # directly: the commitment is linear in b's evaluations
        assert jac_to_affine(_lincomb(b, [to_jac(p) for p in bases])) == want
        S = bucket_sums(bases)
        assert S[5] == JAC_ID
        assert jac_to_affine(_lincomb(scal, S)) == want


def test_every_row_on_one_table_row():
    """The degenerate witness: one table row takes every usable row, so b takes two values."""
    k, bf, N = 5, 5, 8
    rng = B.Xoshiro256ss(7)
    n = 1 << k
    u = n - (bf + 1)
    params = ParamsKZG(k, fr_random(rng))
    dom = EvaluationDomain(4, k)
    t3, beta = fr_random(rng), fr_random(rng)
    beta_inv = inv_mod(beta, P)
    a3 = inv_mod((t3 + beta) % P, P)
    b = [a3] * u + [beta_inv] * (bf + 1)
    b0 = dom.lagrange_to_coeff(b)[1:]
    want = jac_to_affine(best_multiexp(b0 + [0], params.g))
    bases = g_to_lagrange([None] + list(params.g[: n - 1]), k)
    got = jac_add(jac_mul(_sum(bases[:u]), a3), jac_mul(_sum(bases[u:]), beta_inv))
    assert jac_to_affine(got) == want
