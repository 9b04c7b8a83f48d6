"""Reference by known discrete logs for the G1 transforms of the setup path (`csrc/g1fft.hip`): `g_to_lagrange`, the FK
construction of the CQ cached quotients and `StaticTableValues::new`.  Plain Python integers mod r, no GPU.

Every input point is `a_j G` with a KNOWN scalar `a_j` (0 is the identity, encoded (0, 0)).  The transforms are linear in
the points, so every expected output is `e_i G` with `e_i` computed in Fr -- which allows inputs a real SRS `[s^j] G` never
produces: equal points, opposite points, identities, and sums that cancel inside a butterfly.

  g_to_lagrange (arithmetic.rs:277-301):     e_i = n^-1 sum_j w^(-i (j + shift)) a_j
  StaticTableValues::new (static_lookup.rs:78-126) and its FK form:
                                             Q_i = (w^i / N) sum_m q_m^(i) a_m,   q^(i) = (T(X) - T(w^i)) / (X - w^i)

The quotient is evaluated root by root (the Kate quotient's coefficients folded into one recurrence); the FK convolution
is NOT restated here.  Expected bytes come from the C oracle's scalar multiplication of the generator.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import bn254 as B
from oracle.poly import EvaluationDomain, best_fft

P = B.R_MOD


@functools.lru_cache(maxsize=None)
def omega(k: int) -> int:
    """The 2^k-th root of unity of the reference's domains (poly/domain.rs:56-66)."""
    return EvaluationDomain(2, k).omega


# ---- input families: n = 2^k scalars each ------------------------------------------------------------------------
def _rand(k, seed, count):
    rng = B.Xoshiro256ss(0x6731 + 131 * k + seed)
    return [B.fr_random(rng) for _ in range(count)]


def fam_random(k):
    return _rand(k, 1, 1 << k)


def fam_same(k):
    return [1] * (1 << k)


def fam_character(k, r):
    """a_j = w^(r j): an eigenvector of every sub-transform, so every butterfly of every stage sees u = 0 = w t or
    u = +-w t; the output is G at index r and the identity elsewhere."""
    w = pow(omega(k), r, P)
    out, cur = [], 1
    for _ in range(1 << k):
        out.append(cur)
        cur = cur * w % P
    return out


def fam_two_characters(k):
    """w^j + 3 w^((1 + n/2) j).  Both terms are the same character of every smaller sub-transform, so the early stages
    are doublings and cancellations; in the last stage they meet in one butterfly with opposite signs, u = 4 X against
    w t = -2 X, a generic addition next to identity + identity pairs.  (With equal weights the odd entries vanish and
    no butterfly is generic.)  The output is G at 1, 3 G at 1 + n/2 and the identity elsewhere."""
    n = 1 << k
    return [(x + 3 * y) % P for x, y in zip(fam_character(k, 1 % n), fam_character(k, (1 + n // 2) % n))]


def fam_delta(k, j0):
    a = [0] * (1 << k)
    a[j0] = 1
    return a


def fam_zero(k):
    return [0] * (1 << k)


def _half_mirror(k, seed, sign):
    n = 1 << k
    if n == 1:  # a_0 = sign * a_0
        return _rand(k, seed, 1) if sign == 1 else [0]
    h = _rand(k, seed, n // 2)
    return h + [sign * v % P for v in h]


def fam_antisym(k):
    return _half_mirror(k, 2, -1)


def fam_sym(k):
    return _half_mirror(k, 3, 1)


def fam_sparse_mix(k):
    """Random scalars, one third of them zero, and a third of the rest repeats of an earlier entry (or its negative)."""
    n = 1 << k
    rs = np.random.RandomState(900 + k)
    base = _rand(k, 4, n)
    out = []
    for j in range(n):
        kind = int(rs.randint(0, 9))
        if kind < 3:
            out.append(0)
        elif kind < 5 and out:
            v = out[int(rs.randint(0, len(out)))]
            out.append(v if kind == 3 else (-v) % P)
        else:
            out.append(base[j])
    return out


def character_params(k):
    n = 1 << k
    return sorted({r for r in (1, n // 2 - 1, n - 1) if 0 <= r < n})


def delta_params(k):
    n = 1 << k
    return sorted({j for j in (0, 1, n - 1) if 0 <= j < n})


def family_cases(k):
    """[(id, scalars)] of every family at size 2^k; the parameters a size does not have are left out, no family is."""
    cases = [("random", fam_random(k)), ("same", fam_same(k))]
    cases += [("character(%d)" % r, fam_character(k, r)) for r in character_params(k)]
    cases.append(("two_characters", fam_two_characters(k)))
    cases += [("delta(%d)" % j, fam_delta(k, j)) for j in delta_params(k)]
    cases += [("zero", fam_zero(k)), ("antisym", fam_antisym(k)), ("sym", fam_sym(k)), ("sparse_mix", fam_sparse_mix(k))]
    return cases


FAMILY_IDS = ["random", "same", "character", "two_characters", "delta", "zero", "antisym", "sym", "sparse_mix"]


def family(name: str, k: int):
    """[(id, scalars)] of one family (all its parameters) at size 2^k."""
    return [(i, a) for i, a in family_cases(k) if i.split("(")[0] == name]


# ---- table value sets (distinct values) --------------------------------------------------------------------------
def values_range(N):
    """Holds 0: T(w^0) = 0, a zero entry in FFT_2N of the reversed coefficients."""
    return list(range(N))


def values_monomial(N, shuffled: bool):
    """c w^i.  In natural order T = c X: the FK convolution has a single non-identity term and DFT_N runs on a delta.
    Shuffled: the same values, a generic T."""
    k = N.bit_length() - 1
    c = _rand(k, 5, 1)[0]
    v = [c * x % P for x in fam_character(k, 1 % N)]
    if shuffled:
        v = [v[i] for i in np.random.RandomState(77 + N).permutation(N)]
    return v


def values_random(N):
    k = N.bit_length() - 1
    v = list(dict.fromkeys(_rand(k, 6, N + 8)))[:N]
    assert len(v) == N
    return v


VALUE_SETS = {"range": values_range, "monomial": lambda N: values_monomial(N, False),
              "monomial_shuffled": lambda N: values_monomial(N, True), "random": values_random}


# ---- the scalar models ---------------------------------------------------------------------------------------------
def lagrange_scalars(a, k: int, shift: int = 0):
    """e_i = n^-1 sum_j w^(-i (j + shift)) a_j for the n-point array [0 x shift | a | 0 ...] (an FFT over Fr)."""
    n = 1 << k
    assert shift + len(a) <= n
    buf = [0] * shift + [v % P for v in a] + [0] * (n - shift - len(a))
    best_fft(buf, B.inv_mod(omega(k), P), k)
    n_inv = B.inv_mod(n % P, P)
    return [v * n_inv % P for v in buf]


def lagrange_scalars_direct(a, k: int, shift: int = 0):
    """The same sum, term by term (O(n^2): small sizes, the check of the FFT form)."""
    n = 1 << k
    w_inv = B.inv_mod(omega(k), P)
    n_inv = B.inv_mod(n % P, P)
    return [sum(pow(w_inv, i * (j + shift) % n, P) * v for j, v in enumerate(a)) % P * n_inv % P for i in range(n)]


def quotient_scalars(values, a):
    """Q_i = (w^i / N) sum_m q_m^(i) a_m with q^(i) the Kate quotient of T at w^i, T(w^i) = values[i].  With
    q_m = sum_{l > m} c_l x^(l-1-m):  sum_m q_m a_m = sum_l c_l A_l,  A_0 = 0,  A_{l+1} = x A_l + a_l."""
    N = len(values)
    k = N.bit_length() - 1
    assert N == 1 << k and len(a) == N
    c = EvaluationDomain(2, k).lagrange_to_coeff(values)
    n_inv = B.inv_mod(N % P, P)
    out = []
    x = 1
    w = omega(k)
    for _ in range(N):
        A, dot = 0, 0
        for cl, al in zip(c, a):
            dot += cl * A
            A = (x * A + al) % P
        out.append(dot % P * x % P * n_inv % P)
        x = x * w % P
    return out


def closed_form_quotient_scalars(values, s: int):
    """`StaticTableValues.qs_closed_form` (oracle/kzg.py) in Fr: (T(s) - T(w^i)) / (s - w^i) * w^i / N."""
    from oracle.poly import batch_invert, eval_polynomial

    N = len(values)
    k = N.bit_length() - 1
    ts = eval_polynomial(EvaluationDomain(2, k).lagrange_to_coeff(values), s)
    n_inv = B.inv_mod(N % P, P)
    roots = fam_character(k, 1 % N)
    inv = batch_invert([(s - g) % P for g in roots])
    return [(ts - v) % P * d % P * g % P * n_inv % P for v, d, g in zip(values, inv, roots)]


def dit_stages(a, k: int):
    """The radix-2 DIT stages of `best_fft` (arithmetic.rs:186-231) with w^-1, as g_to_lagrange runs them, on scalars:
    yields (stage, [(u, w t, twiddle exponent)]) for every butterfly, before the stage is applied."""
    n = 1 << k
    w_inv = B.inv_mod(omega(k), P)
    x = [v % P for v in a]
    for i in range(n):
        r = int(format(i, "0%db" % k)[::-1], 2) if k else 0
        if i < r:
            x[i], x[r] = x[r], x[i]
    for stage in range(k):
        half = 1 << stage
        m = half << 1
        flies = []
        for j in range(n // 2):
            pos = j & (half - 1)
            i0 = (j >> stage) * m + pos
            ex = pos * (n // m)
            flies.append((i0, i0 + half, x[i0], x[i0 + half] * pow(w_inv, ex, P) % P, ex))
        yield stage, [(u, wt, ex) for _, _, u, wt, ex in flies]
        for i0, i1, u, wt, _ in flies:
            x[i0], x[i1] = (u + wt) % P, (u - wt) % P


# ---- scalars -> points ---------------------------------------------------------------------------------------------
_GEN = None
_BYTES = {0: np.zeros(8, dtype=np.uint64)}


def point_bytes(scalars) -> np.ndarray:
    """uint64[n, 8]: the affine encoding of e G for every scalar, (0, 0) for e = 0 (C oracle: `cqo_g1_mul`, `cqo_g1_to_affine`)."""
    from oracle import cbind as OC

    global _GEN
    if _GEN is None:
        _GEN = B.points_to_mont_limbs([B.G1_GEN])[0]
    out = np.zeros((len(scalars), 8), dtype=np.uint64)
    todo = sorted({int(e) % P for e in scalars} - set(_BYTES))
    if todo:
        limbs = B.to_mont_limbs(todo)
        for e, m in zip(todo, limbs):
            _BYTES[e] = OC.g1_to_affine(OC.g1_mul(_GEN, m))
    for i, e in enumerate(scalars):
        out[i] = _BYTES[int(e) % P]
    return out


def points_affine(scalars):
    """The same points for the Python oracle: (x, y) or None."""
    return [None if e % P == 0 else B.g1_mul(B.G1_GEN, e % P) for e in scalars]
