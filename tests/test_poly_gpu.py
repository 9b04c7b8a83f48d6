"""GPU parity: EvaluationDomain transforms, eval_polynomial, kate_division, batch_invert vs the oracle."""
import functools

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import poly as OP
from tests.util import random_scalars

pytestmark = pytest.mark.gpu
P = B.R_MOD


@pytest.mark.parametrize("j,k", [(3, 3), (3, 5), (2, 4), (4, 6), (9, 7), (3, 11), (5, 12), (17, 5), (18, 5), (18, 6)])
def test_domain_transforms(ctx, j, k):
    from sha2_on_cq_halo2_amd import EvaluationDomain

    od = OP.EvaluationDomain(j, k)
    gd = EvaluationDomain(ctx, j, k)
    assert gd.extended_k == od.extended_k
    cs = gd.constants()
    assert B.from_mont_limbs(cs["omega"])[0] == od.omega
    assert B.from_mont_limbs(cs["omega_inv"])[0] == od.omega_inv
    assert B.from_mont_limbs(cs["extended_omega"])[0] == od.extended_omega
    a = random_scalars(od.n, 100 * j + k)
    coeff = od.lagrange_to_coeff(a)
    assert np.array_equal(gd.lagrange_to_coeff(B.to_mont_limbs(a)), B.to_mont_limbs(coeff))
    ext = od.coeff_to_extended(coeff)
    assert np.array_equal(gd.coeff_to_extended(B.to_mont_limbs(coeff)), B.to_mont_limbs(ext))
    e = random_scalars(od.extended_len, 7 * j + k)
    back = od.extended_to_coeff(e)
    assert np.array_equal(gd.extended_to_coeff(B.to_mont_limbs(e)), B.to_mont_limbs(back))


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 4096, 4097, 70000])
def test_eval_polynomial(ctx, n):
    poly = random_scalars(n, n + 1)
    x = random_scalars(1, 9)[0]
    got = ctx.eval_polynomial(B.to_mont_limbs(poly) if n else np.zeros((0, 4), dtype=np.uint64), B.to_mont_limbs([x])[0])
    assert B.from_mont_limbs(got)[0] == OP.eval_polynomial(poly, x)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129, 4096, 4100, 70000])
def test_kate_division(ctx, n):
    a = random_scalars(n, n + 5)
    z = random_scalars(1, 11)[0]
    got = ctx.kate_division(B.to_mont_limbs(a), B.to_mont_limbs([z])[0])
    exp = OP.kate_division(a, z)
    assert got.shape[0] == n - 1
    if n > 1:
        assert np.array_equal(got, B.to_mont_limbs(exp))


def test_kate_division_at_zero(ctx):
    a = random_scalars(300, 1)
    got = ctx.kate_division(B.to_mont_limbs(a), B.to_mont_limbs([0])[0])
    assert np.array_equal(got, B.to_mont_limbs(a[1:]))


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 1000, 5000])
def test_batch_invert(ctx, n):
    a = random_scalars(n, n + 2)
    for i in range(0, n, 5):
        a[i] = 0
    got = ctx.batch_invert(B.to_mont_limbs(a) if n else np.zeros((0, 4), dtype=np.uint64))
    if n:
        assert np.array_equal(got, B.to_mont_limbs(OP.batch_invert(a)))


@pytest.mark.parametrize("n", [300_001, 400_003, 3_200_001])  # 4, 8 and 16 elements per lane (poly_batch_invert's choice by size)
def test_batch_invert_large_arrays_every_lane_count(ctx, n):
    """Size-independent check at sizes the big-int oracle does not loop over: the words are a R mod p for some a, so the
    result words must be R^2 / w mod p -- compared on a sample of rows, the first and the last block included; zeros stay
    zero (ff::BatchInvert, arithmetic/curves' `batch_invert` call sites poly.rs:192,232)."""
    rs = np.random.RandomState(n & 0xFFFF)
    w = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    w[::7] = 0
    got = ctx.batch_invert(w.copy())
    assert got.shape == w.shape and not got[::7].any()
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(n - 40, n), rs.randint(0, n, size=1500)]))
    r2 = pow(2, 512, B.R_MOD)
    for i in rows:
        x = sum(int(w[i, q]) << (64 * q) for q in range(4))
        y = sum(int(got[i, q]) << (64 * q) for q in range(4))
        assert y == (r2 * pow(x, -1, B.R_MOD) % B.R_MOD if x else 0), i


# ---- kate_division / eval_polynomial at every dispatch threshold, against the C oracle ------------------------------------
def _root_of_unity(log_order):
    w = B.FR_ROOT_OF_UNITY
    for _ in range(log_order, B.FR_S):
        w = w * w % P
    return w


def _mont(v):
    return B.to_mont_limbs([v % P])[0]


def _int(limbs):
    return B.from_mont_limbs(np.asarray(limbs, dtype=np.uint64).reshape(1, 4))[0]


def _full_range_coeffs(n, seed):
    """n Montgomery words over the whole range below r (tests/util.py full_range_words, without its per-row Python loop:
    these arrays reach 2^24 rows), with zeros, r - 1 and words whose lower eight 29-bit limbs are all ones among them --
    at both ends, so the leading coefficient is r - 1 and the one below it zero."""
    rs = np.random.RandomState(seed)
    a = np.frombuffer(rs.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] %= np.uint64(P >> 192)  # below r's top word: below r
    ones = ((5 << 232) + (1 << 232) - 1)
    a[[0, n // 2, n - 1]] = _mont(P - 1)
    a[[1, n // 3, n - 2]] = 0
    a[[2, n // 5, n - 3]] = np.array([(ones >> (64 * q)) & ((1 << 64) - 1) for q in range(4)], dtype=np.uint64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=1)
def _kate_coeffs(n):
    return _full_range_coeffs(n, n & 0xFFFF)


KATE_SIZES = [4095,             # recursive path, three levels
              4096,             # smallest block-path size: E = 4, 4 blocks
              (1 << 17) + 1,    # 129 blocks, 256 scan threads, one coefficient in the last block
              (1 << 18) + 1,    # 257 blocks, 512 scan threads
              (1 << 19) + 3,    # 513 blocks, 1024 scan threads
              1 << 20,          # E = 4, 1024 blocks exactly
              (1 << 20) + 1,    # E = 8, 513 blocks
              (1 << 21) + 1,    # E = 16, 513 blocks
              1 << 22,          # E = 16, 1024 blocks
              (1 << 22) + 1]    # back to the recursion, six levels


@pytest.mark.parametrize("n", KATE_SIZES)
def test_kate_division_dispatch_thresholds_match_c_oracle(ctx, n):
    """poly_kate_division picks 4, 8 or 16 coefficients per thread and 64 .. 1024 carry-scan threads by size, and
    the recursion below 4096 and above 2^22: every choice, with a partial last block, element for element."""
    from oracle import cbind as OC

    a = _kate_coeffs(n)
    z = _mont(B.fr_random(B.Xoshiro256ss(n)))
    got = ctx.kate_division(a, z)
    assert got.shape == (n - 1, 4)
    assert np.array_equal(got, OC.kate_division(a, z))


SPECIAL_POINTS = {"zero": 0, "one": 1, "minus-one": P - 1, "4th-root": _root_of_unity(2), "1024th-root": _root_of_unity(10)}


@pytest.mark.parametrize("name", list(SPECIAL_POINTS))
def test_kate_division_special_points_on_the_block_path(ctx, name):
    """n = 2^18 + 1 (E = 4, 257 blocks): z = 0 (every multiplier vanishes), z = 1 and r - 1, a primitive 4th root of unity
    (z^E = 1: the in-block scan's multiplier is one) and a primitive 1024th root (z^(256 E) = 1: the carry scan's is)."""
    from oracle import cbind as OC

    n = (1 << 18) + 1
    z = SPECIAL_POINTS[name]
    if name == "4th-root":
        assert pow(z, 4, P) == 1 and pow(z, 2, P) != 1
    if name == "1024th-root":
        assert pow(z, 1024, P) == 1 and pow(z, 512, P) != 1
    a = _kate_coeffs(n)
    got = ctx.kate_division(a, _mont(z))
    assert np.array_equal(got, OC.kate_division(a, _mont(z)))
    if z == 0:
        assert np.array_equal(got, a[1:])


def test_kate_division_quotient_identity(ctx):
    """Independent of the oracle's division: q(x) (x - z) + a(z) = a(x) at a random x (n = 2^19 + 3: 513 blocks)."""
    from oracle import cbind as OC

    n = (1 << 19) + 3
    a = _kate_coeffs(n)
    rng = B.Xoshiro256ss(0x4B415445)
    z, x = B.fr_random(rng), B.fr_random(rng)
    q = ctx.kate_division(a, _mont(z))
    ev = lambda poly, pt: _int(OC.eval_polynomial(poly, _mont(pt)))
    assert (ev(q, x) * (x - z) + ev(a, z)) % P == ev(a, x)


@pytest.fixture(scope="module")
def eval_coeffs():
    return _full_range_coeffs(4096 * 4096 + 1, 4096)


@pytest.mark.parametrize("n", [4095, 4096 * 4096, 4096 * 4096 + 1], ids=["4095", "4096^2", "4096^2+1"])
def test_eval_polynomial_level_boundaries_match_c_oracle(ctx, eval_coeffs, n):
    """A level folds EVAL_TILE = 4096 coefficients per block: one partial block, two full levels, and the first size
    with three (4097 -> 2 -> 1 blocks).  The leading coefficient of the longest input is r - 1, alone in its block."""
    from oracle import cbind as OC

    a = eval_coeffs[:n]
    x = _mont(B.fr_random(B.Xoshiro256ss(n)))
    assert np.array_equal(ctx.eval_polynomial(a, x), OC.eval_polynomial(a, x))
