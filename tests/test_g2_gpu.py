"""G2 on the GPU: best_multiexp over G2Affine, the G2 SRS of the table setup and StaticTableValues::commit, checked
against [k]_2 of the C oracle (cqo_g2_mul).  Bases with known discrete logs make every expected value a single [k]_2."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle.poly import EvaluationDomain
from sha2_on_cq_halo2_amd import CqError, G2Srs, StaticTable
from sha2_on_cq_halo2_amd._lib import load
from sha2_on_cq_halo2_amd.sha_circuit import small_to_mont, spread16
from tests.g2_helpers import R, affine_limbs, affine_from_limbs, fr_mont, g2_mul_limbs

pytestmark = pytest.mark.gpu

S_TOXIC = 0x2F5A7C3B1D9E8F60123456789ABCDEF0FEDCBA9876543210A5A5A5A55A5A5A5A % R


def _affine(jac24):
    out = np.zeros(16, dtype=np.uint64)
    j = np.ascontiguousarray(jac24, dtype=np.uint64)
    assert load().cq_g2_to_affine(j.ctypes.data, out.ctypes.data) == 0
    return out


def _s_limbs(s):
    return fr_mont([s])[0]


@pytest.fixture(scope="module")
def srs(ctx):
    """[s^i]_2 for i < 2^18 + 1 (the MSM's large case and the 2^16 tables)"""
    p = G2Srs.setup_from_toxic_waste(ctx, (1 << 18) + 1, _s_limbs(S_TOXIC))
    yield p
    p.close()


def _powers(s, n):
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * s % R
    return out


# ---- 1. G2 MSM ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 256])
def test_g2_msm_small_against_oracle(ctx, n):
    rng = B.Xoshiro256ss(0x6200 + n)
    e = [B.fr_random(rng) for _ in range(n)]
    k = [B.fr_random(rng) for _ in range(n)]
    for i, v in enumerate([0, 1, R - 1]):
        if i < n:
            k[i] = v
    bases = np.array([g2_mul_limbs(x) for x in e], dtype=np.uint64).reshape(n, 16)
    got = _affine(ctx.best_multiexp_g2(fr_mont(k) if n else np.zeros((0, 4), np.uint64), bases))
    assert np.array_equal(got, g2_mul_limbs(sum(a * b for a, b in zip(k, e))))


def test_g2_msm_special_bases(ctx):
    """an identity base, a repeated base, a P / -P pair that cancels, equal scalars throughout"""
    rng = B.Xoshiro256ss(0x62AA)
    e = [B.fr_random(rng) for _ in range(8)]
    e[2] = 0            # identity base
    e[5] = e[4]         # repeated base
    e[7] = R - e[6]     # -P
    bases = np.array([g2_mul_limbs(x) for x in e], dtype=np.uint64)
    assert not bases[2].any()
    for k in ([B.fr_random(rng) for _ in range(8)], [7] * 8, [1] * 8):
        got = _affine(ctx.best_multiexp_g2(fr_mont(k), bases))
        assert np.array_equal(got, g2_mul_limbs(sum(a * b for a, b in zip(k, e))))
    # the cancelling pair alone, with equal scalars: the identity
    got = ctx.best_multiexp_g2(fr_mont([3, 3]), bases[6:8])
    assert not _affine(got).any()


@pytest.mark.parametrize("n", [4099, 1 << 18])
def test_g2_msm_on_srs(ctx, srs, n):
    """bases [s^i]_2 (the SRS, itself checked below): expected [sum_i k_i s^i]_2"""
    rng = B.Xoshiro256ss(0x6240 + n)
    k = [B.fr_random(rng) for _ in range(n)]
    k[0], k[1], k[2] = 0, 1, R - 1
    sc = ctx.to_device(fr_mont(k))
    got = _affine(ctx.best_multiexp_g2_dev(sc, srs.dev, n))
    expect = sum(a * b for a, b in zip(k, _powers(S_TOXIC, n))) % R
    assert np.array_equal(got, g2_mul_limbs(expect))


def test_g2_msm_repeated_scalar_long_bucket(ctx, srs):
    """2^16 equal scalars: every window's entries fall in one bucket (the level tree's worst case)"""
    n = 1 << 16
    k = 0x1F2E3D4C5B6A79880123456789ABCDEF % R
    sc = ctx.to_device(fr_mont([k] * n))
    got = _affine(ctx.best_multiexp_g2_dev(sc, srs.dev, n))
    assert np.array_equal(got, g2_mul_limbs(k * sum(_powers(S_TOXIC, n))))


# ---- 2. G2 SRS ----------------------------------------------------------------------------------------------------
def test_g2_srs_powers(srs):
    pts = srs.download()
    count = pts.shape[0]
    rng = B.Xoshiro256ss(0x6250)
    idx = sorted({0, 1, 2, count - 1} | {int(B.fr_random(rng) % count) for _ in range(16)})
    for i in idx:
        assert np.array_equal(pts[i], g2_mul_limbs(pow(S_TOXIC, i, R))), i


def test_g2_srs_checked_create(ctx):
    pts = np.array([g2_mul_limbs(x) for x in (1, 2, 3)] + [np.zeros(16, np.uint64)], dtype=np.uint64)
    ok = G2Srs(ctx, pts, checked=True)
    assert np.array_equal(ok.download(), pts)
    ok.close()
    bad = pts.copy()
    bad[1, 9] ^= np.uint64(1 << 7)  # one limb flipped: off the twist
    with pytest.raises(CqError) as ei:
        G2Srs(ctx, bad, checked=True)
    assert ei.value.code == -1
    unchecked = G2Srs(ctx, bad, checked=False)  # not validated: stored as given
    assert np.array_equal(unchecked.download(), bad)
    unchecked.close()


# ---- 3. StaticTableValues::commit ---------------------------------------------------------------------------------
def _t_of_s(vals, s):
    """T(s) for T interpolating the SORTED values over the size-N domain: (s^N - 1)/N * sum_i v_i w^i / (s - w^i)"""
    vals = sorted(v % R for v in vals)
    n = len(vals)
    w = B.FR_ROOT_OF_UNITY
    for _ in range(n.bit_length() - 1, B.FR_S):
        w = w * w % R
    acc, wi = 0, 1
    dens = []
    for _ in range(n):
        dens.append((s - wi) % R)
        wi = wi * w % R
    # batch inversion
    pref, run = [], 1
    for d in dens:
        pref.append(run)
        run = run * d % R
    inv = pow(run, -1, R)
    wi_list = _powers(w, n)
    for i in range(n - 1, -1, -1):
        di = pref[i] * inv % R
        inv = inv * dens[i] % R
        acc = (acc + vals[i] * wi_list[i] * di) % R
    return (pow(s, n, R) - 1) * pow(n, -1, R) * acc % R


def test_barycentric_t_of_s_matches_lagrange_to_coeff():
    rng = B.Xoshiro256ss(0x6260)
    vals = [B.fr_random(rng) for _ in range(16)]
    coeffs = EvaluationDomain(2, 4).lagrange_to_coeff(sorted(vals))
    tv = 0
    for c in reversed(coeffs):
        tv = (tv * S_TOXIC + c) % R
    assert tv == _t_of_s(vals, S_TOXIC)


def _commit_and_check(ctx, srs_g2, vals_mont, vals_int, srs_g1_len, circuit_n, s):
    t = StaticTable.setup_from_toxic_waste(ctx, vals_mont, _s_limbs(s))
    try:
        zv, tc, xb = t.commit(srs_g2, srs_g1_len, circuit_n)
    finally:
        t.close()
    n = len(vals_int)
    assert np.array_equal(zv, g2_mul_limbs(pow(s, n, R) - 1))
    assert np.array_equal(xb, g2_mul_limbs(pow(s, srs_g1_len - 1 - (circuit_n - 2), R)))
    assert np.array_equal(tc, g2_mul_limbs(_t_of_s(vals_int, s)))


def test_commit_my_test_shape(ctx):
    """my_test.rs:160-195: N = 16, 16 G1 / 17 G2 points in the table SRS, circuit n = 8 -> x_b0_bound = [s^9]_2"""
    s = 0x5EED5EED % R
    g2 = G2Srs.setup_from_toxic_waste(ctx, 17, _s_limbs(s))
    vals = [(i * 7 + 3) % 16 * 1000 + 5 for i in range(16)]  # unique, not in ascending order
    _commit_and_check(ctx, g2, fr_mont(vals), vals, 16, 8, s)  # x_b0_bound index 16 - 1 - (8 - 2) = 9
    g2.close()


def test_commit_unsorted_random_table(ctx, srs):
    rng = B.Xoshiro256ss(0x6270)
    vals = list({B.fr_random(rng) for _ in range(1 << 10)})
    while len(vals) < 1 << 10:
        vals.append(B.fr_random(rng))
    _commit_and_check(ctx, srs, fr_mont(vals), vals, 1 << 10, 1 << 9, S_TOXIC)


@pytest.mark.parametrize("kind,log_n", [("dense", 12), ("spread", 12), ("spread", 16)])
def test_commit_workload_tables(ctx, srs, kind, log_n):
    idx = np.arange(1 << log_n, dtype=np.uint64)
    vals = idx if kind == "dense" else spread16(idx)
    ints = [int(v) for v in vals]
    _commit_and_check(ctx, srs, small_to_mont(vals), ints, 1 << log_n, 1 << 10, S_TOXIC)


# ---- 4. arguments -------------------------------------------------------------------------------------------------
def test_commit_rejects_short_srs_and_bad_index(ctx):
    s = 0x1234 % R
    vals = list(range(16))
    t = StaticTable.setup_from_toxic_waste(ctx, fr_mont(vals), _s_limbs(s))
    short = G2Srs.setup_from_toxic_waste(ctx, 16, _s_limbs(s))  # needs N + 1 = 17
    g2 = G2Srs.setup_from_toxic_waste(ctx, 17, _s_limbs(s))
    for srs_g2, g1_len, cn in [(short, 16, 8), (g2, 16, 1), (g2, 16, 0), (g2, 5, 8), (g2, 40, 8)]:
        with pytest.raises(CqError) as ei:
            t.commit(srs_g2, g1_len, cn)
        assert ei.value.code == -1
    # still usable afterwards
    zv, _, _ = t.commit(g2, 16, 8)
    assert np.array_equal(zv, g2_mul_limbs(pow(s, 16, R) - 1))
    for o in (t, short, g2):
        o.close()


def test_identity_helpers_roundtrip():
    assert affine_from_limbs(affine_limbs(None)) is None
