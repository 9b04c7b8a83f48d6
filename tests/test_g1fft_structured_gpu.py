"""GPU parity of the G1 transforms of the setup path (`csrc/g1fft.hip`: `g1_fft`, `g1_to_lagrange`, `fk_table_quotients`)
and of `StaticTableValues::new` on STRUCTURED inputs, byte for byte against the reference by known discrete logs
(tests/g1_structured.py, checked on its own in tests/test_g1_structured_cpu.py).

A real SRS `[s^j] G` never sends a butterfly two equal or opposite points, an identity it did not pad itself, or a zero
scalar; the points `a_j G` of the families here do, in every stage (see the family table in g1_structured.py)."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle import kzg
from tests import g1_structured as S

pytestmark = pytest.mark.gpu
P = B.R_MOD


# k = 0 returns before the FFT; 1 is a single butterfly; <= 6 a partial 64-lane butterfly block, 7 exactly one; 8 and 9
# are one and two `g1_bitrev` blocks; 12 many blocks of both.
@pytest.mark.parametrize("k", [0, 1, 2, 5, 7, 8, 9, 12])
@pytest.mark.parametrize("name", S.FAMILY_IDS)
def test_g_to_lagrange_structured_points(ctx, name, k):
    cases = S.family(name, k)
    assert cases
    for cid, a in cases:
        got = ctx.g_to_lagrange(S.point_bytes(a), k)
        exp = S.point_bytes(S.lagrange_scalars(a, k))
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, "%s k=%d: %d of %d points differ, first at %s" % (cid, k, bad.size, 1 << k, bad[:8])


def test_g_to_lagrange_rejects_a_wrong_length(ctx):
    from sha2_on_cq_halo2_amd import CqError

    with pytest.raises(CqError):
        ctx.g_to_lagrange(S.point_bytes([1, 2, 3]), 2)


@pytest.mark.parametrize("k_big,k_small", [(6, 4), (11, 11)])
def test_params_downsize_matches_the_off_device_lagrange_basis(ctx, k_big, k_small):
    """`ParamsKZG::downsize` -> `g_to_lagrange`: the Lagrange basis equals n^-1 sum_j w^(-ij) s^j times G, the form the
    oracle's `ParamsKZG(k, s).g_lagrange` has, computed off the device (C oracle scalar multiplications)."""
    from sha2_on_cq_halo2_amd import ParamsKZG

    s = B.fr_random(B.Xoshiro256ss(77))
    big = ParamsKZG.setup_from_toxic_waste(ctx, k_big, B.to_mont_limbs([s])[0])
    g, gl = big.downsize(k_small).download()
    n = 1 << k_small
    powers = [pow(s, j, P) for j in range(n)]
    assert np.array_equal(g, S.point_bytes(powers))
    e = S.lagrange_scalars(powers, k_small)
    mult = (pow(s, n, P) - 1) * B.inv_mod(n, P) % P  # kzg._lagrange_g1: L_i(s) = (s^n - 1) / n * w^i / (s - w^i)
    roots = S.fam_character(k_small, 1 % n)
    assert e == [mult * rp % P * B.inv_mod((s - rp) % P, P) % P for rp in roots]
    assert np.array_equal(gl, S.point_bytes(e))
    if k_small <= 4:
        assert np.array_equal(gl, B.points_to_mont_limbs(kzg.ParamsKZG(k_small, s).g_lagrange))


SRS_FAMILIES = ["same", "sparse_mix", "antisym", "random", "zero"]


@pytest.fixture(scope="module")
def quotient_bytes():
    """Expected cached quotients per (N, srs family, value set), computed once."""
    cache = {}

    def get(N, fam, vset):
        key = (N, fam, vset)
        if key not in cache:
            k = N.bit_length() - 1
            (_, a), = S.family(fam, k)
            values = S.VALUE_SETS[vset](N)
            cache[key] = (S.point_bytes(a), B.to_mont_limbs(values), S.point_bytes(S.quotient_scalars(values, a)))
        return cache[key]

    return get


def _assert_qs(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d quotients differ, first at %s" % (what, bad.size, len(exp), bad[:8])


# the 2N-point FFT of the FK form has a partial butterfly block up to N = 32 and one full block at N = 64
@pytest.mark.parametrize("N", [2, 4, 32, 64, 128, 1024])
@pytest.mark.parametrize("vset", list(S.VALUE_SETS))
@pytest.mark.parametrize("fam", SRS_FAMILIES)
def test_static_table_fk_on_a_structured_srs(ctx, quotient_bytes, fam, vset, N):
    """`StaticTable.new_fk` over srs[j] = a_j G: `range` holds 0 (a zero scalar in the scale pass), `monomial` is T = c X
    (one non-identity convolution term, DFT_N of a delta), `monomial_shuffled` the same values as a generic T."""
    from sha2_on_cq_halo2_amd import StaticTable

    srs, vm, exp = quotient_bytes(N, fam, vset)
    _assert_qs(StaticTable.new_fk(ctx, vm, srs).download_qs(), exp, "new_fk %s/%s N=%d" % (fam, vset, N))


@pytest.mark.parametrize("N", [2, 16, 64])
@pytest.mark.parametrize("vset", list(S.VALUE_SETS))
@pytest.mark.parametrize("fam", SRS_FAMILIES)
def test_static_table_new_on_a_structured_srs(ctx, quotient_bytes, fam, vset, N):
    """The O(N^2) construction (`StaticTableValues::new`: one MSM per root) over the same inputs."""
    from sha2_on_cq_halo2_amd import StaticTable

    srs, vm, exp = quotient_bytes(N, fam, vset)
    _assert_qs(StaticTable.new(ctx, vm, srs).download_qs(), exp, "new %s/%s N=%d" % (fam, vset, N))


@pytest.mark.parametrize("N", [256, 4096])
@pytest.mark.parametrize("vset", ["range", "monomial", "monomial_shuffled"])
def test_static_table_fk_structured_values_on_a_real_srs(ctx, vset, N):
    """A real SRS [s^j] G with the structured value sets, against `StaticTableValues.qs_closed_form` evaluated in Fr and
    finished with the C oracle's scalar multiplications: an off-device reference at the large sizes."""
    from sha2_on_cq_halo2_amd import ParamsKZG, StaticTable

    s = B.fr_random(B.Xoshiro256ss(31 + N))
    values = S.VALUE_SETS[vset](N)
    srs = ParamsKZG.setup_from_toxic_waste(ctx, N.bit_length() - 1, B.to_mont_limbs([s])[0]).download()[0][:N]
    exp = S.point_bytes(S.closed_form_quotient_scalars(values, s))
    _assert_qs(StaticTable.new_fk(ctx, B.to_mont_limbs(values), srs).download_qs(), exp, "new_fk real srs %s N=%d" % (vset, N))
    if N == 256:  # the closed form in Fr is the oracle's, point for point (Python scalar multiplications)
        assert np.array_equal(exp, B.points_to_mont_limbs(kzg.StaticTableValues.qs_closed_form(values, s)))
