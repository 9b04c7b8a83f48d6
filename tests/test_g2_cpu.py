"""Host G2 helpers of the library (cq_g2_sum, cq_g2_to_affine) against [k]_2 of the C oracle: Jacobian inputs with
Z != 1, doubling, cancellation and identities."""
import numpy as np

from oracle import bn254 as B
from oracle import pairing as PR
from sha2_on_cq_halo2_amd._lib import load
from tests.g2_helpers import R, affine_from_limbs, g2_mul_limbs, jac_limbs

FQ2 = PR.FQ2


def _sum(lib, jacs):
    arr = np.ascontiguousarray(np.array(jacs, dtype=np.uint64).reshape(-1, 24))
    out = np.zeros(24, dtype=np.uint64)
    assert lib.cq_g2_sum(arr.ctypes.data, arr.shape[0], out.ctypes.data) == 0
    aff = np.zeros(16, dtype=np.uint64)
    assert lib.cq_g2_to_affine(out.ctypes.data, aff.ctypes.data) == 0
    return aff


def _pt(k):
    return affine_from_limbs(g2_mul_limbs(k))


def test_g2_sum_and_to_affine_match_oracle():
    lib = load()
    rng = B.Xoshiro256ss(0x62)
    ks = [B.fr_random(rng) for _ in range(5)]
    lams = [FQ2([B.fr_random(rng) + 1, B.fr_random(rng)]) for _ in range(5)]
    jacs = [jac_limbs(_pt(k), lam) for k, lam in zip(ks, lams)]
    got = _sum(lib, jacs)
    assert np.array_equal(got, g2_mul_limbs(sum(ks)))
    # one point alone: Jacobian -> affine with Z != 1
    assert np.array_equal(_sum(lib, jacs[:1]), g2_mul_limbs(ks[0]))


def test_g2_special_cases():
    lib = load()
    k = 0x1234567890ABCDEF1234567890ABCDEF
    p, q = _pt(k), _pt(R - k)
    lam1, lam2 = FQ2([3, 5]), FQ2([7, 11])
    # P + P (different representatives) -> [2k]_2
    assert np.array_equal(_sum(lib, [jac_limbs(p, lam1), jac_limbs(p, lam2)]), g2_mul_limbs(2 * k))
    # P + (-P) -> identity (all-zero affine)
    assert not _sum(lib, [jac_limbs(p, lam1), jac_limbs(q, lam2)]).any()
    # identity inputs on either side, and nothing at all
    ident = jac_limbs(None, None)
    assert np.array_equal(_sum(lib, [ident, jac_limbs(p, lam1), ident]), g2_mul_limbs(k))
    assert not _sum(lib, [ident]).any()
    out = np.zeros(24, dtype=np.uint64)
    assert lib.cq_g2_sum(out.ctypes.data, 0, out.ctypes.data) == 0 and not out.any()
    # the generator itself, [1]_2, against pairing.py's constant
    g = PR.G2_GEN
    assert affine_from_limbs(_sum(lib, [jac_limbs(g, lam2)])) == g
    assert PR.is_on_twist(affine_from_limbs(g2_mul_limbs(k)))


def test_g2_header_symbols_are_exported():
    from sha2_on_cq_halo2_amd._lib import header_symbols

    lib = load()
    for name in ("cq_best_multiexp_g2", "cq_best_multiexp_g2_dev", "cq_g2_sum", "cq_g2_to_affine", "cq_g2_srs_create",
                 "cq_g2_srs_setup_from_toxic_waste", "cq_g2_srs_download", "cq_g2_srs_destroy", "cq_static_table_commit"):
        assert name in header_symbols()
        assert hasattr(lib, name)
