"""Helpers of the G2 tests: limb conversions between the library's G2 layouts and oracle/pairing.py's FQ2 points, and
[k]_2 from the C oracle (cqo_g2_mul)."""
import numpy as np

from oracle import bn254 as B
from oracle import pairing as PR

Q = B.Q_MOD
R = B.R_MOD
_RINV = pow(1 << 256, -1, Q)


def _mont(v):
    v = v * (1 << 256) % Q
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]


def _unmont(limbs):
    return sum(int(limbs[j]) << (64 * j) for j in range(4)) * _RINV % Q


def fq2_limbs(a):
    return _mont(a.c[0]) + _mont(a.c[1])


def fq2_from_limbs(l8):
    return PR.FQ2([_unmont(l8[:4]), _unmont(l8[4:8])])


def affine_limbs(pt):
    """uint64[16] (x.c0, x.c1, y.c0, y.c1, Montgomery); None = identity = all zero"""
    if pt is None:
        return np.zeros(16, dtype=np.uint64)
    return np.array(fq2_limbs(pt[0]) + fq2_limbs(pt[1]), dtype=np.uint64)


def affine_from_limbs(a16):
    a16 = [int(v) for v in a16]
    if not any(a16):
        return None
    return (fq2_from_limbs(a16[:8]), fq2_from_limbs(a16[8:]))


def jac_limbs(pt, lam):
    """Jacobian (lam^2 x, lam^3 y, lam) of an affine FQ2 point, uint64[24]; None -> z = 0"""
    if pt is None:
        return np.zeros(24, dtype=np.uint64)
    l2 = lam * lam
    return np.array(fq2_limbs(pt[0] * l2) + fq2_limbs(pt[1] * l2 * lam) + fq2_limbs(lam), dtype=np.uint64)


def jac_to_affine_py(j24):
    """Python normalisation of a uint64[24] Jacobian point (independent of the library's)."""
    j24 = [int(v) for v in j24]
    z = fq2_from_limbs(j24[16:24])
    if z == PR.FQ2.zero():
        return None
    zi = z.inv()
    return (fq2_from_limbs(j24[:8]) * zi * zi, fq2_from_limbs(j24[8:16]) * zi * zi * zi)


def g2_mul_limbs(k):
    """[k]_2 as uint64[16] from the C oracle's cqo_g2_mul"""
    from oracle import cbind as OC

    k %= R
    kk = np.array([(k >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    OC.lib().cqo_g2_mul(kk.ctypes.data, out.ctypes.data)
    return out


def fr_mont(vals):
    """Montgomery limbs uint64[n,4] of Python ints (mod r)"""
    return B.to_mont_limbs([v % R for v in vals])
