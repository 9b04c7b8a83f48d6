"""The three EvaluationDomain transforms (poly/domain.rs:238-315) at any size, composed from the C oracle's exported
primitives, so that the fused GPU passes can be compared element for element at sizes the big-int oracle does not loop
over.  Every domain constant comes from oracle.poly.EvaluationDomain (domain.rs:39-142), never from the library under
test; tests/test_oracle_c.py holds this composition to that class's own three methods at small sizes.

Arrays are uint64[n, 4] Montgomery words, in and out."""
import numpy as np

from oracle import bn254 as B
from oracle import cbind as OC
from oracle import poly as OP

P = B.R_MOD


def mont(v):
    return B.to_mont_limbs([v % P])[0]


def omega_of(log_n):
    """The primitive 2^log_n-th root of unity `EvaluationDomain::new` derives (domain.rs:59-61)."""
    w = B.FR_ROOT_OF_UNITY
    for _ in range(log_n, B.FR_S):
        w = w * w % P
    return w


def grid(max_ek=21):
    """The (j, k) pairs of the fused-transform sweep, by extended size 2^ek: j = 2 is ext == n (no padding, no truncation),
    j = 3 pads only, j = 4 stores 3n of 4n rows, j = 7 stores 6n of 8n; j = 6 and 8 (5n and 7n of 8n) at four sizes whose
    last pass is 4, 5 and 6 bits wide; (17, 3) has 8 live rows in a domain of 128, so whole tiles load only padding."""
    out = []
    for ek in range(1, max_ek + 1):
        for j, k in ((2, ek), (3, ek - 1), (4, ek - 2), (7, ek - 3)):
            if k >= 0:
                out.append((j, k))
        if ek in (12, 17, 18, 21):
            out += [(6, ek - 3), (8, ek - 3)]
    for jk in ((2, 0), (3, 0), (2, 1), (17, 3)):
        if jk not in out and OP.EvaluationDomain(*jk).extended_k <= max_ek:
            out.append(jk)
    return out


class DomainModel:
    def __init__(self, j, k):
        self.od = od = OP.EvaluationDomain(j, k)
        self.j, self.k, self.n = j, k, od.n
        self.extended_k, self.ext = od.extended_k, od.extended_len
        self.out_len = od.n * od.quotient_poly_degree

    def lagrange_to_coeff(self, a):
        """domain.rs:238-248"""
        assert a.shape == (self.n, 4)
        od = self.od
        return OC.ifft(a, mont(od.omega_inv), self.k, mont(od.ifft_divisor))

    def coeff_to_extended(self, a):
        """domain.rs:252-266"""
        assert a.shape == (self.n, 4)
        od = self.od
        e = np.zeros((self.ext, 4), dtype=np.uint64)
        e[:self.n] = OC.distribute_powers(a, mont(od.g_coset), mont(od.g_coset_inv))
        return OC.best_fft(e, mont(od.extended_omega), self.extended_k)

    def extended_to_coeff(self, e):
        """domain.rs:293-315"""
        assert e.shape == (self.ext, 4)
        od = self.od
        c = OC.ifft(e, mont(od.extended_omega_inv), self.extended_k, mont(od.extended_ifft_divisor))
        return OC.distribute_powers(c, mont(od.g_coset_inv), mont(od.g_coset))[:self.out_len]
