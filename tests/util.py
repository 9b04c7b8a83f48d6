"""Shared helpers for the parity tests (seeded synthetic inputs)."""
import numpy as np

from oracle import bn254 as B


def random_points(n, seed):
    """n pseudo-random G1 points: P_i = (a + i*b) * G built with additions only."""
    rng = B.Xoshiro256ss(seed)
    base = B.jac_mul(B.to_jac(B.G1_GEN), B.fr_random(rng))
    step = B.jac_mul(B.to_jac(B.G1_GEN), B.fr_random(rng))
    out = []
    cur = base
    for _ in range(n):
        out.append(cur)
        cur = B.jac_add(cur, step)
    return B.batch_to_affine(out)


def random_scalars(n, seed):
    rng = B.Xoshiro256ss(seed)
    return [B.fr_random(rng) for _ in range(n)]


def jac_limbs_to_affine(arr12):
    return B.jac_from_mont_limbs(np.asarray(arr12, dtype=np.uint64).reshape(1, 12))[0]


def full_range_words(n, seed):
    """n Montgomery words (uint64[n, 4]) over the whole range below r, not just below 2^252: uniform ones, then a block of
    r - 1 and a block whose lower eight 29-bit limbs are all 2^29 - 1 (the kernels read these words directly as lazy limbs)"""
    rs = np.random.RandomState(seed)
    r3 = B.R_MOD >> 192
    a = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    a[:, 3] = rs.randint(0, r3, size=n).astype(np.uint64)  # below r's top word: below r
    blk = max(1, n // 16)
    a[n // 4:n // 4 + blk] = B.to_mont_limbs([B.R_MOD - 1])[0]
    low = (1 << 232) - 1
    tops = rs.randint(0, B.R_MOD >> 232, size=blk)
    a[n // 2:n // 2 + blk] = np.array([[((int(t) << 232) + low) >> (64 * q) & ((1 << 64) - 1) for q in range(4)] for t in tops], dtype=np.uint64)
    return a
