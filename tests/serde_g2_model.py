"""Big-integer model of the G2 side of the on-disk formats (test infrastructure; nothing here touches the code under test).

  * `fq2_sqrt`: `Fq2::sqrt` restated literally as the reference has it (bn256/fq2.rs:344-398, Algorithm 9 of eprint
    2012/685) -- the same exponents, the same order of operations -- so that WHICH of the two roots comes back is pinned.
    That matters in one case only: a root with c0 == 0 (both roots then have parity 0), which is what a real non-residue
    operand has; everywhere else the parity rule of `from_bytes` decides.
  * `g2_to_bytes` / `g2_from_bytes`: `GroupEncoding` for G2Affine (derive/curve.rs:603-646, compressed size 64): the
    canonical x.c0 | x.c1 little-endian (`Fq2::to_bytes`, fq2.rs:134-155), bit 7 of byte 63 = parity of the canonical y.c0,
    64 zero bytes = identity; no subgroup check.
  * transcoders raw -> Processed for point arrays and for the complete `ParamsKZG` stream
    (k:u32 LE | n g | n g_lagrange | g2 | s_g2, kzg/commitment.rs:366-459), in the style of tests/serde_processed_model.py.

Points are oracle/pairing.py's: (FQ2 x, FQ2 y) or None for the identity.
"""
from oracle import bn254 as B
from oracle import pairing as PR
from tests import serde_processed_model as SM

Q = B.Q_MOD
FQ2 = PR.FQ2
B2 = PR.B2
_QINV = pow(1 << 256, -1, Q)
EXP_Q_MINUS_3_OVER_4 = 0x0C19139CB84C680A6E14116DA060561765E05AA45A1C72A34F082305B61F3F51  # fq2.rs:351-358
EXP_Q_MINUS_1_OVER_2 = 0x183227397098D014DC2822DB40C0AC2ECBC0B548B438E5469E10460B6C3E7EA3  # fq2.rs:383-390
assert EXP_Q_MINUS_3_OVER_4 == (Q - 3) // 4 and EXP_Q_MINUS_1_OVER_2 == (Q - 1) // 2


def fq2_conj(a):
    """frobenius_map(1): (c0, c1) -> (c0, -c1)"""
    return FQ2([a.c[0], -a.c[1]])


def fq2_sqrt(a):
    """`Fq2::sqrt` (fq2.rs:344-398), step for step; None where the reference returns CtOption::none"""
    if a == FQ2.zero():
        return FQ2.zero()
    a1 = a ** EXP_Q_MINUS_3_OVER_4
    alpha = a1 * a1 * a
    a0 = fq2_conj(alpha) * alpha
    neg1 = FQ2([Q - 1, 0])
    if a0 == neg1:
        return None
    a1 = a1 * a
    if alpha == neg1:
        a1 = a1 * FQ2([0, 1])
    else:
        alpha = (alpha + FQ2.one()) ** EXP_Q_MINUS_1_OVER_2
        a1 = a1 * alpha
    return a1


def fq2_is_square(a):
    """by the norm's Legendre symbol (`Fq2::legendre`, fq2.rs:157-159)"""
    n = (a.c[0] * a.c[0] + a.c[1] * a.c[1]) % Q
    return n == 0 or pow(n, (Q - 1) // 2, Q) == 1


def apply_sign(y, ysign):
    """`conditional_select(&y, &-y, ysign ^ sign)` with sign the parity of the canonical y.c0 (curve.rs:615-619); None stays None"""
    if y is None:
        return None
    return -y if (ysign ^ (y.c[0] & 1)) else y


def decoded_y(a, ysign):
    """the y `from_bytes` ends with for x^3 + b' = a and the given sign bit; None when a is not a square"""
    return apply_sign(fq2_sqrt(a), ysign)


def fq2_to_bytes(a):
    return a.c[0].to_bytes(32, "little") + a.c[1].to_bytes(32, "little")


def g2_to_bytes(pt):
    if pt is None:
        return bytes(64)
    b = bytearray(fq2_to_bytes(pt[0]))
    b[63] |= (pt[1].c[0] & 1) << 7
    return bytes(b)


def g2_from_bytes(b):
    """raises ValueError where the reference returns CtOption::none"""
    assert len(b) == 64
    ysign = b[63] >> 7
    c0 = int.from_bytes(b[:32], "little")
    c1 = int.from_bytes(b[32:], "little") & ((1 << 255) - 1)
    if c0 >= Q or c1 >= Q:
        raise ValueError("x is not canonical")
    x = FQ2([c0, c1])
    if x == FQ2.zero() and not ysign:
        return None
    y = decoded_y(x * x * x + B2, ysign)
    if y is None:
        raise ValueError("x^3 + b' is not a square")
    return (x, y)


# ---- raw layout: x.c0 | x.c1 | y.c0 | y.c1, 32 B little-endian Montgomery words (R = 2^256) each -------------------------
def point_raw_to_affine(raw128):
    assert len(raw128) == 128
    m = [int.from_bytes(raw128[32 * i:32 * i + 32], "little") for i in range(4)]
    assert all(v < Q for v in m)
    if not any(m):
        return None
    c = [v * _QINV % Q for v in m]
    return (FQ2(c[:2]), FQ2(c[2:]))


def point_affine_to_raw(pt):
    if pt is None:
        return bytes(128)
    return b"".join((v * (1 << 256) % Q).to_bytes(32, "little") for v in pt[0].c + pt[1].c)


def points_raw_to_processed(raw):
    assert len(raw) % 128 == 0
    return b"".join(g2_to_bytes(point_raw_to_affine(raw[i:i + 128])) for i in range(0, len(raw), 128))


def params_full_raw_to_processed(raw):
    """k | n x 64 B g | n x 64 B g_lagrange | 128 B g2 | 128 B s_g2  ->  k | n x 32 B | n x 32 B | 64 B | 64 B"""
    k = int.from_bytes(raw[:4], "little")
    n = 1 << k
    assert len(raw) == 4 + 128 * n + 256
    return SM.params_raw_to_processed(raw[:4 + 128 * n]) + points_raw_to_processed(raw[4 + 128 * n:])
