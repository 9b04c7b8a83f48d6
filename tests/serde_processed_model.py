"""Pure-Python transcoder RawBytes -> Processed for the serialized params and proving keys (test infrastructure).

`SerdeFormat::Processed` (helpers.rs:8-20) stores a G1 point as `CurveAffine::to_bytes` does -- the canonical x, little-endian,
with the parity of the canonical y in bit 7 of byte 31, 32 zero bytes for the identity (derive/curve.rs:635-646) -- and a
scalar as `to_repr`, the canonical value little-endian (helpers.rs:81-91).  The functions below take the raw streams
(Montgomery limbs; layouts of oracle/serde.py and of `ParamsKZG::write_custom`) apart with big-integer arithmetic alone and
re-emit them in that format.  Nothing here touches the code under test.
"""
import struct

from oracle import bn254 as B

Q, R = B.Q_MOD, B.R_MOD
_QINV = pow(1 << 256, -1, Q)
_RINV = pow(1 << 256, -1, R)


def point_raw_to_processed(raw64: bytes) -> bytes:
    """64 B raw Montgomery x || y  ->  32 B compressed"""
    assert len(raw64) == 64
    xm, ym = int.from_bytes(raw64[:32], "little"), int.from_bytes(raw64[32:], "little")
    assert xm < Q and ym < Q
    if xm == 0 and ym == 0:
        return bytes(32)
    x, y = xm * _QINV % Q, ym * _QINV % Q
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= (y & 1) << 7
    return bytes(b)


def point_raw_to_affine(raw64: bytes):
    """the oracle's point (None = identity) of 64 raw bytes"""
    xm, ym = int.from_bytes(raw64[:32], "little"), int.from_bytes(raw64[32:], "little")
    if xm == 0 and ym == 0:
        return None
    return (xm * _QINV % Q, ym * _QINV % Q)


def points_raw_to_processed(raw: bytes) -> bytes:
    assert len(raw) % 64 == 0
    return b"".join(point_raw_to_processed(raw[i:i + 64]) for i in range(0, len(raw), 64))


def scalar_raw_to_processed(raw32: bytes) -> bytes:
    m = int.from_bytes(raw32, "little")
    assert m < R
    return (m * _RINV % R).to_bytes(32, "little")


def scalars_raw_to_processed(raw: bytes) -> bytes:
    assert len(raw) % 32 == 0
    return b"".join(scalar_raw_to_processed(raw[i:i + 32]) for i in range(0, len(raw), 32))


def params_raw_to_processed(raw: bytes) -> bytes:
    """k:u32 LE | n x 64 B g | n x 64 B g_lagrange  ->  k | n x 32 B | n x 32 B  (the G1 part; a G2 tail is the caller's)"""
    k = int.from_bytes(raw[:4], "little")
    n = 1 << k
    assert len(raw) == 4 + 128 * n
    return raw[:4] + points_raw_to_processed(raw[4:])


class _Cursor:
    def __init__(self, data):
        self.d, self.o = data, 0

    def take(self, n):
        assert self.o + n <= len(self.d)
        out = self.d[self.o:self.o + n]
        self.o += n
        return out

    def be32(self):
        return struct.unpack(">I", self.take(4))[0]


def pk_raw_to_processed(raw: bytes, num_perm: int, num_selectors: int, layout=None) -> bytes:
    """The stream of oracle/serde.py proving_key_to_bytes: k:u32 BE | #fixed:u32 BE | commitments | selector bits | l0 | l_last |
    l_active_row | three slices of fixed polynomials | three slices of permutation polynomials.  `layout`, when a dict,
    receives the Processed-stream offsets the tests poke at: 'commitments' (offset of the first) and 'polys' (a list of
    (offset of the first scalar, length) per polynomial in stream order)."""
    c = _Cursor(raw)
    out = bytearray()
    k, nfix = c.be32(), c.be32()
    n = 1 << k
    out += struct.pack(">II", k, nfix)
    cm_off = len(out)
    out += points_raw_to_processed(c.take(64 * (nfix + num_perm)))
    out += c.take(num_selectors * ((n + 7) // 8))
    polys = []

    def poly():
        ln = c.be32()
        out.extend(struct.pack(">I", ln))
        polys.append((len(out), ln))
        out.extend(scalars_raw_to_processed(c.take(32 * ln)))

    def slice_():
        cnt = c.be32()
        out.extend(struct.pack(">I", cnt))
        for _ in range(cnt):
            poly()

    for _ in range(3):
        poly()
    for _ in range(6):
        slice_()
    assert c.o == len(raw), "trailing bytes in the raw key"
    if layout is not None:
        layout["commitments"] = cm_off
        layout["polys"] = polys
    return bytes(out)
