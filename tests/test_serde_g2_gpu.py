"""GPU: G2 in the on-disk formats -- batch G2 decompression / compression, the complete ParamsKZG stream and the G2 SRS stream
in the three SerdeFormats, against the big-integer model of tests/serde_g2_model.py (a literal Algorithm 9 and the
reference's byte layout) and [k]_2 of the C oracle.  Expectations never come from the code under test."""
import functools

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import pairing as PR
from tests import serde_g2_model as G
from tests.g2_helpers import R, affine_from_limbs, fr_mont, g2_mul_limbs

pytestmark = pytest.mark.gpu
Q = B.Q_MOD
PROCESSED, RAW, RAW_UNCHECKED = 0, 1, 2
FORMATS = (PROCESSED, RAW, RAW_UNCHECKED)
POINT_SIZE = {PROCESSED: 64, RAW: 128, RAW_UNCHECKED: 128}
# the kernels run 256 lanes a block: two whole blocks, one whole wave of the third and a partial one
SPAN = 2 * 256 + 64 + 7
S_TOXIC = 0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF0 % R


@functools.lru_cache(maxsize=None)
def _pool():
    """SPAN points with their model encodings, computed once: [k]_2 for seeded k, each followed by its negation [r - k]_2
    (both sign bits for one x); raw limbs from the C oracle, bytes from the model"""
    rng = B.Xoshiro256ss(0x62E5)
    ks = []
    for _ in range((SPAN + 1) // 2):
        k = B.fr_random(rng) or 1
        ks += [k, R - k]
    raw = np.array([g2_mul_limbs(k) for k in ks[:SPAN]], dtype=np.uint64)
    pts = [affine_from_limbs(r) for r in raw]
    assert pts[1] == PR.ec_neg(pts[0]) and all(PR.is_on_twist(p) for p in pts[:4])
    comp = np.frombuffer(b"".join(G.g2_to_bytes(p) for p in pts), dtype=np.uint8).reshape(SPAN, 64)
    assert {int(c[63]) >> 7 for c in comp} == {0, 1}
    return pts, raw, comp


def _batch(n):
    """the first n pool points with the identity at the first, the last and an interior index (n >= 3)"""
    _, raw, comp = _pool()
    raw, comp = raw[:n].copy(), comp[:n].copy()
    if n >= 3:
        for i in (0, n // 2, n - 1):
            raw[i] = 0
            comp[i] = 0
    return raw, comp


def _decompress(ctx, comp, n):
    src, dst = ctx.to_device(comp[:n]), ctx.alloc(max(128 * n, 128))
    ctx.g2_decompress(src, n, dst)
    return dst.download((n, 16))


def _compress(ctx, raw, n):
    src, dst = ctx.to_device(raw[:n]), ctx.alloc(max(64 * n, 64))
    ctx.g2_compress(src, n, dst)
    ctx.sync()
    return dst.download((n, 64), np.uint8)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SPAN])
def test_batch_decompress_and_compress_match_the_model(ctx, n):
    raw, comp = _batch(n)
    got_raw = _decompress(ctx, comp, n)
    assert np.array_equal(got_raw, raw)
    got_comp = _compress(ctx, raw, n)
    assert np.array_equal(got_comp, comp)
    assert np.array_equal(_decompress(ctx, got_comp, n), raw)  # decompress(compress(P)) == P
    if n == 1:  # the lone identity
        zero = np.zeros((1, 64), dtype=np.uint8)
        assert not _decompress(ctx, zero, 1).any()
        assert not _compress(ctx, np.zeros((1, 16), dtype=np.uint64), 1).any()
    if n >= 3:  # the model decodes the bytes to the very points (spot check; the CPU suite checks the model)
        pts = _pool()[0]
        for i in (1, 2, n - 2):
            assert G.g2_from_bytes(bytes(got_comp[i])) == pts[i]
        assert G.g2_from_bytes(bytes(got_comp[0])) is None


def _enc(c0, c1, sign=0):
    b = bytearray(c0.to_bytes(32, "little") + c1.to_bytes(32, "little"))
    b[63] |= sign << 7
    return bytes(b)


def _nonsquare_x():
    """from a valid point's x: x.c0 + 1, + 2, ... until x^3 + b' is no square (half of all x are)"""
    x = _pool()[0][5][0]
    for d in range(1, 200):
        c = PR.FQ2([x.c[0] + d, x.c[1]])
        if not G.fq2_is_square(c * c * c + PR.B2):
            return c
    raise AssertionError("no non-square x found")


def _model_accepts(b):
    try:
        G.g2_from_bytes(b)
        return True
    except ValueError:
        return False


def test_invalid_encodings_are_rejected_and_the_lowest_index_is_named(ctx):
    from sha2_on_cq_halo2_amd import CqError

    pts, raw, comp = _pool()
    n = 257
    x = pts[7][0]
    ns = _nonsquare_x()
    cases = {
        "c0 == q": _enc(Q, x.c[1]),
        "c1 == q": _enc(x.c[0], Q),
        "c1 with bit 254 set": _enc(x.c[0], x.c[1] | (1 << 254)),
        "x^3 + b' not a square": _enc(ns.c[0], ns.c[1]),
        "zero with the sign bit": _enc(0, 0, 1),
    }
    for name, b in cases.items():
        assert not _model_accepts(b), name
        bad = np.frombuffer(b, dtype=np.uint8)
        for where in (0, 131, n - 1):  # alone at the first, an interior and the last index
            batch = comp[:n].copy()
            batch[where] = bad
            with pytest.raises(CqError) as e:
                _decompress(ctx, batch, n)
            assert e.value.code == -1 and e.value.first_bad == where, (name, where)
            assert "index %d " % where in str(e.value) and "(1 invalid" in str(e.value), (name, where)
    batch = comp[:n].copy()
    for where, name in ((200, "c1 == q"), (64, "x^3 + b' not a square"), (256, "zero with the sign bit")):
        batch[where] = np.frombuffer(cases[name], dtype=np.uint8)
    with pytest.raises(CqError) as e:
        _decompress(ctx, batch, n)
    assert e.value.first_bad == 64 and "index 64 " in str(e.value) and "(3 invalid" in str(e.value)
    # the context is usable afterwards
    assert np.array_equal(_decompress(ctx, comp, 10), raw[:10])


def _s_limbs(s):
    return fr_mont([s])[0]


def _off_twist(raw128: bytes) -> bytes:
    b = bytearray(raw128)
    b[64 + 9] ^= 0x80  # one bit of y.c0: still below q (a low byte), no longer on the twist
    return bytes(b)


@pytest.mark.parametrize("k", [3, 6])
def test_params_full_stream_round_trips(ctx, k):
    from sha2_on_cq_halo2_amd import CqError, ParamsKZG

    n = 1 << k
    p = ParamsKZG.setup_from_toxic_waste(ctx, k, _s_limbs(S_TOXIC))
    gen, s_g2 = g2_mul_limbs(1), g2_mul_limbs(S_TOXIC)
    assert np.array_equal(p.g2, gen) and affine_from_limbs(gen) == PR.G2_GEN
    assert np.array_equal(p.s_g2, s_g2)
    full = {fmt: p.write_full(fmt) for fmt in FORMATS}
    assert full[RAW] == full[RAW_UNCHECKED] and len(full[RAW]) == 4 + 128 * n + 256 and len(full[PROCESSED]) == 4 + 64 * n + 128
    assert full[RAW][-256:] == gen.tobytes() + s_g2.tobytes()
    assert full[PROCESSED] == G.params_full_raw_to_processed(full[RAW])
    for fmt in FORMATS:
        b = full[fmt]
        assert ctx.lib.cq_params_serialized_size_full(p.h, fmt) == len(b)
        assert b[:ctx.lib.cq_params_serialized_size(p.h, fmt)] == p.write(fmt) and len(p.write(fmt)) == len(b) - 2 * POINT_SIZE[fmt]
        q = ParamsKZG.read_full(ctx, b, fmt)
        assert q.k == k and q.write_full(fmt) == b
        assert np.array_equal(q.g2, gen) and np.array_equal(q.s_g2, s_g2)
        for other in FORMATS:  # and across formats
            assert q.write_full(other) == full[other]
        q.close()
        # the G1 reader still takes the full bytes, and what it returns holds no tail
        g1 = ParamsKZG.read(ctx, b, fmt)
        assert g1.write(fmt) == p.write(fmt)
        with pytest.raises(CqError):
            g1.g2
        with pytest.raises(CqError):
            g1.s_g2
        with pytest.raises(CqError):
            g1.write_full(fmt)
        g1.close()
        with pytest.raises(CqError):  # one byte short of the full stream
            ParamsKZG.read_full(ctx, b[:-1], fmt)
    assert ctx.lib.cq_params_serialized_size_full(p.h, 7) == 0
    with pytest.raises(CqError):
        ParamsKZG.read_full(ctx, full[RAW], 7)
    # params built from host arrays hold no tail until they are given one
    g, gl = p.download()
    created = ParamsKZG(ctx, k, g, gl)
    with pytest.raises(CqError):
        created.write_full(PROCESSED)
    created.set_g2(gen, s_g2)
    assert created.write_full(PROCESSED) == full[PROCESSED]
    created.close()
    # a tail point whose x is on no point: named
    ns = _nonsquare_x()
    bad = bytearray(full[PROCESSED])
    bad[-64:] = _enc(ns.c[0], ns.c[1])
    with pytest.raises(CqError) as e:
        ParamsKZG.read_full(ctx, bytes(bad), PROCESSED)
    assert e.value.code == -1 and "at s_g2 " in str(e.value)
    bad = bytearray(full[PROCESSED])
    bad[-128:-64] = _enc(ns.c[0], ns.c[1], 1)
    with pytest.raises(CqError) as e:
        ParamsKZG.read_full(ctx, bytes(bad), PROCESSED)
    assert "at g2 " in str(e.value)
    # a tail point off the twist: rejected where the format checks, stored as given where it does not
    for which, name in ((0, "g2"), (1, "s_g2")):
        off = len(full[RAW]) - 256 + 128 * which
        bad = full[RAW][:off] + _off_twist(full[RAW][off:off + 128]) + full[RAW][off + 128:]
        with pytest.raises(CqError) as e:
            ParamsKZG.read_full(ctx, bad, RAW)
        assert e.value.code == -1 and "at %s " % name in str(e.value)
        q = ParamsKZG.read_full(ctx, bad, RAW_UNCHECKED)
        assert q.write_full(RAW_UNCHECKED) == bad
        q.close()
    # downsize keeps g2 and s_g2
    d = p.downsize(k - 1)
    assert np.array_equal(d.g2, gen) and np.array_equal(d.s_g2, s_g2)
    assert d.write_full(RAW)[-256:] == full[RAW][-256:] and len(d.write_full(PROCESSED)) == 4 + 32 * n + 128
    d.close()
    p.close()


@pytest.mark.parametrize("count", [1, 5, 65])
def test_g2_srs_stream_round_trips(ctx, count):
    from sha2_on_cq_halo2_amd import CqError, G2Srs

    srs = G2Srs.setup_from_toxic_waste(ctx, count, _s_limbs(S_TOXIC))
    pts = srs.download()
    for i in sorted({0, 1, count - 1} & set(range(count))):
        assert np.array_equal(pts[i], g2_mul_limbs(pow(S_TOXIC, i, R))), i
    streams = {fmt: srs.write(fmt) for fmt in FORMATS}
    assert streams[RAW] == streams[RAW_UNCHECKED] == pts.tobytes()
    assert streams[PROCESSED] == G.points_raw_to_processed(streams[RAW])
    for fmt in FORMATS:
        assert ctx.lib.cq_g2_srs_serialized_size(srs.h, fmt) == len(streams[fmt]) == count * POINT_SIZE[fmt]
        back = G2Srs.read(ctx, streams[fmt], fmt)
        assert back.count == count and np.array_equal(back.download(), pts)
        assert back.write(fmt) == streams[fmt]
        back.close()
        with pytest.raises(CqError):  # not a whole number of points
            G2Srs.read(ctx, streams[fmt] + b"\0", fmt)
        with pytest.raises(CqError):
            G2Srs.read(ctx, streams[fmt][:-1], fmt)
    assert ctx.lib.cq_g2_srs_serialized_size(srs.h, 7) == 0
    if count == 65:  # one point off the twist, one encoding on no point: named by their index in the array
        bad = streams[RAW][:128 * 37] + _off_twist(streams[RAW][128 * 37:128 * 38]) + streams[RAW][128 * 38:]
        with pytest.raises(CqError) as e:
            G2Srs.read(ctx, bad, RAW)
        assert e.value.code == -1 and "index 37 " in str(e.value)
        unchecked = G2Srs.read(ctx, bad, RAW_UNCHECKED)
        assert unchecked.download().tobytes() == bad
        unchecked.close()
        ns = _nonsquare_x()
        badp = streams[PROCESSED][:64 * 37] + _enc(ns.c[0], ns.c[1]) + streams[PROCESSED][64 * 38:]
        with pytest.raises(CqError) as e:
            G2Srs.read(ctx, badp, PROCESSED)
        assert "index 37 " in str(e.value)
    srs.close()


def test_static_table_commit_with_an_srs_read_from_processed_bytes(ctx):
    """the use it exists for: the verifying key's StaticCommittedTable from a G2 SRS that came out of a file"""
    from sha2_on_cq_halo2_amd import G2Srs, StaticTable

    s = 0x5EED5EED % R
    toxic = G2Srs.setup_from_toxic_waste(ctx, 17, _s_limbs(s))
    loaded = G2Srs.read(ctx, toxic.write(PROCESSED), PROCESSED)
    vals = [(i * 7 + 3) % 16 * 1000 + 5 for i in range(16)]
    t = StaticTable.setup_from_toxic_waste(ctx, fr_mont(vals), _s_limbs(s))
    want = t.commit(toxic, 16, 8)
    got = t.commit(loaded, 16, 8)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0], g2_mul_limbs(pow(s, 16, R) - 1))  # zv = [s^N - 1]_2
    assert np.array_equal(got[2], g2_mul_limbs(pow(s, 9, R)))       # x_b0_bound = [s^(16 - 1 - (8 - 2))]_2
    for o in (t, toxic, loaded):
        o.close()
