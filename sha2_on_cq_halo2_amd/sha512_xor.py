"""XOR-wired message words on the SHA-512 / SHA-384 circuit, and HMAC-SHA-512 / HMAC-SHA-384 built from them (DESIGN.md,
"XOR-wired message words on the 64-bit circuit").  A message word of a plan may be the XOR of two sources (`Xor`): every
distinct Xor is a unit of two regions behind the last segment, forced by the gate `xor_word` of the XOR variant of
sha512_circuit.py's constraint system, and synthesised on the GPU by `cq_sha512_synthesize_xors_dev`.

sha512_segments.py's width has no gated kind and keeps the plain constraint system, gate for gate; the width here is that
one with `Xor` gated and the variant's constraint system, and `describe`, `lower`, `rows_for`, `xor_first_region` and
`_check_plan` are sha2_segments.py's functions at it.  `Segment` and `Plan` are sha512_segments.py's.  A plan without an
Xor is described here as it is there.  A `Choice` is still refused, and an Xor as an initial word is refused as at 32 bits.
"""
from __future__ import annotations

import struct
from functools import partial

from . import sha2_segments as S
from . import sha512_circuit as SC
from . import sha512_segments as SS
from .context import Context
from .sha2_segments import PRIVATE, Const, DigestWord, Var, Xor, has_init, xor_units  # noqa: F401
from .sha512_segments import SOURCE_DIGEST, SOURCE_IV, VARIANT_384, VARIANT_512, Plan, Segment  # noqa: F401


def _constraint_system(table_bits, dense, spread, choice, xor):
    return (SC.FIXED_XOR if xor else SC.FIXED,) + SC._constraint_system(table_bits, dense, spread, xor=xor)


WIDTH = SS.WIDTH._replace(gated=(Xor,), constraint_system=_constraint_system)
describe, lower, rows_for, first_regions, xor_first_region, _check_plan = (
    partial(f, WIDTH) for f in (S.describe, S.lower, S.rows_for, S.first_regions, S.xor_first_region, S._check_plan))

HMAC_IPAD, HMAC_OPAD = 0x3636363636363636, 0x5C5C5C5C5C5C5C5C
BLOCK_BYTES = 128


def hmac_sha512(key_bytes: int, message_bytes: int, commit_key: bool = False, variant: int = VARIANT_512) -> Plan:
    """HMAC-SHA-512 (RFC 2104; HMAC-SHA-384 with variant=VARIANT_384) of a private message of `message_bytes` bytes under a
    private key of `key_bytes` bytes, 8 .. 128, both multiples of 8: tag = H((K' ^ opad) || H((K' ^ ipad) || m)), K' the key
    padded with zeros to 128 bytes.  The key is Var 0 .. key_bytes / 8 - 1.  Segment 0, the inner hash: words
    t < key_bytes / 8 are Xor(Var(t), Const(ipad)), the rest of the key block Const(ipad) -- a zero key byte xor ipad -- then
    the message words, Private, then the padding of a 128 + message_bytes byte message, Const word for word.  Segment 1, the
    outer hash, two blocks: the key block with opad, the 8 (SHA-384: 6) words of the inner digest, the pinned padding of a
    192- (176-) byte message.  The first 8 (6) words of its final state, the tag, are public.  `commit_key`: a third segment
    hashes the key Vars under pinned padding with the same variant and its digest is public too, behind the tag: "the key
    whose hash is C".  A key above 128 bytes is not offered: RFC 2104 hashes it first, which a plan can say with a segment
    over the key and DigestWord operands in the two key blocks."""
    if variant not in SC.DIGEST_WORDS:
        raise ValueError(f"hmac_sha512: the variant {variant!r} is neither VARIANT_512 nor VARIANT_384")
    if key_bytes % 8 or message_bytes % 8 or not 8 <= key_bytes <= BLOCK_BYTES or message_bytes < 0:
        raise ValueError(f"hmac_sha512: a key of {key_bytes} bytes and a message of {message_bytes}: both are multiples of 8, the key "
                         "from 8 to 128 bytes (a longer key is hashed first, other byte lengths need a variable-length circuit)")
    key = tuple(Var(t) for t in range(key_bytes // 8))
    digest_words = SC.DIGEST_WORDS[variant]

    def key_block(pad):
        return tuple(Xor(v, Const(pad)) for v in key) + (Const(pad),) * (16 - len(key))

    def padding(data_bytes):  # the words behind the data of a message of that many bytes, as PAD_128_BYTES is built
        return S.padding(WIDTH, data_bytes // 8, 16 * -(-(data_bytes + 17) // BLOCK_BYTES))

    inner = key_block(HMAC_IPAD) + (PRIVATE,) * (message_bytes // 8) + padding(BLOCK_BYTES + message_bytes)
    outer = key_block(HMAC_OPAD) + tuple(DigestWord(0, i) for i in range(digest_words)) + padding(BLOCK_BYTES + 8 * digest_words)
    segs = [Segment(len(inner) // 16, inner, None, variant), Segment(2, outer, None, variant)]
    public = [(1, digest_words)]
    if commit_key:
        committed = key + padding(key_bytes)
        segs.append(Segment(len(committed) // 16, committed, None, variant))
        public.append((2, digest_words))
    assert segs[0].blocks == 1 + -(-(message_bytes + 17) // BLOCK_BYTES) and len(outer) == 32
    return Plan(tuple(segs), tuple(public))


class Sha512XorSegmentsCircuit(SS.Sha512SegmentsCircuit):
    """Sha512SegmentsCircuit for plans that may hold Xor words: the XOR variant's key for a plan with an Xor -- one fixed
    column and one gate more, so another key than the plain circuit's -- and the plain circuit's for a plan without."""

    width = WIDTH

    def _call(self, arr):
        """The entry point alone, on the word buffer as it is on the device: the one with XOR units only for a plan with an
        Xor."""
        ctx, low = self.ctx, self._lowered
        if not len(low.xors):
            return super()._call(arr)
        ctx._chk(ctx.lib.cq_sha512_synthesize_xors_dev(ctx.h, self.table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks),
                                                       low.seg_variant.ctypes.data, low.sources.ctypes.data,
                                                       low.init_sources.ctypes.data if has_init(self.plan) else None, low.xors.ctypes.data,
                                                       len(low.xors), self._words.ptr, low.words_len, self.n, arr, self._digests.ptr))


class HmacSha512Circuit(Sha512XorSegmentsCircuit):
    """HMAC-SHA-512 of a private message of exactly `message_bytes` bytes under a private key of exactly `key_bytes` bytes
    (8 .. 128), both multiples of 8 (the plan `hmac_sha512`); the tag is public, with `commit_key` the hash of the key too.
    The methods take (key, message) as bytes.  Forced: the key block's zero padding and both pads (Const words and Xor
    units), the message's padding, the wiring of the inner digest into the outer hash, and that both hashes -- and the
    commitment -- use one key.  The message is private.  Not offered: keys above 128 bytes (a Plan with DigestWord operands
    a user can write: hash the key in a segment of its own) and byte lengths that are no multiple of 8."""

    variant = VARIANT_512

    def __init__(self, ctx: Context, k: int, key_bytes: int, message_bytes: int, commit_key: bool = False, **kw):
        self.key_bytes, self.message_bytes, self.commit_key = key_bytes, message_bytes, commit_key
        super().__init__(ctx, k, hmac_sha512(key_bytes, message_bytes, commit_key, self.variant), **kw)

    def _inputs(self, key, message=None):
        key, message = (bytes(x) for x in (key if message is None else (key, message)))  # (key, message) as one pair too
        if (len(key), len(message)) != (self.key_bytes, self.message_bytes):
            raise ValueError(f"a key of {self.key_bytes} bytes and a message of {self.message_bytes}, not {len(key)} and {len(message)}")
        words = lambda data: list(struct.unpack(f">{len(data) // 8}Q", data))
        return [words(message)] + [[]] * (len(self.plan.segments) - 1), words(key), []

    def tag(self) -> bytes:
        """The tag of the last synthesis, 64 bytes (HMAC-SHA-384: 48): what `prove` returns beside the proof.  The public
        inputs are the tag's words, then with `commit_key` those of the hash of the key."""
        return self.digests[0]

    def key_commitment(self) -> bytes:
        """SHA-512(key) (HMAC-SHA-384: SHA-384(key)) of the last synthesis (`commit_key` only)."""
        if not self.commit_key:
            raise ValueError("the circuit was built without commit_key")
        return self.digests[1]

    def _result(self):
        return self.tag()


class HmacSha384Circuit(HmacSha512Circuit):
    """The same for HMAC-SHA-384: both hashes, and the commitment, start from SHA-384's initial hash value; the tag is the
    first six words of the outer hash's final state, 48 bytes."""

    variant = VARIANT_384
