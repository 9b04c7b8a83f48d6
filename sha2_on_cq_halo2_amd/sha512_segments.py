"""Wired multi-segment SHA-512 circuits: several compression chains ("segments") one behind another in the columns of
the SHA-512 / SHA-384 compression circuit, tied to each other and to constants by copy constraints ("Wired
SHA-512 segments"): message words and initial-state words that are private, constants, shared private words or digest
words of earlier segments, and public digests of 1 .. 8 words.  The constraint system is the one of sha512_circuit.py, gate
for gate; only the fixed columns and the copies differ.  The witness is synthesised on the GPU by
`cq_sha512_synthesize_segments_dev`, which runs the chains level by level on the device.  `Choice` and `Xor` words need
gates the 64-bit circuit does not have yet and are rejected.

The source kinds, the check of a plan, `describe`, `lower`, `word_buffer` and the circuit object are sha2_segments.py's,
written once for this width and the 32-bit one; here are the width, and the plans and front ends of SHA-512 alone.
"""
from __future__ import annotations

import struct
from functools import partial
from typing import NamedTuple

import numpy as np

from . import sha2_segments as S
from . import sha512_circuit as SC
from ._lib import constants
from .context import Context
from .sha2_segments import PRIVATE, Choice, Const, DigestWord, Lowered, Private, Var, Xor, _words_to_mont, has_init, shared_counts, word_buffer  # noqa: F401

SOURCE_DIGEST, SOURCE_IV = (constants()["CQ_SHA512_SOURCE_" + s] for s in ("DIGEST", "IV"))
VARIANT_512, VARIANT_384 = SC.VARIANT_512, SC.VARIANT_384
# FIPS 180-4, 5.3.6.2: SHA-512 of "SHA-512/256" from the initial hash value whose words are SHA-512's xor 0xa5a5a5a5a5a5a5a5
IV512_256 = (0x22312194FC2BF72C, 0x9F555FA3C84C64C2, 0x2393B86B6F53B151, 0x963877195940EABD,
             0x96283EE2A88EFFE3, 0xBE5E1E2553863992, 0x2B0199FC2C85B8AA, 0x0EB72DDC81C52CA2)


class Segment(NamedTuple):
    """One compression chain: `blocks` blocks of 128 bytes and the source of each of its 16 * blocks message words -- a
    Private, a Const, a Var (constants and vars are 64-bit words here) or a DigestWord of an earlier segment, whose words
    0 .. 7 are all readable whatever that segment makes public.  `init` is the state its first block starts from: None for
    the initial hash value of `variant`, else 8 sources for H[0..7] of the same kinds."""

    blocks: int
    sources: tuple
    init: tuple | None = None
    variant: int = VARIANT_512


class Plan(NamedTuple):
    """Segments in row order, and what is public: `public` holds (segment, words) -- the first `words` (1 .. 8) words of that
    segment's final state; their instance rows run consecutively in that order.  `public_init`: segments (each with an
    `init`) whose 8 initial words are public too, behind all of those, 8 rows each."""

    segments: tuple
    public: tuple
    public_init: tuple = ()


def _public(plan: Plan):
    pub = tuple(plan.public)
    if not pub or not all(isinstance(p, tuple) and len(p) == 2 and all(isinstance(x, int) for x in p) for p in pub):
        raise ValueError(f"public {pub!r}: at least one (segment, words) pair")
    if len({s for s, _ in pub}) != len(pub) or not all(0 <= s < len(plan.segments) for s, _ in pub):
        raise ValueError(f"public {pub!r}: each segment an index below {len(plan.segments)}, none twice")
    for s, words in pub:
        if not 1 <= words <= 8:
            raise ValueError(f"public: segment {s} has 1 .. 8 public words, not {words}")
    return pub


WIDTH = S.Width(circuit=SC, constraint_system=lambda table_bits, dense, spread, choice, xor: (SC.FIXED,) + SC._constraint_system(table_bits, dense, spread),
                description=SC.Description, instance_copies_last=False, dtype=np.dtype(np.uint64), letter="Q", source_digest=SOURCE_DIGEST,
                source_choice=None, source_iv=SOURCE_IV, iv=SC.IV, gated=(), segment=Segment, plan=Plan, public=_public)
describe, lower, rows_for, first_regions, merkle_tree, midstate, double_sha512, _check_plan = (
    partial(f, WIDTH) for f in (S.describe, S.lower, S.rows_for, S.first_regions, S.merkle_tree, S.midstate, S.double_hash, S._check_plan))
PAD_128_BYTES = S.padding(WIDTH, 16, 32)  # the second block of a 128-byte message


def batch(blocks_list, variants=None) -> Plan:
    """Independent messages of the given block counts (SHA-512, or variants[j]): every word private, every digest public
    -- 8 words of a SHA-512 message, 6 of a SHA-384 one.  The circuit of sha512_circuit.describe_batch."""
    blocks_list = list(blocks_list)
    variants = [VARIANT_512] * len(blocks_list) if variants is None else list(variants)
    if len(variants) != len(blocks_list) or any(v not in SC.DIGEST_WORDS for v in variants):
        raise ValueError("one variant (VARIANT_512 or VARIANT_384) per message")
    segs = tuple(Segment(b, (PRIVATE,) * (16 * b), None, v) for b, v in zip(blocks_list, variants))
    return Plan(segs, tuple((j, SC.DIGEST_WORDS[v]) for j, v in enumerate(variants)))


def sha512_256(blocks: int) -> Plan:
    """SHA-512/256 of a private message of exactly `blocks` padded blocks: SHA-512's compression from the SHA-512/256
    initial hash value, pinned as constants; the first four words of the final state are the public digest."""
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks), tuple(Const(v) for v in IV512_256)),), ((0, 4),))


def var_count(plan: Plan) -> int:
    """One more than the largest Var index the plan uses, 0 if it uses none."""
    return shared_counts(plan)[0]


def instance_rows(plan: Plan) -> int:
    return sum(words for _, words in plan.public) + 8 * len(plan.public_init)


class Sha512SegmentsCircuit(S.Sha2SegmentsCircuit):
    """Proving key and GPU witness synthesis for a plan of wired SHA-512 / SHA-384 segments at 2^k rows (sha2_segments.py's
    circuit at this width; a plan has no bits): `state_words` holds every segment's final state of the last synthesis,
    `digests` the public words, 8 big-endian bytes each."""

    width = WIDTH

    def _call(self, arr):
        """The entry point alone, on the word buffer as it is on the device."""
        ctx, low = self.ctx, self._lowered
        ctx._chk(ctx.lib.cq_sha512_synthesize_segments_dev(ctx.h, self.table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks),
                                                           low.seg_variant.ctypes.data, low.sources.ctypes.data,
                                                           low.init_sources.ctypes.data if has_init(self.plan) else None, self._words.ptr,
                                                           low.words_len, self.n, arr, self._digests.ptr))


class Sha512dCircuit(Sha512SegmentsCircuit):
    """SHA-512(SHA-512(message)) for a message of exactly `blocks` padded blocks; the double digest is public, the inner one
    is not.  The methods take the message (bytes) and pad it here: that padding is private and not constrained; the second
    hash's input is wired to the first digest and its padding is pinned."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, double_sha512(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks), []]

    def _result(self):
        return self.digests[0]


class Sha512MerkleCircuit(Sha512SegmentsCircuit):
    """The SHA-512 Merkle root over 2^depth private 64-byte leaves (node = SHA-512(left || right)); the root is public.
    The methods take the list of leaves.  Every node's children are wired and its padding block is pinned, so nothing but
    the leaves is free."""

    def __init__(self, ctx: Context, k: int, depth: int, **kw):
        self.depth = depth
        super().__init__(ctx, k, merkle_tree(depth), **kw)

    def _values(self, leaves):
        if len(leaves) != 1 << self.depth or any(len(leaf) != 64 for leaf in leaves):
            raise ValueError(f"{1 << self.depth} leaves of 64 bytes each")
        pairs = 1 << (self.depth - 1)
        return [list(struct.unpack(">16Q", bytes(leaves[2 * i]) + bytes(leaves[2 * i + 1]))) for i in range(pairs)] + [[]] * (pairs - 1)

    def _result(self):
        return self.digests[0]


class Sha512MidstateCircuit(Sha512SegmentsCircuit):
    """`blocks` private 128-byte blocks take the public chaining value H_in to the public chaining value H_out (the plan
    `midstate`): instance rows 0 .. 7 are H_out, rows 8 .. 15 H_in.  The methods take (h_in, data): 8 words and exactly
    128 * blocks bytes; nothing is padded.  A proof says nothing about where H_in comes from: a verifier links it to the
    initial hash value or to the H_out of another proof."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, midstate(blocks), **kw)

    def _values(self, item):
        h_in, data = item
        blocks = self.plan.segments[0].blocks
        if len(h_in) != 8 or len(data) != 128 * blocks:
            raise ValueError(f"a state of 8 words and {128 * blocks} bytes of data")
        return [[int(x) for x in h_in] + list(struct.unpack(f">{16 * blocks}Q", bytes(data)))]

    @property
    def h_out(self):
        return self.state_words[0]

    def _result(self):
        return self.instance_words


class Sha512_256Circuit(Sha512SegmentsCircuit):
    """SHA-512/256 of a message of exactly `blocks` padded blocks (the plan `sha512_256`): the methods take the message and
    pad it here, as Sha512Circuit does.  The instance is the four words of the digest, 32 bytes."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, sha512_256(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks)]

    def _result(self):
        return self.digests[0]
