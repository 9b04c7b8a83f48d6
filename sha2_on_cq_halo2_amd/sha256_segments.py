"""Wired multi-segment SHA-256 circuits: several compression chains ("segments") one behind another in the columns of
the SHA-256 compression circuit, tied to each other and to constants by copy constraints ("Wired SHA-256
segments").

A plan says, for every message word of every segment, where the word comes from -- a private value, a constant, a
digest word of an earlier segment, a shared private word, or a choice between two of the latter under a private bit --
and which segments' digests are public.  The constraint system is the one of sha256_circuit.py, gate for gate; only the
fixed columns and the copies differ -- and, for a plan with a choice, one selector and two gates (DESIGN.md,
"Choice-wired message words").  The witness is synthesised on the GPU by `cq_sha256_synthesize_segments_dev`
(`cq_sha256_synthesize_choices_dev` for a plan with a choice), which runs the chains level by level on the device.

A segment may also start from a state other than the IV (`Segment.init`, DESIGN.md "Wired initial states"): eight sources
for H[0..7], tied by the same kinds of copies; such a plan is synthesised by `cq_sha256_synthesize_states_dev`.

A message word may also be the XOR of two sources (`Xor`, DESIGN.md "XOR-wired message words"): every distinct Xor is a
unit of two regions behind the last segment, one selector and one gate are added, and the plan is synthesised by
`cq_sha256_synthesize_xors_dev`.  `hmac_sha256` / `HmacSha256Circuit` build HMAC-SHA-256 from it.

The source kinds, the check of a plan, `describe`, `lower`, `word_buffer` and the circuit object are sha2_segments.py's,
written once for this width and the 64-bit one; here are the width, the plans and front ends of SHA-256 alone, and the
choice among the four entry points.
"""
from __future__ import annotations

import ctypes as C
import struct
from functools import partial
from typing import NamedTuple

import numpy as np

from . import sha256_circuit as SC
from . import sha2_segments as S
from ._lib import constants
from .context import Context
from .sha2_segments import (PRIVATE, Choice, Const, DigestWord, Lowered, Private, Var, Xor, _words_to_mont, has_choice,  # noqa: F401
                            has_init, has_xor, shared_counts, word_buffer, xor_units)

SOURCE_DIGEST, SOURCE_CHOICE, SOURCE_IV = (constants()["CQ_SHA256_SOURCE_" + s] for s in ("DIGEST", "CHOICE", "IV"))
IV224 = (0xC1059ED8, 0x367CD507, 0x3070DD17, 0xF70E5939, 0xFFC00B31, 0x68581511, 0x64F98FA7, 0xBEFA4FA4)  # FIPS 180-4, 5.3.2


class Segment(NamedTuple):
    """One compression chain: `blocks` blocks and the source of each of its 16 * blocks message words.  `init` is the state
    its first block starts from: None for the IV, else 8 sources for H[0..7], each a Const, Private, Var or a DigestWord of
    an earlier segment (no Choice, no Xor)."""

    blocks: int
    sources: tuple
    init: tuple | None = None


class Plan(NamedTuple):
    """Segments in row order, and the segments whose digests are the instance: rows 8p .. 8p + 7 for public[p].
    `public_init`: segments (each with an `init`) whose 8 initial words are public too, behind all the digests: instance
    row 8 * len(public) + 8q + i holds initial word i of segment public_init[q]."""

    segments: tuple
    public: tuple
    public_init: tuple = ()


def _public(plan: Plan):
    if not plan.public or len(set(plan.public)) != len(plan.public) or not all(0 <= p < len(plan.segments) for p in plan.public):
        raise ValueError(f"public segments {plan.public!r}: at least one, each an index below {len(plan.segments)}, none twice")
    return tuple((p, 8) for p in plan.public)


def _constraint_system(table_bits, dense, spread, choice, xor):
    names = SC.FIXED_CHOICE if choice else SC.FIXED_XOR if xor else SC.FIXED
    return (names,) + SC._constraint_system(table_bits, dense, spread, choice, xor=xor)


WIDTH = S.Width(circuit=SC, constraint_system=_constraint_system, description=lambda *a: SC.Description(*a[:9], *a[10:]),  # no variants
                instance_copies_last=True, dtype=np.dtype(np.uint32), letter="I", source_digest=SOURCE_DIGEST, source_choice=SOURCE_CHOICE,
                source_iv=SOURCE_IV, iv={0: SC.IV256}, gated=(Choice, Xor), segment=Segment,
                plan=lambda segments, public, public_init=(): Plan(segments, tuple(s for s, _ in public), public_init), public=_public)
describe, lower, rows_for, first_regions, xor_first_region, merkle_tree, midstate, double_sha256, _check_plan = (
    partial(f, WIDTH) for f in (S.describe, S.lower, S.rows_for, S.first_regions, S.xor_first_region, S.merkle_tree, S.midstate, S.double_hash,
                                S._check_plan))
PAD_64_BYTES = S.padding(WIDTH, 16, 32)  # the second block of a 64-byte message


def batch(blocks_list) -> Plan:
    """Independent messages of the given block counts: every word private, every digest public."""
    segs = tuple(Segment(b, (PRIVATE,) * (16 * b)) for b in blocks_list)
    return Plan(segs, tuple(range(len(segs))))


def merkle_path(depth: int, paths: int = 1, leaf_blocks: int | None = None, public_leaf: bool = False) -> Plan:
    """Membership of a leaf under a Merkle root, `paths` independent times: per path `depth` two-block segments bottom-up,
    the second block pinned padding.  At level l, word t < 8 is Choice(bit, cur_t, sib_t) and word 8 + t is
    Choice(bit, sib_t, cur_t) under the one bit of that level and path (bit depth * p + l): the running node is the left
    half for bit 0, the right half for bit 1.  sib_t is a Var; cur_t is the digest of the level below, and at level 0 a
    Var holding the 32-byte leaf -- or, with `leaf_blocks`, the digest of a private segment of that many blocks laid before
    the path (public iff `public_leaf`).  A path's vars: the leaf's 8 (without `leaf_blocks`), then 8 per level.  Every
    path's top segment is public; instance order per path: the leaf digest if public, then the root."""
    if depth < 1 or paths < 1:
        raise ValueError("a Merkle path has at least one level (depth >= 1), a plan at least one path")
    if public_leaf and leaf_blocks is None:
        raise ValueError("public_leaf: the leaf digest of a leaf_blocks segment; a 32-byte leaf is a private Var")
    segs, public, var = [], [], 0
    for p in range(paths):
        if leaf_blocks is None:
            cur = tuple(Var(var + t) for t in range(8))
            var += 8
        else:
            cur = tuple(DigestWord(len(segs), t) for t in range(8))
            if public_leaf:
                public.append(len(segs))
            segs.append(Segment(leaf_blocks, (PRIVATE,) * (16 * leaf_blocks)))
        for level in range(depth):
            bit, sib = depth * p + level, tuple(Var(var + t) for t in range(8))
            var += 8
            words = tuple(Choice(bit, c, s) for c, s in zip(cur, sib)) + tuple(Choice(bit, s, c) for c, s in zip(cur, sib))
            cur = tuple(DigestWord(len(segs), t) for t in range(8))
            segs.append(Segment(2, words + PAD_64_BYTES))
        public.append(len(segs) - 1)
    return Plan(tuple(segs), tuple(public))


def sha224(blocks: int) -> Plan:
    """SHA-224 of a private message of exactly `blocks` padded blocks: SHA-256's compression from the SHA-224 initial
    value, pinned as constants.  The public digest has 8 words as in every plan; words 0 .. 6 are the SHA-224 digest, and
    word 7, which SHA-224 drops, stays public too -- a verifier compares the first seven and may ignore the eighth."""
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks), tuple(Const(v) for v in IV224)),), (0,))


HMAC_IPAD, HMAC_OPAD = 0x36363636, 0x5C5C5C5C


def hmac_sha256(key_bytes: int, message_bytes: int, commit_key: bool = False) -> Plan:
    """HMAC-SHA-256 (RFC 2104) of a private message of `message_bytes` bytes under a private key of `key_bytes` <= 64 bytes,
    both multiples of 4: tag = H((K' ^ opad) || H((K' ^ ipad) || m)), K' the key padded with zeros to 64 bytes.  The key is
    Var 0 .. key_bytes / 4 - 1.  Segment 0, the inner hash: words t < key_bytes / 4 are Xor(Var(t), Const(ipad)), the rest of
    the key block Const(ipad) -- a zero key byte xor ipad -- then the message words, Private, then the padding of a
    64 + message_bytes byte message, Const word for word.  Segment 1, the outer hash, two blocks: the key block with opad,
    the inner digest, the pinned padding of a 96-byte message.  Its digest, the tag, is public.  `commit_key`: a third segment
    hashes the key Vars under pinned padding and its digest is public too, behind the tag: "the key whose SHA-256 is C"."""
    if key_bytes % 4 or message_bytes % 4 or not 0 <= key_bytes <= 64 or message_bytes < 0:
        raise ValueError(f"hmac_sha256: a key of {key_bytes} bytes and a message of {message_bytes}: both are multiples of 4, the key at "
                         "most 64 bytes (a longer key is hashed first, any byte length needs the variable-length circuit)")
    key = tuple(Var(t) for t in range(key_bytes // 4))

    def key_block(pad):
        return tuple(Xor(v, Const(pad)) for v in key) + (Const(pad),) * (16 - len(key))

    def padding(total_bytes):  # the words behind the data of a message of that many bytes: 0x80, zeros, the bit length
        return tuple(Const(w) for w in SC.pad(bytes(total_bytes))[total_bytes // 4:])

    inner = key_block(HMAC_IPAD) + (PRIVATE,) * (message_bytes // 4) + padding(64 + message_bytes)
    outer = key_block(HMAC_OPAD) + tuple(DigestWord(0, i) for i in range(8)) + padding(96)
    segs = [Segment(len(inner) // 16, inner), Segment(2, outer)]
    if commit_key:
        committed = key + padding(key_bytes)
        segs.append(Segment(len(committed) // 16, committed))
    assert segs[0].blocks == 1 + -(-(message_bytes + 9) // 64)
    return Plan(tuple(segs), (1, 2) if commit_key else (1,))


def _digest_words(message: bytes):
    return list(struct.unpack(">8I", message))


class Sha256SegmentsCircuit(S.Sha2SegmentsCircuit):
    """Proving key and GPU witness synthesis for a plan of wired SHA-256 segments at 2^k rows (sha2_segments.py's circuit at
    this width): `digest_words` holds every segment's digest of the last synthesis, `digests` the public ones, 32 big-endian
    bytes each."""

    width = WIDTH

    def __init__(self, ctx: Context, k: int, plan: Plan, **kw):
        super().__init__(ctx, k, plan, **kw)
        low = self._lowered
        self._seg_blocks, self._sources, self._choices, self._xors, self._words_len = low.seg_blocks, low.sources, low.choices, low.xors, low.words_len
        self._init_sources = low.init_sources if has_init(plan) else None

    def _call(self, arr, words_ptr=None, digests_ptr=None):
        """The entry point alone, on the word buffer as it is on the device (`words_ptr`, `digests_ptr`: other device arrays
        than the circuit's own): the one with choices only for a plan that has some, the one with states only for a plan
        with an `init`, the one with XOR units only for a plan with an Xor."""
        ctx = self.ctx
        if len(self._xors):
            ctx._chk(ctx.lib.cq_sha256_synthesize_xors_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                           self._sources.ctypes.data, None, 0,
                                                           None if self._init_sources is None else self._init_sources.ctypes.data,
                                                           self._xors.ctypes.data, len(self._xors), words_ptr or self._words.ptr, self._words_len,
                                                           self.n, arr, digests_ptr or self._digests.ptr))
        elif self._init_sources is not None:
            ctx._chk(ctx.lib.cq_sha256_synthesize_states_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                             self._sources.ctypes.data, self._choices.ctypes.data if len(self._choices) else None,
                                                             len(self._choices), self._init_sources.ctypes.data, words_ptr or self._words.ptr,
                                                             self._words_len, self.n, arr, digests_ptr or self._digests.ptr))
        elif len(self._choices):
            ctx._chk(ctx.lib.cq_sha256_synthesize_choices_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                              self._sources.ctypes.data, self._choices.ctypes.data, len(self._choices),
                                                              self._words.ptr, self._words_len, self.n, arr, self._digests.ptr))
        else:
            ctx._chk(ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                               self._sources.ctypes.data, self._words.ptr, self._words_len, self.n, arr,
                                                               self._digests.ptr))


class Sha256BatchCircuit(Sha256SegmentsCircuit):
    """Several independent messages in one proof, message j of exactly blocks_list[j] padded blocks; every digest is
    public.  The methods take the list of messages (bytes) and pad them here: the padding is private words like the rest
    of a message and is not constrained."""

    def __init__(self, ctx: Context, k: int, blocks_list, **kw):
        super().__init__(ctx, k, batch(blocks_list), **kw)

    def _values(self, messages):
        if len(messages) != len(self.plan.segments):
            raise ValueError(f"{len(self.plan.segments)} messages, not {len(messages)}")
        return [SC.pad(m, seg.blocks) for m, seg in zip(messages, self.plan.segments)]


class Sha256dCircuit(Sha256SegmentsCircuit):
    """SHA-256(SHA-256(message)) for a message of exactly `blocks` padded blocks; the double digest is public, the inner one
    is not.  The methods take the message (bytes) and pad it here: that padding is private and not constrained; the second
    hash's input is wired to the first digest and its padding is pinned."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, double_sha256(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks), []]

    def _result(self):
        return self.digests[0]


class Sha256MidstateCircuit(Sha256SegmentsCircuit):
    """`blocks` private 64-byte blocks take the public chaining value H_in to the public chaining value H_out (the plan
    `midstate`): instance rows 0 .. 7 are H_out, rows 8 .. 15 H_in.  The methods take (h_in, data): 8 words and exactly
    64 * blocks bytes; nothing is padded.  A proof says nothing about where H_in comes from: a verifier links it to the
    IV or to the H_out of another proof (sha256_stream.link)."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, midstate(blocks), **kw)

    def _values(self, item):
        h_in, data = item
        blocks = self.plan.segments[0].blocks
        if len(h_in) != 8 or len(data) != 64 * blocks:
            raise ValueError(f"a state of 8 words and {64 * blocks} bytes of data")
        return [[int(x) for x in h_in] + list(struct.unpack(f">{16 * blocks}I", bytes(data)))]

    def synthesize_dev(self, words_ptr: int, digests_ptr: int, h_in):
        """The synthesis on a word buffer that is on the device already -- 8 state words, then the 16 * blocks message words
        -- with the digest stored to `digests_ptr` (8 words): a chain of syntheses hands H_out on as the next H_in without a
        copy.  `h_in` is the host's copy of the state, for the instance."""
        ctx = self.ctx
        self._call((C.c_void_p * SC.ADVICE_COLUMNS)(*[c.ptr for c in self.cols]), words_ptr, digests_ptr)
        out = np.empty(8, dtype=np.uint32)
        ctx._chk(ctx.lib.cq_dev_download(ctx.h, out.ctypes.data, digests_ptr, out.nbytes))
        self.state_words = self.digest_words = [out.tolist()]
        self.init_words = [[int(x) for x in h_in]]
        self.instance_words = self.digest_words[0] + self.init_words[0]
        self.instances = [_words_to_mont(self.instance_words)]
        return self.cols, self.instances

    @property
    def h_out(self):
        return self.digest_words[0]

    def _result(self):
        return self.instance_words


class Sha224Circuit(Sha256SegmentsCircuit):
    """SHA-224 of a message of exactly `blocks` padded blocks (the plan `sha224`): the methods take the message and pad it
    here, as Sha256BatchCircuit does.  All 8 words of the final state are public; the SHA-224 digest is the first 28 bytes."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, sha224(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks)]

    def _result(self):
        return self.digests[0][:28]


class Sha256MerkleCircuit(Sha256SegmentsCircuit):
    """The SHA-256 Merkle root over 2^depth private 32-byte leaves (node = SHA-256(left || right)); the root is public.
    The methods take the list of leaves.  Every node's children are wired and its padding block is pinned, so nothing but
    the leaves is free."""

    def __init__(self, ctx: Context, k: int, depth: int, **kw):
        self.depth = depth
        super().__init__(ctx, k, merkle_tree(depth), **kw)

    def _values(self, leaves):
        if len(leaves) != 1 << self.depth or any(len(leaf) != 32 for leaf in leaves):
            raise ValueError(f"{1 << self.depth} leaves of 32 bytes each")
        pairs = 1 << (self.depth - 1)
        return [_digest_words(leaves[2 * i]) + _digest_words(leaves[2 * i + 1]) for i in range(pairs)] + [[]] * (pairs - 1)

    def _result(self):
        return self.digests[0]


class Sha256MerklePathCircuit(Sha256SegmentsCircuit):
    """Membership under a SHA-256 Merkle root (node = SHA-256(left || right)): `paths` independent paths of `depth` levels;
    every root is public, the leaf, its position and the siblings are private.  The methods take, per path,
    (leaf, index, siblings): the 32-byte leaf -- with `leaf_blocks` the message of exactly that many padded blocks whose
    digest is the leaf, public iff `public_leaf` -- the leaf's index in [0, 2^depth), whose bit l says whether the running
    node is the right half at level l, and the `depth` 32-byte siblings bottom-up.  The siblings, the direction bits and
    a 32-byte leaf are constrained to nothing but the hashes they enter; a `leaf_blocks` message's padding is private
    words, as in Sha256BatchCircuit."""

    def __init__(self, ctx: Context, k: int, depth: int, paths: int = 1, leaf_blocks: int | None = None, public_leaf: bool = False, **kw):
        self.depth, self.paths, self.leaf_blocks = depth, paths, leaf_blocks
        super().__init__(ctx, k, merkle_path(depth, paths, leaf_blocks, public_leaf), **kw)

    def _inputs(self, items, shared=(), bits=()):
        if shared or bits:
            raise ValueError("a Merkle path takes (leaf, index, siblings) per path and nothing else")
        if len(items) != self.paths:
            raise ValueError(f"{self.paths} paths, not {len(items)}")
        values, shared, bits = [], [], []
        for leaf, index, siblings in items:
            if not 0 <= index < 1 << self.depth or len(siblings) != self.depth or any(len(s) != 32 for s in siblings):
                raise ValueError(f"an index below 2^{self.depth} and {self.depth} siblings of 32 bytes each")
            if self.leaf_blocks is None:
                if len(leaf) != 32:
                    raise ValueError("a leaf of 32 bytes")
                shared += _digest_words(leaf)
            else:
                values.append(SC.pad(leaf, self.leaf_blocks))
            values += [[]] * self.depth
            for level, sibling in enumerate(siblings):
                shared += _digest_words(sibling)
                bits.append(index >> level & 1)
        return values, shared, bits

    @property
    def roots(self):
        """The roots of the last synthesis, one per path, 32 big-endian bytes each."""
        per_path = len(self.plan.public) // self.paths  # the public segments of a path: its leaf digest if public, then its root
        return self.digests[per_path - 1:: per_path]

    def _result(self):
        return self.roots


class HmacSha256Circuit(Sha256SegmentsCircuit):
    """HMAC-SHA-256 of a private message of exactly `message_bytes` bytes under a private key of exactly `key_bytes` <= 64
    bytes, both multiples of 4 (the plan `hmac_sha256`); the tag is public, with `commit_key` SHA-256(key) too.  The methods
    take (key, message) as bytes.  Forced: the key block's zero padding and both pads (Const words and Xor units), the
    message's padding, the wiring of the inner digest into the outer hash, and that both hashes -- and the commitment -- use
    one key.  Not offered: keys above 64 bytes (a Plan with DigestWord operands a user can write) and byte lengths that
    are no multiple of 4 (the variable-length variant, which does not combine with plan variants)."""

    def __init__(self, ctx: Context, k: int, key_bytes: int, message_bytes: int, commit_key: bool = False, **kw):
        self.key_bytes, self.message_bytes, self.commit_key = key_bytes, message_bytes, commit_key
        super().__init__(ctx, k, hmac_sha256(key_bytes, message_bytes, commit_key), **kw)

    def _inputs(self, key, message=None):
        key, message = (bytes(x) for x in (key if message is None else (key, message)))  # (key, message) as one pair too
        if (len(key), len(message)) != (self.key_bytes, self.message_bytes):
            raise ValueError(f"a key of {self.key_bytes} bytes and a message of {self.message_bytes}, not {len(key)} and {len(message)}")
        words = lambda data: list(struct.unpack(f">{len(data) // 4}I", data))
        return [words(message)] + [[]] * (len(self.plan.segments) - 1), words(key), []

    def tag(self) -> bytes:
        """The tag of the last synthesis, 32 bytes: what `prove` returns beside the proof.  The public inputs are the tag's
        words, then with `commit_key` those of SHA-256(key)."""
        return self.digests[0]

    def key_commitment(self) -> bytes:
        """SHA-256(key) of the last synthesis (`commit_key` only)."""
        if not self.commit_key:
            raise ValueError("the circuit was built without commit_key")
        return self.digests[1]

    def _result(self):
        return self.tag()
