"""The SHA-512 / SHA-384 compression circuit: proves that SHA-512(message) = digest (or SHA-384's) for messages of
exactly `blocks` padded 128-byte blocks each ("SHA-512 and SHA-384 circuits").

The digest words (64 bits each: 8 per SHA-512 message, 6 per SHA-384 message) are the instance column, the message words
are private advice, the initial hash values and the round constants are fixed cells tied to their uses by copy
constraints.  The cells are laid out by the table of csrc/sha512_layout.hpp, read here through `cq_sha512_layout`; the
witness is synthesised on the GPU by `cq_sha512_synthesize_dev`.  Several messages in one proof are independent segments
one behind another; sha512_segments.py wires segments to each other and to constants.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple

import numpy as np

from . import plonk as GP
from . import sha2_family as F
from ._lib import constants
from ._marshal import fr_to_mont
from .context import Context
from .sha256_circuit import _build_key, _close_key, _mont_column  # noqa: F401
from .sha2_family import ADVICE_COLUMNS, FIXED, FORM_PAIR, FORM_SPREAD, FORM_WORD, GATES, PAIRS, SRC, Cell  # noqa: F401

_CQ = constants()
REGION_ROWS, BLOCK_REGIONS, TAIL_REGIONS = (_CQ["CQ_SHA512_" + s] for s in ("REGION_ROWS", "BLOCK_REGIONS", "TAIL_REGIONS"))
MIN_TABLE_BITS, MAX_TABLE_BITS, CHUNKS = _CQ["CQ_SHA512_MIN_TABLE_BITS"], _CQ["CQ_SHA512_MAX_TABLE_BITS"], _CQ["CQ_SHA512_CHUNKS"]
VARIANT_512, VARIANT_384 = _CQ["CQ_SHA512_VARIANT_512"], _CQ["CQ_SHA512_VARIANT_384"]
ROUNDS = BLOCK_REGIONS - 4
WORD_BITS = 64

K512 = [
    0x428A2F98D728AE22, 0x7137449123EF65CD, 0xB5C0FBCFEC4D3B2F, 0xE9B5DBA58189DBBC, 0x3956C25BF348B538, 0x59F111F1B605D019,
    0x923F82A4AF194F9B, 0xAB1C5ED5DA6D8118, 0xD807AA98A3030242, 0x12835B0145706FBE, 0x243185BE4EE4B28C, 0x550C7DC3D5FFB4E2,
    0x72BE5D74F27B896F, 0x80DEB1FE3B1696B1, 0x9BDC06A725C71235, 0xC19BF174CF692694, 0xE49B69C19EF14AD2, 0xEFBE4786384F25E3,
    0x0FC19DC68B8CD5B5, 0x240CA1CC77AC9C65, 0x2DE92C6F592B0275, 0x4A7484AA6EA6E483, 0x5CB0A9DCBD41FBD4, 0x76F988DA831153B5,
    0x983E5152EE66DFAB, 0xA831C66D2DB43210, 0xB00327C898FB213F, 0xBF597FC7BEEF0EE4, 0xC6E00BF33DA88FC2, 0xD5A79147930AA725,
    0x06CA6351E003826F, 0x142929670A0E6E70, 0x27B70A8546D22FFC, 0x2E1B21385C26C926, 0x4D2C6DFC5AC42AED, 0x53380D139D95B3DF,
    0x650A73548BAF63DE, 0x766A0ABB3C77B2A8, 0x81C2C92E47EDAEE6, 0x92722C851482353B, 0xA2BFE8A14CF10364, 0xA81A664BBC423001,
    0xC24B8B70D0F89791, 0xC76C51A30654BE30, 0xD192E819D6EF5218, 0xD69906245565A910, 0xF40E35855771202A, 0x106AA07032BBD1B8,
    0x19A4C116B8D2D0C8, 0x1E376C085141AB53, 0x2748774CDF8EEB99, 0x34B0BCB5E19B48A8, 0x391C0CB3C5C95A63, 0x4ED8AA4AE3418ACB,
    0x5B9CCA4F7763E373, 0x682E6FF3D6B2B8A3, 0x748F82EE5DEFB2FC, 0x78A5636F43172F60, 0x84C87814A1F0AB72, 0x8CC702081A6439EC,
    0x90BEFFFA23631E28, 0xA4506CEBDE82BDE9, 0xBEF9A3F7B2C67915, 0xC67178F2E372532B, 0xCA273ECEEA26619C, 0xD186B8C721C0C207,
    0xEADA7DD6CDE0EB1E, 0xF57D4F7FEE6ED178, 0x06F067AA72176FBA, 0x0A637DC5A2C898A6, 0x113F9804BEF90DAE, 0x1B710B35131C471B,
    0x28DB77F523047D84, 0x32CAAB7B40C72493, 0x3C9EBE0A15C9BEBC, 0x431D67C49C100D4C, 0x4CC5D4BECB3E42B6, 0x597F299CFC657E2A,
    0x5FCB6FAB3AD6FAEC, 0x6C44198C4A475817,
]
IV512 = [0x6A09E667F3BCC908, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1,
         0x510E527FADE682D1, 0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179]
IV384 = [0xCBBB9D5DC1059ED8, 0x629A292A367CD507, 0x9159015A3070DD17, 0x152FECD8F70E5939,
         0x67332667FFC00B31, 0x8EB44A8768581511, 0xDB0C2E0D64F98FA7, 0x47B5481DBEFA4FA4]
IV = {VARIANT_512: IV512, VARIANT_384: IV384}
DIGEST_WORDS = {VARIANT_512: 8, VARIANT_384: 6}
FAMILY = F.Family(WORD_BITS, "CQ_SHA512_", "cq_sha512_layout", (((28, 34, 39), None), ((14, 18, 41), None), ((1, 8), 7), ((19, 61), 6)),
                  tuple(K512), chunk_length_checked=True)
SPREAD_ONES = FAMILY.spread_ones  # the spread form of 2^64 - 1
# the XOR variant (plans with an Xor word, sha512_xor.py): one selector behind `const`, one gate behind the others; a unit
# is XOR_REGIONS regions behind the last segment, and the gate reads cells the layout has already ("XOR-wired
# message words on the 64-bit circuit")
GATES_XOR = GATES + ("xor_word",)
FIXED_XOR = FIXED + ("q_xor",)
XOR_REGIONS, XOR_WORDS = _CQ["CQ_SHA512_XOR_REGIONS"], _CQ["CQ_SHA512_XOR_WORDS"]


def layout():
    """The layout table of csrc/sha512_layout.hpp as the library exports it (host only: no GPU needed)."""
    return F.layout(FAMILY)


def rows_for(blocks: int) -> int:
    return F.rows_for(FAMILY, blocks)


def pad(message: bytes, blocks: int | None = None):
    """SHA-512 / SHA-384 padding: the big-endian 64-bit words of message || 0x80 || zeros || 128-bit bit length;
    ValueError when `blocks` is given and the padded message is not that many blocks."""
    message = bytes(message)
    padded = message + b"\x80" + b"\x00" * ((111 - len(message)) % 128) + (8 * len(message)).to_bytes(16, "big")
    if blocks is not None and len(padded) != 128 * blocks:
        raise ValueError(f"a message of {len(message)} bytes pads to {len(padded) // 128} blocks, the circuit has {blocks}")
    return list(struct.unpack(f">{len(padded) // 8}Q", padded))


class Description(NamedTuple):
    """The circuit without a device: constraint system, fixed columns (integers, by name; `fixed_names` is their
    allocation order), copy constraints ((column, row), (column, row)), and per segment its block count and variant."""

    cs: GP.ConstraintSystem
    advice: list
    fixed_columns: dict
    fixed: dict
    instance: GP.Column
    copies: list
    cells: list
    table_bits: int
    blocks_list: tuple
    variants: tuple
    k: int
    fixed_names: tuple = FIXED

    @property
    def blocks(self):
        """The block count of a one-message description."""
        (b,) = self.blocks_list
        return b


def _field_of(cell: Cell, tb: int):
    """(bit offset, length) of the cell's field within its word at table size 2^tb; a chunk that starts at or above
    bit 64 has length 0."""
    return F.field_of(FAMILY, cell, tb)


def describe(k: int, blocks: int, table_bits: int = 12, dense="dense", spread="spread", variant: int = VARIANT_512) -> Description:
    """One message.  `dense` / `spread` stand for the two static tables (any objects; the proving key wants StaticTable
    handles)."""
    return describe_batch(k, [blocks], [variant], table_bits, dense, spread)


def describe_batch(k: int, blocks_list, variants=None, table_bits: int = 12, dense="dense", spread="spread") -> Description:
    """Several independent messages, segment after segment in row order; `variants` defaults to SHA-512 for all."""
    blocks_list = tuple(int(b) for b in blocks_list)
    variants = tuple(VARIANT_512 for _ in blocks_list) if variants is None else tuple(int(v) for v in variants)
    if not MIN_TABLE_BITS <= table_bits <= MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{MIN_TABLE_BITS}, {MAX_TABLE_BITS}]: the widest piece has {MIN_TABLE_BITS} bits")
    if not blocks_list or len(variants) != len(blocks_list) or min(blocks_list) < 1 or any(v not in IV for v in variants):
        raise ValueError("one block count of at least 1 and one variant (VARIANT_512 or VARIANT_384) per message")
    cs, adv, fcol, inst, cells, word = _constraint_system(table_bits, dense, spread)
    n = 1 << k
    rows = sum(rows_for(b) for b in blocks_list)
    usable = n - (cs.blinding_factors() + 1)
    if rows > usable:
        raise ValueError(f"blocks {list(blocks_list)} need {rows} rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in FIXED}
    copies = []
    first_region = public = 0
    for blocks, variant in zip(blocks_list, variants):
        _assign_segment(fixed, copies, first_region, blocks, variant, public, table_bits, adv, fcol, inst, cells, word)
        first_region += BLOCK_REGIONS * blocks + TAIL_REGIONS
        public += DIGEST_WORDS[variant]
    return Description(cs, adv, fcol, fixed, inst, copies, cells, table_bits, blocks_list, variants, k)


def _constraint_system(tb: int, dense, spread, xor: bool = False):
    """`xor`: the variant for plans with XOR-wired message words -- the fixed column `q_xor` and the gate `xor_word`;
    everything else is the plain system, built by the same lines."""
    if not xor:
        return F.finish(F.base_system(FAMILY, tb), dense, spread)
    system = F.base_system(FAMILY, tb, FIXED_XOR)
    system.polys["xor_word"] = F.xor_word(system)
    out = F.finish(system, dense, spread, GATES_XOR)
    # the gate adds the dense CHP_EVEN cells that hold a chunk below bit 64 and one fixed column to the queries, nothing to
    # the blinding rows or the degree: a dense column has at most 16 distinct rotations inside a region, X has more
    assert (system.cs.blinding_factors(), system.cs.degree()) == (20, 4)
    return out


def _assign_segment(fixed, copies, first_region, blocks, variant, public, tb, adv, fcol, inst, cells, word, pinned=None, public_words=None):
    """F.assign_segment for a SHA-512 / SHA-384 chain: instance rows public .. public + public_words - 1 are copied to the
    first digest words of its tail.  `pinned`: H[0..7] of the state it starts from, each a constant pinned through `const`
    or None for a cell the caller ties (or leaves free) itself; the default is the variant's initial hash value.
    `public_words`: 0 .. 8, by default DIGEST_WORDS[variant]."""
    digest_words = DIGEST_WORDS[variant] if public_words is None else public_words
    F.assign_segment(FAMILY, fixed, copies, first_region, blocks, IV[variant] if pinned is None else pinned,
                     lambda h: public + h if h < digest_words else None, False, tb, adv, fcol, inst, cells, word)


def usable_rows(k: int, table_bits: int = 12) -> int:
    """The rows of 2^k a circuit may use: all but the blinding rows and the one behind them."""
    return F.usable_rows(FAMILY, k, table_bits)


def max_blocks(k: int, table_bits: int = 12) -> int:
    """The largest block count of one message whose rows fit the usable rows of 2^k."""
    return F.max_blocks(FAMILY, k, table_bits)


class Sha512BatchCircuit:
    """Proving key and GPU witness synthesis for several independent messages in one proof: message j has exactly
    blocks_list[j] padded blocks and is hashed with SHA-512 or SHA-384 (variants[j]; default SHA-512).  The instance column
    holds the digest words of every message in order, 8 per SHA-512 message and 6 per SHA-384 message.  One key proves
    one list of message lengths."""

    rows_per_block = BLOCK_REGIONS * REGION_ROWS

    def __init__(self, ctx: Context, k: int, blocks_list, variants=None, table_bits: int = 12, setup: str = "toxic",
                 seed: int = 0x5348413243515F):
        _build_key(self, ctx, k, table_bits, setup, seed,
                   lambda dense, spread: describe_batch(k, blocks_list, variants, table_bits, dense, spread))
        self.blocks_list, self.variants = self.description.blocks_list, self.description.variants
        self.rows = sum(rows_for(b) for b in self.blocks_list)
        self.state_words = None
        self.digest_words = None

    # ---- host side ----
    def pad(self, messages):
        """The padded words of every message, back to back."""
        messages = list(messages)
        if len(messages) != len(self.blocks_list):
            raise ValueError(f"{len(messages)} messages, the circuit has {len(self.blocks_list)}")
        return [x for m, b in zip(messages, self.blocks_list) for x in pad(m, b)]

    # ---- witness ----
    def synthesize(self, messages):
        """Fills the advice columns on the GPU (cq_sha512_synthesize_dev); returns (device columns, instances)."""
        ctx = self.ctx
        words = np.array(self.pad(messages), dtype=np.uint64)
        seg_blocks, seg_variant = np.array(self.blocks_list, dtype=np.uint32), np.array(self.variants, dtype=np.uint32)
        states = np.zeros(8 * len(seg_blocks), dtype=np.uint64)
        arr = (C.c_void_p * ADVICE_COLUMNS)(*[c.ptr for c in self.cols])
        ctx._chk(ctx.lib.cq_sha512_synthesize_dev(ctx.h, self.table_bits, seg_blocks.ctypes.data, len(seg_blocks), seg_variant.ctypes.data,
                                                  words.ctypes.data, self.n, arr, states.ctypes.data))
        self.state_words = [[int(x) for x in states[8 * j: 8 * j + 8]] for j in range(len(seg_blocks))]
        self.digest_words = [x for s, v in zip(self.state_words, self.variants) for x in s[:DIGEST_WORDS[v]]]
        return self.cols, self.instances

    @property
    def instances(self):
        return [np.stack([fr_to_mont(x) for x in self.digest_words])]

    @property
    def digests(self):
        """The digest of every message of the last synthesis: 64 or 48 big-endian bytes."""
        return [struct.pack(f">{DIGEST_WORDS[v]}Q", *s[:DIGEST_WORDS[v]]) for s, v in zip(self.state_words, self.variants)]

    digest = digests

    def check(self, messages, max_failures: int = 64):
        cols, inst = self.synthesize(messages)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, messages):
        cols, inst = self.synthesize(messages)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, messages, seed: int = 1):
        """(proof bytes, digests): create_proof with the digest words as the public inputs."""
        cols, inst = self.synthesize(messages)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self.digest

    close = _close_key


class Sha512Circuit(Sha512BatchCircuit):
    """Proving key and GPU witness synthesis for SHA-512 over exactly `blocks` padded 128-byte blocks at 2^k rows.  One
    key proves one message length; the methods take the message itself, and `digest` is its 64 bytes."""

    variant = VARIANT_512

    def __init__(self, ctx: Context, k: int, blocks: int | None = None, table_bits: int = 12, setup: str = "toxic",
                 seed: int = 0x5348413243515F):
        if blocks is None:
            blocks = max_blocks(k, table_bits)
        if blocks < 1:
            raise ValueError(f"2^{k} rows hold no block ({rows_for(1)} rows are needed)")
        super().__init__(ctx, k, [blocks], [self.variant], table_bits, setup, seed)
        self.blocks = blocks

    def pad(self, message: bytes):
        return pad(message, self.blocks)

    @property
    def digest(self) -> bytes:
        """The instance words of the last synthesised message as big-endian bytes."""
        return self.digests[0]


class Sha384Circuit(Sha512Circuit):
    """The same for SHA-384: the chain starts from SHA-384's initial hash value and the instance column holds the first
    six words of the final state; `digest` is its 48 bytes."""

    variant = VARIANT_384
