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
from ._lib import constants, load
from ._marshal import fr_to_mont
from .context import Context
from .sha256_circuit import ADVICE_COLUMNS, FORM_PAIR, FORM_SPREAD, FORM_WORD, PAIRS, SRC, Cell, _build_key, _close_key, _mont_column  # noqa: F401

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
SPREAD_ONES = (4 ** WORD_BITS - 1) // 3  # the spread form of 2^64 - 1

# gate polynomials in cs.gates order (the `index` of a FAIL_GATE finding): the 23 kinds of the SHA-256 circuit, every one
# anchored on row 0 of a region
GATES = ("a_word", "a_spread", "e_word", "e_spread", "w_word", "Sigma0_even_odd", "Sigma0_word", "Sigma1_even_odd", "Sigma1_word",
         "sigma0_even_odd", "sigma0_word", "sigma1_even_odd", "sigma1_word", "maj_even_odd", "maj_word", "chp_even_odd",
         "chq_even_odd", "ch_word", "e_add", "a_add", "w_add", "chain_a", "chain_e")
# fixed columns in allocation order
FIXED = ("q_all", "q_f3", "q_round", "q_sched", "q_chain") + tuple(f"scale{j}" for j in range(PAIRS)) + ("const",)


def layout():
    """The layout table of csrc/sha512_layout.hpp as the library exports it (host only: no GPU needed)."""
    lib = load()
    count = C.c_size_t()
    assert lib.cq_sha512_layout(None, 0, C.byref(count)) == 0
    words = _CQ["CQ_SHA256_CELL_WORDS"]
    assert words == len(Cell._fields)
    arr = (C.c_uint32 * (words * count.value))()
    assert lib.cq_sha512_layout(arr, count.value, C.byref(count)) == 0
    return [Cell(*arr[words * i: words * (i + 1)]) for i in range(count.value)]


def rows_for(blocks: int) -> int:
    return (BLOCK_REGIONS * blocks + TAIL_REGIONS) * REGION_ROWS


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
    off = cell.offset + cell.per_table_bits * tb
    return off, (cell.len if cell.len else max(0, min(tb, WORD_BITS - off)))


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


def _constraint_system(tb: int, dense, spread):
    cells = layout()
    cs = GP.ConstraintSystem()
    adv = [cs.advice_column() for _ in range(ADVICE_COLUMNS)]
    fcol = {name: cs.fixed_column() for name in FIXED}
    inst = cs.instance_column()
    X = adv[2 * PAIRS]
    for c in (X, fcol["const"], inst):
        cs.enable_equality(c)

    pieces = {s: sorted((c for c in cells if c.kind == s and c.form == FORM_PAIR and c.len), key=lambda c: c.offset) for s in SRC.values()}
    # a chunk that starts at or above bit 64 holds zero (the length lookup of its cell says so): the gates leave it out
    chunks = {s: sorted((c for c in cells if c.kind == s and c.form == FORM_PAIR and not c.len and c.per_table_bits * tb < WORD_BITS),
                        key=lambda c: c.per_table_bits) for s in SRC.values()}
    word = {(c.kind, c.form): c for c in cells if c.form != FORM_PAIR}

    def q(cell, spread_form=False, regions_back=0):
        return cs.query_advice(adv[cell.column + (1 if spread_form else 0)], cell.row - REGION_ROWS * regions_back)

    def lin(terms):
        acc = None
        for coef, e in terms:
            t = e if coef == 1 else e * coef
            acc = t if acc is None else acc + t
        return acc

    def w(name, form=FORM_WORD, back=0):
        return q(word[(SRC[name], form)], regions_back=back)

    def rotated_spread(name, rots, shift):
        """sum over the rotations (and the one shift) of the word's spread form, from its pieces' spread cells"""
        terms = []
        for p in pieces[SRC[name]]:
            for r in rots:
                assert p.offset + p.len <= r or p.offset >= r, "a piece straddles a rotation"
                terms.append((4 ** ((p.offset - r) % WORD_BITS), q(p, True)))
            if shift is not None and p.offset >= shift:
                terms.append((4 ** (p.offset - shift), q(p, True)))
            assert shift is None or p.offset + p.len <= shift or p.offset >= shift, "a piece straddles the shift"
        return lin(terms)

    def even_odd(name):
        return lin([(4 ** (c.per_table_bits * tb) * m, q(c, True)) for m, s in ((1, name + "_EVEN"), (2, name + "_ODD")) for c in chunks[SRC[s]]])

    def from_chunks(*names):
        return lin([(2 ** (c.per_table_bits * tb), q(c)) for s in names for c in chunks[SRC[s]]])

    def carry(name):
        (c,) = pieces[SRC[name]]
        return q(c) * (1 << WORD_BITS)

    sel = {name: cs.query_fixed(fcol[name]) for name in ("q_all", "q_f3", "q_round", "q_sched", "q_chain")}
    polys = {}
    for name, s in (("a", "A"), ("e", "E"), ("w", "W")):
        polys[name + "_word"] = sel["q_all"] * (w(s) - lin([(2 ** p.offset, q(p)) for p in pieces[SRC[s]]]))
        if s != "W":
            polys[name + "_spread"] = sel["q_all"] * (w(s, FORM_SPREAD) - lin([(4 ** p.offset, q(p, True)) for p in pieces[SRC[s]]]))
    for gate, s, src, rots, shift in (("Sigma0", "S0", "A", (28, 34, 39), None), ("Sigma1", "S1", "E", (14, 18, 41), None),
                                      ("sigma0", "G0", "W", (1, 8), 7), ("sigma1", "G1", "W", (19, 61), 6)):
        polys[gate + "_even_odd"] = sel["q_all"] * (rotated_spread(src, rots, shift) - even_odd(s))
        polys[gate + "_word"] = sel["q_all"] * (w(s + "_EVEN") - from_chunks(s + "_EVEN"))
    sa, se = (lambda back: w("A", FORM_SPREAD, back)), (lambda back: w("E", FORM_SPREAD, back))
    polys["maj_even_odd"] = sel["q_f3"] * (sa(0) + sa(1) + sa(2) - even_odd("MAJ"))
    polys["maj_word"] = sel["q_f3"] * (w("MAJ_ODD") - from_chunks("MAJ_ODD"))
    polys["chp_even_odd"] = sel["q_f3"] * (se(0) + se(1) - even_odd("CHP"))
    polys["chq_even_odd"] = sel["q_f3"] * (GP.Expression.constant(SPREAD_ONES) - se(0) + se(2) - even_odd("CHQ"))
    polys["ch_word"] = sel["q_f3"] * (w("CH") - from_chunks("CHP_ODD", "CHQ_ODD"))
    # T1 = h + Sigma1(e) + Ch(e, f, g) + K + W with e, f, g, h = e_(r-1) .. e_(r-4); e_r = d + T1; a_r = T1 + Sigma0 + Maj
    t1 = w("E", back=4) + w("S1_EVEN", back=1) + w("CH", back=1) + w("K") + w("W")
    polys["e_add"] = sel["q_round"] * (w("E") + carry("CARRY_E") - w("A", back=4) - t1)
    polys["a_add"] = sel["q_round"] * (w("A") + carry("CARRY_A") - t1 - w("S0_EVEN", back=1) - w("MAJ_ODD", back=1))
    polys["w_add"] = sel["q_sched"] * (w("W") + carry("CARRY_W") - w("G1_EVEN", back=2) - w("W", back=7) - w("G0_EVEN", back=15) - w("W", back=16))
    for name, s in (("a", "A"), ("e", "E")):  # H + (a .. h): the same slot one block and four regions back
        polys["chain_" + name] = sel["q_chain"] * (w(s) + carry("CARRY_" + s) - w(s, back=BLOCK_REGIONS) - w(s, back=4))
    assert tuple(polys) != () and set(polys) == set(GATES)
    for name in GATES:
        cs.create_gate(name, [polys[name]])
    # lookups 0 .. 7: (dense_j, spread_j) in (dense, spread); 8 .. 15: dense_j * scale_j in dense -- the length check
    for j in range(PAIRS):
        cs.lookup_static(f"pair{j}", [(adv[2 * j], dense), (adv[2 * j + 1], spread)])
    for j in range(PAIRS):
        cs.lookup_static(f"length{j}", [(cs.query_advice(adv[2 * j]) * cs.query_fixed(fcol[f"scale{j}"]), dense)])
    return cs, adv, fcol, inst, cells, word


def _assign_segment(fixed, copies, first_region, blocks, variant, public, tb, adv, fcol, inst, cells, word, pinned=None, public_words=None):
    """The fixed cells and the copies of one chain of `blocks` blocks whose regions start at `first_region`: selectors and
    scales, the round constants, the state it starts from on its first four regions (no q_chain before its second block),
    and the copies of instance rows public .. public + public_words - 1 to the first digest words of its tail.  `pinned`:
    H[0..7] of the state, each a constant pinned through `const` or None for a cell the caller ties (or leaves free) itself;
    the default is the variant's initial hash value.  `public_words`: 0 .. 8, by default DIGEST_WORDS[variant]."""
    X = adv[2 * PAIRS]
    regions = BLOCK_REGIONS * blocks + TAIL_REGIONS
    g = np.arange(regions)
    in_block, base = g % BLOCK_REGIONS, (first_region + g) * REGION_ROWS
    is_tail = g >= BLOCK_REGIONS * blocks
    is_round = (in_block >= 4) & ~is_tail
    fixed["q_all"][base] = 1
    fixed["q_f3"][base[in_block >= 2]] = 1
    fixed["q_round"][base[is_round]] = 1
    fixed["q_sched"][base[is_round & (in_block >= 20)]] = 1
    fixed["q_chain"][base[(in_block < 4) & (g >= BLOCK_REGIONS)]] = 1
    for c in cells:
        if c.form == FORM_PAIR:  # dense * 2^(tb - len) is in the table: dense < 2^len; a chunk past the word (len 0) is zero
            _, ln = _field_of(c, tb)
            fixed[f"scale{c.column // 2}"][base + c.row] = 1 << (tb - ln)
    krow = word[(SRC["K"], FORM_WORD)].row
    arow, erow = word[(SRC["A"], FORM_WORD)].row, word[(SRC["E"], FORM_WORD)].row
    kvals = np.array(K512, dtype=np.uint64)
    rb = base[is_round]
    fixed["const"][rb + krow] = kvals[(in_block[is_round] - 4)]
    copies += [((fcol["const"], int(r) + krow), (X, int(r) + krow)) for r in rb]
    init = IV[variant] if pinned is None else pinned
    digest_words = DIGEST_WORDS[variant] if public_words is None else public_words
    for i in range(4):  # region i of the first block holds a_(i-4) = H[3 - i] and e_(i-4) = H[7 - i]
        head, tail = int(base[i]), int(base[BLOCK_REGIONS * blocks + i])
        for row, h in ((arow, 3 - i), (erow, 7 - i)):
            if init[h] is not None:
                fixed["const"][head + row] = init[h]
                copies.append(((fcol["const"], head + row), (X, head + row)))
            if h < digest_words:
                copies.append(((inst, public + h), (X, tail + row)))


def usable_rows(k: int, table_bits: int = 12) -> int:
    """The rows of 2^k a circuit may use: all but the blinding rows and the one behind them."""
    return (1 << k) - (_constraint_system(table_bits, "dense", "spread")[0].blinding_factors() + 1)


def max_blocks(k: int, table_bits: int = 12) -> int:
    """The largest block count of one message whose rows fit the usable rows of 2^k."""
    return (usable_rows(k, table_bits) // REGION_ROWS - TAIL_REGIONS) // BLOCK_REGIONS


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
