"""The SHA-256 compression circuit: proves that SHA-256(message) = digest for a message of exactly `blocks` padded
64-byte blocks ("SHA-256 compression circuit").

The digest (8 words) is the instance column, the message words are private advice, the IV and the round constants are
fixed cells tied to their uses by copy constraints.  The cells are laid out by the table of csrc/sha256_layout.hpp, read
here through `cq_sha256_layout`; the witness is synthesised on the GPU by `cq_sha256_synthesize_dev`.
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
from .params import ParamsKZG, StaticTable, TableConfig
from .proving_key import ProvingKey
from .sha2_family import ADVICE_COLUMNS, FIXED, FORM_PAIR, FORM_SPREAD, FORM_WORD, GATES, PAIRS, SRC, Cell  # noqa: F401

_CQ = constants()
REGION_ROWS, BLOCK_REGIONS, TAIL_REGIONS = (_CQ["CQ_SHA256_" + s] for s in ("REGION_ROWS", "BLOCK_REGIONS", "TAIL_REGIONS"))
MIN_TABLE_BITS, MAX_TABLE_BITS = _CQ["CQ_SHA256_MIN_TABLE_BITS"], _CQ["CQ_SHA256_MAX_TABLE_BITS"]

K256 = [
    0x428A2F98, 0x71374491, 0xB5C0FBCF, 0xE9B5DBA5, 0x3956C25B, 0x59F111F1, 0x923F82A4, 0xAB1C5ED5,
    0xD807AA98, 0x12835B01, 0x243185BE, 0x550C7DC3, 0x72BE5D74, 0x80DEB1FE, 0x9BDC06A7, 0xC19BF174,
    0xE49B69C1, 0xEFBE4786, 0x0FC19DC6, 0x240CA1CC, 0x2DE92C6F, 0x4A7484AA, 0x5CB0A9DC, 0x76F988DA,
    0x983E5152, 0xA831C66D, 0xB00327C8, 0xBF597FC7, 0xC6E00BF3, 0xD5A79147, 0x06CA6351, 0x14292967,
    0x27B70A85, 0x2E1B2138, 0x4D2C6DFC, 0x53380D13, 0x650A7354, 0x766A0ABB, 0x81C2C92E, 0x92722C85,
    0xA2BFE8A1, 0xA81A664B, 0xC24B8B70, 0xC76C51A3, 0xD192E819, 0xD6990624, 0xF40E3585, 0x106AA070,
    0x19A4C116, 0x1E376C08, 0x2748774C, 0x34B0BCB5, 0x391C0CB3, 0x4ED8AA4A, 0x5B9CCA4F, 0x682E6FF3,
    0x748F82EE, 0x78A5636F, 0x84C87814, 0x8CC70208, 0x90BEFFFA, 0xA4506CEB, 0xBEF9A3F7, 0xC67178F2,
]
IV256 = [0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19]
FAMILY = F.Family(32, "CQ_SHA256_", "cq_sha256_layout", (((2, 13, 22), None), ((6, 11, 25), None), ((7, 18), 3), ((17, 19), 10)),
                  tuple(K256), chunk_length_checked=False)
SPREAD_ONES = FAMILY.spread_ones  # the spread form of 0xFFFFFFFF

# the choice variant of the constraint system (plans with a Choice word, sha256_segments.py): one selector behind `const`,
# two gates behind the others, and three cells in the rows column Y leaves free in a region
GATES_CHOICE = GATES + ("choice", "choice_bit")
FIXED_CHOICE = FIXED + ("q_choice",)
CHOICE_ROW_ZERO, CHOICE_ROW_ONE, CHOICE_ROW_BIT = (_CQ["CQ_SHA256_CHOICE_ROW_" + s] for s in ("ZERO", "ONE", "BIT"))
# the variable-length variant (sha256_varlen.py): six selectors behind `const`, thirteen gates behind the others, equality
# on column Y; its cells sit in rows 4 .. 7 of Y, in pair slot 7 of rows 0 and 1, and -- in a message-word region, whose
# schedule carry nothing reads -- in the carry's slot ("Variable-length messages")
GATES_VARLEN = GATES + ("var_m_bool", "var_b_bool", "var_c0_bool", "var_c1_bool", "var_c_product", "var_len", "var_boundary",
                        "var_pad_zero", "var_length_word", "var_last_final", "var_carry", "var_final", "var_select")
FIXED_VARLEN = FIXED + ("q_vpad", "q_vlength", "q_vlast", "q_vcarry", "q_vfinal", "q_vsum")
VAR = {name[len("CQ_SHA256_VAR_"):]: v for name, v in _CQ.items() if name.startswith("CQ_SHA256_VAR_")}
# the XOR variant (plans with an Xor word, sha256_segments.py): one selector behind `const`, one gate behind the others; a
# unit is XOR_REGIONS regions behind the last segment, and the gate reads cells the layout has already (DESIGN.md,
# "XOR-wired message words")
GATES_XOR = GATES + ("xor_word",)
FIXED_XOR = FIXED + ("q_xor",)
XOR_REGIONS, XOR_WORDS = _CQ["CQ_SHA256_XOR_REGIONS"], _CQ["CQ_SHA256_XOR_WORDS"]


def layout():
    """The layout table of csrc/sha256_layout.hpp as the library exports it (host only: no GPU needed)."""
    return F.layout(FAMILY)


def rows_for(blocks: int) -> int:
    return F.rows_for(FAMILY, blocks)


def pad(message: bytes, blocks: int | None = None):
    """SHA-256 padding: the big-endian words of message || 0x80 || zeros || bit length; ValueError when `blocks` is given
    and the padded message is not that many blocks."""
    message = bytes(message)
    padded = message + b"\x80" + b"\x00" * ((55 - len(message)) % 64) + struct.pack(">Q", 8 * len(message))
    if blocks is not None and len(padded) != 64 * blocks:
        raise ValueError(f"a message of {len(message)} bytes pads to {len(padded) // 64} blocks, the circuit has {blocks}")
    return list(struct.unpack(f">{len(padded) // 4}I", padded))


class Description(NamedTuple):
    """The circuit without a device: constraint system, fixed columns (integers, by name; `fixed_names` is their
    allocation order: FIXED, or FIXED_CHOICE for the choice variant), copy constraints ((column, row), (column, row)) and
    the instance rows' sources."""

    cs: GP.ConstraintSystem
    advice: list
    fixed_columns: dict
    fixed: dict
    instance: GP.Column
    copies: list
    cells: list
    table_bits: int
    blocks: int
    k: int
    fixed_names: tuple = FIXED


def _field_of(cell: Cell, tb: int):
    """(bit offset, length) of the cell's field within its word at table size 2^tb."""
    return F.field_of(FAMILY, cell, tb)


def describe(k: int, blocks: int, table_bits: int = 12, dense="dense", spread="spread") -> Description:
    """Builds the constraint system from the layout table.  `dense` / `spread` stand for the two static tables (any
    objects; the proving key wants StaticTable handles)."""
    if not MIN_TABLE_BITS <= table_bits <= MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{MIN_TABLE_BITS}, {MAX_TABLE_BITS}]: the widest piece has {MIN_TABLE_BITS} bits")
    cs, adv, fcol, inst, cells, word = _constraint_system(table_bits, dense, spread)
    return _assign_fixed(k, blocks, table_bits, cs, adv, fcol, inst, cells, word)


def _constraint_system(tb: int, dense, spread, choice: bool = False, varlen: bool = False, xor: bool = False):
    """`choice`: the variant for plans with choice-wired message words -- the fixed column `q_choice`, equality on column
    Y and the gates `choice` and `choice_bit`; everything else is the plain system, built by the same lines.  `varlen`:
    the variant for messages of variable length -- the selectors of FIXED_VARLEN, equality on Y and the gates of
    GATES_VARLEN.  `xor`: the variant for plans with XOR-wired message words -- the fixed column `q_xor` and the gate
    `xor_word`.  The variants do not combine."""
    if choice and varlen:
        raise ValueError("a variable-length segment does not combine with choice-wired words")
    if xor and (choice or varlen):
        raise ValueError("XOR-wired words do not combine with choice-wired words or a variable-length segment")
    names = FIXED_CHOICE if choice else FIXED_VARLEN if varlen else FIXED_XOR if xor else FIXED
    system = F.base_system(FAMILY, tb, names, equality_on_y=choice or varlen)
    cs, adv, fcol, cells, polys, w = system.cs, system.advice, system.fixed_columns, system.cells, system.polys, system.w
    Y = adv[2 * PAIRS + 1]
    if choice:  # W = x + d * (y - x) with d boolean: x, y, d in the rows of Y that no layout cell uses
        assert not any(c.column == Y.index and c.row in (CHOICE_ROW_ZERO, CHOICE_ROW_ONE, CHOICE_ROW_BIT) for c in cells)
        q_choice = cs.query_fixed(fcol["q_choice"])
        x, y, d = (cs.query_advice(Y, r) for r in (CHOICE_ROW_ZERO, CHOICE_ROW_ONE, CHOICE_ROW_BIT))
        polys["choice"] = q_choice * (w("W") - x - d * (y - x))
        polys["choice_bit"] = q_choice * (d * (GP.Expression.constant(1) - d))
    if varlen:
        _varlen_gates(cs, polys, cells, adv, fcol, w)
    if xor:  # W = e_r ^ e_(r-1): under q_f3 `chp_even_odd` makes the CHP_EVEN chunks the even bits of spread(e_r) + spread(e_(r-1))
        polys["xor_word"] = F.xor_word(system)
    out = F.finish(system, dense, spread, GATES_CHOICE if choice else GATES_VARLEN if varlen else GATES_XOR if xor else GATES)
    if xor:  # the gate adds three dense cells of row 6 and one fixed column to the queries, nothing to the blinding rows or the degree
        assert (cs.blinding_factors(), cs.degree()) == (20, 4)
    return out


def _varlen_gates(cs, polys, cells, adv, fcol, w):
    """The gates of GATES_VARLEN into `polys` ("Variable-length messages").  In the region of message word g,
    column Y: m_g (the word lies wholly inside the message), len_g (the message's bytes up to and with the word) and two
    bits c0, c1; e = c0 * c1 in the schedule carry's slot; d0, d1, the 12-bit halves of D, in pair slot 7 of rows 0 and 1.
    The cells of word g - 1 are one region up -- for word 0 of a block in the block's carry-in region.  b_g = m_(g-1) - m_g
    marks the boundary word, which holds r = 3 - c0 - 2 c1 bytes of the message (the integer D), 0x80 and zeros:
    W = 2^(8 (3 - r)) * (256 D + 128).  Every gate is anchored on row 0 of its region and has degree <= 4; Y is read at no
    rotation beyond two regions up."""
    Y = adv[2 * PAIRS + 1]
    free = {(Y.index, r) for r in range(4, REGION_ROWS)} | {(2 * VAR["SLOT_DATA"], r) for r in (0, 1)}
    assert not any((c.column, c.row) in free for c in cells), "the layout uses a cell of the variable-length gates"
    assert (2 * VAR["SLOT_PRODUCT"], 0) == next((c.column, c.row) for c in cells if c.kind == SRC["CARRY_W"])

    def y(row, regions_back=0):
        return cs.query_advice(Y, row - REGION_ROWS * regions_back)

    q_pad, q_length, q_last, q_carry, q_final, q_sum = (cs.query_fixed(fcol[name]) for name in FIXED_VARLEN[len(FIXED):])
    q_word = q_pad + q_length  # words 0 .. 14 and word 15: every message-word region
    one = GP.Expression.constant(1)
    m, ln, c0, c1 = (y(VAR["ROW_" + s]) for s in ("M", "LEN", "C0", "C1"))
    m_prev, len_prev, m_13 = y(VAR["ROW_M"], 1), y(VAR["ROW_LEN"], 1), y(VAR["ROW_M"], 2)
    e = cs.query_advice(adv[2 * VAR["SLOT_PRODUCT"]], 0)
    d0, d1 = (cs.query_advice(adv[2 * VAR["SLOT_DATA"]], r) for r in (0, 1))
    b = m_prev - m
    u = one + c0 * 255 + c1 * 65535 + e * (255 * 65535)  # (1 + 255 c0)(1 + 65535 c1) = 2^(8 (c0 + 2 c1))
    polys["var_m_bool"] = q_word * (m * (one - m))
    polys["var_b_bool"] = q_word * (b * (one - b))
    polys["var_c0_bool"] = q_word * (c0 * (one - c0))
    polys["var_c1_bool"] = q_word * (c1 * (one - c1))
    polys["var_c_product"] = q_word * (e - c0 * c1)
    polys["var_len"] = q_word * (ln - len_prev - m * 4 - b * (GP.Expression.constant(3) - c0 - c1 * 2))
    polys["var_boundary"] = q_word * (b * (w("W") - u * (d0 * 256 + d1 * (256 << 12) + GP.Expression.constant(128))))
    polys["var_pad_zero"] = q_pad * ((one - m_prev) * w("W"))  # behind the boundary word: zero, words 0 .. 14
    # word 15 behind the boundary: the bit length if word 13 is not message (this block is the final one: behind it the
    # carried length is zero, and so is this word), else zero (the boundary is word 14, the next block is final)
    polys["var_length_word"] = q_length * ((one - m_prev) * (w("W") - (ln * 8) * (one - m_13)))
    polys["var_last_final"] = q_last * m  # word 13 of the last block is no message word: some block is final
    row = {s: y(VAR["ROW_" + s]) for s in ("IN", "FLAG", "VALUE", "OUT")}
    # carry-in region of a block after the first: the length it starts from = the length behind the block before (VALUE)
    # times that block's m_13 (OUT) -- zero behind the final block
    polys["var_carry"] = q_carry * (y(VAR["ROW_LEN"]) - row["VALUE"] * row["OUT"])
    polys["var_final"] = q_final * (row["VALUE"] - row["IN"] + row["FLAG"])  # fin = m_13 of the block before - m_13
    polys["var_select"] = q_sum * (row["OUT"] - row["IN"] - row["FLAG"] * row["VALUE"])


def _assign_fixed(k, blocks, tb, cs, adv, fcol, inst, cells, word) -> Description:
    n = 1 << k
    rows = rows_for(blocks)
    usable = n - (cs.blinding_factors() + 1)
    if rows > usable:
        raise ValueError(f"{blocks} blocks need {rows} rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in FIXED}
    copies = []
    _assign_segment(fixed, copies, 0, blocks, 0, tb, adv, fcol, inst, cells, word)
    return Description(cs, adv, fcol, fixed, inst, copies, cells, tb, blocks, k)


def _assign_segment(fixed, copies, first_region, blocks, public, tb, adv, fcol, inst, cells, word, init=None):
    """F.assign_segment for a SHA-256 chain: where `public` is not None, instance rows 8 * public .. 8 * public + 7 are
    copied to the digest words of its tail.  `init`: H[0..7] of the state it starts from, each a constant pinned through
    `const` or None for a cell the caller ties (or leaves free) itself; the default is the IV."""
    F.assign_segment(FAMILY, fixed, copies, first_region, blocks, IV256 if init is None else init,
                     lambda h: None if public is None else 8 * public + h, True, tb, adv, fcol, inst, cells, word)


def usable_rows(k: int, table_bits: int = 12) -> int:
    """The rows of 2^k a circuit may use: all but the blinding rows and the one behind them."""
    return F.usable_rows(FAMILY, k, table_bits)


def max_blocks(k: int, table_bits: int = 12) -> int:
    """The largest block count whose rows fit the usable rows of 2^k."""
    return F.max_blocks(FAMILY, k, table_bits)


def _mont_column(vals: np.ndarray) -> np.ndarray:
    """small integers -> uint64[n, 4] Montgomery limbs, one conversion per distinct value"""
    uniq, inv = np.unique(vals, return_inverse=True)
    return np.stack([fr_to_mont(int(u)) for u in uniq])[inv.reshape(-1)]


def _build_key(self, ctx: Context, k: int, table_bits: int, setup: str, seed: int, make_description):
    """What every SHA-256 circuit object holds: the params, the two static tables, the description
    (`make_description(dense, spread)`), the proving key built from it and the 18 device columns."""
    from .sha_circuit import small_to_mont, spread16, srs_powers_dev

    self.ctx, self.k, self.table_bits, self.seed = ctx, k, table_bits, seed
    n, N = 1 << k, 1 << table_bits
    self.n = n
    self.srs = None
    idx = np.arange(N)
    if setup == "powers":  # the powers [s^i]_1 stand in for a ceremony file: s appears here and nowhere below
        count = max(n, N)
        self.srs = srs_powers_dev(ctx, seed * 0x9E3779B97F4A7C15 + 12345, count)
        self.params = ParamsKZG.from_powers(ctx, k, self.srs)
        self.cfg = TableConfig.from_srs(ctx, N, self.srs, srs_len=count)
        self.dense = StaticTable.new_fk(ctx, small_to_mont(idx), srs_dev=self.srs)
        self.spread = StaticTable.new_fk(ctx, small_to_mont(spread16(idx)), srs_dev=self.srs)
    else:
        if setup != "toxic":
            raise ValueError(f"setup: 'toxic' or 'powers', not {setup!r}")
        s = fr_to_mont(seed * 0x9E3779B97F4A7C15 + 12345)
        self.params = ParamsKZG.setup_from_toxic_waste(ctx, k, s)
        self.cfg = TableConfig.setup_from_toxic_waste(ctx, N, s)
        self.dense = StaticTable.setup_from_toxic_waste(ctx, small_to_mont(idx), s)
        self.spread = StaticTable.setup_from_toxic_waste(ctx, small_to_mont(spread16(idx)), s)
    self.description = d = make_description(self.dense, self.spread)
    self.cs = d.cs
    asm = GP.PermutationAssembly(ctx.lib, n, d.cs.permutation_columns)
    for (lc, lr), (rc, rr) in d.copies:
        asm.copy(lc, lr, rc, rr)
    self.vk_repr = 0x534841323536 + k
    self.pk = ProvingKey(ctx, self.params, k, 0, [], self.cfg, self.params.g_dev + 64, fr_to_mont(self.vk_repr), cs=d.cs,
                         fixed=[_mont_column(d.fixed[name]) for name in d.fixed_names], permutation=asm.mapping)
    self.cols = [ctx.alloc(n * 32) for _ in range(ADVICE_COLUMNS)]


def _close_key(self):
    for o in [self.pk] + list(self.cols) + [self.dense, self.spread, self.cfg, self.params] + ([self.srs] if self.srs is not None else []):
        o.close()


class Sha256Circuit:
    """Proving key and GPU witness synthesis for SHA-256 over exactly `blocks` padded blocks at 2^k rows.  One key
    proves one message length; there is no variable-length selection (several messages, a hash of a hash, a Merkle root
    over private leaves or Merkle membership of one leaf in one proof: sha256_segments.py; any length under one key, with
    the padding constrained: sha256_varlen.py)."""

    rows_per_block = BLOCK_REGIONS * REGION_ROWS

    def __init__(self, ctx: Context, k: int, blocks: int | None = None, table_bits: int = 12, setup: str = "toxic",
                 seed: int = 0x5348413243515F):
        if blocks is None:
            blocks = max_blocks(k, table_bits)
        if blocks < 1:
            raise ValueError(f"2^{k} rows hold no block ({rows_for(1)} rows are needed)")
        self.blocks = blocks
        _build_key(self, ctx, k, table_bits, setup, seed, lambda dense, spread: describe(k, blocks, table_bits, dense, spread))
        self.rows = rows_for(blocks)
        self.digest_words = None

    # ---- host side ----
    def pad(self, message: bytes):
        return pad(message, self.blocks)

    # ---- witness ----
    def synthesize(self, message: bytes):
        """Fills the advice columns on the GPU (cq_sha256_synthesize_dev); returns (device columns, instances)."""
        ctx = self.ctx
        words = np.array(self.pad(message), dtype=np.uint32)
        digest = (C.c_uint32 * 8)()
        arr = (C.c_void_p * ADVICE_COLUMNS)(*[c.ptr for c in self.cols])
        ctx._chk(ctx.lib.cq_sha256_synthesize_dev(ctx.h, self.table_bits, words.ctypes.data, self.blocks, self.n, arr, digest))
        self.digest_words = [int(x) for x in digest]
        return self.cols, self.instances

    @property
    def instances(self):
        return [np.stack([fr_to_mont(x) for x in self.digest_words])]

    @property
    def digest(self) -> bytes:
        """The 8 instance words of the last synthesised message as 32 big-endian bytes."""
        return struct.pack(">8I", *self.digest_words)

    def check(self, message: bytes, max_failures: int = 64):
        cols, inst = self.synthesize(message)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, message: bytes):
        cols, inst = self.synthesize(message)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, message: bytes, seed: int = 1):
        """(proof bytes, digest bytes): create_proof with the digest words as the public inputs."""
        cols, inst = self.synthesize(message)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self.digest

    close = _close_key
