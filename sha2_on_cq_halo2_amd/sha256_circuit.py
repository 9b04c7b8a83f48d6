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
from ._lib import constants, load
from ._marshal import fr_to_mont
from .context import Context
from .params import ParamsKZG, StaticTable, TableConfig
from .proving_key import ProvingKey

_CQ = constants()
REGION_ROWS, BLOCK_REGIONS, TAIL_REGIONS = (_CQ["CQ_SHA256_" + s] for s in ("REGION_ROWS", "BLOCK_REGIONS", "TAIL_REGIONS"))
PAIRS, ADVICE_COLUMNS = _CQ["CQ_SHA256_PAIRS"], _CQ["CQ_SHA256_ADVICE_COLUMNS"]
MIN_TABLE_BITS, MAX_TABLE_BITS = _CQ["CQ_SHA256_MIN_TABLE_BITS"], _CQ["CQ_SHA256_MAX_TABLE_BITS"]
FORM_WORD, FORM_PAIR, FORM_SPREAD = (_CQ["CQ_SHA256_FORM_" + s] for s in ("WORD", "PAIR", "SPREAD"))
SRC = {name[len("CQ_SHA256_SRC_"):]: v for name, v in _CQ.items() if name.startswith("CQ_SHA256_SRC_") and name != "CQ_SHA256_SRC_COUNT"}

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
SPREAD_ONES = (4 ** 32 - 1) // 3  # the spread form of 0xFFFFFFFF

# gate polynomials in cs.gates order (the `index` of a FAIL_GATE finding); every one is anchored on row 0 of a region
GATES = ("a_word", "a_spread", "e_word", "e_spread", "w_word", "Sigma0_even_odd", "Sigma0_word", "Sigma1_even_odd", "Sigma1_word",
         "sigma0_even_odd", "sigma0_word", "sigma1_even_odd", "sigma1_word", "maj_even_odd", "maj_word", "chp_even_odd",
         "chq_even_odd", "ch_word", "e_add", "a_add", "w_add", "chain_a", "chain_e")
# fixed columns in allocation order
FIXED = ("q_all", "q_f3", "q_round", "q_sched", "q_chain") + tuple(f"scale{j}" for j in range(PAIRS)) + ("const",)
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


class Cell(NamedTuple):
    """One entry of the layout table (cq_sha256_layout)."""

    kind: int
    form: int
    column: int
    row: int
    offset: int
    per_table_bits: int
    len: int


def layout():
    """The layout table of csrc/sha256_layout.hpp as the library exports it (host only: no GPU needed)."""
    lib = load()
    count = C.c_size_t()
    assert lib.cq_sha256_layout(None, 0, C.byref(count)) == 0
    words = _CQ["CQ_SHA256_CELL_WORDS"]
    assert words == len(Cell._fields)
    arr = (C.c_uint32 * (words * count.value))()
    assert lib.cq_sha256_layout(arr, count.value, C.byref(count)) == 0
    return [Cell(*arr[words * i: words * (i + 1)]) for i in range(count.value)]


def rows_for(blocks: int) -> int:
    return (BLOCK_REGIONS * blocks + TAIL_REGIONS) * REGION_ROWS


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
    off = cell.offset + cell.per_table_bits * tb
    return off, (cell.len if cell.len else max(0, min(tb, 32 - off)))


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
    cells = layout()
    cs = GP.ConstraintSystem()
    adv = [cs.advice_column() for _ in range(ADVICE_COLUMNS)]
    fcol = {name: cs.fixed_column() for name in (FIXED_CHOICE if choice else FIXED_VARLEN if varlen else FIXED_XOR if xor else FIXED)}
    inst = cs.instance_column()
    X, Y = adv[2 * PAIRS], adv[2 * PAIRS + 1]
    for c in (X, fcol["const"], inst) + ((Y,) if choice or varlen else ()):
        cs.enable_equality(c)

    pieces = {s: sorted((c for c in cells if c.kind == s and c.form == FORM_PAIR and c.len), key=lambda c: c.offset) for s in SRC.values()}
    chunks = {s: sorted((c for c in cells if c.kind == s and c.form == FORM_PAIR and not c.len), key=lambda c: c.per_table_bits)
              for s in SRC.values()}
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
                terms.append((4 ** ((p.offset - r) % 32), q(p, True)))
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
        return q(c) * (1 << 32)

    sel = {name: cs.query_fixed(fcol[name]) for name in ("q_all", "q_f3", "q_round", "q_sched", "q_chain")}
    polys = {}
    for name, s in (("a", "A"), ("e", "E"), ("w", "W")):
        polys[name + "_word"] = sel["q_all"] * (w(s) - lin([(2 ** p.offset, q(p)) for p in pieces[SRC[s]]]))
        if s != "W":
            polys[name + "_spread"] = sel["q_all"] * (w(s, FORM_SPREAD) - lin([(4 ** p.offset, q(p, True)) for p in pieces[SRC[s]]]))
    for gate, s, src, rots, shift in (("Sigma0", "S0", "A", (2, 13, 22), None), ("Sigma1", "S1", "E", (6, 11, 25), None),
                                      ("sigma0", "G0", "W", (7, 18), 3), ("sigma1", "G1", "W", (17, 19), 10)):
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
    if choice:  # W = x + d * (y - x) with d boolean: x, y, d in the rows of Y that no layout cell uses
        assert not any(c.column == Y.index and c.row in (CHOICE_ROW_ZERO, CHOICE_ROW_ONE, CHOICE_ROW_BIT) for c in cells)
        q_choice = cs.query_fixed(fcol["q_choice"])
        x, y, d = (cs.query_advice(Y, r) for r in (CHOICE_ROW_ZERO, CHOICE_ROW_ONE, CHOICE_ROW_BIT))
        polys["choice"] = q_choice * (w("W") - x - d * (y - x))
        polys["choice_bit"] = q_choice * (d * (GP.Expression.constant(1) - d))
    if varlen:
        _varlen_gates(cs, polys, cells, adv, fcol, w)
    if xor:  # W = e_r ^ e_(r-1): under q_f3 `chp_even_odd` makes the CHP_EVEN chunks the even bits of spread(e_r) + spread(e_(r-1))
        polys["xor_word"] = cs.query_fixed(fcol["q_xor"]) * (w("W") - from_chunks("CHP_EVEN"))
    gates = GATES_CHOICE if choice else GATES_VARLEN if varlen else GATES_XOR if xor else GATES
    assert tuple(polys) != () and set(polys) == set(gates)
    for name in gates:
        cs.create_gate(name, [polys[name]])
    # lookups 0 .. 7: (dense_j, spread_j) in (dense, spread); 8 .. 15: dense_j * scale_j in dense -- the length check
    for j in range(PAIRS):
        cs.lookup_static(f"pair{j}", [(adv[2 * j], dense), (adv[2 * j + 1], spread)])
    for j in range(PAIRS):
        cs.lookup_static(f"length{j}", [(cs.query_advice(adv[2 * j]) * cs.query_fixed(fcol[f"scale{j}"]), dense)])
    if xor:  # the gate adds three dense cells of row 6 and one fixed column to the queries, nothing to the blinding rows or the degree
        assert (cs.blinding_factors(), cs.degree()) == (20, 4)
    return cs, adv, fcol, inst, cells, word


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
    """The fixed cells and the copies of one chain of `blocks` blocks whose regions start at `first_region`: selectors and
    scales, the round constants, the state it starts from on its first four regions (no q_chain before its second block),
    and -- where `public` is not None -- the copies of instance rows 8 * public .. 8 * public + 7 to the digest words of its
    tail.  `init`: H[0..7] of that state, each a constant pinned through `const` or None for a cell the caller ties (or
    leaves free) itself; the default is the IV."""
    init = IV256 if init is None else init
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
        if c.form == FORM_PAIR:
            _, ln = _field_of(c, tb)
            fixed[f"scale{c.column // 2}"][base + c.row] = 1 << (tb - ln) if c.len else 1
    krow = word[(SRC["K"], FORM_WORD)].row
    arow, erow = word[(SRC["A"], FORM_WORD)].row, word[(SRC["E"], FORM_WORD)].row
    kvals = np.array(K256, dtype=np.uint64)
    rb = base[is_round]
    fixed["const"][rb + krow] = kvals[(in_block[is_round] - 4)]
    copies += [((fcol["const"], int(r) + krow), (X, int(r) + krow)) for r in rb]
    for i in range(4):  # region i of the first block holds a_(i-4) = H[3 - i] and e_(i-4) = H[7 - i]
        head = int(base[i])
        for row, val in ((arow, init[3 - i]), (erow, init[7 - i])):
            if val is None:
                continue
            fixed["const"][head + row] = val
            copies.append(((fcol["const"], head + row), (X, head + row)))
        if public is not None:
            tail = int(base[BLOCK_REGIONS * blocks + i])
            copies.append(((inst, 8 * public + 3 - i), (X, tail + arow)))
            copies.append(((inst, 8 * public + 7 - i), (X, tail + erow)))


def usable_rows(k: int, table_bits: int = 12) -> int:
    """The rows of 2^k a circuit may use: all but the blinding rows and the one behind them."""
    return (1 << k) - (_constraint_system(table_bits, "dense", "spread")[0].blinding_factors() + 1)


def max_blocks(k: int, table_bits: int = 12) -> int:
    """The largest block count whose rows fit the usable rows of 2^k."""
    return (usable_rows(k, table_bits) // REGION_ROWS - TAIL_REGIONS) // BLOCK_REGIONS


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
