"""What the SHA-256 and the SHA-512 compression circuits share, written once over a `Family` record: the layout table's
reader, the 23 gates and 16 lookups of the constraint system, and a chain's fixed cells and copies.
sha256_circuit.py and sha512_circuit.py define their families and everything that is theirs alone: padding, the public
rows, the 32-bit circuit's choice and variable-length variants; the XOR variant's gate polynomial is written here once.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import plonk as GP
from ._lib import constants, load

_CQ = constants()
# the cell record, the word kinds, the forms and the column counts are one set for both widths (sha256_layout.hpp)
PAIRS, ADVICE_COLUMNS = _CQ["CQ_SHA256_PAIRS"], _CQ["CQ_SHA256_ADVICE_COLUMNS"]
FORM_WORD, FORM_PAIR, FORM_SPREAD = (_CQ["CQ_SHA256_FORM_" + s] for s in ("WORD", "PAIR", "SPREAD"))
SRC = {name[len("CQ_SHA256_SRC_"):]: v for name, v in _CQ.items() if name.startswith("CQ_SHA256_SRC_") and name != "CQ_SHA256_SRC_COUNT"}

# gate polynomials in cs.gates order (the `index` of a FAIL_GATE finding); every one is anchored on row 0 of a region
GATES = ("a_word", "a_spread", "e_word", "e_spread", "w_word", "Sigma0_even_odd", "Sigma0_word", "Sigma1_even_odd", "Sigma1_word",
         "sigma0_even_odd", "sigma0_word", "sigma1_even_odd", "sigma1_word", "maj_even_odd", "maj_word", "chp_even_odd",
         "chq_even_odd", "ch_word", "e_add", "a_add", "w_add", "chain_a", "chain_e")
# fixed columns in allocation order
FIXED = ("q_all", "q_f3", "q_round", "q_sched", "q_chain") + tuple(f"scale{j}" for j in range(PAIRS)) + ("const",)


class Family(NamedTuple):
    """One word width of SHA-2.  `prefix`: of the header's REGION_ROWS, BLOCK_REGIONS, TAIL_REGIONS and table_bits bounds;
    `layout_entry`: the library's export of the layout table; `sigmas`: (rotations, shift or None) of Sigma0, Sigma1,
    sigma0 and sigma1; `K`: the round constants.  `chunk_length_checked`: whether a chunk cell's scale holds it to the bits
    the word has left above it (the 64-bit circuit, whose chunks may start past the word) or leaves it at the table's width
    (the 32-bit circuit)."""

    word_bits: int
    prefix: str
    layout_entry: str
    sigmas: tuple
    K: tuple
    chunk_length_checked: bool

    region_rows = property(lambda self: _CQ[self.prefix + "REGION_ROWS"])
    block_regions = property(lambda self: _CQ[self.prefix + "BLOCK_REGIONS"])
    tail_regions = property(lambda self: _CQ[self.prefix + "TAIL_REGIONS"])
    spread_ones = property(lambda self: (4 ** self.word_bits - 1) // 3)  # the spread form of the all-ones word


class Cell(NamedTuple):
    """One entry of a layout table (cq_sha256_layout, cq_sha512_layout)."""

    kind: int
    form: int
    column: int
    row: int
    offset: int
    per_table_bits: int
    len: int


def layout(fam: Family):
    """The family's layout table as the library exports it (host only: no GPU needed)."""
    entry = getattr(load(), fam.layout_entry)
    count = C.c_size_t()
    assert entry(None, 0, C.byref(count)) == 0
    words = _CQ["CQ_SHA256_CELL_WORDS"]
    assert words == len(Cell._fields)
    arr = (C.c_uint32 * (words * count.value))()
    assert entry(arr, count.value, C.byref(count)) == 0
    return [Cell(*arr[words * i: words * (i + 1)]) for i in range(count.value)]


def rows_for(fam: Family, blocks: int) -> int:
    return (fam.block_regions * blocks + fam.tail_regions) * fam.region_rows


def field_of(fam: Family, cell: Cell, tb: int):
    """(bit offset, length) of the cell's field within its word at table size 2^tb; a chunk that starts at or above the
    word's width has length 0."""
    off = cell.offset + cell.per_table_bits * tb
    return off, (cell.len if cell.len else max(0, min(tb, fam.word_bits - off)))


class System(NamedTuple):
    """The constraint system while it is built: the 23 polynomials of GATES are in `polys`, no gate is created yet.  A
    variant adds its polynomials (`w` and `from_chunks` query the layout's cells) and names every gate in `finish`."""

    cs: GP.ConstraintSystem
    advice: list
    fixed_columns: dict
    instance: GP.Column
    cells: list
    word: dict
    polys: dict
    w: object
    from_chunks: object


def base_system(fam: Family, tb: int, fixed_names=FIXED, equality_on_y: bool = False) -> System:
    """Columns, equality and the polynomials of GATES.  `fixed_names`: FIXED, then a variant's own columns."""
    rows = fam.region_rows
    cells = layout(fam)
    cs = GP.ConstraintSystem()
    adv = [cs.advice_column() for _ in range(ADVICE_COLUMNS)]
    fcol = {name: cs.fixed_column() for name in fixed_names}
    inst = cs.instance_column()
    X, Y = adv[2 * PAIRS], adv[2 * PAIRS + 1]
    for c in (X, fcol["const"], inst) + ((Y,) if equality_on_y else ()):
        cs.enable_equality(c)

    pair_cells = lambda s, chunk: [c for c in cells if c.kind == s and c.form == FORM_PAIR and bool(c.len) != chunk]
    pieces = {s: sorted(pair_cells(s, False), key=lambda c: c.offset) for s in SRC.values()}
    # where the scales check a chunk's length, a chunk that starts at or above the word's width holds zero (the length lookup
    # of its cell says so) and the gates leave it out.  Where they do not, nothing else would hold such a chunk to zero, so
    # it stays in its gates: the 32-bit layout's third chunk starts at bit 32 at table_bits 16.
    in_gates = lambda c: not fam.chunk_length_checked or c.per_table_bits * tb < fam.word_bits
    chunks = {s: sorted(filter(in_gates, pair_cells(s, True)), key=lambda c: c.per_table_bits) for s in SRC.values()}
    word = {(c.kind, c.form): c for c in cells if c.form != FORM_PAIR}

    def q(cell, spread_form=False, regions_back=0):
        return cs.query_advice(adv[cell.column + (1 if spread_form else 0)], cell.row - rows * regions_back)

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
                terms.append((4 ** ((p.offset - r) % fam.word_bits), q(p, True)))
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
        return q(c) * (1 << fam.word_bits)

    sel = {name: cs.query_fixed(fcol[name]) for name in ("q_all", "q_f3", "q_round", "q_sched", "q_chain")}
    polys = {}
    for name, s in (("a", "A"), ("e", "E"), ("w", "W")):
        polys[name + "_word"] = sel["q_all"] * (w(s) - lin([(2 ** p.offset, q(p)) for p in pieces[SRC[s]]]))
        if s != "W":
            polys[name + "_spread"] = sel["q_all"] * (w(s, FORM_SPREAD) - lin([(4 ** p.offset, q(p, True)) for p in pieces[SRC[s]]]))
    for (gate, s, src), (rots, shift) in zip((("Sigma0", "S0", "A"), ("Sigma1", "S1", "E"), ("sigma0", "G0", "W"), ("sigma1", "G1", "W")),
                                             fam.sigmas):
        polys[gate + "_even_odd"] = sel["q_all"] * (rotated_spread(src, rots, shift) - even_odd(s))
        polys[gate + "_word"] = sel["q_all"] * (w(s + "_EVEN") - from_chunks(s + "_EVEN"))
    sa, se = (lambda back: w("A", FORM_SPREAD, back)), (lambda back: w("E", FORM_SPREAD, back))
    polys["maj_even_odd"] = sel["q_f3"] * (sa(0) + sa(1) + sa(2) - even_odd("MAJ"))
    polys["maj_word"] = sel["q_f3"] * (w("MAJ_ODD") - from_chunks("MAJ_ODD"))
    polys["chp_even_odd"] = sel["q_f3"] * (se(0) + se(1) - even_odd("CHP"))
    polys["chq_even_odd"] = sel["q_f3"] * (GP.Expression.constant(fam.spread_ones) - se(0) + se(2) - even_odd("CHQ"))
    polys["ch_word"] = sel["q_f3"] * (w("CH") - from_chunks("CHP_ODD", "CHQ_ODD"))
    # T1 = h + Sigma1(e) + Ch(e, f, g) + K + W with e, f, g, h = e_(r-1) .. e_(r-4); e_r = d + T1; a_r = T1 + Sigma0 + Maj
    t1 = w("E", back=4) + w("S1_EVEN", back=1) + w("CH", back=1) + w("K") + w("W")
    polys["e_add"] = sel["q_round"] * (w("E") + carry("CARRY_E") - w("A", back=4) - t1)
    polys["a_add"] = sel["q_round"] * (w("A") + carry("CARRY_A") - t1 - w("S0_EVEN", back=1) - w("MAJ_ODD", back=1))
    polys["w_add"] = sel["q_sched"] * (w("W") + carry("CARRY_W") - w("G1_EVEN", back=2) - w("W", back=7) - w("G0_EVEN", back=15) - w("W", back=16))
    for name, s in (("a", "A"), ("e", "E")):  # H + (a .. h): the same slot one block and four regions back
        polys["chain_" + name] = sel["q_chain"] * (w(s) + carry("CARRY_" + s) - w(s, back=fam.block_regions) - w(s, back=4))
    return System(cs, adv, fcol, inst, cells, word, polys, w, from_chunks)


def xor_word(sys: System):
    """The polynomial of the gate `xor_word` of a circuit's XOR variant, whose fixed column is `q_xor`: W = e_r ^ e_(r-1).
    Under q_f3 `chp_even_odd` makes the CHP_EVEN chunks the even bits of spread(e_r) + spread(e_(r-1)); the gate, anchored on
    row 0 of a unit's second region, equates W with the word those chunks make up."""
    return sys.cs.query_fixed(sys.fixed_columns["q_xor"]) * (sys.w("W") - sys.from_chunks("CHP_EVEN"))


def finish(sys: System, dense, spread, gates=GATES):
    """Creates the gates in `gates` order and the lookups; returns what the circuits' `_constraint_system` returns."""
    cs, adv, fcol = sys.cs, sys.advice, sys.fixed_columns
    assert tuple(sys.polys) != () and set(sys.polys) == set(gates)
    for name in gates:
        cs.create_gate(name, [sys.polys[name]])
    # lookups 0 .. 7: (dense_j, spread_j) in (dense, spread); 8 .. 15: dense_j * scale_j in dense -- the length check
    for j in range(PAIRS):
        cs.lookup_static(f"pair{j}", [(adv[2 * j], dense), (adv[2 * j + 1], spread)])
    for j in range(PAIRS):
        cs.lookup_static(f"length{j}", [(cs.query_advice(adv[2 * j]) * cs.query_fixed(fcol[f"scale{j}"]), dense)])
    return cs, adv, fcol, sys.instance, sys.cells, sys.word


def assign_segment(fam: Family, fixed, copies, first_region, blocks, init, instance_row, public_last, tb, adv, fcol, inst, cells, word):
    """The fixed cells and the copies of one chain of `blocks` blocks whose regions start at `first_region`: selectors and
    scales, the round constants, the state it starts from on its first four regions (no q_chain before its second block),
    and the copies of the instance column to the digest words of its tail.  `init`: H[0..7] of that state, each a constant
    pinned through `const` or None for a cell the caller ties (or leaves free) itself.  `instance_row(h)`: the instance row
    of digest word h, or None where the word is not public.  `public_last`: region by region, the instance copies come
    behind both pins (the 32-bit circuit) or each behind its word's pin (the 64-bit circuit); the order of the copy list
    decides the permutation's cycles, so each circuit keeps its own."""
    X = adv[2 * PAIRS]
    rows, per_block = fam.region_rows, fam.block_regions
    g = np.arange(per_block * blocks + fam.tail_regions)
    in_block, base = g % per_block, (first_region + g) * rows
    is_tail = g >= per_block * blocks
    is_round = (in_block >= 4) & ~is_tail
    fixed["q_all"][base] = 1
    fixed["q_f3"][base[in_block >= 2]] = 1
    fixed["q_round"][base[is_round]] = 1
    fixed["q_sched"][base[is_round & (in_block >= 20)]] = 1
    fixed["q_chain"][base[(in_block < 4) & (g >= per_block)]] = 1
    for c in cells:
        if c.form == FORM_PAIR:  # dense * 2^(tb - len) is in the table: dense < 2^len
            fixed[f"scale{c.column // 2}"][base + c.row] = pair_scale(fam, c, tb)
    krow = word[(SRC["K"], FORM_WORD)].row
    arow, erow = word[(SRC["A"], FORM_WORD)].row, word[(SRC["E"], FORM_WORD)].row
    rb = base[is_round]
    fixed["const"][rb + krow] = np.array(fam.K, dtype=np.uint64)[(in_block[is_round] - 4)]
    copies += [((fcol["const"], int(r) + krow), (X, int(r) + krow)) for r in rb]
    for i in range(4):  # region i of the first block holds a_(i-4) = H[3 - i] and e_(i-4) = H[7 - i]
        head, tail = int(base[i]), int(base[per_block * blocks + i])
        pins, publics = [], []
        for row, h in ((arow, 3 - i), (erow, 7 - i)):
            pin = public = None
            if init[h] is not None:
                fixed["const"][head + row] = init[h]
                pin = ((fcol["const"], head + row), (X, head + row))
            if instance_row(h) is not None:
                public = ((inst, instance_row(h)), (X, tail + row))
            pins.append(pin)
            publics.append(public)
        order = pins + publics if public_last else [pins[0], publics[0], pins[1], publics[1]]
        copies += [c for c in order if c is not None]


def pair_scale(fam: Family, cell: Cell, tb: int) -> int:
    """The scale of a pair cell's length lookup: 2^(tb - len), so that dense * scale is in the table only for dense < 2^len."""
    if not cell.len and not fam.chunk_length_checked:
        return 1
    return 1 << (tb - field_of(fam, cell, tb)[1])


def usable_rows(fam: Family, k: int, table_bits: int = 12) -> int:
    """The rows of 2^k a circuit may use: all but the blinding rows and the one behind them."""
    return (1 << k) - (finish(base_system(fam, table_bits), "dense", "spread")[0].blinding_factors() + 1)


def max_blocks(fam: Family, k: int, table_bits: int = 12) -> int:
    """The largest block count of one message whose rows fit the usable rows of 2^k."""
    return (usable_rows(fam, k, table_bits) // fam.region_rows - fam.tail_regions) // fam.block_regions
