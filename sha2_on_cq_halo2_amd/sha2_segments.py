"""What the wired SHA-256 and SHA-512 segments share, written once over a `Width` record: the source kinds of a plan, its
check, its description -- the fixed columns and the copy constraints, in one order -- its lowering to the arrays of the
synthesis entry points, the word buffer, and the circuit object ("Wired segments, once for both widths").
sha256_segments.py and sha512_segments.py define their widths, their `Segment` and `Plan`, the plans and the front ends
that are theirs alone, and the call of their entry points; sha512_xor.py is the 64-bit width with `Xor` gated.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple

import numpy as np

from . import sha2_family as F
from ._marshal import FR_MODULUS
from .context import Context


class Private(NamedTuple):
    """A word the prover chooses: no constraint ties it to anything."""


class Const(NamedTuple):
    """A word pinned to `value` through the `const` fixed column."""

    value: int


class DigestWord(NamedTuple):
    """A word tied to word `word` (0 .. 7) of the final state of the earlier segment `segment`."""

    segment: int
    word: int


class Var(NamedTuple):
    """Shared private word number `index` of the plan: it may stand in several places -- as a message word, as an initial
    word or as an operand of a Choice or an Xor -- and all its cells are tied by copies."""

    index: int


class Choice(NamedTuple):
    """A message word that equals `one` if private bit number `bit` of the plan is 1, else `zero`; each operand is a Var
    or a DigestWord of an earlier segment.  One bit may steer many choices."""

    bit: int
    zero: tuple
    one: tuple


class Xor(NamedTuple):
    """A message word that equals `x` XOR `y`; each operand is a Const, a Var or a DigestWord of an earlier segment.  Equal
    Xors are one unit: any number of message words may read it.  A plan with an Xor holds no Choice."""

    x: tuple
    y: tuple


PRIVATE = Private()
OPERANDS = {Choice: ("a choice", ("zero", "one"), "a Var or a DigestWord", (Var, DigestWord)),  # a compound kind's last two fields
            Xor: ("an xor", ("x", "y"), "a Const, a Var or a DigestWord", (Const, Var, DigestWord))}


class Width(NamedTuple):
    """One word width of the wired segments.  `circuit`: sha256_circuit or sha512_circuit -- its FAMILY, its table_bits
    bounds, `_build_key` and, where the width has them, the constants of the choice and XOR variants.
    `constraint_system(table_bits, dense, spread, choice, xor)`: (fixed names,) + the circuit's `_constraint_system`.
    `description(cs, advice, fixed columns, fixed, instance, copies, cells, table_bits, blocks, variants, k, fixed names)`:
    the circuit's Description.  `instance_copies_last`: F.assign_segment's `public_last`.  `dtype`, `letter`: a word in numpy
    and in struct.  `source_digest`, `source_choice`, `source_iv`: the header's CQ_SHA..._SOURCE_* (None: the width has none).
    `iv`: {variant: H[0..7]}; a Segment without a `variant` has variant 0.  `gated`: the kinds among Choice and Xor that the
    width's constraint system has gates for.  `segment`, `plan`: the width's Segment and its Plan from (segments, public as
    (segment, words) pairs, public_init).  `public(plan)`: the plan's `public`, checked, as such pairs."""

    circuit: object
    constraint_system: object
    description: object
    instance_copies_last: bool
    dtype: type
    letter: str
    source_digest: int
    source_choice: int | None
    source_iv: int
    iv: dict
    gated: tuple
    segment: object
    plan: object
    public: object

    fam = property(lambda self: self.circuit.FAMILY)
    bits = property(lambda self: self.circuit.FAMILY.word_bits)


# ---- plans -------------------------------------------------------------------------------------------------------------------

def padding(w: Width, data_words: int, words: int):
    """The pinned words behind a message of `data_words` words that is padded to `words`: the 1 bit, zeros, the bit length."""
    return (Const(1 << (w.bits - 1)),) + (Const(0),) * (words - data_words - 2) + (Const(w.bits * data_words),)


def double_hash(w: Width, blocks: int):
    """H(H(message)): a private message of `blocks` blocks, then the one-block hash of its digest, whose padding is pinned;
    only the second digest is public."""
    second = tuple(DigestWord(0, i) for i in range(8)) + padding(w, 8, 16)
    return w.plan((w.segment(blocks, (PRIVATE,) * (16 * blocks)), w.segment(1, second)), ((1, 8),))


def merkle_tree(w: Width, depth: int):
    """The root over 2^depth private leaves of 8 words: every node hashes left || right (two blocks, the second one pinned
    padding); nodes level by level, the 2^(depth - 1) nodes over the leaves first; only the root is public."""
    if depth < 1:
        raise ValueError("a Merkle tree has at least two leaves (depth >= 1)")
    segs, below = [], None
    for level in range(depth):
        first = len(segs)
        for i in range(1 << (depth - 1 - level)):
            if level == 0:
                children = (PRIVATE,) * 16
            else:
                children = tuple(DigestWord(below + 2 * i + side, word) for side in (0, 1) for word in range(8))
            segs.append(w.segment(2, children + padding(w, 16, 32)))
        below = first
    return w.plan(tuple(segs), ((len(segs) - 1, 8),))


def midstate(w: Width, blocks: int):
    """Compressing `blocks` private blocks takes the public state H_in to the public state H_out: one segment, every
    message word and every initial word Private, the final state (instance rows 0 .. 7) and the initial state (rows
    8 .. 15) public.  Nothing says the blocks are padded or where a message ends: it is the link of a chain of proofs."""
    return w.plan((w.segment(blocks, (PRIVATE,) * (16 * blocks), (PRIVATE,) * 8),), ((0, 8),), (0,))


def _sources(plan):
    return [s for seg in plan.segments for s in tuple(seg.init or ()) + tuple(seg.sources)]


def has_init(plan) -> bool:
    return any(seg.init is not None for seg in plan.segments)


def has_choice(plan) -> bool:
    return any(isinstance(s, Choice) for seg in plan.segments for s in seg.sources)


def xor_units(plan):
    """The plan's XOR units: its distinct Xor words in the order of their first use, by (segment, word)."""
    return list(dict.fromkeys(s for seg in plan.segments for s in seg.sources if isinstance(s, Xor)))


def has_xor(plan) -> bool:
    return any(isinstance(s, Xor) for seg in plan.segments for s in seg.sources)


def shared_counts(plan):
    """(vars, bits) of the plan: one more than the largest index used, 0 if none is."""
    srcs = _sources(plan)
    operands = [o for s in srcs if isinstance(s, (Choice, Xor)) for o in s[-2:]]
    return (max([v.index + 1 for v in srcs + operands if isinstance(v, Var)], default=0),
            max([s.bit + 1 for s in srcs if isinstance(s, Choice)], default=0))


def _regions(w: Width, seg) -> int:
    return w.fam.block_regions * seg.blocks + w.fam.tail_regions


def first_regions(w: Width, plan):
    """The first region of every segment."""
    out, at = [], 0
    for seg in plan.segments:
        out.append(at)
        at += _regions(w, seg)
    return out


def xor_first_region(w: Width, plan) -> int:
    """The first region of the XOR area: the one directly behind the last segment's tail.  Unit u takes regions
    XOR_REGIONS * u (e = x) and XOR_REGIONS * u + 1 (e = y, W = x ^ y) from there."""
    return sum(_regions(w, seg) for seg in plan.segments)


def rows_for(w: Width, plan) -> int:
    """The rows the plan uses: its segments one behind another, then XOR_REGIONS regions per XOR unit."""
    units = xor_units(plan)
    return w.fam.region_rows * (xor_first_region(w, plan) + (w.circuit.XOR_REGIONS * len(units) if units else 0))


def _check_plan(w: Width, plan):
    """ValueError, naming segment and word, for a plan that is malformed; else its `public` as (segment, words) pairs."""
    if not plan.segments:
        raise ValueError("a plan has at least one segment")
    kinds = [k.__name__ for k in (Private, Const, DigestWord, Var) + w.gated]

    def check(j, where, src, allowed, what=""):
        if not isinstance(src, allowed):
            return False
        if isinstance(src, DigestWord):
            if not 0 <= src.segment < j:
                raise ValueError(f"segment {j}, {where}: the digest of segment {src.segment}{what} does not come before it")
            if not 0 <= src.word < 8:
                raise ValueError(f"segment {j}, {where}: a digest has words 0 .. 7, not {src.word}{what}")
        elif isinstance(src, Var) and src.index < 0:
            raise ValueError(f"segment {j}, {where}: the var index {src.index}{what} is negative")
        elif isinstance(src, Const) and not 0 <= src.value < 1 << w.bits:
            raise ValueError(f"segment {j}, {where}: the constant {src.value}{what} is no {w.bits}-bit word")
        elif isinstance(src, Choice) and src.bit < 0:
            raise ValueError(f"segment {j}, {where}: the bit index {src.bit} is negative")
        if isinstance(src, (Choice, Xor)):
            gate, names, operand_kinds, operand_types = OPERANDS[type(src)]
            for name, o in zip(names, src[-2:]):
                if not check(j, where, o, operand_types, f" (the {name} operand)"):
                    raise ValueError(f"segment {j}, {where}: the {name} operand of {gate} is {operand_kinds}, not {o!r}")
        return True

    for j, seg in enumerate(plan.segments):
        if seg.blocks < 1 or len(seg.sources) != 16 * seg.blocks:
            raise ValueError(f"segment {j}: {seg.blocks} blocks and {len(seg.sources)} word sources (16 per block, at least one block)")
        if getattr(seg, "variant", 0) not in w.iv:
            raise ValueError(f"segment {j}: the variant {seg.variant!r} is none of {sorted(w.iv)}")
        if seg.init is not None and len(seg.init) != 8:
            raise ValueError(f"segment {j}: an initial state has 8 words, not {len(seg.init)}")
        for where, src, allowed in [(f"initial word {i}", s, ()) for i, s in enumerate(seg.init or ())] + \
                                   [(f"word {t}", s, w.gated) for t, s in enumerate(seg.sources)]:
            if isinstance(src, (Choice, Xor)) and type(src) not in w.gated:
                raise ValueError(f"segment {j}, {where}: {type(src).__name__} words are not built on the {w.bits}-bit circuit yet")
            if not check(j, where, src, (Private, Const, DigestWord, Var) + allowed):
                what = f"a source is {', '.join(kinds[:-1])} or {kinds[-1]}" if allowed or not w.gated else "an initial word is Private, Const, DigestWord or Var"
                raise ValueError(f"segment {j}, {where}: {what}, not {src!r}")
    if has_xor(plan) and has_choice(plan):
        j, t = next((j, t) for j, seg in enumerate(plan.segments) for t, s in enumerate(seg.sources) if isinstance(s, Choice))
        raise ValueError(f"segment {j}, word {t}: a Choice in a plan that holds an Xor -- the two variants do not combine")
    public = w.public(plan)
    pi = tuple(plan.public_init)
    if len(set(pi)) != len(pi) or not all(isinstance(q, int) and 0 <= q < len(plan.segments) and plan.segments[q].init is not None for q in pi):
        raise ValueError(f"public_init segments {pi!r}: each an index below {len(plan.segments)} of a segment with an init, none twice")
    return public


def describe(w: Width, k: int, plan, table_bits: int = 12, dense="dense", spread="spread"):
    """The constraint system of the width's compression circuit with the fixed columns and copies of `plan`.  ValueError for
    a plan that is malformed or does not fit 2^k rows.

    The copy list, in this order: segment after segment its own copies (round constants, pinned initial words, instance
    rows of its public words) and those of its Const and DigestWord message words; the choices' digest operands; vars, then
    bits, in ascending index, every later cell to the first; the digest-wired initial words; the vars' initial-word cells;
    the public initial words in instance order; the XOR area.  A plan without choices and XOR units leaves their parts empty."""
    SC, fam = w.circuit, w.fam
    if not SC.MIN_TABLE_BITS <= table_bits <= SC.MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{SC.MIN_TABLE_BITS}, {SC.MAX_TABLE_BITS}]: the widest piece has {SC.MIN_TABLE_BITS} bits")
    public = _check_plan(w, plan)
    choice, units = has_choice(plan), xor_units(plan)
    names, cs, adv, fcol, inst, cells, word = w.constraint_system(table_bits, dense, spread, choice, bool(units))
    n, X, Y, region_rows = 1 << k, adv[2 * F.PAIRS], adv[2 * F.PAIRS + 1], fam.region_rows
    rows, usable = rows_for(w, plan), n - (cs.blinding_factors() + 1)
    instance_rows = sum(words for _, words in public) + 8 * len(plan.public_init)
    if max(rows, instance_rows) > usable:
        area = f" and {len(units)} xor units" if units else ""
        raise ValueError(f"{len(plan.segments)} segments{area} need {rows} rows and {instance_rows} instance rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in names}
    copies = []
    firsts = first_regions(w, plan)
    public_at, at = {}, 0  # segment -> (the instance row of its word 0, its public words): the rows run on in `public` order
    for s, words in public:
        public_at[s] = (at, words)
        at += words
    init_row = {q: at + 8 * i for i, q in enumerate(plan.public_init)}
    arow, erow, wrow = (word[(F.SRC[s], F.FORM_WORD)].row for s in "AEW")

    def tail_cell(src):  # tail region 3 - i % 4 holds word i of the final state: its A row for i < 4, its E row otherwise
        tail = region_rows * (firsts[src.segment] + fam.block_regions * plan.segments[src.segment].blocks + 3 - src.word % 4)
        return X, tail + (arow if src.word < 4 else erow)

    # the cells of the choices' digest operands, of every var and of every bit, in (segment, word, zero-then-one) order
    digest_cells, var_cells, bit_cells = [], {}, {}
    init_digest_cells, init_var_cells, init_public_cells = [], {}, []
    xor_first, xor_readers = xor_first_region(w, plan), []  # every reader's W cell, tied to its unit's, in (segment, word) order
    for j, seg in enumerate(plan.segments):
        # a constant initial word is pinned where the initial hash value's is, by the same lines; the others are tied behind
        init = w.iv[getattr(seg, "variant", 0)] if seg.init is None else [s.value if isinstance(s, Const) else None for s in seg.init]
        row, words = public_at.get(j, (0, 0))
        F.assign_segment(fam, fixed, copies, firsts[j], seg.blocks, init, lambda h: row + h if h < words else None, w.instance_copies_last,
                         table_bits, adv, fcol, inst, cells, word)
        for i, src in enumerate(seg.init or ()):  # state word i: region 3 - i % 4 of the first block, A row for i < 4, else E row
            cell = (X, region_rows * (firsts[j] + 3 - i % 4) + (arow if i < 4 else erow))
            if isinstance(src, DigestWord):
                init_digest_cells.append((tail_cell(src), cell))
            elif isinstance(src, Var):
                init_var_cells.setdefault(src.index, []).append(cell)
            if j in init_row:
                init_public_cells.append(((inst, init_row[j] + i), cell))
        for t, src in enumerate(seg.sources):
            base = region_rows * (firsts[j] + fam.block_regions * (t // 16) + 4 + t % 16)
            w_cell = base + wrow
            if isinstance(src, Const):
                fixed["const"][w_cell] = src.value
                copies.append(((fcol["const"], w_cell), (X, w_cell)))
            elif isinstance(src, DigestWord):
                copies.append((tail_cell(src), (X, w_cell)))
            elif isinstance(src, Var):
                var_cells.setdefault(src.index, []).append((X, w_cell))
            elif isinstance(src, Choice):
                fixed["q_choice"][base] = 1
                for o, r in ((src.zero, SC.CHOICE_ROW_ZERO), (src.one, SC.CHOICE_ROW_ONE)):
                    if isinstance(o, DigestWord):
                        digest_cells.append((tail_cell(o), (Y, base + r)))
                    else:
                        var_cells.setdefault(o.index, []).append((Y, base + r))
                bit_cells.setdefault(src.bit, []).append((Y, base + SC.CHOICE_ROW_BIT))
            elif isinstance(src, Xor):
                xor_readers.append(((X, region_rows * (xor_first + SC.XOR_REGIONS * units.index(src) + 1) + wrow), (X, w_cell)))
    # behind the segments' own copies: every digest operand to its tail cell, then every later cell of a var to the var's
    # first cell (vars in ascending index), then the same for every bit
    copies += digest_cells
    for shared in (var_cells, bit_cells):
        for i in sorted(shared):
            copies += [(shared[i][0], cell) for cell in shared[i][1:]]
    # behind all of those, the initial states: every digest-wired state cell to its tail cell in (segment, word) order;
    # then, vars in ascending index, every state cell of a var to the var's first cell (its first message or operand cell
    # if it has one, else its first state cell); then the public initial words to their instance rows, in instance order
    copies += init_digest_cells
    for i in sorted(init_var_cells):
        first, rest = (var_cells[i][0], init_var_cells[i]) if i in var_cells else (init_var_cells[i][0], init_var_cells[i][1:])
        copies += [(first, cell) for cell in rest]
    copies += sorted(init_public_cells, key=lambda c: c[0][1])
    # behind all of those, the XOR area.  Unit u: region xor_first + 2u holds e = x under q_all; the next one e = y and
    # W = x ^ y under q_all, q_f3 and q_xor; scales in both as F.assign_segment sets them.  Copies, all in X: (1) unit after
    # unit, x then y, a Const operand's E cell to `const` and a DigestWord operand's E cell to its tail cell; (2) vars in
    # ascending index: every operand cell of the var to the var's first cell -- its first message cell if it has one, else
    # its first state cell, else its first operand cell; (3) every reader's W cell to its unit's W cell
    xor_var_cells = {}
    for u, unit in enumerate(units):
        for o, region in ((unit.x, xor_first + SC.XOR_REGIONS * u), (unit.y, xor_first + SC.XOR_REGIONS * u + 1)):
            base = region_rows * region
            fixed["q_all"][base] = 1
            for c in cells:
                if c.form == F.FORM_PAIR:
                    fixed[f"scale{c.column // 2}"][base + c.row] = F.pair_scale(fam, c, table_bits)
            if isinstance(o, Const):
                fixed["const"][base + erow] = o.value
                copies.append(((fcol["const"], base + erow), (X, base + erow)))
            elif isinstance(o, DigestWord):
                copies.append((tail_cell(o), (X, base + erow)))
            else:
                xor_var_cells.setdefault(o.index, []).append((X, base + erow))
        fixed["q_f3"][base] = fixed["q_xor"][base] = 1  # `base`: the unit's second region
    for i in sorted(xor_var_cells):
        own = var_cells.get(i) or init_var_cells.get(i)
        first, rest = (own[0], xor_var_cells[i]) if own else (xor_var_cells[i][0], xor_var_cells[i][1:])
        copies += [(first, cell) for cell in rest]
    copies += xor_readers
    return w.description(cs, adv, fcol, fixed, inst, copies, cells, table_bits, tuple(s.blocks for s in plan.segments),
                         tuple(getattr(s, "variant", 0) for s in plan.segments), k, names)


# ---- the word buffer -----------------------------------------------------------------------------------------------------------

class Lowered(NamedTuple):
    """A plan as the synthesis entry points take it, and the shape of the word buffer its sources index: the distinct
    constants, then every Private word in (segment, word) order -- a segment's initial ones first -- then the vars, then
    the bits.  A plain source is a word index or source_digest + 8 * segment + word."""

    seg_blocks: np.ndarray      # uint32[segments]
    seg_variant: np.ndarray     # uint32[segments]; None at a width with one variant
    sources: np.ndarray         # uint32[16 * blocks]: a plain source, source_choice + entry, or source_digest + 8 * segments + unit
    init_sources: np.ndarray    # uint32[8 * segments]: source_iv or a plain source
    choices: np.ndarray         # uint32[entries, 4]: {bit, zero, one, 0}, bit a word index, the operands plain sources
    xors: np.ndarray            # uint32[units, 4]: {x, y, 0, 0}, plain sources
    consts: np.ndarray          # the width's dtype: the head of the word buffer
    words_len: int
    private_counts: list        # Private words per segment: its initial words' first, then its message words'
    shared_counts: tuple        # (vars, bits)

    var_count = property(lambda self: self.shared_counts[0])


def lower(w: Width, plan) -> Lowered:
    """The plan's sources as indices into its word buffer; needs no key and no device.  ValueError for a malformed plan."""
    _check_plan(w, plan)
    units = xor_units(plan)
    consts = sorted({s.value for s in _sources(plan) + [o for unit in units for o in unit] if isinstance(s, Const)})
    at_const = {v: i for i, v in enumerate(consts)}
    private_counts = [sum(isinstance(s, Private) for s in tuple(seg.init or ()) + tuple(seg.sources)) for seg in plan.segments]
    nvars, nbits = shared_counts(plan)
    first_var = len(consts) + sum(private_counts)
    first_bit = first_var + nvars
    at_unit = {unit: w.source_digest + 8 * len(plan.segments) + u for u, unit in enumerate(units)}
    choices, nxt = [], len(consts)

    def index(s):
        nonlocal nxt
        if isinstance(s, Private):  # the next one: a segment's Private initial words come before its Private message words
            nxt += 1
            return nxt - 1
        if isinstance(s, Const):
            return at_const[s.value]
        if isinstance(s, Var):
            return first_var + s.index
        if isinstance(s, DigestWord):
            return w.source_digest + 8 * s.segment + s.word
        if isinstance(s, Xor):  # the unit's result word, behind the segments' digests
            return at_unit[s]
        choices.append((first_bit + s.bit, index(s.zero), index(s.one), 0))  # entry c of the choice table
        return w.source_choice + len(choices) - 1

    sources, init_sources = [], []
    for seg in plan.segments:
        init_sources += [w.source_iv] * 8 if seg.init is None else [index(s) for s in seg.init]
        sources += [index(s) for s in seg.sources]
    assert nxt == first_var
    u32 = lambda values, *shape: np.array(values, dtype=np.uint32).reshape(*shape or (-1,))
    return Lowered(u32([seg.blocks for seg in plan.segments]), u32([seg.variant for seg in plan.segments]) if len(w.iv) > 1 else None,
                   u32(sources), u32(init_sources), u32(choices, -1, 4), u32([(index(unit.x), index(unit.y), 0, 0) for unit in units], -1, 4),
                   np.array(consts, dtype=w.dtype), first_bit + nbits, private_counts, (nvars, nbits))


def word_buffer(low: Lowered, values, shared=(), bits=()) -> np.ndarray:
    """The word buffer of a lowered plan for one witness: `values` per segment its Private words in word order, `shared`
    the Var words by index, `bits` the bits.  ValueError for counts that are not the plan's or values out of range."""
    dtype = low.consts.dtype
    if [len(v) for v in values] != low.private_counts:
        raise ValueError(f"private words per segment: {low.private_counts}, not {[len(v) for v in values]}")
    if (len(shared), len(bits)) != low.shared_counts:
        raise ValueError(f"(shared words, bits): {low.shared_counts}, not {(len(shared), len(bits))}")
    words, bits = [x for v in values for x in v] + list(shared), [int(b) for b in bits]  # one list, one check, one array: a batch has hundreds of segments
    if (words and not 0 <= min(words) <= max(words) < 1 << 8 * dtype.itemsize) or any(b not in (0, 1) for b in bits):
        raise ValueError(f"private and shared words are {8 * dtype.itemsize}-bit words, bits are 0 or 1")
    return np.concatenate([low.consts, np.array(words, dtype=dtype), np.array(bits, dtype=dtype)])


def _words_to_mont(words) -> np.ndarray:
    """words -> uint64[len, 4] Montgomery limbs (a batch has thousands of instance words: one bytes join, no array per word)."""
    r = (1 << 256) % FR_MODULUS
    return np.frombuffer(b"".join((int(x) * r % FR_MODULUS).to_bytes(32, "little") for x in words), dtype=np.uint64).reshape(-1, 4).copy()


# ---- the circuit ---------------------------------------------------------------------------------------------------------------

class Sha2SegmentsCircuit:
    """Proving key and GPU witness synthesis for a plan of wired segments at 2^k rows; a subclass names its `width` and calls
    its entry point (`_call`).  A key fixes the plan: the segments, their block counts, their wiring and what is public.

    The methods synthesize, check, assert_satisfied and prove take what `_inputs` takes -- (values, shared, bits), or a front
    end's own arguments.  `values` is one sequence per segment: the segment's Private words in word order -- for a segment
    with an `init`, its Private initial words first; `shared` holds the plan's Var words by index and `bits` its bits (each 0
    or 1).  The instance is the public words of the final states in the order of `plan.public`, then the public initial
    states' words.  Private words are unconstrained -- a private message's padding included: the circuit proves the
    compression of the words it is given, not that they are a padded message.  Const words and DigestWord wirings are
    constrained; a Choice word is constrained to the operand its bit selects, an Xor word to the XOR of its operands."""

    width: Width = None

    def __init__(self, ctx: Context, k: int, plan, table_bits: int = 12, setup: str = "toxic", seed: int = 0x5348413243515F):
        w = self.width
        self.plan = plan
        w.circuit._build_key(self, ctx, k, table_bits, setup, seed, lambda dense, spread: describe(w, k, plan, table_bits, dense, spread))
        self.rows, self._public = rows_for(w, plan), w.public(plan)
        self._lowered = low = lower(w, plan)
        size = low.consts.dtype.itemsize
        self._words = ctx.alloc(size * max(low.words_len, 1))
        self._digests = ctx.alloc(size * (8 * len(plan.segments) + len(low.xors)))  # behind the final states: every XOR unit's result word
        self.state_words = self.digest_words = self.instances = self.init_words = self.instance_words = None

    # ---- witness ----
    def _values(self, values):
        """What a front end's methods take in place of `values`-> the plan's `values`."""
        return values

    def _inputs(self, values, shared=(), bits=()):
        """What the methods take -> (values, shared, bits) of the plan."""
        return self._values(values), shared, bits

    def _call(self, arr):
        """The entry point alone, on the word buffer as it is on the device."""
        raise NotImplementedError

    def synthesize(self, *inputs):
        """Uploads the word buffer, fills the advice columns on the GPU and downloads the final states; returns (device
        columns, instances)."""
        words = word_buffer(self._lowered, *self._inputs(*inputs))
        if len(words):
            self._words.upload(words)
        return self._finish(words)

    def _finish(self, words):
        """The entry point on the word buffer as it is on the device (`words`: its host copy), then the instances."""
        w, low = self.width, self._lowered
        self._call((C.c_void_p * F.ADVICE_COLUMNS)(*[c.ptr for c in self.cols]))
        self.state_words = self.digest_words = self._digests.download((len(low.seg_blocks), 8), w.dtype).tolist()
        flat = [x for s in self.state_words for x in s]
        self.init_words = [[int(flat[s - w.source_digest] if s & w.source_digest else words[s]) for s in low.init_sources[8 * q: 8 * q + 8].tolist()]
                           for q in self.plan.public_init]
        self.instance_words = [x for s, count in self._public for x in self.state_words[s][:count]] + [x for ws in self.init_words for x in ws]
        self.instances = [_words_to_mont(self.instance_words)]
        return self.cols, self.instances

    @property
    def digests(self):
        """The public digests of the last synthesis in instance order, big-endian bytes."""
        return [struct.pack(f">{count}{self.width.letter}", *self.state_words[s][:count]) for s, count in self._public]

    def _result(self):
        return self.digests

    def check(self, *inputs, max_failures: int = 64):
        cols, inst = self.synthesize(*inputs)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, *inputs):
        cols, inst = self.synthesize(*inputs)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, *inputs, seed: int = 1):
        """(proof bytes, what the front end makes public): create_proof with the instance words as the public inputs."""
        cols, inst = self.synthesize(*inputs)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self._result()

    def close(self):
        for o in (self._words, self._digests):
            o.close()
        self.width.circuit._close_key(self)
