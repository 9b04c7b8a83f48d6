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
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple

import numpy as np

from . import sha256_circuit as SC
from ._lib import constants
from ._marshal import FR_MODULUS
from .context import Context

SOURCE_DIGEST, SOURCE_CHOICE, SOURCE_IV = (constants()["CQ_SHA256_SOURCE_" + s] for s in ("DIGEST", "CHOICE", "IV"))
IV224 = (0xC1059ED8, 0x367CD507, 0x3070DD17, 0xF70E5939, 0xFFC00B31, 0x68581511, 0x64F98FA7, 0xBEFA4FA4)  # FIPS 180-4, 5.3.2


class Private(NamedTuple):
    """A message word the prover chooses: no constraint ties it to anything."""


class Const(NamedTuple):
    """A message word pinned to `value` through the `const` fixed column."""

    value: int


class DigestWord(NamedTuple):
    """A message word tied to digest word `word` of the earlier segment `segment`."""

    segment: int
    word: int


class Var(NamedTuple):
    """Shared private 32-bit word number `index` of the plan: it may stand in several places -- as a message word or as
    an operand of a Choice -- and all its cells are tied by copies."""

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


PRIVATE = Private()
PAD_64_BYTES = (Const(0x80000000),) + (Const(0),) * 14 + (Const(512),)  # the second block of a 64-byte message


def batch(blocks_list) -> Plan:
    """Independent messages of the given block counts: every word private, every digest public."""
    segs = tuple(Segment(b, (PRIVATE,) * (16 * b)) for b in blocks_list)
    return Plan(segs, tuple(range(len(segs))))


def double_sha256(blocks: int) -> Plan:
    """SHA-256d: a private message of `blocks` blocks, then the one-block hash of its digest, whose padding is pinned;
    only the second digest is public."""
    second = tuple(DigestWord(0, i) for i in range(8)) + (Const(0x80000000),) + (Const(0),) * 6 + (Const(256),)
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks)), Segment(1, second)), (1,))


def merkle_tree(depth: int) -> Plan:
    """The root over 2^depth private 32-byte leaves: every node hashes left || right (64 bytes, two blocks, the second
    one pinned padding); nodes level by level, the 2^(depth - 1) nodes over the leaves first; only the root is public."""
    if depth < 1:
        raise ValueError("a Merkle tree has at least two leaves (depth >= 1)")
    segs, below = [], None
    for level in range(depth):
        first = len(segs)
        for i in range(1 << (depth - 1 - level)):
            if level == 0:
                children = (PRIVATE,) * 16
            else:
                children = tuple(DigestWord(below + 2 * i + side, w) for side in (0, 1) for w in range(8))
            segs.append(Segment(2, children + PAD_64_BYTES))
        below = first
    return Plan(tuple(segs), (len(segs) - 1,))


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


def midstate(blocks: int) -> Plan:
    """Compressing `blocks` private blocks takes the public state H_in to the public state H_out: one segment, every
    message word and every initial word Private, the digest (instance rows 0 .. 7) and the initial state (rows 8 .. 15)
    public.  Nothing says the blocks are padded or where a message ends: it is the link of a chain of proofs."""
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks), (PRIVATE,) * 8),), (0,), (0,))


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


def has_init(plan: Plan) -> bool:
    return any(seg.init is not None for seg in plan.segments)


def has_choice(plan: Plan) -> bool:
    return any(isinstance(s, Choice) for seg in plan.segments for s in seg.sources)


def xor_units(plan: Plan):
    """The plan's XOR units: its distinct Xor words in the order of their first use, by (segment, word)."""
    return list(dict.fromkeys(s for seg in plan.segments for s in seg.sources if isinstance(s, Xor)))


def has_xor(plan: Plan) -> bool:
    return any(isinstance(s, Xor) for seg in plan.segments for s in seg.sources)


def shared_counts(plan: Plan):
    """(vars, bits) of the plan: one more than the largest index used, 0 if none is."""
    srcs = [s for seg in plan.segments for s in tuple(seg.sources) + tuple(seg.init or ())]
    operands = [o for s in srcs if isinstance(s, Choice) for o in (s.zero, s.one)] + [o for s in srcs if isinstance(s, Xor) for o in (s.x, s.y)]
    return (max([v.index + 1 for v in srcs + operands if isinstance(v, Var)], default=0),
            max([s.bit + 1 for s in srcs if isinstance(s, Choice)], default=0))


def rows_for(plan: Plan) -> int:
    """The rows the plan uses: its segments one behind another, then SC.XOR_REGIONS regions per XOR unit."""
    return sum(SC.rows_for(s.blocks) for s in plan.segments) + SC.XOR_REGIONS * SC.REGION_ROWS * len(xor_units(plan))


def xor_first_region(plan: Plan) -> int:
    """The first region of the XOR area: the one directly behind the last segment's tail.  Unit u takes regions
    SC.XOR_REGIONS * u (e = x) and SC.XOR_REGIONS * u + 1 (e = y, W = x ^ y) from there."""
    return sum(SC.BLOCK_REGIONS * s.blocks + SC.TAIL_REGIONS for s in plan.segments)


def first_regions(plan: Plan):
    """The first region of every segment."""
    out, at = [], 0
    for s in plan.segments:
        out.append(at)
        at += SC.BLOCK_REGIONS * s.blocks + SC.TAIL_REGIONS
    return out


def _check_plan(plan: Plan):
    if not plan.segments:
        raise ValueError("a plan has at least one segment")

    def digest_word(j, t, src, what=""):
        where = t if isinstance(t, str) else f"word {t}"
        if not 0 <= src.segment < j:
            raise ValueError(f"segment {j}, {where}: the digest of segment {src.segment}{what} does not come before it")
        if not 0 <= src.word < 8:
            raise ValueError(f"segment {j}, {where}: a digest has words 0 .. 7, not {src.word}")

    for j, seg in enumerate(plan.segments):
        if seg.blocks < 1 or len(seg.sources) != 16 * seg.blocks:
            raise ValueError(f"segment {j}: {seg.blocks} blocks and {len(seg.sources)} word sources (16 per block, at least one block)")
        if seg.init is not None and len(seg.init) != 8:
            raise ValueError(f"segment {j}: an initial state has 8 words, not {len(seg.init)}")
        for i, src in enumerate(seg.init or ()):
            if isinstance(src, DigestWord):
                digest_word(j, f"initial word {i}", src)
            elif isinstance(src, Var):
                if src.index < 0:
                    raise ValueError(f"segment {j}, initial word {i}: the var index {src.index} is negative")
            elif isinstance(src, Const):
                if not 0 <= src.value < 1 << 32:
                    raise ValueError(f"segment {j}, initial word {i}: the constant {src.value} is no 32-bit word")
            elif not isinstance(src, Private):
                raise ValueError(f"segment {j}, initial word {i}: an initial word is Private, Const, DigestWord or Var, not {src!r}")
        for t, src in enumerate(seg.sources):
            if isinstance(src, DigestWord):
                digest_word(j, t, src)
            elif isinstance(src, Var):
                if src.index < 0:
                    raise ValueError(f"segment {j}, word {t}: the var index {src.index} is negative")
            elif isinstance(src, Choice):
                if src.bit < 0:
                    raise ValueError(f"segment {j}, word {t}: the bit index {src.bit} is negative")
                for name, o in (("zero", src.zero), ("one", src.one)):
                    if isinstance(o, DigestWord):
                        digest_word(j, t, o, f" (the {name} operand)")
                    elif not isinstance(o, Var):
                        raise ValueError(f"segment {j}, word {t}: the {name} operand of a choice is a Var or a DigestWord, not {o!r}")
                    elif o.index < 0:
                        raise ValueError(f"segment {j}, word {t}: the var index {o.index} of the {name} operand is negative")
            elif isinstance(src, Xor):
                for name, o in (("x", src.x), ("y", src.y)):
                    if isinstance(o, DigestWord):
                        digest_word(j, t, o, f" (the {name} operand)")
                    elif isinstance(o, Var):
                        if o.index < 0:
                            raise ValueError(f"segment {j}, word {t}: the var index {o.index} of the {name} operand is negative")
                    elif isinstance(o, Const):
                        if not 0 <= o.value < 1 << 32:
                            raise ValueError(f"segment {j}, word {t}: the constant {o.value} of the {name} operand is no 32-bit word")
                    else:
                        raise ValueError(f"segment {j}, word {t}: the {name} operand of an xor is a Const, a Var or a DigestWord, not {o!r}")
            elif isinstance(src, Const):
                if not 0 <= src.value < 1 << 32:
                    raise ValueError(f"segment {j}, word {t}: the constant {src.value} is no 32-bit word")
            elif not isinstance(src, Private):
                raise ValueError(f"segment {j}, word {t}: a source is Private, Const, DigestWord, Var, Choice or Xor, not {src!r}")
    if has_xor(plan) and has_choice(plan):
        j, t = next((j, t) for j, seg in enumerate(plan.segments) for t, s in enumerate(seg.sources) if isinstance(s, Choice))
        raise ValueError(f"segment {j}, word {t}: a Choice in a plan that holds an Xor -- the two variants do not combine")
    if not plan.public or len(set(plan.public)) != len(plan.public) or not all(0 <= p < len(plan.segments) for p in plan.public):
        raise ValueError(f"public segments {plan.public!r}: at least one, each an index below {len(plan.segments)}, none twice")
    pi = tuple(plan.public_init)
    if len(set(pi)) != len(pi) or not all(isinstance(q, int) and 0 <= q < len(plan.segments) and plan.segments[q].init is not None for q in pi):
        raise ValueError(f"public_init segments {pi!r}: each an index below {len(plan.segments)} of a segment with an init, none twice")


def describe(k: int, plan: Plan, table_bits: int = 12, dense="dense", spread="spread") -> SC.Description:
    """The constraint system of sha256_circuit.describe with the fixed columns and copies of `plan`; `blocks` is the
    tuple of the segments' block counts.  ValueError for a plan that is malformed or does not fit 2^k rows."""
    if not SC.MIN_TABLE_BITS <= table_bits <= SC.MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{SC.MIN_TABLE_BITS}, {SC.MAX_TABLE_BITS}]: the widest piece has {SC.MIN_TABLE_BITS} bits")
    _check_plan(plan)
    choice, units = has_choice(plan), xor_units(plan)
    names = SC.FIXED_CHOICE if choice else SC.FIXED_XOR if units else SC.FIXED
    cs, adv, fcol, inst, cells, word = SC._constraint_system(table_bits, dense, spread, choice, xor=bool(units))
    n, X, Y = 1 << k, adv[2 * SC.PAIRS], adv[2 * SC.PAIRS + 1]
    rows, usable = rows_for(plan), n - (cs.blinding_factors() + 1)
    instance_rows = 8 * (len(plan.public) + len(plan.public_init))
    if max(rows, instance_rows) > usable:
        area = f" and {len(units)} xor units" if units else ""
        raise ValueError(f"{len(plan.segments)} segments{area} need {rows} rows and {instance_rows} instance rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in names}
    copies = []
    firsts = first_regions(plan)
    public = {s: p for p, s in enumerate(plan.public)}
    arow, erow, wrow = (word[(SC.SRC[s], SC.FORM_WORD)].row for s in "AEW")

    def tail_cell(src):  # tail region 3 - i % 4 holds digest word i: its A row for i < 4, its E row otherwise
        s = plan.segments[src.segment]
        tail = SC.REGION_ROWS * (firsts[src.segment] + SC.BLOCK_REGIONS * s.blocks + 3 - src.word % 4)
        return X, tail + (arow if src.word < 4 else erow)

    # the cells of the choices' digest operands, of every var and of every bit, in (segment, word, zero-then-one) order
    digest_cells, var_cells, bit_cells = [], {}, {}
    init_digest_cells, init_var_cells, init_public_cells = [], {}, []
    xor_first, xor_readers = xor_first_region(plan), []  # every reader's W cell, tied to its unit's, in (segment, word) order
    for j, seg in enumerate(plan.segments):
        # a constant initial word is pinned where the IV's is, by the same lines; the others are tied behind everything else
        pinned = None if seg.init is None else [s.value if isinstance(s, Const) else None for s in seg.init]
        SC._assign_segment(fixed, copies, firsts[j], seg.blocks, public.get(j), table_bits, adv, fcol, inst, cells, word, pinned)
        for i, src in enumerate(seg.init or ()):  # state word i: region 3 - i % 4 of the first block, A row for i < 4, else E row
            cell = (X, SC.REGION_ROWS * (firsts[j] + 3 - i % 4) + (arow if i < 4 else erow))
            if isinstance(src, DigestWord):
                init_digest_cells.append((tail_cell(src), cell))
            elif isinstance(src, Var):
                init_var_cells.setdefault(src.index, []).append(cell)
            if j in plan.public_init:
                init_public_cells.append(((inst, 8 * len(plan.public) + 8 * plan.public_init.index(j) + i), cell))
        for t, src in enumerate(seg.sources):
            base = SC.REGION_ROWS * (firsts[j] + SC.BLOCK_REGIONS * (t // 16) + 4 + t % 16)
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
                for o, row in ((src.zero, SC.CHOICE_ROW_ZERO), (src.one, SC.CHOICE_ROW_ONE)):
                    if isinstance(o, DigestWord):
                        digest_cells.append((tail_cell(o), (Y, base + row)))
                    else:
                        var_cells.setdefault(o.index, []).append((Y, base + row))
                bit_cells.setdefault(src.bit, []).append((Y, base + SC.CHOICE_ROW_BIT))
            elif isinstance(src, Xor):
                xor_readers.append(((X, SC.REGION_ROWS * (xor_first + SC.XOR_REGIONS * units.index(src) + 1) + wrow), (X, w_cell)))
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
    # W = x ^ y under q_all, q_f3 and q_xor; scales in both as _assign_segment sets them.  Copies, all in X: (1) unit after
    # unit, x then y, a Const operand's E cell to `const` and a DigestWord operand's E cell to its tail cell; (2) vars in
    # ascending index: every operand cell of the var to the var's first cell -- its first message cell if it has one, else
    # its first state cell, else its first operand cell; (3) every reader's W cell to its unit's W cell
    xor_var_cells = {}
    for u, unit in enumerate(units):
        for o, region in ((unit.x, xor_first + SC.XOR_REGIONS * u), (unit.y, xor_first + SC.XOR_REGIONS * u + 1)):
            base = SC.REGION_ROWS * region
            fixed["q_all"][base] = 1
            for c in cells:
                if c.form == SC.FORM_PAIR:
                    fixed[f"scale{c.column // 2}"][base + c.row] = 1 << (table_bits - SC._field_of(c, table_bits)[1]) if c.len else 1
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
    return SC.Description(cs, adv, fcol, fixed, inst, copies, cells, table_bits, tuple(s.blocks for s in plan.segments), k, names)


class Lowered(NamedTuple):
    """A plan as the entry points take it: the arrays of cq_sha256_synthesize_segments_dev / _choices_dev / _states_dev /
    _xors_dev and the shape of the word buffer they index -- the distinct constants, then every Private word in (segment,
    word) order, then the vars, then the bits."""

    seg_blocks: np.ndarray      # uint32[segments]
    sources: np.ndarray         # uint32[16 * blocks]: a word index, SOURCE_DIGEST + 8 * segment + word, or SOURCE_CHOICE + entry
    choices: np.ndarray         # uint32[entries, 4]: {bit, zero, one, 0}, bit a word index, the operands plain sources
    consts: np.ndarray          # uint32: the head of the word buffer
    words_len: int
    private_counts: list        # Private words per segment: its initial words' first, then its message words'
    shared_counts: tuple        # (vars, bits)
    init_sources: np.ndarray = None  # uint32[8 * segments]: SOURCE_IV, a word index or SOURCE_DIGEST + 8 * segment + word
    xors: np.ndarray = None     # uint32[units, 4]: {x, y, 0, 0}, plain sources; a reader's source is SOURCE_DIGEST + 8 * segments + unit


def lower(plan: Plan) -> Lowered:
    """The plan's sources as indices into its word buffer; needs no key and no device."""
    units = xor_units(plan)
    consts = sorted({s.value for seg in plan.segments for s in tuple(seg.sources) + tuple(seg.init or ()) if isinstance(s, Const)} |
                    {o.value for unit in units for o in unit if isinstance(o, Const)})
    at_const = {v: i for i, v in enumerate(consts)}
    private_counts = [sum(isinstance(s, Private) for s in tuple(seg.init or ()) + tuple(seg.sources)) for seg in plan.segments]
    nvars, nbits = shared_counts(plan)
    first_var = len(consts) + sum(private_counts)
    first_bit = first_var + nvars

    def plain(s):
        if isinstance(s, Const):
            return at_const[s.value]
        return first_var + s.index if isinstance(s, Var) else SOURCE_DIGEST + 8 * s.segment + s.word

    at_unit = {unit: SOURCE_DIGEST + 8 * len(plan.segments) + u for u, unit in enumerate(units)}
    sources, choices, init_sources, nxt = [], [], [], len(consts)
    for seg in plan.segments:
        for s in seg.init or (None,) * 8:  # a segment's Private initial words come before its Private message words
            if s is None:
                init_sources.append(SOURCE_IV)
            elif isinstance(s, Private):
                init_sources.append(nxt)
                nxt += 1
            else:
                init_sources.append(at_const[s.value] if isinstance(s, Const) else plain(s))
        for s in seg.sources:
            if isinstance(s, Private):
                sources.append(nxt)
                nxt += 1
            elif isinstance(s, Choice):  # entry c of the choice table: {bit, zero, one, 0}
                sources.append(SOURCE_CHOICE + len(choices))
                choices.append((first_bit + s.bit, plain(s.zero), plain(s.one), 0))
            elif isinstance(s, Xor):  # the unit's result word, behind the segments' digests
                sources.append(at_unit[s])
            else:
                sources.append(at_const[s.value] if isinstance(s, Const) else plain(s))
    assert nxt == first_var
    xors = [(plain(unit.x), plain(unit.y), 0, 0) for unit in units]
    return Lowered(np.array([seg.blocks for seg in plan.segments], dtype=np.uint32), np.array(sources, dtype=np.uint32),
                   np.array(choices, dtype=np.uint32).reshape(-1, 4), np.array(consts, dtype=np.uint32), first_bit + nbits,
                   private_counts, (nvars, nbits), np.array(init_sources, dtype=np.uint32),
                   np.array(xors, dtype=np.uint32).reshape(-1, SC.XOR_WORDS))


def word_buffer(low: Lowered, values, shared=(), bits=()) -> np.ndarray:
    """The word buffer of a lowered plan for one witness: `values` per segment its Private words in word order, `shared`
    the Var words by index, `bits` the bits.  ValueError for counts that are not the plan's or values out of range."""
    values = [np.asarray(v, dtype=np.uint32).reshape(-1) for v in values]
    if [len(v) for v in values] != low.private_counts:
        raise ValueError(f"private words per segment: {low.private_counts}, not {[len(v) for v in values]}")
    if any(not 0 <= int(w) < 1 << 32 for w in shared) or any(int(b) not in (0, 1) for b in bits):
        raise ValueError("shared words are 32-bit words, bits are 0 or 1")
    if (len(shared), len(bits)) != low.shared_counts:
        raise ValueError(f"(shared words, bits): {low.shared_counts}, not {(len(shared), len(bits))}")
    tail = [np.array([int(x) for x in part], dtype=np.uint32) for part in (shared, bits)]
    return np.concatenate([low.consts] + values + tail)


def _words_to_mont(words) -> np.ndarray:
    """32-bit words -> uint64[len, 4] Montgomery limbs (a batch has thousands of instance words: one bytes join, no
    array per word)."""
    r = (1 << 256) % FR_MODULUS
    return np.frombuffer(b"".join((int(w) * r % FR_MODULUS).to_bytes(32, "little") for w in words), dtype=np.uint64).reshape(-1, 4).copy()


def _digest_words(message: bytes):
    return list(struct.unpack(">8I", message))


class Sha256SegmentsCircuit:
    """Proving key and GPU witness synthesis for a plan of wired SHA-256 segments at 2^k rows.  A key fixes the plan:
    the number of segments, their block counts, their wiring and which digests are public.

    `values` (synthesize, check, assert_satisfied, prove) is one sequence per segment: the segment's Private words in
    word order -- for a segment with an `init`, its Private initial words first.  With `public_init` the instance is the
    public digests' words, then the public initial states' words.  Private words are unconstrained -- a private message's padding included, exactly as in Sha256Circuit:
    the circuit proves the compression of the words it is given, not that they are a padded message.  Const words and
    DigestWord wirings are constrained.  `shared` holds the plan's Var words by index and `bits` its bits (each 0 or 1);
    a Choice word is constrained to the operand its bit selects."""

    def __init__(self, ctx: Context, k: int, plan: Plan, table_bits: int = 12, setup: str = "toxic", seed: int = 0x5348413243515F):
        self.plan = plan
        SC._build_key(self, ctx, k, table_bits, setup, seed, lambda dense, spread: describe(k, plan, table_bits, dense, spread))
        self.rows = rows_for(plan)
        self._lowered = low = lower(plan)
        self._seg_blocks, self._sources, self._choices, self._words_len = low.seg_blocks, low.sources, low.choices, low.words_len
        self._init_sources = low.init_sources if has_init(plan) else None
        self._xors = low.xors
        self._words = ctx.alloc(4 * max(self._words_len, 1))
        self._digests = ctx.alloc(32 * len(plan.segments) + 4 * len(low.xors))  # behind the digests: every XOR unit's result word
        self.digest_words = self.instances = self.init_words = self.instance_words = None

    # ---- witness ----
    def _values(self, values):
        return values

    def _inputs(self, values, shared, bits):
        """What a front end's methods take -> (values, shared, bits) of the plan."""
        return self._values(values), shared, bits

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

    def synthesize(self, values, shared=(), bits=()):
        """Uploads the word buffer, fills the advice columns on the GPU (cq_sha256_synthesize_segments_dev,
        cq_sha256_synthesize_choices_dev for a plan with choices, cq_sha256_synthesize_states_dev for one with an initial
        state) and downloads the digests; returns (device columns, instances)."""
        values, shared, bits = self._inputs(values, shared, bits)
        words = word_buffer(self._lowered, values, shared, bits)
        self._words.upload(words)
        return self._finish(words)

    def _finish(self, words):
        """The entry point on the word buffer as it is on the device (`words`: its host copy), then the instances."""
        self._call((C.c_void_p * SC.ADVICE_COLUMNS)(*[c.ptr for c in self.cols]))
        self.digest_words = self._digests.download((len(self._seg_blocks), 8), np.uint32).tolist()
        flat = [x for d in self.digest_words for x in d]
        self.init_words = [[int(flat[s - SOURCE_DIGEST] if s & SOURCE_DIGEST else words[s]) for s in self._lowered.init_sources[8 * q: 8 * q + 8]]
                           for q in self.plan.public_init]
        self.instance_words = [x for p in self.plan.public for x in self.digest_words[p]] + [x for ws in self.init_words for x in ws]
        self.instances = [_words_to_mont(self.instance_words)]
        return self.cols, self.instances

    @property
    def digests(self):
        """The digests of the public segments of the last synthesis, 32 big-endian bytes each, in instance order."""
        return [struct.pack(">8I", *self.digest_words[p]) for p in self.plan.public]

    def _result(self):
        return self.digests

    def check(self, values, shared=(), bits=(), max_failures: int = 64):
        cols, inst = self.synthesize(values, shared, bits)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, values, shared=(), bits=()):
        cols, inst = self.synthesize(values, shared, bits)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, values, shared=(), bits=(), seed: int = 1):
        """(proof bytes, public digests): create_proof with the public segments' digest words as the public inputs."""
        cols, inst = self.synthesize(values, shared, bits)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self._result()

    def close(self):
        for o in (self._words, self._digests):
            o.close()
        SC._close_key(self)


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
        self.digest_words, self.init_words = [out.tolist()], [[int(x) for x in h_in]]
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

    def _inputs(self, item, shared=(), bits=()):
        if shared or bits:
            raise ValueError("an HMAC takes (key, message) and nothing else")
        key, message = (bytes(x) for x in item)
        if (len(key), len(message)) != (self.key_bytes, self.message_bytes):
            raise ValueError(f"a key of {self.key_bytes} bytes and a message of {self.message_bytes}, not {len(key)} and {len(message)}")
        words = lambda data: list(struct.unpack(f">{len(data) // 4}I", data))
        return [words(message)] + [[]] * (len(self.plan.segments) - 1), words(key), []

    def synthesize(self, key, message):
        return super().synthesize((key, message))

    def check(self, key, message, max_failures: int = 64):
        cols, inst = self.synthesize(key, message)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, key, message):
        cols, inst = self.synthesize(key, message)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, key, message, seed: int = 1):
        """(proof bytes, tag): the public inputs are the tag's words, then with `commit_key` those of SHA-256(key)."""
        cols, inst = self.synthesize(key, message)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self.tag()

    def tag(self) -> bytes:
        """The tag of the last synthesis, 32 bytes."""
        return self.digests[0]

    def key_commitment(self) -> bytes:
        """SHA-256(key) of the last synthesis (`commit_key` only)."""
        if not self.commit_key:
            raise ValueError("the circuit was built without commit_key")
        return self.digests[1]

    def _result(self):
        return self.tag()
