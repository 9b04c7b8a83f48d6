"""Wired multi-segment SHA-512 circuits: several compression chains ("segments") one behind another in the columns of
the SHA-512 / SHA-384 compression circuit, tied to each other and to constants by copy constraints ("Wired
SHA-512 segments").  The 64-bit counterpart of sha256_segments.py's copy-constraint half: message words and initial-state
words that are private, constants, shared private words or digest words of earlier segments, and public digests of 1 .. 8
words.  The constraint system is the one of sha512_circuit.py, gate for gate; only the fixed columns and the copies
differ.  The witness is synthesised on the GPU by `cq_sha512_synthesize_segments_dev`, which runs the chains level by
level on the device.  `Choice` and `Xor` words need gates the 64-bit circuit does not have yet and are rejected.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple

import numpy as np

from . import sha512_circuit as SC
from ._lib import constants
from .context import Context
from .sha256_segments import Choice, Const, DigestWord, Private, Var, Xor, _words_to_mont  # noqa: F401

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


PRIVATE = Private()
PAD_128_BYTES = (Const(1 << 63),) + (Const(0),) * 14 + (Const(1024),)  # the second block of a 128-byte message


def batch(blocks_list, variants=None) -> Plan:
    """Independent messages of the given block counts (SHA-512, or variants[j]): every word private, every digest public
    -- 8 words of a SHA-512 message, 6 of a SHA-384 one.  The circuit of sha512_circuit.describe_batch."""
    blocks_list = list(blocks_list)
    variants = [VARIANT_512] * len(blocks_list) if variants is None else list(variants)
    if len(variants) != len(blocks_list) or any(v not in SC.DIGEST_WORDS for v in variants):
        raise ValueError("one variant (VARIANT_512 or VARIANT_384) per message")
    segs = tuple(Segment(b, (PRIVATE,) * (16 * b), None, v) for b, v in zip(blocks_list, variants))
    return Plan(segs, tuple((j, SC.DIGEST_WORDS[v]) for j, v in enumerate(variants)))


def double_sha512(blocks: int) -> Plan:
    """SHA-512(SHA-512(message)): a private message of `blocks` blocks, then the one-block hash of its digest, whose padding
    is pinned; only the second digest is public."""
    second = tuple(DigestWord(0, i) for i in range(8)) + (Const(1 << 63),) + (Const(0),) * 6 + (Const(512),)
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks)), Segment(1, second)), ((1, 8),))


def merkle_tree(depth: int) -> Plan:
    """The root over 2^depth private 64-byte leaves: every node hashes left || right (128 bytes, two blocks, the second
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
            segs.append(Segment(2, children + PAD_128_BYTES))
        below = first
    return Plan(tuple(segs), ((len(segs) - 1, 8),))


def midstate(blocks: int) -> Plan:
    """Compressing `blocks` private blocks takes the public state H_in to the public state H_out: one segment, every
    message word and every initial word Private, the final state (instance rows 0 .. 7) and the initial state (rows
    8 .. 15) public.  Nothing says the blocks are padded or where a message ends: it is the link of a chain of proofs."""
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks), (PRIVATE,) * 8),), ((0, 8),), (0,))


def sha512_256(blocks: int) -> Plan:
    """SHA-512/256 of a private message of exactly `blocks` padded blocks: SHA-512's compression from the SHA-512/256
    initial hash value, pinned as constants; the first four words of the final state are the public digest."""
    return Plan((Segment(blocks, (PRIVATE,) * (16 * blocks), tuple(Const(v) for v in IV512_256)),), ((0, 4),))


def has_init(plan: Plan) -> bool:
    return any(seg.init is not None for seg in plan.segments)


def var_count(plan: Plan) -> int:
    """One more than the largest Var index the plan uses, 0 if it uses none."""
    return max([s.index + 1 for seg in plan.segments for s in tuple(seg.sources) + tuple(seg.init or ()) if isinstance(s, Var)], default=0)


def rows_for(plan: Plan) -> int:
    """The rows the plan uses: its segments one behind another."""
    return sum(SC.rows_for(s.blocks) for s in plan.segments)


def first_regions(plan: Plan):
    """The first region of every segment."""
    out, at = [], 0
    for s in plan.segments:
        out.append(at)
        at += SC.BLOCK_REGIONS * s.blocks + SC.TAIL_REGIONS
    return out


def instance_rows(plan: Plan) -> int:
    return sum(words for _, words in plan.public) + 8 * len(plan.public_init)


def _check_plan(plan: Plan):
    """ValueError, naming segment and word, for: no segment; a block count below 1 or a source count that is not 16 per
    block; a variant that is neither of the two; an `init` that has not 8 words; per message word and per initial word a
    DigestWord of the segment itself or a later one or with a word outside 0 .. 7, a negative Var index, a Const that is
    no 64-bit word, a Choice or an Xor (not built on the 64-bit circuit yet), anything else that is no source; `public`
    empty, not (segment, words) pairs, a segment out of range or twice, a word count outside 1 .. 8; `public_init` naming
    a segment out of range, twice, or without an `init`."""
    if not plan.segments:
        raise ValueError("a plan has at least one segment")
    for j, seg in enumerate(plan.segments):
        if seg.blocks < 1 or len(seg.sources) != 16 * seg.blocks:
            raise ValueError(f"segment {j}: {seg.blocks} blocks and {len(seg.sources)} word sources (16 per block, at least one block)")
        if seg.variant not in SC.IV:
            raise ValueError(f"segment {j}: the variant is VARIANT_512 or VARIANT_384, not {seg.variant!r}")
        if seg.init is not None and len(seg.init) != 8:
            raise ValueError(f"segment {j}: an initial state has 8 words, not {len(seg.init)}")
        for where, src in [(f"initial word {i}", s) for i, s in enumerate(seg.init or ())] + [(f"word {t}", s) for t, s in enumerate(seg.sources)]:
            if isinstance(src, DigestWord):
                if not 0 <= src.segment < j:
                    raise ValueError(f"segment {j}, {where}: the digest of segment {src.segment} does not come before it")
                if not 0 <= src.word < 8:
                    raise ValueError(f"segment {j}, {where}: a digest has words 0 .. 7, not {src.word}")
            elif isinstance(src, Var):
                if src.index < 0:
                    raise ValueError(f"segment {j}, {where}: the var index {src.index} is negative")
            elif isinstance(src, Const):
                if not 0 <= src.value < 1 << 64:
                    raise ValueError(f"segment {j}, {where}: the constant {src.value} is no 64-bit word")
            elif isinstance(src, (Choice, Xor)):
                raise ValueError(f"segment {j}, {where}: {type(src).__name__} words are not built on the 64-bit circuit yet")
            elif not isinstance(src, Private):
                raise ValueError(f"segment {j}, {where}: a source is Private, Const, DigestWord or Var, not {src!r}")
    pub = tuple(plan.public)
    if not pub or not all(isinstance(p, tuple) and len(p) == 2 and all(isinstance(x, int) for x in p) for p in pub):
        raise ValueError(f"public {pub!r}: at least one (segment, words) pair")
    if len({s for s, _ in pub}) != len(pub) or not all(0 <= s < len(plan.segments) for s, _ in pub):
        raise ValueError(f"public {pub!r}: each segment an index below {len(plan.segments)}, none twice")
    for s, words in pub:
        if not 1 <= words <= 8:
            raise ValueError(f"public: segment {s} has 1 .. 8 public words, not {words}")
    pi = tuple(plan.public_init)
    if len(set(pi)) != len(pi) or not all(isinstance(q, int) and 0 <= q < len(plan.segments) and plan.segments[q].init is not None for q in pi):
        raise ValueError(f"public_init segments {pi!r}: each an index below {len(plan.segments)} of a segment with an init, none twice")


def describe(k: int, plan: Plan, table_bits: int = 12, dense="dense", spread="spread") -> SC.Description:
    """The constraint system of sha512_circuit.describe_batch with the fixed columns and copies of `plan`.  ValueError for a
    plan that is malformed or does not fit 2^k rows."""
    if not SC.MIN_TABLE_BITS <= table_bits <= SC.MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{SC.MIN_TABLE_BITS}, {SC.MAX_TABLE_BITS}]: the widest piece has {SC.MIN_TABLE_BITS} bits")
    _check_plan(plan)
    cs, adv, fcol, inst, cells, word = SC._constraint_system(table_bits, dense, spread)
    n, X = 1 << k, adv[2 * SC.PAIRS]
    rows, usable = rows_for(plan), n - (cs.blinding_factors() + 1)
    if max(rows, instance_rows(plan)) > usable:
        raise ValueError(f"{len(plan.segments)} segments need {rows} rows and {instance_rows(plan)} instance rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in SC.FIXED}
    copies = []
    firsts = first_regions(plan)
    public_words, public_row, at = {}, {}, 0
    for s, words in plan.public:
        public_words[s], public_row[s] = words, at
        at += words
    init_row = {q: at + 8 * i for i, q in enumerate(plan.public_init)}
    arow, erow, wrow = (word[(SC.SRC[s], SC.FORM_WORD)].row for s in "AEW")

    def tail_cell(src):  # tail region 3 - i % 4 holds word i of the final state: its A row for i < 4, its E row otherwise
        s = plan.segments[src.segment]
        tail = SC.REGION_ROWS * (firsts[src.segment] + SC.BLOCK_REGIONS * s.blocks + 3 - src.word % 4)
        return X, tail + (arow if src.word < 4 else erow)

    var_cells, init_digest_cells, init_var_cells, init_public_cells = {}, [], {}, []
    for j, seg in enumerate(plan.segments):
        # a constant initial word is pinned where the initial hash value's is, by the same lines; the others are tied behind
        pinned = None if seg.init is None else [s.value if isinstance(s, Const) else None for s in seg.init]
        SC._assign_segment(fixed, copies, firsts[j], seg.blocks, seg.variant, public_row.get(j, 0), table_bits, adv, fcol, inst, cells, word,
                           pinned, public_words.get(j, 0))
        for i, src in enumerate(seg.init or ()):  # state word i: region 3 - i % 4 of the first block, A row for i < 4, else E row
            cell = (X, SC.REGION_ROWS * (firsts[j] + 3 - i % 4) + (arow if i < 4 else erow))
            if isinstance(src, DigestWord):
                init_digest_cells.append((tail_cell(src), cell))
            elif isinstance(src, Var):
                init_var_cells.setdefault(src.index, []).append(cell)
            if j in init_row:
                init_public_cells.append(((inst, init_row[j] + i), cell))
        for t, src in enumerate(seg.sources):
            w_cell = SC.REGION_ROWS * (firsts[j] + SC.BLOCK_REGIONS * (t // 16) + 4 + t % 16) + wrow
            if isinstance(src, Const):
                fixed["const"][w_cell] = src.value
                copies.append(((fcol["const"], w_cell), (X, w_cell)))
            elif isinstance(src, DigestWord):
                copies.append((tail_cell(src), (X, w_cell)))
            elif isinstance(src, Var):
                var_cells.setdefault(src.index, []).append((X, w_cell))
    # behind the segments' own copies: vars in ascending index, every later cell of a var to its first cell; then the
    # initial states: every digest-wired state cell to its tail cell in (segment, word) order; then, vars in ascending index,
    # every state cell of a var to the var's first cell (its first message cell if it has one, else its first state cell);
    # then the public initial words to their instance rows, in instance order
    for i in sorted(var_cells):
        copies += [(var_cells[i][0], cell) for cell in var_cells[i][1:]]
    copies += init_digest_cells
    for i in sorted(init_var_cells):
        first, rest = (var_cells[i][0], init_var_cells[i]) if i in var_cells else (init_var_cells[i][0], init_var_cells[i][1:])
        copies += [(first, cell) for cell in rest]
    copies += sorted(init_public_cells, key=lambda c: c[0][1])
    return SC.Description(cs, adv, fcol, fixed, inst, copies, cells, table_bits, tuple(s.blocks for s in plan.segments),
                          tuple(s.variant for s in plan.segments), k)


class Lowered(NamedTuple):
    """A plan as cq_sha512_synthesize_segments_dev takes it, and the shape of the word buffer its sources index: the
    distinct constants, then every Private word in (segment, word) order -- a segment's initial ones first -- then the vars."""

    seg_blocks: np.ndarray      # uint32[segments]
    seg_variant: np.ndarray     # uint32[segments]
    sources: np.ndarray         # uint32[16 * blocks]: a word index or SOURCE_DIGEST + 8 * segment + word
    init_sources: np.ndarray    # uint32[8 * segments]: SOURCE_IV, a word index or SOURCE_DIGEST + 8 * segment + word
    consts: np.ndarray          # uint64: the head of the word buffer
    words_len: int
    private_counts: list        # Private words per segment: its initial words' first, then its message words'
    var_count: int


def lower(plan: Plan) -> Lowered:
    """The plan's sources as indices into its word buffer; needs no key and no device."""
    _check_plan(plan)
    consts = sorted({s.value for seg in plan.segments for s in tuple(seg.sources) + tuple(seg.init or ()) if isinstance(s, Const)})
    at_const = {v: i for i, v in enumerate(consts)}
    private_counts = [sum(isinstance(s, Private) for s in tuple(seg.init or ()) + tuple(seg.sources)) for seg in plan.segments]
    nvars = var_count(plan)
    first_var = len(consts) + sum(private_counts)
    nxt = len(consts)

    def index(s):
        nonlocal nxt
        if isinstance(s, Private):
            nxt += 1
            return nxt - 1
        if isinstance(s, Const):
            return at_const[s.value]
        return first_var + s.index if isinstance(s, Var) else SOURCE_DIGEST + 8 * s.segment + s.word

    sources, init_sources = [], []
    for seg in plan.segments:
        init_sources += [SOURCE_IV] * 8 if seg.init is None else [index(s) for s in seg.init]
        sources += [index(s) for s in seg.sources]
    assert nxt == first_var
    return Lowered(np.array([seg.blocks for seg in plan.segments], dtype=np.uint32), np.array([seg.variant for seg in plan.segments], dtype=np.uint32),
                   np.array(sources, dtype=np.uint32), np.array(init_sources, dtype=np.uint32), np.array(consts, dtype=np.uint64),
                   first_var + nvars, private_counts, nvars)


def word_buffer(low: Lowered, values, shared=()) -> np.ndarray:
    """The word buffer of a lowered plan for one witness: `values` per segment its Private words in word order, `shared`
    the Var words by index.  ValueError for counts that are not the plan's or values that are no 64-bit words."""
    values = [[int(x) for x in v] for v in values]
    shared = [int(x) for x in shared]
    if [len(v) for v in values] != low.private_counts:
        raise ValueError(f"private words per segment: {low.private_counts}, not {[len(v) for v in values]}")
    if len(shared) != low.var_count:
        raise ValueError(f"shared words: {low.var_count}, not {len(shared)}")
    if any(not 0 <= x < 1 << 64 for v in values + [shared] for x in v):
        raise ValueError("private and shared words are 64-bit words")
    return np.concatenate([low.consts] + [np.array(v, dtype=np.uint64) for v in values + [shared]])


class Sha512SegmentsCircuit:
    """Proving key and GPU witness synthesis for a plan of wired SHA-512 / SHA-384 segments at 2^k rows.  A key fixes the
    plan: the segments, their block counts and variants, their wiring and what is public.

    `values` (synthesize, check, assert_satisfied, prove) is one sequence per segment: the segment's Private words in word
    order -- for a segment with an `init`, its Private initial words first; `shared` holds the plan's Var words by index.
    The instance is the public digest words in the order of `plan.public`, then the public initial states' words.  Private
    words are unconstrained, a private message's padding included, exactly as in Sha512Circuit; Const words and
    DigestWord wirings are constrained."""

    def __init__(self, ctx: Context, k: int, plan: Plan, table_bits: int = 12, setup: str = "toxic", seed: int = 0x5348413243515F):
        self.plan = plan
        SC._build_key(self, ctx, k, table_bits, setup, seed, lambda dense, spread: describe(k, plan, table_bits, dense, spread))
        self.rows = rows_for(plan)
        self._lowered = low = lower(plan)
        self._words = ctx.alloc(8 * max(low.words_len, 1))
        self._digests = ctx.alloc(64 * len(plan.segments))
        self.state_words = self.instances = self.init_words = self.instance_words = None

    # ---- witness ----
    def _inputs(self, values, shared):
        """What a front end's methods take -> (values, shared) of the plan."""
        return values, shared

    def _call(self, arr):
        """The entry point alone, on the word buffer as it is on the device."""
        ctx, low = self.ctx, self._lowered
        ctx._chk(ctx.lib.cq_sha512_synthesize_segments_dev(ctx.h, self.table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks),
                                                           low.seg_variant.ctypes.data, low.sources.ctypes.data,
                                                           low.init_sources.ctypes.data if has_init(self.plan) else None, self._words.ptr,
                                                           low.words_len, self.n, arr, self._digests.ptr))

    def synthesize(self, values, shared=()):
        """Uploads the word buffer, fills the advice columns on the GPU (cq_sha512_synthesize_segments_dev) and downloads
        the final states; returns (device columns, instances)."""
        values, shared = self._inputs(values, shared)
        words = word_buffer(self._lowered, values, shared)
        if len(words):
            self._words.upload(words)
        self._call((C.c_void_p * SC.ADVICE_COLUMNS)(*[c.ptr for c in self.cols]))
        self.state_words = [[int(x) for x in s] for s in self._digests.download((len(self.plan.segments), 8), np.uint64)]
        flat = [x for s in self.state_words for x in s]
        self.init_words = [[int(flat[s - SOURCE_DIGEST] if s & SOURCE_DIGEST else words[s]) for s in self._lowered.init_sources[8 * q: 8 * q + 8].tolist()]
                           for q in self.plan.public_init]
        self.instance_words = [x for s, count in self.plan.public for x in self.state_words[s][:count]] + [x for ws in self.init_words for x in ws]
        self.instances = [_words_to_mont(self.instance_words)]
        return self.cols, self.instances

    @property
    def digests(self):
        """The public digests of the last synthesis in instance order: 8 big-endian bytes per public word."""
        return [struct.pack(f">{count}Q", *self.state_words[s][:count]) for s, count in self.plan.public]

    def _result(self):
        return self.digests

    def check(self, values, shared=(), max_failures: int = 64):
        cols, inst = self.synthesize(values, shared)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, values, shared=()):
        cols, inst = self.synthesize(values, shared)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def prove(self, values, shared=(), seed: int = 1):
        """(proof bytes, public digests): create_proof with the instance words as the public inputs."""
        cols, inst = self.synthesize(values, shared)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self._result()

    def close(self):
        for o in (self._words, self._digests):
            o.close()
        SC._close_key(self)


class _FrontEnd(Sha512SegmentsCircuit):
    """A circuit whose methods take one item -- a message, a list of leaves -- in place of (values, shared)."""

    def _values(self, item):
        raise NotImplementedError

    def _inputs(self, item, shared=()):
        if shared:
            raise ValueError("the circuit takes its own input and no shared words")
        return self._values(item), ()


class Sha512dCircuit(_FrontEnd):
    """SHA-512(SHA-512(message)) for a message of exactly `blocks` padded blocks; the double digest is public, the inner one
    is not.  The methods take the message (bytes) and pad it here: that padding is private and not constrained; the second
    hash's input is wired to the first digest and its padding is pinned."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, double_sha512(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks), []]

    def _result(self):
        return self.digests[0]


class Sha512MerkleCircuit(_FrontEnd):
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


class Sha512MidstateCircuit(_FrontEnd):
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


class Sha512_256Circuit(_FrontEnd):
    """SHA-512/256 of a message of exactly `blocks` padded blocks (the plan `sha512_256`): the methods take the message and
    pad it here, as Sha512Circuit does.  The instance is the four words of the digest, 32 bytes."""

    def __init__(self, ctx: Context, k: int, blocks: int, **kw):
        super().__init__(ctx, k, sha512_256(blocks), **kw)

    def _values(self, message):
        return [SC.pad(message, self.plan.segments[0].blocks)]

    def _result(self):
        return self.digests[0]
