"""Pure-Python model of plans with choice-wired message words (sha256_segments.Var / Choice): the plan is resolved, segment
by segment, into one whose chosen and shared words are plain private words -- every digest an operand reads comes from
hashlib over the earlier segment's message -- and the witness is sha256_segments_model's for that plan plus the three cells
of every choice in column Y."""
import hashlib
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_circuit_model as M
from tests import sha256_segments_model as SM

findings = M.findings  # over the fixed columns the description itself names (`fixed_names`)


def resolve(plan, values, shared, bits):
    """(plain plan, plain values, choices): the plan with every Var and Choice word replaced by a Private word, what
    sha256_segments_model takes for it, and per Choice word (segment, word, zero operand, one operand, bit) as integers."""
    assert all(b in (0, 1) for b in bits)
    done, segs, plain_values, choices = [], [], [], []  # done: the unpadded message of every earlier segment

    def operand(o):
        if isinstance(o, SS.Var):
            return int(shared[o.index])
        d = hashlib.sha256(done[o.segment]).digest()
        return int.from_bytes(d[4 * o.word: 4 * o.word + 4], "big")

    for j, (seg, private) in enumerate(zip(plan.segments, values)):
        private, sources, words, free = iter(private), [], [], []
        for t, src in enumerate(seg.sources):
            if isinstance(src, (SS.Const, SS.DigestWord)):
                sources.append(src)
                words.append(src.value if isinstance(src, SS.Const) else operand(src))
                continue
            if isinstance(src, SS.Private):
                word = int(next(private))
            elif isinstance(src, SS.Var):
                word = operand(src)
            else:
                zero, one, bit = operand(src.zero), operand(src.one), int(bits[src.bit])
                choices.append((j, t, zero, one, bit))
                word = one if bit else zero
            sources.append(SS.PRIVATE)
            words.append(word)
            free.append(word)
        assert next(private, None) is None
        raw = struct.pack(f">{len(words)}I", *words)
        length = int.from_bytes(raw[-8:], "big")
        assert length % 8 == 0 and SC.pad(raw[: length // 8], seg.blocks) == words, "the segment's words are not a padded message"
        done.append(raw[: length // 8])
        segs.append(SS.Segment(seg.blocks, tuple(sources)))
        plain_values.append(free)
    return SS.Plan(tuple(segs), plan.public), plain_values, choices


def digests(plan, values, shared=(), bits=()):
    """The 8 digest words of every segment, from hashlib."""
    plain, plain_values, _ = resolve(plan, values, shared, bits)
    return SM.digests(plain, plain_values)


def instance_words(plan, values, shared=(), bits=()):
    ds = digests(plan, values, shared, bits)
    return [w for p in plan.public for w in ds[p]]


def choice_cells(plan, segment, word):
    """Rows of the zero operand, the one operand and the bit of the Choice at (segment, word) in column Y, and the first
    row of their region."""
    _, base = SM.w_cell(plan, segment, word)
    return base + SC.CHOICE_ROW_ZERO, base + SC.CHOICE_ROW_ONE, base + SC.CHOICE_ROW_BIT, base


def witness(plan, values, shared, bits, table_bits, n):
    """18 advice columns of n integers: the resolved plan's witness, and the cells of every choice."""
    plain, plain_values, choices = resolve(plan, values, shared, bits)
    cols = SM.witness(plain, plain_values, table_bits, n)
    y = cols[2 * SC.PAIRS + 1]
    for segment, word, zero, one, bit in choices:
        r0, r1, rb, _ = choice_cells(plan, segment, word)
        assert y[r0] == y[r1] == y[rb] == 0, "the layout uses a choice cell"
        y[r0], y[r1], y[rb] = zero, one, bit
    return cols


def path_inputs(depth, items, leaf_blocks=None):
    """(values, shared, bits) of merkle_path(depth, len(items), leaf_blocks) for per-path (leaf, index, siblings), packed
    here independently of the front end: per path the leaf's words (or the padded leaf message as its segment's private
    words), then per level the sibling's words and the index's bit."""
    values, shared, bits = [], [], []
    for leaf, index, siblings in items:
        if leaf_blocks is None:
            shared += struct.unpack(">8I", leaf)
        else:
            values.append(SC.pad(leaf, leaf_blocks))
        values += [[] for _ in range(depth)]
        for level, sibling in enumerate(siblings):
            shared += struct.unpack(">8I", sibling)
            bits.append(index >> level & 1)
    return values, shared, bits


def path_root(leaf, index, siblings):
    """The root a path leads to, from hashlib."""
    node = leaf
    for level, sibling in enumerate(siblings):
        node = hashlib.sha256(sibling + node if index >> level & 1 else node + sibling).digest()
    return node
