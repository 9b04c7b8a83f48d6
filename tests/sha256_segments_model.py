"""Pure-Python model of a plan of wired SHA-256 segments: every segment's expected witness is the single-message model's
(sha256_circuit_model.witness) for that segment's message, shifted to the segment's first row; a wired segment's message
and every expected digest come from hashlib alone, never from the model's own compression."""
import hashlib
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_circuit_model as M


def messages(plan, values):
    """The unpadded message (bytes) of every segment.  `values` is what Sha256SegmentsCircuit.synthesize takes: per segment
    its Private words in word order.  Digest words come from hashlib over the earlier segment's message; the words must
    be a padded message, whose length field says where the message ends."""
    out = []
    for seg, private in zip(plan.segments, values):
        private = iter(private)
        words = []
        for src in seg.sources:
            if isinstance(src, SS.Private):
                words.append(int(next(private)))
            elif isinstance(src, SS.Const):
                words.append(src.value)
            else:
                d = hashlib.sha256(out[src.segment]).digest()
                words.append(int.from_bytes(d[4 * src.word: 4 * src.word + 4], "big"))
        assert next(private, None) is None
        raw = struct.pack(f">{len(words)}I", *words)
        bits = int.from_bytes(raw[-8:], "big")
        assert bits % 8 == 0 and SC.pad(raw[: bits // 8], seg.blocks) == words, "the segment's words are not a padded message"
        out.append(raw[: bits // 8])
    return out


def digests(plan, values):
    """The 8 digest words of every segment, from hashlib."""
    return [list(struct.unpack(">8I", hashlib.sha256(m).digest())) for m in messages(plan, values)]


def instance_words(plan, values):
    ds = digests(plan, values)
    return [w for p in plan.public for w in ds[p]]


def witness(plan, values, table_bits, n):
    """18 advice columns of n integers: per segment the single-message model's witness at the segment's first row."""
    cols = [[0] * n for _ in range(SC.ADVICE_COLUMNS)]
    for seg, first, msg in zip(plan.segments, SS.first_regions(plan), messages(plan, values)):
        rows = SC.rows_for(seg.blocks)
        part, digest = M.witness(msg, seg.blocks, table_bits, rows)
        assert M.digest_bytes(digest) == hashlib.sha256(msg).digest()
        for col, p in zip(cols, part):
            col[SC.REGION_ROWS * first: SC.REGION_ROWS * first + rows] = p
    return cols


def w_cell(plan, segment, word):
    """Row of message word `word` (0 .. 16 * blocks - 1) of `segment` in the word column X, and the first row of its region."""
    base = SC.REGION_ROWS * (SS.first_regions(plan)[segment] + SC.BLOCK_REGIONS * (word // 16) + 4 + word % 16)
    wrow = next(c.row for c in SC.layout() if c.kind == SC.SRC["W"] and c.form == SC.FORM_WORD)
    return base + wrow, base


def gates_reading_w(base, t):
    """(gate name, anchor row) of every gate that reads the word-column copy of W_t of the round region at `base`: the
    word's recomposition and the two additions of its own round, and the schedule additions of rounds t + 16 and t + 7."""
    out = [("w_word", base), ("e_add", base), ("a_add", base)]
    out += [("w_add", base + SC.REGION_ROWS * d) for d in (7, 16) if 16 <= t + d < 64]
    return {("gate", SC.GATES.index(name), row) for name, row in out}
