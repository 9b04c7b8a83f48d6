"""Pure-Python model of the variable-length SHA-256 circuit (sha256_varlen.py), also continued from a state after `base`
bytes: the padding, every cell of the witness -- the compression circuit's from tests/sha2_model.py for the padded words,
the variable-length gates' from the recurrences the gates state (not from the closed forms the kernel uses) -- and
`findings`, which evaluates every gate, lookup and copy of a description over a witness."""
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha2_model as M2
from tests import sha256_circuit_model as M

W = M.W
M32 = M.M32
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
VAR = SC.VAR
findings = M.findings  # a gate's first factor may be a sum of selectors here


def pad_words(message: bytes, max_blocks: int, base: int = 0):
    """(the 16 * max_blocks words a segment of max_blocks blocks holds for `message`, the index of its final block):
    message || 0x80 || zeros || the 64-bit bit length, counted from `base` bytes before the message, up to the end of the
    first block with room for them, zero words behind it."""
    length = len(message)
    assert length <= 64 * max_blocks - 9 and base % 64 == 0
    final = next(i for i in range(max_blocks) if 64 * i + 55 >= length)
    padded = message + b"\x80" + bytes(64 * final + 55 - length) + struct.pack(">Q", 8 * (base + length))
    assert len(padded) == 64 * (final + 1)
    return M2.words_of(padded) + [0] * (16 * (max_blocks - final - 1)), final


def digest_of(message: bytes, max_blocks: int):
    """The 8 digest words: the chaining value behind the final block of the model's own padding."""
    words, final = pad_words(message, max_blocks)
    return M2.compress(W, words, max_blocks, M.IV)[1][final + 1]


def segment_cells(message: bytes, max_blocks: int, table_bits: int, init=None, base: int = 0):
    """(18 columns over the segment's rows, its digest words): the compression circuit's cells of the padded words from
    the state `init` (by default the IV) after `base` bytes, then the variable-length cells by the gates' own recurrences:
    the padding's length word and every length cell count from the base."""
    words, final = pad_words(message, max_blocks, base)
    cols, chaining = M2.cells_of(W, words, max_blocks, table_bits, M.IV if init is None else init)
    y, length = cols[Y], len(message)
    ROW = {s: VAR["ROW_" + s] for s in ("M", "LEN", "C0", "C1", "IN", "FLAG", "VALUE", "OUT")}
    m, ln, selected, m13_before = 1, base, [0] * 9, 1  # what the first block starts from
    for i in range(max_blocks):
        at = lambda region: SV.region_row(0, i, region)
        carry = at(VAR["REGION_CARRY"])
        if i:
            y[carry + ROW["VALUE"]], y[carry + ROW["OUT"]] = ln, m13_before
            ln = ln * m13_before
        y[carry + ROW["M"]], y[carry + ROW["LEN"]] = m, ln
        for t in range(16):
            row, g = at(4 + t), 16 * i + t
            m_now = 1 if 4 * (g + 1) <= length else 0
            if m - m_now:  # the boundary word
                r = length - 4 * g
                c0, c1 = (3 - r) & 1, (3 - r) >> 1
                data = words[g] >> (32 - 8 * r) if r else 0
                assert 0 <= r < 4 and words[g] == (1 << (8 * (c0 + 2 * c1))) * (256 * data + 128)
                ln += r
                y[row + ROW["C0"]], y[row + ROW["C1"]] = c0, c1
                cols[2 * VAR["SLOT_PRODUCT"]][row] = cols[2 * VAR["SLOT_PRODUCT"] + 1][row] = c0 * c1
                for r_, piece in ((0, data & 0xFFF), (1, data >> 12)):
                    cols[2 * VAR["SLOT_DATA"]][row + r_], cols[2 * VAR["SLOT_DATA"] + 1][row + r_] = piece, M.spread(piece)
            m, ln = m_now, ln + 4 * m_now
            y[row + ROW["M"]], y[row + ROW["LEN"]] = m, ln
            if t == 13:
                m13 = m
        final_region = at(VAR["REGION_FINAL"])
        fin = m13_before - m13
        y[final_region + ROW["IN"]], y[final_region + ROW["FLAG"]], y[final_region + ROW["VALUE"]] = m13_before, m13, fin
        assert fin == (1 if i == final else 0)
        for w in range(9):
            s = at(VAR["REGION_SUM"] + w if w < 8 else VAR["REGION_LENGTH"])
            value = chaining[i + 1][w] if w < 8 else ln
            y[s + ROW["IN"]], y[s + ROW["FLAG"]], y[s + ROW["VALUE"]] = selected[w], fin, value
            selected[w] += fin * value
            y[s + ROW["OUT"]] = selected[w]
        m13_before = m13
    assert selected[8] == base + length and selected[:8] == chaining[final + 1]
    return cols, selected[:8]


def witness(messages, max_blocks_list, table_bits, n, inits=None, bases=None):
    """(18 advice columns of n integers, the digest words of every message); `inits` and `bases`: per message the state it
    continues from and the bytes before it, by default the IV and none."""
    cols, digests, count = M2.columns(W, n), [], len(max_blocks_list)
    firsts = SS.first_regions(SS.batch(max_blocks_list))
    for message, blocks, first, init, base in zip(messages, max_blocks_list, firsts, inits or [None] * count, bases or [0] * count):
        part, digest = segment_cells(message, blocks, table_bits, init, base)
        M2.put(W, cols, first, part)
        digests.append(digest)
    return cols, digests


def instance_words(messages, max_blocks_list, public_length=False):
    return [w for m, b in zip(messages, max_blocks_list) for w in digest_of(m, b)] + ([len(m) for m in messages] if public_length else [])


def word_row(max_blocks_list, message, word):
    """Row 0 of the region of word `word` (16 * block + t) of message `message`."""
    first = SS.first_regions(SS.batch(max_blocks_list))[message]
    return SV.region_row(first, word // 16, 4 + word % 16)
