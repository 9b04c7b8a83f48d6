"""Pure-Python model of SHA-256 segments that start from a given state (sha256_segments.Segment.init, the continued
sha256_varlen circuit): sha256_varlen_model's compression and cells restated with the initial state and the base length as
arguments -- that model has the IV and a base of zero fixed -- and a plan-level witness that resolves every source, the
initial words included, from the model's own chaining values.  hashlib is the reference the tests hold all of it to."""
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha256_circuit_model as M

M32 = 0xFFFFFFFF
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
VAR = SC.VAR


def compress(words, blocks, init=None):
    """(per region (a, e, W, round or None, chained), the chaining values H_0 (`init`, or the IV) .. H_blocks)."""
    h = list(SC.IV256 if init is None else init)
    chaining, regions = [list(h)], []
    for b in range(blocks):
        regions += [(h[3 - i], h[7 - i], 0, None, b > 0) for i in range(4)]
        w = list(words[16 * b: 16 * b + 16])
        for t in range(16, 64):
            s0 = M.rotr(w[t - 15], 7) ^ M.rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
            s1 = M.rotr(w[t - 2], 17) ^ M.rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M32)
        s = list(h)
        for t in range(64):
            a, e = s[0], s[4]
            t1 = s[7] + (M.rotr(e, 6) ^ M.rotr(e, 11) ^ M.rotr(e, 25)) + ((e & s[5]) ^ (~e & M32 & s[6])) + SC.K256[t] + w[t]
            t2 = (M.rotr(a, 2) ^ M.rotr(a, 13) ^ M.rotr(a, 22)) + ((a & s[1]) ^ (a & s[2]) ^ (s[1] & s[2]))
            s = [(t1 + t2) & M32] + s[:3] + [(s[3] + t1) & M32] + s[4:7]
            regions.append((s[0], s[4], w[t], t, False))
        h = [(x + y) & M32 for x, y in zip(h, s)]
        chaining.append(list(h))
    regions += [(h[3 - i], h[7 - i], 0, None, True) for i in range(4)]
    return regions, chaining


def state_after(data: bytes, init=None):
    """The chaining value behind the whole 64-byte blocks of `data`."""
    assert len(data) % 64 == 0
    return compress(struct.unpack(f">{len(data) // 4}I", data), len(data) // 64, init)[1][-1]


def cells_of(words, blocks, table_bits, init=None):
    """(18 columns over the segment's rows, the chaining values): the compression circuit's cells for any 16 * blocks words."""
    regions, chaining = compress(words, blocks, init)
    out = []
    for g, (a, e, w_, t, chained) in enumerate(regions):
        s = {name: 0 for name in SC.SRC}
        s["A"], s["E"], s["W"] = a, e, w_
        s["S0_EVEN"], s["S0_ODD"] = M.bitsum(M.rotr(a, 2), M.rotr(a, 13), M.rotr(a, 22))
        s["S1_EVEN"], s["S1_ODD"] = M.bitsum(M.rotr(e, 6), M.rotr(e, 11), M.rotr(e, 25))
        s["G0_EVEN"], s["G0_ODD"] = M.bitsum(M.rotr(w_, 7), M.rotr(w_, 18), w_ >> 3)
        s["G1_EVEN"], s["G1_ODD"] = M.bitsum(M.rotr(w_, 17), M.rotr(w_, 19), w_ >> 10)
        if g % SC.BLOCK_REGIONS >= 2:
            (a1, e1), (a2, e2) = regions[g - 1][:2], regions[g - 2][:2]
            s["MAJ_EVEN"], s["MAJ_ODD"] = M.bitsum(a, a1, a2)
            s["CHP_EVEN"], s["CHP_ODD"] = M.bitsum(e, e1)
            s["CHQ_EVEN"], s["CHQ_ODD"] = M.bitsum(~e & M32, e2)
            s["CH"] = s["CHP_ODD"] + s["CHQ_ODD"]
        if t is not None:
            prev = out[g - 1]
            t1 = regions[g - 4][1] + prev["S1_EVEN"] + prev["CH"] + SC.K256[t] + w_
            s["K"] = SC.K256[t]
            s["CARRY_E"] = (t1 + regions[g - 4][0]) >> 32
            s["CARRY_A"] = (t1 + prev["S0_EVEN"] + prev["MAJ_ODD"]) >> 32
            if t >= 16:
                s["CARRY_W"] = (out[g - 2]["G1_EVEN"] + regions[g - 7][2] + out[g - 15]["G0_EVEN"] + regions[g - 16][2]) >> 32
        if chained:
            s["CARRY_A"] = (regions[g - SC.BLOCK_REGIONS][0] + regions[g - 4][0]) >> 32
            s["CARRY_E"] = (regions[g - SC.BLOCK_REGIONS][1] + regions[g - 4][1]) >> 32
        out.append(s)
    cols = [[0] * SC.rows_for(blocks) for _ in range(SC.ADVICE_COLUMNS)]
    names = {v: k for k, v in SC.SRC.items()}
    for g, s in enumerate(out):
        for c in SC.layout():
            off = c.offset + c.per_table_bits * table_bits
            field = (s[names[c.kind]] >> off) & ((1 << (c.len if c.len else table_bits)) - 1)
            row = g * SC.REGION_ROWS + c.row
            cols[c.column][row] = M.spread(field) if c.form == SC.FORM_SPREAD else field
            if c.form == SC.FORM_PAIR:
                cols[c.column + 1][row] = M.spread(field)
    return cols, chaining


def state_row(first_region: int, word: int) -> int:
    """The row of initial word `word` in column X: region 3 - word % 4 of the first block, the A row or the E row."""
    row = next(c.row for c in SC.layout() if c.kind == SC.SRC["A" if word < 4 else "E"] and c.form == SC.FORM_WORD)
    return SC.REGION_ROWS * (first_region + 3 - word % 4) + row


def plan_witness(plan, values, shared, bits, table_bits, n):
    """(18 advice columns of n integers, every segment's 8 digest words, every segment's 8 initial words) of a plan whose
    segments may have an `init`: Private words come from `values` (a segment's initial ones first), everything else is
    resolved from `shared`, `bits` and the model's own digests; a Choice's three cells go to column Y."""
    cols, digests, inits = [[0] * n for _ in range(SC.ADVICE_COLUMNS)], [], []

    def plain(o):
        return int(shared[o.index]) if isinstance(o, SS.Var) else digests[o.segment][o.word]

    for seg, first, private in zip(plan.segments, SS.first_regions(plan), values):
        private, words, choices = iter(private), [], []

        def resolve(src, t=None):
            if isinstance(src, SS.Private):
                return int(next(private))
            if isinstance(src, SS.Const):
                return src.value
            if isinstance(src, SS.Choice):
                zero, one, bit = plain(src.zero), plain(src.one), int(bits[src.bit])
                choices.append((t, zero, one, bit))
                return one if bit else zero
            return plain(src)

        init = None if seg.init is None else [resolve(s) for s in seg.init]
        words = [resolve(s, t) for t, s in enumerate(seg.sources)]
        assert next(private, None) is None
        part, chaining = cells_of(words, seg.blocks, table_bits, init)
        at = SC.REGION_ROWS * first
        for col, p in zip(cols, part):
            col[at: at + len(p)] = p
        for t, zero, one, bit in choices:
            base = SC.REGION_ROWS * (first + SC.BLOCK_REGIONS * (t // 16) + 4 + t % 16)
            cols[Y][base + SC.CHOICE_ROW_ZERO], cols[Y][base + SC.CHOICE_ROW_ONE], cols[Y][base + SC.CHOICE_ROW_BIT] = zero, one, bit
        digests.append(chaining[-1])
        inits.append(chaining[0])
    return cols, digests, inits


def varlen_cells(message: bytes, max_blocks: int, table_bits: int, init=None, base: int = 0):
    """sha256_varlen_model.segment_cells from the state `init` after `base` bytes: the padding's length word and every
    length cell count from the base, by the gates' own recurrences.  (18 columns over the segment's rows, the digest words)."""
    length = len(message)
    assert length <= 64 * max_blocks - 9 and base % 64 == 0
    final = next(i for i in range(max_blocks) if 64 * i + 55 >= length)
    padded = message + b"\x80" + bytes(64 * final + 55 - length) + struct.pack(">Q", 8 * (base + length))
    words = list(struct.unpack(f">{16 * (final + 1)}I", padded)) + [0] * (16 * (max_blocks - final - 1))
    cols, chaining = cells_of(words, max_blocks, table_bits, init)
    y = cols[Y]
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


def varlen_witness(messages, max_blocks_list, table_bits, n, inits, bases):
    """(18 advice columns of n integers, the digest words of every message)"""
    cols, digests, at = [[0] * n for _ in range(SC.ADVICE_COLUMNS)], [], 0
    for message, blocks, init, base in zip(messages, max_blocks_list, inits, bases):
        part, digest = varlen_cells(message, blocks, table_bits, init, base)
        for col, p in zip(cols, part):
            col[at: at + len(p)] = p
        at += SC.rows_for(blocks)
        digests.append(digest)
    return cols, digests
