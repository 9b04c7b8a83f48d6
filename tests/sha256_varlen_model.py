"""Pure-Python model of the variable-length SHA-256 circuit (sha256_varlen.py): the padding, the compression of the padded
words block by block, every cell of the witness -- the compression circuit's from the words, the variable-length gates'
from the recurrences the gates state (not from the closed forms the kernel uses) -- and `findings`, which evaluates every
gate, lookup and copy of a description over a witness."""
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha256_circuit_model as M

M32 = 0xFFFFFFFF
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
VAR = SC.VAR


def pad_words(message: bytes, max_blocks: int):
    """(the 16 * max_blocks words a segment of max_blocks blocks holds for `message`, the index of its final block):
    message || 0x80 || zeros || the 64-bit bit length up to the end of the first block with room for them, zero words
    behind it."""
    length = len(message)
    assert length <= 64 * max_blocks - 9
    final = next(i for i in range(max_blocks) if 64 * i + 55 >= length)
    padded = message + b"\x80" + bytes(64 * final + 55 - length) + struct.pack(">Q", 8 * length)
    assert len(padded) == 64 * (final + 1)
    return list(struct.unpack(f">{16 * (final + 1)}I", padded)) + [0] * (16 * (max_blocks - final - 1)), final


def compress(words, blocks):
    """(per region (a, e, W, round or None, chained), the chaining values H_0 (the IV) .. H_blocks) of any 16 * blocks words."""
    h, chaining, regions = list(SC.IV256), [list(SC.IV256)], []
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


def regions_of(words, blocks):
    """Per region the dict of its 32-bit words by CQ_SHA256_SRC_* name, as sha256_circuit_model.region_words gives them for
    a padded message, for any 16 * blocks words; and the chaining values."""
    regions, chaining = compress(words, blocks)
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
    return out, chaining


def digest_of(message: bytes, max_blocks: int):
    """The 8 digest words: the chaining value behind the final block of the model's own padding."""
    words, final = pad_words(message, max_blocks)
    return compress(words, max_blocks)[1][final + 1]


def segment_cells(message: bytes, max_blocks: int, table_bits: int):
    """(18 columns over the segment's rows, its digest words): the compression circuit's cells of the padded words, then
    the variable-length cells by the gates' own recurrences."""
    words, final = pad_words(message, max_blocks)
    regions, chaining = regions_of(words, max_blocks)
    rows = SC.rows_for(max_blocks)
    cols = [[0] * rows for _ in range(SC.ADVICE_COLUMNS)]
    names = {v: k for k, v in SC.SRC.items()}
    for g, s in enumerate(regions):
        for c in SC.layout():
            off = c.offset + c.per_table_bits * table_bits
            field = (s[names[c.kind]] >> off) & ((1 << (c.len if c.len else table_bits)) - 1)
            row = g * SC.REGION_ROWS + c.row
            cols[c.column][row] = M.spread(field) if c.form == SC.FORM_SPREAD else field
            if c.form == SC.FORM_PAIR:
                cols[c.column + 1][row] = M.spread(field)
    y, length = cols[Y], len(message)
    ROW = {s: VAR["ROW_" + s] for s in ("M", "LEN", "C0", "C1", "IN", "FLAG", "VALUE", "OUT")}
    m, ln, selected, m13_before = 1, 0, [0] * 9, 1  # what the first block starts from
    for i in range(max_blocks):
        at = lambda region: SV.region_row(0, i, region)
        carry = at(VAR["REGION_CARRY"])
        if i:
            y[carry + ROW["VALUE"]], y[carry + ROW["OUT"]] = ln, m13_before
            ln = ln * m13_before
        y[carry + ROW["M"]], y[carry + ROW["LEN"]] = m, ln
        for t in range(16):
            base, g = at(4 + t), 16 * i + t
            m_now = 1 if 4 * (g + 1) <= length else 0
            if m - m_now:  # the boundary word
                r = length - 4 * g
                c0, c1 = (3 - r) & 1, (3 - r) >> 1
                data = words[g] >> (32 - 8 * r) if r else 0
                assert 0 <= r < 4 and words[g] == (1 << (8 * (c0 + 2 * c1))) * (256 * data + 128)
                ln += r
                y[base + ROW["C0"]], y[base + ROW["C1"]] = c0, c1
                cols[2 * VAR["SLOT_PRODUCT"]][base] = cols[2 * VAR["SLOT_PRODUCT"] + 1][base] = c0 * c1
                for r_, piece in ((0, data & 0xFFF), (1, data >> 12)):
                    cols[2 * VAR["SLOT_DATA"]][base + r_], cols[2 * VAR["SLOT_DATA"] + 1][base + r_] = piece, M.spread(piece)
            m, ln = m_now, ln + 4 * m_now
            y[base + ROW["M"]], y[base + ROW["LEN"]] = m, ln
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
    assert selected[8] == length and selected[:8] == chaining[final + 1]
    return cols, selected[:8]


def witness(messages, max_blocks_list, table_bits, n):
    """(18 advice columns of n integers, the digest words of every message)"""
    cols, digests, at = [[0] * n for _ in range(SC.ADVICE_COLUMNS)], [], 0
    for message, blocks in zip(messages, max_blocks_list):
        part, digest = segment_cells(message, blocks, table_bits)
        for col, p in zip(cols, part):
            col[at: at + len(p)] = p
        at += SC.rows_for(blocks)
        digests.append(digest)
    return cols, digests


def instance_words(messages, max_blocks_list, public_length=False):
    return [w for m, b in zip(messages, max_blocks_list) for w in digest_of(m, b)] + ([len(m) for m in messages] if public_length else [])


def word_row(max_blocks_list, message, word):
    """Row 0 of the region of word `word` (16 * block + t) of message `message`."""
    first = SS.first_regions(SS.batch(max_blocks_list))[message]
    return SV.region_row(first, word // 16, 4 + word % 16)


def findings(desc, advice, instance_words):
    """[(kind, index, row)] of every unsatisfied gate ("gate": a product whose first factor -- a selector or a sum of
    selectors -- is evaluated first), static lookup ("lookup") and copy ("copy"), as sha256_circuit_model.findings, over the
    fixed columns the description names."""
    cs, n = desc.cs, 1 << desc.k
    usable = n - (cs.blinding_factors() + 1)
    fixed = [[int(v) for v in desc.fixed[name]] for name in desc.fixed_names]
    inst = [list(instance_words)]
    out = []
    for gi, g in enumerate(cs.gates):
        assert g.op == "mul"
        out += [("gate", gi, r) for r in range(n)
                if M.evaluate(g.a, r, n, advice, fixed, inst) and M.evaluate(g.b, r, n, advice, fixed, inst)]
    N = 1 << desc.table_bits
    index = {"dense": {i: i for i in range(N)}, "spread": {M.spread(i): i for i in range(N)}}
    exprs = iter(cs._lookup_exprs)
    for li, lk in enumerate(cs.static_lookups):
        ins = [(next(exprs), t) for _, t in lk]
        for r in range(usable):
            rows = {index[t].get(M.evaluate(e, r, n, advice, fixed, inst)) for e, t in ins}
            if None in rows or len(rows) != 1:
                out.append(("lookup", li, r))
    val = lambda col, r: (advice, fixed, inst)[col.kind][col.index][r]
    out += [("copy", i, lr) for i, ((lc, lr), (rc, rr)) in enumerate(desc.copies) if val(lc, lr) != val(rc, rr)]
    return out
