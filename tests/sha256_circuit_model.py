"""Pure-Python model of the SHA-256 compression circuit: integer cells from FIPS 180-4 computed here (no library call
but the layout table, which says where a bit field goes, not what it holds), and an evaluator of the constraint
system's gates, static lookups and copy constraints over Python integers."""
import struct

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha256_circuit as SC

P = GP.FR_MODULUS
M32 = 0xFFFFFFFF


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def spread(x):
    return sum(((x >> i) & 1) << (2 * i) for i in range(32))


def bitsum(*ws):
    """(even, odd) words of the bitwise sum of up to three words: even = parity, odd = carry of every bit position"""
    ev = od = 0
    for i in range(32):
        s = sum((w >> i) & 1 for w in ws)
        assert s <= 3
        ev |= (s & 1) << i
        od |= (s >> 1) << i
    return ev, od


def region_words(message: bytes, blocks: int):
    """Per region the dict of its 32-bit words by CQ_SHA256_SRC_* name, and the digest words."""
    msg = SC.pad(message, blocks)
    h = list(SC.IV256)
    regions = []  # (a, e, w, round or None, chained)
    for b in range(blocks):
        regions += [(h[3 - i], h[7 - i], 0, None, b > 0) for i in range(4)]
        w = msg[16 * b: 16 * b + 16]
        for t in range(16, 64):
            s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
            s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M32)
        a, bb, c, d, e, f, g, hh = h
        for t in range(64):
            t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & M32 & g)) + SC.K256[t] + w[t]
            t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c))
            hh, g, f, e, d, c, bb, a = g, f, e, (d + t1) & M32, c, bb, a, (t1 + t2) & M32
            regions.append((a, e, w[t], t, False))
        h = [(x + y) & M32 for x, y in zip(h, (a, bb, c, d, e, f, g, hh))]
    regions += [(h[3 - i], h[7 - i], 0, None, True) for i in range(4)]
    out = []
    for g_, (a, e, w_, t, chained) in enumerate(regions):
        s = {name: 0 for name in SC.SRC}
        s["A"], s["E"], s["W"] = a, e, w_
        s["S0_EVEN"], s["S0_ODD"] = bitsum(rotr(a, 2), rotr(a, 13), rotr(a, 22))
        s["S1_EVEN"], s["S1_ODD"] = bitsum(rotr(e, 6), rotr(e, 11), rotr(e, 25))
        s["G0_EVEN"], s["G0_ODD"] = bitsum(rotr(w_, 7), rotr(w_, 18), w_ >> 3)
        s["G1_EVEN"], s["G1_ODD"] = bitsum(rotr(w_, 17), rotr(w_, 19), w_ >> 10)
        if g_ % SC.BLOCK_REGIONS >= 2:  # Maj and Ch of this region's state words and the two before
            (a1, e1), (a2, e2) = regions[g_ - 1][:2], regions[g_ - 2][:2]
            s["MAJ_EVEN"], s["MAJ_ODD"] = bitsum(a, a1, a2)
            s["CHP_EVEN"], s["CHP_ODD"] = bitsum(e, e1)
            s["CHQ_EVEN"], s["CHQ_ODD"] = bitsum(~e & M32, e2)
            s["CH"] = s["CHP_ODD"] + s["CHQ_ODD"]
        if t is not None:
            prev = out[g_ - 1]
            t1 = regions[g_ - 4][1] + prev["S1_EVEN"] + prev["CH"] + SC.K256[t] + w_
            s["K"] = SC.K256[t]
            s["CARRY_E"], low = divmod(t1 + regions[g_ - 4][0], 1 << 32)
            assert low == e
            s["CARRY_A"], low = divmod(t1 + prev["S0_EVEN"] + prev["MAJ_ODD"], 1 << 32)
            assert low == a
            if t >= 16:
                s["CARRY_W"], low = divmod(out[g_ - 2]["G1_EVEN"] + regions[g_ - 7][2] + out[g_ - 15]["G0_EVEN"] + regions[g_ - 16][2], 1 << 32)
                assert low == w_
        if chained:
            s["CARRY_A"] = (regions[g_ - SC.BLOCK_REGIONS][0] + regions[g_ - 4][0]) >> 32
            s["CARRY_E"] = (regions[g_ - SC.BLOCK_REGIONS][1] + regions[g_ - 4][1]) >> 32
        out.append(s)
    return out, h


def witness(message: bytes, blocks: int, table_bits: int, n: int):
    """(18 advice columns of n integers, the 8 instance words)"""
    words, digest = region_words(message, blocks)
    names = {v: k for k, v in SC.SRC.items()}
    cols = [[0] * n for _ in range(SC.ADVICE_COLUMNS)]
    cells = SC.layout()
    for g, s in enumerate(words):
        for c in cells:
            off = c.offset + c.per_table_bits * table_bits
            ln = c.len if c.len else table_bits
            field = (s[names[c.kind]] >> off) & ((1 << ln) - 1)
            row = g * SC.REGION_ROWS + c.row
            cols[c.column][row] = spread(field) if c.form == SC.FORM_SPREAD else field
            if c.form == SC.FORM_PAIR:
                cols[c.column + 1][row] = spread(field)
    return cols, digest


def evaluate(e, row, n, advice, fixed, instance):
    if e.op == "const":
        return e.a
    if e.op == "query":
        src = (advice, fixed, instance)[e.a.kind][e.a.index]
        r = (row + e.b) % n
        return src[r] if r < len(src) else 0
    if e.op == "neg":
        return -evaluate(e.a, row, n, advice, fixed, instance) % P
    if e.op == "scale":
        return evaluate(e.a, row, n, advice, fixed, instance) * e.b % P
    x, y = evaluate(e.a, row, n, advice, fixed, instance), evaluate(e.b, row, n, advice, fixed, instance)
    return (x + y) % P if e.op == "add" else x * y % P


def findings(desc, advice, instance_words):
    """[(kind, index, row)] of every unsatisfied gate ("gate"), static lookup ("lookup") and copy ("copy") on the usable
    rows.  Tables: dense = [0, 2^tb), spread = its bit-spread form; a lookup's inputs must sit on one table row."""
    cs, n = desc.cs, 1 << desc.k
    usable = n - (cs.blinding_factors() + 1)
    fixed = [[int(v) for v in desc.fixed[name]] for name in SC.FIXED]
    inst = [list(instance_words)]
    out = []
    for gi, g in enumerate(cs.gates):
        assert g.op == "mul" and g.a.op == "query" and g.a.a.kind == GP.COL_FIXED  # selector * (...)
        selector = fixed[g.a.a.index]
        out += [("gate", gi, r) for r in range(n) if selector[r] and evaluate(g.b, r, n, advice, fixed, inst)]
    N = 1 << desc.table_bits
    index = {"dense": {i: i for i in range(N)}, "spread": {spread(i): i for i in range(N)}}
    exprs = iter(cs._lookup_exprs)
    for li, lk in enumerate(cs.static_lookups):
        ins = [(next(exprs), t) for _, t in lk]
        for r in range(usable):
            rows = {index[t].get(evaluate(e, r, n, advice, fixed, inst)) for e, t in ins}
            if None in rows or len(rows) != 1:
                out.append(("lookup", li, r))
    val = lambda col, r: (advice, fixed, inst)[col.kind][col.index][r]
    out += [("copy", i, lr) for i, ((lc, lr), (rc, rr)) in enumerate(desc.copies) if val(lc, lr) != val(rc, rr)]
    return out


def digest_bytes(words):
    return struct.pack(">8I", *words)
