"""Pure-Python model of the SHA-512 / SHA-384 compression circuit: integer cells from FIPS 180-4 computed here (no library
call but the layout table, which says where a bit field goes, not what it holds; the round constants and initial hash
values come from the primes' roots, not from the package), and an evaluator of the constraint system's gates, static
lookups and copy constraints over Python integers."""
import struct
from math import isqrt

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha512_circuit as SC

P = GP.FR_MODULUS
M64 = (1 << 64) - 1


def _primes(count):
    out, x = [], 2
    while len(out) < count:
        if all(x % p for p in out):
            out.append(x)
        x += 1
    return out


def _icbrt(x):
    lo, hi = 0, 1 << (x.bit_length() // 3 + 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** 3 <= x else (lo, mid)
    return lo


# FIPS 180-4, 4.2.3 and 5.3.4 / 5.3.5: the first 64 bits of the fractional parts of the cube roots of the first 80 primes,
# of the square roots of the first 8 primes (SHA-512) and of the 9th to the 16th (SHA-384)
K = [_icbrt(p << 192) & M64 for p in _primes(80)]
IV = {SC.VARIANT_512: [isqrt(p << 128) & M64 for p in _primes(8)], SC.VARIANT_384: [isqrt(p << 128) & M64 for p in _primes(16)[8:]]}


def rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


_SPREAD8 = [sum(((b >> i) & 1) << (2 * i) for i in range(8)) for b in range(256)]
_DIGITS8 = {}  # a byte of base-4 digits (0 .. 3 each, four of them) -> (their low bits, their high bits)
for _b in range(256):
    _DIGITS8[_b] = (sum(((_b >> (2 * i)) & 1) << i for i in range(4)), sum(((_b >> (2 * i + 1)) & 1) << i for i in range(4)))


def spread(x):
    """bit i -> bit 2i, a byte at a time"""
    out = shift = 0
    while x:
        out |= _SPREAD8[x & 0xFF] << shift
        x >>= 8
        shift += 16
    return out


def bitsum(*ws):
    """(even, odd) words of the bitwise sum of up to three words: even = parity, odd = carry of every bit position --
    the low and the high bit of every base-4 digit of the sum of the words' spread forms (no digit exceeds 3)"""
    assert len(ws) <= 3
    s = sum(spread(w) for w in ws)
    ev = od = shift = 0
    while s:
        lo, hi = _DIGITS8[s & 0xFF]
        ev |= lo << shift
        od |= hi << shift
        s >>= 8
        shift += 4
    return ev, od


def region_words(message: bytes, blocks: int, variant: int = SC.VARIANT_512):
    """Per region of one message the dict of its 64-bit words by CQ_SHA256_SRC_* name, and the eight words of the final
    state."""
    msg = SC.pad(message, blocks)
    h = list(IV[variant])
    regions = []  # (a, e, w, round or None, chained)
    for b in range(blocks):
        regions += [(h[3 - i], h[7 - i], 0, None, b > 0) for i in range(4)]
        w = msg[16 * b: 16 * b + 16]
        for t in range(16, 80):
            s0 = rotr(w[t - 15], 1) ^ rotr(w[t - 15], 8) ^ (w[t - 15] >> 7)
            s1 = rotr(w[t - 2], 19) ^ rotr(w[t - 2], 61) ^ (w[t - 2] >> 6)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M64)
        a, bb, c, d, e, f, g, hh = h
        for t in range(80):
            t1 = hh + (rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)) + ((e & f) ^ (~e & M64 & g)) + K[t] + w[t]
            t2 = (rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)) + ((a & bb) ^ (a & c) ^ (bb & c))
            hh, g, f, e, d, c, bb, a = g, f, e, (d + t1) & M64, c, bb, a, (t1 + t2) & M64
            regions.append((a, e, w[t], t, False))
        h = [(x + y) & M64 for x, y in zip(h, (a, bb, c, d, e, f, g, hh))]
    regions += [(h[3 - i], h[7 - i], 0, None, True) for i in range(4)]
    out = []
    for g_, (a, e, w_, t, chained) in enumerate(regions):
        s = {name: 0 for name in SC.SRC}
        s["A"], s["E"], s["W"] = a, e, w_
        s["S0_EVEN"], s["S0_ODD"] = bitsum(rotr(a, 28), rotr(a, 34), rotr(a, 39))
        s["S1_EVEN"], s["S1_ODD"] = bitsum(rotr(e, 14), rotr(e, 18), rotr(e, 41))
        s["G0_EVEN"], s["G0_ODD"] = bitsum(rotr(w_, 1), rotr(w_, 8), w_ >> 7)
        s["G1_EVEN"], s["G1_ODD"] = bitsum(rotr(w_, 19), rotr(w_, 61), w_ >> 6)
        if g_ % SC.BLOCK_REGIONS >= 2:  # Maj and Ch of this region's state words and the two before
            (a1, e1), (a2, e2) = regions[g_ - 1][:2], regions[g_ - 2][:2]
            s["MAJ_EVEN"], s["MAJ_ODD"] = bitsum(a, a1, a2)
            s["CHP_EVEN"], s["CHP_ODD"] = bitsum(e, e1)
            s["CHQ_EVEN"], s["CHQ_ODD"] = bitsum(~e & M64, e2)
            s["CH"] = s["CHP_ODD"] + s["CHQ_ODD"]
        if t is not None:
            prev = out[g_ - 1]
            t1 = regions[g_ - 4][1] + prev["S1_EVEN"] + prev["CH"] + K[t] + w_
            s["K"] = K[t]
            s["CARRY_E"], low = divmod(t1 + regions[g_ - 4][0], 1 << 64)
            assert low == e
            s["CARRY_A"], low = divmod(t1 + prev["S0_EVEN"] + prev["MAJ_ODD"], 1 << 64)
            assert low == a
            if t >= 16:
                s["CARRY_W"], low = divmod(out[g_ - 2]["G1_EVEN"] + regions[g_ - 7][2] + out[g_ - 15]["G0_EVEN"] + regions[g_ - 16][2], 1 << 64)
                assert low == w_
        if chained:
            s["CARRY_A"] = (regions[g_ - SC.BLOCK_REGIONS][0] + regions[g_ - 4][0]) >> 64
            s["CARRY_E"] = (regions[g_ - SC.BLOCK_REGIONS][1] + regions[g_ - 4][1]) >> 64
        out.append(s)
    return out, h


def witness(messages, blocks_list, variants, table_bits: int, n: int):
    """(18 advice columns of n integers, the instance words, the final state of every message): the messages' regions one
    behind another, zero behind the last."""
    names = {v: k for k, v in SC.SRC.items()}
    cols = [[0] * n for _ in range(SC.ADVICE_COLUMNS)]
    cells = SC.layout()
    instance, states, first = [], [], 0
    for message, blocks, variant in zip(messages, blocks_list, variants):
        words, state = region_words(message, blocks, variant)
        for g, s in enumerate(words):
            for c in cells:
                off = c.offset + c.per_table_bits * table_bits
                ln = c.len if c.len else table_bits
                field = (s[names[c.kind]] >> off) & ((1 << ln) - 1)
                row = (first + g) * SC.REGION_ROWS + c.row
                cols[c.column][row] = spread(field) if c.form == SC.FORM_SPREAD else field
                if c.form == SC.FORM_PAIR:
                    cols[c.column + 1][row] = spread(field)
        first += len(words)
        states.append(state)
        instance += state[:SC.DIGEST_WORDS[variant]]
    return cols, instance, states


def witness_one(message: bytes, blocks: int, table_bits: int, n: int, variant: int = SC.VARIANT_512):
    """(18 advice columns of n integers, the instance words) of a one-message circuit"""
    cols, instance, _ = witness([message], [blocks], [variant], table_bits, n)
    return cols, instance


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


def digest_bytes(state, variant: int = SC.VARIANT_512):
    count = SC.DIGEST_WORDS[variant]
    return struct.pack(f">{count}Q", *state[:count])
