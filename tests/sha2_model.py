"""Pure-Python model of the SHA-2 compression circuits, written once over a width record: the compression of FIPS 180-4 with
its constants derived from the primes, every source word of every region, their cells through the layout table, plans of
wired segments, and an evaluator of a description's gates, static lookups and copy constraints over Python integers.  The
models are the independent side of every SHA-2 test: from the package they read the layout table and the counts around it
(where a bit field goes, not what it holds), its padding, and the plan a test hands them -- never a constant or a digest.
tests/sha256_*_model.py and tests/sha512_*_model.py bind a width and add what one feature alone has."""
import struct
from math import isqrt
from typing import NamedTuple

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha2_segments as G
from sha2_on_cq_halo2_amd import sha256_circuit as S256
from sha2_on_cq_halo2_amd import sha512_circuit as S512

P = GP.FR_MODULUS


class Width(NamedTuple):
    """What differs between SHA-256 and SHA-512.  S0, S1: the three rotations of Sigma0 (of a) and Sigma1 (of e); G0, G1:
    the two rotations and the shift of sigma0 and sigma1 (of W).  `iv`: the initial hash values by hash name.  `circuit`:
    the package's circuit module, read for SRC, layout(), REGION_ROWS, BLOCK_REGIONS, ADVICE_COLUMNS, PAIRS, FORM_*,
    rows_for, pad, FIXED, DIGEST_WORDS and VARIANT_* only."""

    bits: int
    rounds: int
    S0: tuple
    S1: tuple
    G0: tuple
    G1: tuple
    K: list
    iv: dict
    circuit: object
    letter: str  # of a word in struct

    @property
    def mask(self):
        return (1 << self.bits) - 1


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


def _width(bits, rounds, s0, s1, g0, g1, circuit, letter, names):
    """FIPS 180-4, 4.2.2 / 4.2.3 and 5.3: K is the first `bits` bits of the fractional parts of the cube roots of the first
    `rounds` primes, the initial hash values those of the square roots of the first 8 primes and of the 9th to the 16th."""
    mask = (1 << bits) - 1
    K = [_icbrt(p << (3 * bits)) & mask for p in _primes(rounds)]
    roots = [isqrt(p << (2 * bits)) & mask for p in _primes(16)]
    return Width(bits, rounds, s0, s1, g0, g1, K, dict(zip(names, (roots[:8], roots[8:]))), circuit, letter)


W32 = _width(32, 64, (2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10), S256, "I", ("sha256",))
W64 = _width(64, 80, (28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6), S512, "Q", ("sha512", "sha384"))
# FIPS 180-4, 5.3.2: the second 32 bits of the fractional parts of the square roots of the 9th to the 16th primes
W32.iv["sha224"] = [x & W32.mask for x in W64.iv["sha384"]]

_SPREAD8 = [sum(((b >> i) & 1) << (2 * i) for i in range(8)) for b in range(256)]
_DIGITS8 = {}  # a byte of base-4 digits (0 .. 3 each, four of them) -> (their low bits, their high bits)
for _b in range(256):
    _DIGITS8[_b] = (sum(((_b >> (2 * i)) & 1) << i for i in range(4)), sum(((_b >> (2 * i + 1)) & 1) << i for i in range(4)))


def rotr(x, n, bits):
    return ((x >> n) | (x << (bits - n))) & ((1 << bits) - 1)


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


def terms(w: Width, name, x):
    """The three words whose XOR is Sigma0 / Sigma1 ("S0", "S1": three rotations) or sigma0 / sigma1 ("G0", "G1": two
    rotations and a shift) of x; the circuit holds their bitwise sum (`bitsum`), whose even word is that XOR."""
    p, q, r = getattr(w, name)
    return rotr(x, p, w.bits), rotr(x, q, w.bits), rotr(x, r, w.bits) if name[0] == "S" else x >> r


def _xor3(w, name, x):
    p, q, r = terms(w, name, x)
    return p ^ q ^ r


def words_of(data: bytes, w: Width = W32):
    """The big-endian words of `data`"""
    return list(struct.unpack(f">{len(data) // (w.bits // 8)}{w.letter}", data))


def message(length, salt=0):
    return bytes((7 * i + 13 * salt + 1) % 256 for i in range(length))


def nonzero_message(length, salt=0):
    return bytes((37 * i + 11 + salt) % 251 + 1 for i in range(length))  # no zero byte: a cleared byte always shows


def compress(w: Width, words, blocks, init):
    """(per region (a, e, W, round or None, chained), the chaining values H_0 = `init` .. H_blocks) of any 16 * blocks
    words from any state."""
    mask = w.mask
    h = list(init)
    chaining, regions = [list(h)], []
    for b in range(blocks):
        regions += [(h[3 - i], h[7 - i], 0, None, b > 0) for i in range(4)]
        x = list(words[16 * b: 16 * b + 16])
        for t in range(16, w.rounds):
            x.append((x[t - 16] + _xor3(w, "G0", x[t - 15]) + x[t - 7] + _xor3(w, "G1", x[t - 2])) & mask)
        s = list(h)
        for t in range(w.rounds):
            a, e = s[0], s[4]
            t1 = s[7] + _xor3(w, "S1", e) + ((e & s[5]) ^ (~e & mask & s[6])) + w.K[t] + x[t]
            t2 = _xor3(w, "S0", a) + ((a & s[1]) ^ (a & s[2]) ^ (s[1] & s[2]))
            s = [(t1 + t2) & mask] + s[:3] + [(s[3] + t1) & mask] + s[4:7]
            regions.append((s[0], s[4], x[t], t, False))
        h = [(p + q) & mask for p, q in zip(h, s)]
        chaining.append(list(h))
    regions += [(h[3 - i], h[7 - i], 0, None, True) for i in range(4)]
    return regions, chaining


W64.iv["sha512/256"] = compress(W64, S512.pad(b"SHA-512/256", 1), 1, [x ^ 0xA5A5A5A5A5A5A5A5 for x in W64.iv["sha512"]])[1][-1]  # 5.3.6


def region_sources(w: Width, regions):
    """Per region the dict of its words by CQ_SHA256_SRC_* name: the bit sums, the round's addends and the carries of its
    three additions, each sum checked to leave the word the compression computed."""
    SC, mask = w.circuit, w.mask
    out = []
    for g, (a, e, x, t, chained) in enumerate(regions):
        s = {name: 0 for name in SC.SRC}
        s["A"], s["E"], s["W"] = a, e, x
        s["S0_EVEN"], s["S0_ODD"] = bitsum(*terms(w, "S0", a))
        s["S1_EVEN"], s["S1_ODD"] = bitsum(*terms(w, "S1", e))
        s["G0_EVEN"], s["G0_ODD"] = bitsum(*terms(w, "G0", x))
        s["G1_EVEN"], s["G1_ODD"] = bitsum(*terms(w, "G1", x))
        if g % SC.BLOCK_REGIONS >= 2:  # Maj and Ch of this region's state words and the two before
            (a1, e1), (a2, e2) = regions[g - 1][:2], regions[g - 2][:2]
            s["MAJ_EVEN"], s["MAJ_ODD"] = bitsum(a, a1, a2)
            s["CHP_EVEN"], s["CHP_ODD"] = bitsum(e, e1)
            s["CHQ_EVEN"], s["CHQ_ODD"] = bitsum(~e & mask, e2)
            s["CH"] = s["CHP_ODD"] + s["CHQ_ODD"]
        if t is not None:
            prev = out[g - 1]
            t1 = regions[g - 4][1] + prev["S1_EVEN"] + prev["CH"] + w.K[t] + x
            s["K"] = w.K[t]
            s["CARRY_E"], low = divmod(t1 + regions[g - 4][0], 1 << w.bits)
            assert low == e
            s["CARRY_A"], low = divmod(t1 + prev["S0_EVEN"] + prev["MAJ_ODD"], 1 << w.bits)
            assert low == a
            if t >= 16:
                s["CARRY_W"], low = divmod(out[g - 2]["G1_EVEN"] + regions[g - 7][2] + out[g - 15]["G0_EVEN"] + regions[g - 16][2], 1 << w.bits)
                assert low == x
        if chained:
            s["CARRY_A"] = (regions[g - SC.BLOCK_REGIONS][0] + regions[g - 4][0]) >> w.bits
            s["CARRY_E"] = (regions[g - SC.BLOCK_REGIONS][1] + regions[g - 4][1]) >> w.bits
        out.append(s)
    return out


_LAYOUT = {}


def layout(w: Width):
    """[(cell, its source's name)] of the width's layout table, read once"""
    if w.bits not in _LAYOUT:
        names = {v: k for k, v in w.circuit.SRC.items()}
        _LAYOUT[w.bits] = [(c, names[c.kind]) for c in w.circuit.layout()]
    return _LAYOUT[w.bits]


def place(w: Width, sources, table_bits, cols, first_row=0):
    """The regions' words into the columns from `first_row` on, cell by cell of the layout table."""
    SC = w.circuit
    for g, s in enumerate(sources):
        base = first_row + g * SC.REGION_ROWS
        for c, name in layout(w):
            off = c.offset + c.per_table_bits * table_bits
            field = (s[name] >> off) & ((1 << (c.len if c.len else table_bits)) - 1)
            cols[c.column][base + c.row] = spread(field) if c.form == SC.FORM_SPREAD else field
            if c.form == SC.FORM_PAIR:
                cols[c.column + 1][base + c.row] = spread(field)


def columns(w: Width, n):
    return [[0] * n for _ in range(w.circuit.ADVICE_COLUMNS)]


def cells_of(w: Width, words, blocks, table_bits, init):
    """(18 columns over the segment's rows, the chaining values): the compression circuit's cells for any 16 * blocks
    words from any state."""
    regions, chaining = compress(w, words, blocks, init)
    cols = columns(w, w.circuit.rows_for(blocks))
    place(w, region_sources(w, regions), table_bits, cols)
    return cols, chaining


def put(w: Width, cols, first_region, part):
    """A segment's columns into the circuit's, at the segment's first region."""
    at = w.circuit.REGION_ROWS * first_region
    for col, p in zip(cols, part):
        col[at: at + len(p)] = p


def word_row(w: Width, name):
    """The row, within its region, of the word-column copy of source `name`"""
    return next(c.row for c, n in layout(w) if n == name and c.form == w.circuit.FORM_WORD)


def state_row(w: Width, first_region: int, word: int) -> int:
    """The row of initial word `word` in column X: region 3 - word % 4 of the first block, the A row or the E row."""
    return w.circuit.REGION_ROWS * (first_region + 3 - word % 4) + word_row(w, "A" if word < 4 else "E")


def message_region(w: Width, first_region: int, t: int) -> int:
    """The region of message word t of the segment that starts at `first_region`"""
    return first_region + w.circuit.BLOCK_REGIONS * (t // 16) + 4 + t % 16


def _segments_read(src):
    if isinstance(src, G.DigestWord):
        return [src.segment]
    operands = (src.zero, src.one) if isinstance(src, G.Choice) else (src.x, src.y) if isinstance(src, G.Xor) else ()
    return [s for o in operands for s in _segments_read(o)]


def levels(plan):
    """Every segment's level: 0 if neither its message words nor its initial words read a digest, themselves or through
    an operand, else one more than the highest level it reads."""
    out = []
    for seg in plan.segments:
        read = [r for s in tuple(seg.sources) + tuple(seg.init or ()) for r in _segments_read(s)]
        out.append(1 + max(out[r] for r in read) if read else 0)
    return out


def plan_witness(w: Width, plan, first_regions, default_init, values, shared, bits, table_bits, n):
    """(18 advice columns of n integers, every segment's 8 final words, every segment's 8 initial words, per segment its
    choices (word, zero, one, bit)) of a plan of Private, Const, DigestWord, Var, Choice and Xor words: Private words come
    from `values` (a segment's initial ones first), everything else is resolved from `shared`, `bits` and the model's own
    final states.  The segments are evaluated level by level, as the device runs them: a level reads the levels below,
    nothing of its own.  `default_init(segment)`: the state a segment without an `init` starts from."""
    cols = columns(w, n)
    count = len(plan.segments)
    states, inits, choices, level = [None] * count, [None] * count, [[] for _ in range(count)], levels(plan)
    for lv in range(max(level) + 1):
        done = list(states)

        def plain(o):
            if isinstance(o, G.Const):
                return o.value
            return int(shared[o.index]) if isinstance(o, G.Var) else done[o.segment][o.word]

        for j in (j for j in range(count) if level[j] == lv):
            seg, private = plan.segments[j], iter(values[j])

            def resolve(src, t=None):
                if isinstance(src, G.Private):
                    return int(next(private))
                if isinstance(src, G.Choice):
                    zero, one, bit = plain(src.zero), plain(src.one), int(bits[src.bit])
                    choices[j].append((t, zero, one, bit))
                    return one if bit else zero
                return plain(src.x) ^ plain(src.y) if isinstance(src, G.Xor) else plain(src)

            init = list(default_init(seg)) if seg.init is None else [resolve(s) for s in seg.init]
            words = [resolve(s, t) for t, s in enumerate(seg.sources)]
            assert next(private, None) is None
            part, chaining = cells_of(w, words, seg.blocks, table_bits, init)
            put(w, cols, first_regions[j], part)
            states[j], inits[j] = chaining[-1], chaining[0]
    return cols, states, inits, choices


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


def _selectors_only(e):
    """Whether an expression reads fixed columns alone: a selector, or a sum of selectors"""
    if e.op == "query":
        return e.a.kind == GP.COL_FIXED
    return e.op == "add" and _selectors_only(e.a) and _selectors_only(e.b)


def findings(desc, advice, instance_words):
    """[(kind, index, row)] of every unsatisfied gate ("gate": a product whose first factor -- a selector or a sum of
    selectors -- is evaluated first), static lookup ("lookup") and copy ("copy") on the usable rows, over the fixed columns
    the description names.  Tables: dense = [0, 2^tb), spread = its bit-spread form; a lookup's inputs must sit on one
    table row."""
    cs, n = desc.cs, 1 << desc.k
    usable = n - (cs.blinding_factors() + 1)
    fixed = [[int(v) for v in desc.fixed[name]] for name in desc.fixed_names]
    inst = [list(instance_words)]
    out = []
    for gi, g in enumerate(cs.gates):
        assert g.op == "mul" and _selectors_only(g.a)
        out += [("gate", gi, r) for r in range(n) if evaluate(g.a, r, n, advice, fixed, inst) and evaluate(g.b, r, n, advice, fixed, inst)]
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
