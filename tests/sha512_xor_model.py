"""Pure-Python model of plans with XOR-wired message words on the 64-bit circuit (sha512_xor.Xor): what
tests/sha256_xor_model.py is at 32 bits, bound to tests/sha2_model.py's 64-bit width.  The segments' cells are
tests/sha2_model.py's for the resolved words; the 32 rows of every XOR unit are placed cell by cell of the layout table as a
segment's regions are -- which word of which of the unit's two regions holds what is stated in `unit_regions`, and where
the units lie in `unit_rows`, neither taken from the package -- and `run_lowered` interprets the arrays of sha512_xor.lower
the way the entry point's description says the device does.  hashlib / hmac are the references the tests hold all of it to."""
from tests import sha2_model as M2
from tests import sha512_circuit_model as M
from tests.sha2_model import bitsum

W = M2.W64
SC = W.circuit  # read for the layout table and the counts around it only
M64 = W.mask
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
ROW = {s: M2.word_row(W, s) for s in "AEW"}
XOR_REGIONS = 2  # a unit's regions: e = x, then e = y and W = x ^ y
SOURCE_DIGEST, SOURCE_IV = 1 << 31, (1 << 32) - 1  # the encoding of a source, as the header states it
IPAD, OPAD = (int.from_bytes(bytes([b]) * 8, "big") for b in (0x36, 0x5C))  # RFC 2104


def unit_regions(x, y, before):
    """The words, by CQ_SHA256_SRC_* name, of a unit's two regions.  `before`: (a, e) of the region directly before the
    unit -- the last tail region behind unit 0, else the second region of the unit before.  u0: e = x and its Sigma1 cells,
    nothing else.  u1: e = y, W = x ^ y with its sigma cells, and what q_f3 lays out over (u1, u0, `before`): Maj of the
    three a words (0, 0, before's), e + e one back (even word: x ^ y), ~e + e two back, and their Ch."""
    u0, u1 = ({name: 0 for name in SC.SRC} for _ in range(2))
    for s, e in ((u0, x), (u1, y)):
        s["E"] = e
        s["S1_EVEN"], s["S1_ODD"] = bitsum(*M2.terms(W, "S1", e))
    w = u1["W"] = x ^ y
    u1["G0_EVEN"], u1["G0_ODD"] = bitsum(*M2.terms(W, "G0", w))
    u1["G1_EVEN"], u1["G1_ODD"] = bitsum(*M2.terms(W, "G1", w))
    u1["MAJ_EVEN"], u1["MAJ_ODD"] = bitsum(0, 0, before[0])
    u1["CHP_EVEN"], u1["CHP_ODD"] = bitsum(y, x)
    u1["CHQ_EVEN"], u1["CHQ_ODD"] = bitsum(~y & M64, before[1])
    u1["CH"] = u1["CHP_ODD"] + u1["CHQ_ODD"]
    assert u1["CHP_EVEN"] == w
    return u0, u1


def first_regions(plan):
    """The first region of every segment, and the one behind the last: the segments lie one behind another."""
    out = [0]
    for seg in plan.segments:
        out.append(out[-1] + SC.rows_for(seg.blocks) // SC.REGION_ROWS)
    return out


def unit_rows(plan, unit):
    """First rows of unit `unit`'s two regions: the units lie directly behind the last segment's tail."""
    first = first_regions(plan)[-1] + XOR_REGIONS * unit
    return SC.REGION_ROWS * first, SC.REGION_ROWS * (first + 1)


def xor_units(plan):
    """The plan's distinct Xor words in the order of their first use, by (segment, word)."""
    return list(dict.fromkeys(s for seg in plan.segments for s in seg.sources if isinstance(s, M2.G.Xor)))


def plan_witness(plan, values, shared, table_bits, n, extra=()):
    """(18 advice columns of n integers, every segment's 8 final words, every unit's (x, y)) of a plan with Xor words:
    Private words from `values` (a segment's initial ones first), the rest resolved from `shared` and the model's own final
    states.  `extra`: Xor units behind the plan's own that no word reads; their operands may be digest words of any segment."""
    cols, states, _, _ = M2.plan_witness(W, plan, first_regions(plan)[:-1], lambda seg: M.IV[seg.variant], values, shared, (), table_bits, n)

    def plain(o):
        if isinstance(o, M2.G.Const):
            return o.value
        return int(shared[o.index]) if isinstance(o, M2.G.Var) else states[o.segment][o.word]

    operands = [(plain(u.x), plain(u.y)) for u in xor_units(plan) + list(extra)]
    before = (states[-1][0], states[-1][4])  # tail region 3 holds H[0] and H[4]
    for u, (x, y) in enumerate(operands):
        M2.place(W, unit_regions(x, y, before), table_bits, cols, unit_rows(plan, u)[0])
        before = (0, y)
    return cols, states, operands


def instance_of(plan, states):
    return [x for s, words in plan.public for x in states[s][:words]]


def run_lowered(low, words):
    """(every segment's final words, every unit's result) from the lowered arrays alone: a source below SOURCE_DIGEST is a
    word of the buffer, SOURCE_DIGEST + i word i of the digests -- behind the 8 * segments state words the units' results,
    each the XOR of its two plain sources."""
    segments = len(low.seg_blocks)
    digests = {}

    def load(s):
        s = int(s)
        if not s & SOURCE_DIGEST:
            return int(words[s])
        i = s & (SOURCE_DIGEST - 1)
        if i < 8 * segments:
            return digests[i]
        x, y, zero, zero_ = (int(v) for v in low.xors[i - 8 * segments])
        assert zero == zero_ == 0 and all(int(o) & (SOURCE_DIGEST - 1) < 8 * segments or not int(o) & SOURCE_DIGEST for o in (x, y))
        return load(x) ^ load(y)

    at = 0
    for j, (blocks, variant) in enumerate(zip((int(b) for b in low.seg_blocks), (int(v) for v in low.seg_variant))):
        init = [M.IV[variant][i] if int(s) == SOURCE_IV else load(s) for i, s in enumerate(low.init_sources[8 * j: 8 * j + 8])]
        chaining = M2.compress(W, [load(s) for s in low.sources[at: at + 16 * blocks]], blocks, init)[1]
        digests.update({8 * j + i: w for i, w in enumerate(chaining[-1])})
        at += 16 * blocks
    return [[digests[8 * j + i] for i in range(8)] for j in range(segments)], [load(SOURCE_DIGEST + 8 * segments + u) for u in range(len(low.xors))]
