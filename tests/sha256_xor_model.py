"""Pure-Python model of plans with XOR-wired message words (sha256_segments.Xor): the segments' cells are
tests/sha2_model.py's for the resolved words; the 16 rows of every XOR unit are placed cell by cell of layout() as a
segment's regions are -- which word of which of the unit's two regions holds what is stated in `unit_regions`, not taken
from the library -- and `run_lowered` interprets the arrays of sha256_segments.lower the way the entry point's description says
the device does.  hashlib / hmac are the references the tests hold all of it to."""
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha2_model as M2
from tests import sha256_circuit_model as M
from tests import sha256_states_model as IM

W = M.W
M32 = M.M32
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
ROW = {s: M2.word_row(W, s) for s in "AEW"}
findings = M.findings  # over the description's own fixed-column names


def unit_regions(x, y, before):
    """The words, by CQ_SHA256_SRC_* name, of a unit's two regions.  `before`: (a, e) of the region directly before the
    unit -- the last tail region behind unit 0, else the second region of the unit before.  u0: e = x and its Sigma1 cells,
    nothing else.  u1: e = y, W = x ^ y with its sigma cells, and what q_f3 lays out over (u1, u0, `before`): Maj of the
    three a words (0, 0, before's), e + e one back (even word: x ^ y), ~e + e two back, and their Ch."""
    u0, u1 = ({name: 0 for name in SC.SRC} for _ in range(2))
    for s, e in ((u0, x), (u1, y)):
        s["E"] = e
        s["S1_EVEN"], s["S1_ODD"] = M.bitsum(*M2.terms(W, "S1", e))
    w = u1["W"] = x ^ y
    u1["G0_EVEN"], u1["G0_ODD"] = M.bitsum(*M2.terms(W, "G0", w))
    u1["G1_EVEN"], u1["G1_ODD"] = M.bitsum(*M2.terms(W, "G1", w))
    u1["MAJ_EVEN"], u1["MAJ_ODD"] = M.bitsum(0, 0, before[0])
    u1["CHP_EVEN"], u1["CHP_ODD"] = M.bitsum(y, x)
    u1["CHQ_EVEN"], u1["CHQ_ODD"] = M.bitsum(~y & M32, before[1])
    u1["CH"] = u1["CHP_ODD"] + u1["CHQ_ODD"]
    assert u1["CHP_EVEN"] == w
    return u0, u1


def unit_rows(plan, unit):
    """First rows of unit `unit`'s two regions."""
    first = SS.xor_first_region(plan) + SC.XOR_REGIONS * unit
    return SC.REGION_ROWS * first, SC.REGION_ROWS * (first + 1)


def plan_witness(plan, values, shared, table_bits, n, extra=()):
    """(18 advice columns of n integers, every segment's 8 digest words, every unit's (x, y)) of a plan with Xor words and
    no Choice: Private words from `values` (a segment's initial ones first), the rest resolved from `shared` and the
    model's own digests.  `extra`: Xor units behind the plan's own that no word reads; their operands may be digest words
    of any segment."""
    cols, digests, _, _ = M2.plan_witness(W, plan, SS.first_regions(plan), lambda seg: M.IV, values, shared, (), table_bits, n)

    def plain(o):
        if isinstance(o, SS.Const):
            return o.value
        return int(shared[o.index]) if isinstance(o, SS.Var) else digests[o.segment][o.word]

    operands = [(plain(u.x), plain(u.y)) for u in SS.xor_units(plan) + list(extra)]
    before = (digests[-1][0], digests[-1][4])  # tail region 3 holds H[0] and H[4]
    for u, (x, y) in enumerate(operands):
        M2.place(W, unit_regions(x, y, before), table_bits, cols, unit_rows(plan, u)[0])
        before = (0, y)
    return cols, digests, operands


def run_lowered(low, words):
    """(every segment's digest words, every unit's result) from the lowered arrays alone: a source below SOURCE_DIGEST is
    a word of the buffer, SOURCE_DIGEST + i word i of the digests -- behind the 8 * segments digest words the units'
    results, each the XOR of its two plain sources."""
    segments = len(low.seg_blocks)
    digests = {}

    def load(s):
        s = int(s)
        if not s & SS.SOURCE_DIGEST:
            return int(words[s])
        i = s & (SS.SOURCE_DIGEST - 1)
        if i < 8 * segments:
            return digests[i]
        x, y, zero, zero_ = (int(v) for v in low.xors[i - 8 * segments])
        assert zero == zero_ == 0 and all(int(o) & (SS.SOURCE_DIGEST - 1) < 8 * segments or not int(o) & SS.SOURCE_DIGEST for o in (x, y))
        return load(x) ^ load(y)

    at = 0
    for j, blocks in enumerate(int(b) for b in low.seg_blocks):
        init = [M.IV[i] if int(s) == SS.SOURCE_IV else load(s) for i, s in enumerate(low.init_sources[8 * j: 8 * j + 8])]
        chaining = IM.compress([load(s) for s in low.sources[at: at + 16 * blocks]], blocks, init)[1]
        digests.update({8 * j + i: w for i, w in enumerate(chaining[-1])})
        at += 16 * blocks
    return [[digests[8 * j + i] for i in range(8)] for j in range(segments)], [load(SS.SOURCE_DIGEST + 8 * segments + u) for u in range(len(low.xors))]
