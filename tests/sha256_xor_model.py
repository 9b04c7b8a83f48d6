"""Pure-Python model of plans with XOR-wired message words (sha256_segments.Xor): the segments' cells are
sha256_states_model's for the resolved words; the 16 rows of every XOR unit are built here cell by cell from layout() --
which word of which of the unit's two regions holds what is stated in `unit_regions`, not taken from the library -- and
`run_lowered` interprets the arrays of sha256_segments.lower the way the entry point's description says the device does.
hashlib / hmac are the references the tests hold all of it to."""
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_choice_model as CM
from tests import sha256_circuit_model as M
from tests import sha256_states_model as IM

M32 = 0xFFFFFFFF
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
ROW = {s: next(c.row for c in SC.layout() if c.kind == SC.SRC[s] and c.form == SC.FORM_WORD) for s in "AEW"}
findings = CM.findings  # over the description's own fixed-column names


def unit_regions(x, y, before):
    """The words, by CQ_SHA256_SRC_* name, of a unit's two regions.  `before`: (a, e) of the region directly before the
    unit -- the last tail region behind unit 0, else the second region of the unit before.  u0: e = x and its Sigma1 cells,
    nothing else.  u1: e = y, W = x ^ y with its sigma cells, and what q_f3 lays out over (u1, u0, `before`): Maj of the
    three a words (0, 0, before's), e + e one back (even word: x ^ y), ~e + e two back, and their Ch."""
    u0, u1 = ({name: 0 for name in SC.SRC} for _ in range(2))
    for s, e in ((u0, x), (u1, y)):
        s["E"] = e
        s["S1_EVEN"], s["S1_ODD"] = M.bitsum(M.rotr(e, 6), M.rotr(e, 11), M.rotr(e, 25))
    w = u1["W"] = x ^ y
    u1["G0_EVEN"], u1["G0_ODD"] = M.bitsum(M.rotr(w, 7), M.rotr(w, 18), w >> 3)
    u1["G1_EVEN"], u1["G1_ODD"] = M.bitsum(M.rotr(w, 17), M.rotr(w, 19), w >> 10)
    u1["MAJ_EVEN"], u1["MAJ_ODD"] = M.bitsum(0, 0, before[0])
    u1["CHP_EVEN"], u1["CHP_ODD"] = M.bitsum(y, x)
    u1["CHQ_EVEN"], u1["CHQ_ODD"] = M.bitsum(~y & M32, before[1])
    u1["CH"] = u1["CHP_ODD"] + u1["CHQ_ODD"]
    assert u1["CHP_EVEN"] == w
    return u0, u1


def place(cols, region, words, table_bits):
    """The words of one region into the columns, cell by cell of the layout table."""
    names = {v: k for k, v in SC.SRC.items()}
    for c in SC.layout():
        off = c.offset + c.per_table_bits * table_bits
        field = (words[names[c.kind]] >> off) & ((1 << (c.len if c.len else table_bits)) - 1)
        row = region * SC.REGION_ROWS + c.row
        cols[c.column][row] = M.spread(field) if c.form == SC.FORM_SPREAD else field
        if c.form == SC.FORM_PAIR:
            cols[c.column + 1][row] = M.spread(field)


def unit_rows(plan, unit):
    """First rows of unit `unit`'s two regions."""
    first = SS.xor_first_region(plan) + SC.XOR_REGIONS * unit
    return SC.REGION_ROWS * first, SC.REGION_ROWS * (first + 1)


def plan_witness(plan, values, shared, table_bits, n, extra=()):
    """(18 advice columns of n integers, every segment's 8 digest words, every unit's (x, y)) of a plan with Xor words and
    no Choice: Private words from `values` (a segment's initial ones first), the rest resolved from `shared` and the
    model's own digests.  `extra`: Xor units behind the plan's own that no word reads; their operands may be digest words
    of any segment."""
    cols, digests = [[0] * n for _ in range(SC.ADVICE_COLUMNS)], []
    units = SS.xor_units(plan) + list(extra)

    def plain(o):
        if isinstance(o, SS.Const):
            return o.value
        return int(shared[o.index]) if isinstance(o, SS.Var) else digests[o.segment][o.word]

    for seg, first, private in zip(plan.segments, SS.first_regions(plan), values):
        private = iter(private)

        def resolve(src):
            if isinstance(src, SS.Private):
                return int(next(private))
            return plain(src.x) ^ plain(src.y) if isinstance(src, SS.Xor) else plain(src)

        init = None if seg.init is None else [resolve(s) for s in seg.init]
        words = [resolve(s) for s in seg.sources]
        assert next(private, None) is None
        part, chaining = IM.cells_of(words, seg.blocks, table_bits, init)
        at = SC.REGION_ROWS * first
        for col, p in zip(cols, part):
            col[at: at + len(p)] = p
        digests.append(chaining[-1])
    operands = [(plain(u.x), plain(u.y)) for u in units]
    before = (digests[-1][0], digests[-1][4])  # tail region 3 holds H[0] and H[4]
    for u, (x, y) in enumerate(operands):
        u0, u1 = unit_regions(x, y, before)
        first = SS.xor_first_region(plan) + SC.XOR_REGIONS * u
        place(cols, first, u0, table_bits)
        place(cols, first + 1, u1, table_bits)
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
        init = [SC.IV256[i] if int(s) == SS.SOURCE_IV else load(s) for i, s in enumerate(low.init_sources[8 * j: 8 * j + 8])]
        chaining = IM.compress([load(s) for s in low.sources[at: at + 16 * blocks]], blocks, init)[1]
        digests.update({8 * j + i: w for i, w in enumerate(chaining[-1])})
        at += 16 * blocks
    return [[digests[8 * j + i] for i in range(8)] for j in range(segments)], [load(SS.SOURCE_DIGEST + 8 * segments + u) for u in range(len(low.xors))]
