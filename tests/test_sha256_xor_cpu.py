"""CPU: XOR-wired message words and HMAC-SHA-256 -- `hmac_sha256` plans lowered and run through a pure-Python chain
against Python's hmac / hashlib, the plans that must be refused, what `describe` adds for an Xor plan (selector rows, the
gate, the copies and their order) and what it must leave as it was, and the model's witness against every gate, lookup
and copy of the description, honest and tampered."""
import hashlib
import hmac
import struct

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_segments_model as SM
from tests import sha256_xor_model as XM
from tests.test_sha256_segments_cpu import DESCRIBED as DESCRIBED_FIXED_AND_COPIES
from tests.test_sha256_varlen_cpu import DESCRIBED, description_hash
from tests.sha2_model import words_of

P16 = (SS.PRIVATE,) * 16
# description_hash of midstate(2) at k = 11, recorded on the commit before the XOR variant was added to _constraint_system
# (no earlier test pins a plan with an initial state by hash)
MIDSTATE_11_2 = "de29013555df3a82ef5ec9c410290b7665093a22c8d92e4b1edf8de7a84fa803"
# RFC 4231 test cases 1 and 2, a 64-byte key with an empty message, a 0-byte key
CASES = {"rfc4231_1": (b"\x0b" * 20, b"Hi There"), "rfc4231_2": (b"Jefe", b"what do ya want for nothing?"),
         "key64_empty": (bytes(range(64)), b""), "key0": (b"", b"twelve bytes")}
RFC_TAGS = {"rfc4231_1": "b0344c61d8db38535ca8afceaf0bf12b881dc200c9833da726e9376c2e32cff7",
            "rfc4231_2": "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843"}


def hmac_inputs(plan, key, message):
    return [words_of(message)] + [[]] * (len(plan.segments) - 1), words_of(key)


# ---- 1. hmac_sha256 plans, lowered ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("commit", [False, True])
def test_a_lowered_hmac_plan_gives_pythons_tag(name, commit):
    key, message = CASES[name]
    want = hmac.new(key, message, "sha256").digest()
    assert name not in RFC_TAGS or want.hex() == RFC_TAGS[name]
    plan = SS.hmac_sha256(len(key), len(message), commit)
    low = SS.lower(plan)
    values, shared = hmac_inputs(plan, key, message)
    digests, results = XM.run_lowered(low, SS.word_buffer(low, values, shared))
    assert struct.pack(">8I", *digests[1]) == want
    assert plan.public == ((1, 2) if commit else (1,))
    if commit:
        assert struct.pack(">8I", *digests[2]) == hashlib.sha256(key).digest()
    kw = len(key) // 4
    assert len(low.xors) == 2 * kw == len(results)
    assert results == [w ^ pad for pad in (SS.HMAC_IPAD, SS.HMAC_OPAD) for w in words_of(key)]
    assert SS.rows_for(plan) == 2240 + (SC.rows_for(1) if len(message) > 54 else 0) + 32 * kw + (SC.rows_for(1 + (len(key) > 55)) if commit else 0)
    # the model's own resolution of the plan agrees
    assert XM.plan_witness(plan, values, shared, 12, 1 << 13)[1] == digests


def test_the_hmac_plan_word_for_word():
    p = SS.hmac_sha256(8, 60, commit_key=True)
    inner, outer, commit = p.segments
    assert (inner.blocks, outer.blocks, commit.blocks) == (1 + 2, 2, 1) and SS.shared_counts(p) == (2, 0)
    assert inner.sources[:16] == (SS.Xor(SS.Var(0), SS.Const(0x36363636)), SS.Xor(SS.Var(1), SS.Const(0x36363636))) + (SS.Const(0x36363636),) * 14
    assert inner.sources[16:31] == (SS.PRIVATE,) * 15 and [s.value for s in inner.sources[31:]] == SC.pad(bytes(124))[31:]
    assert outer.sources[:16] == (SS.Xor(SS.Var(0), SS.Const(0x5C5C5C5C)), SS.Xor(SS.Var(1), SS.Const(0x5C5C5C5C))) + (SS.Const(0x5C5C5C5C),) * 14
    assert outer.sources[16:24] == tuple(SS.DigestWord(0, i) for i in range(8)) and [s.value for s in outer.sources[24:]] == SC.pad(bytes(96))[24:]
    assert commit.sources[:2] == (SS.Var(0), SS.Var(1)) and [s.value for s in commit.sources[2:]] == SC.pad(bytes(8))[2:]
    assert SS.hmac_sha256(64, 0, commit_key=True).segments[2].blocks == 2  # a 64-byte key pads to two blocks
    for args in ((68, 0), (6, 0), (4, 3), (-4, 0), (4, -4)):
        with pytest.raises(ValueError, match="multiples of 4"):
            SS.hmac_sha256(*args)


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------

def test_plans_that_are_refused():
    var = tuple(SS.Var(t) for t in range(16))
    first = SS.Segment(1, P16)

    def plan(word, at=2):
        return SS.Plan((first, SS.Segment(1, var[:at] + (word,) + var[at + 1:])), (1,))

    for good in (SS.Xor(var[0], SS.Const(5)), SS.Xor(SS.DigestWord(0, 7), var[3]), SS.Xor(SS.Const(1), SS.Const(0xFFFFFFFF)), SS.Xor(var[0], var[0])):
        SS.describe(11, plan(good))
    for bad in (SS.Xor(SS.Xor(var[0], var[1]), var[1]), SS.Xor(var[0], SS.Choice(0, var[0], var[1])), SS.Xor(SS.PRIVATE, var[1]),
                SS.Xor(var[0], SS.PRIVATE), SS.Xor(var[0], 7), SS.Xor(SS.Var(-1), var[1]), SS.Xor(var[0], SS.Const(1 << 32)),
                SS.Xor(SS.DigestWord(1, 0), var[1]), SS.Xor(var[0], SS.DigestWord(2, 0)), SS.Xor(var[0], SS.DigestWord(0, 8))):
        with pytest.raises(ValueError, match="segment 1, word 2"):
            SS.describe(11, plan(bad))
    # a shared unit: every reader must come behind the unit's digest operand
    shared = SS.Xor(SS.DigestWord(0, 0), var[0])
    with pytest.raises(ValueError, match="segment 0, word 5"):
        SS.describe(11, SS.Plan((SS.Segment(1, P16[:5] + (shared,) + P16[6:]), SS.Segment(1, (shared,) + P16[1:])), (1,)))
    # an Xor as an initial word, as a Choice is
    with pytest.raises(ValueError, match="segment 1, initial word 3"):
        SS.describe(11, SS.Plan((first, SS.Segment(1, P16, (SS.PRIVATE,) * 3 + (SS.Xor(var[0], var[1]),) + (SS.PRIVATE,) * 4)), (1,)))
    # an Xor and a Choice in one plan
    with pytest.raises(ValueError, match="segment 1, word 4.*do not combine"):
        SS.describe(12, SS.Plan((first, SS.Segment(1, (SS.Xor(var[0], var[1]),) + P16[1:4] + (SS.Choice(0, var[0], var[1]),) + P16[5:])), (1,)))
    with pytest.raises(ValueError, match="combine"):
        SC._constraint_system(12, "dense", "spread", choice=True, xor=True)
    with pytest.raises(ValueError, match="combine"):
        SC._constraint_system(12, "dense", "spread", varlen=True, xor=True)
    # the area counts: 3 one-block segments and 19 units are 2032 rows, 2^11 has 2027
    def area(units):
        xs = tuple(SS.Xor(SS.Var(t), SS.Const(t)) for t in range(units))
        return SS.Plan((first, SS.Segment(1, xs[:16] + P16[len(xs[:16]):]), SS.Segment(1, xs[16:] + P16[len(xs[16:]):])), (2,))

    assert SS.rows_for(area(18)) == 3 * 576 + 16 * 18 == 2016 and len(SS.first_regions(area(18))) == 3
    SS.describe(11, area(18))
    with pytest.raises(ValueError, match="19 xor units need 2032 rows"):
        SS.describe(11, area(19))


# ---- 3. the description of an Xor plan ----------------------------------------------------------------------------------------

def xor_case():
    """Two segments and four units, numbered by first use: unit 0 = Var 0 ^ Const, read twice (segment 0 word 3, segment 1
    word 0); unit 1 = Var 2 ^ Const 7 (segment 1 word 8); unit 2 = digest word 5 of segment 0 ^ Var 1 (segment 1 word 9);
    unit 3 = Var 0 ^ Var 0 (segment 1 word 15).  Var 1 is also segment 1's initial word 2; Vars 0 and 2 stand in units only."""
    a, b, c = SS.Xor(SS.Var(0), SS.Const(0xFFFF0000)), SS.Xor(SS.DigestWord(0, 5), SS.Var(1)), SS.Xor(SS.Var(0), SS.Var(0))
    d = SS.Xor(SS.Var(2), SS.Const(7))
    first = SS.Segment(1, P16[:3] + (a,) + P16[4:])
    init = (SS.PRIVATE, SS.PRIVATE, SS.Var(1)) + (SS.PRIVATE,) * 5
    second = SS.Segment(1, (a,) + P16[1:8] + (d, b) + P16[10:15] + (c,), init)
    plan = SS.Plan((first, second), (1,))
    values = [list(range(100, 115)), list(range(200, 207)) + list(range(300, 312))]  # segment 1: 7 initial words, 12 message words
    return plan, values, [0x12345678, 0x9ABCDEF0, 0x0F0F0F0F]


@pytest.fixture(scope="module")
def described():
    plan, values, shared = xor_case()
    d = SS.describe(11, plan)
    cols, digests, operands = XM.plan_witness(plan, values, shared, d.table_bits, 1 << 11)
    return plan, d, cols, digests, operands


def test_the_description_of_an_xor_plan(described):
    plan, d, _, _, _ = described
    units = SS.xor_units(plan)
    assert len(units) == 4 and SS.rows_for(plan) == 2 * 576 + 4 * 16 and SS.xor_first_region(plan) == 144
    assert units[0].y == SS.Const(0xFFFF0000) and units[1] == SS.Xor(SS.Var(2), SS.Const(7))  # by first use: (1, 8) before (1, 9)
    base = SC._constraint_system(12, "dense", "spread")[0]
    assert (d.cs.blinding_factors(), d.cs.degree()) == (base.blinding_factors(), base.degree()) == (20, 4)
    assert SC.usable_rows(11) == 2048 - 21 and SC.max_blocks(12) == 7
    assert d.fixed_names == SC.FIXED_XOR == SC.FIXED + ("q_xor",) and tuple(d.fixed) == SC.FIXED_XOR
    assert SC.GATES_XOR == SC.GATES + ("xor_word",) and [g for g in d.cs.gates] and len(d.cs.gates) == len(SC.GATES_XOR)
    X = d.advice[2 * SC.PAIRS]
    assert d.cs.permutation_columns == [X, d.fixed_columns["const"], d.instance]  # no equality on Y
    # the new queries: the three dense CHP_EVEN cells of row 6, and q_xor
    new = sorted(set(d.cs.advice_queries) - set(base.advice_queries))
    assert new == [(0, 6), (2, 6), (4, 6)] and len(d.cs.fixed_queries) == len(base.fixed_queries) + 1
    u1 = [XM.unit_rows(plan, u)[1] for u in range(4)]
    u0 = [XM.unit_rows(plan, u)[0] for u in range(4)]
    assert np.nonzero(d.fixed["q_xor"])[0].tolist() == u1
    assert [r for r in np.nonzero(d.fixed["q_all"])[0].tolist() if r >= 1152] == sorted(u0 + u1)
    assert [r for r in np.nonzero(d.fixed["q_f3"])[0].tolist() if r >= 1152] == u1
    assert not any(d.fixed[name][1152:].any() for name in ("q_round", "q_sched", "q_chain"))
    for row in u0 + u1:  # scales as in a segment's region
        for j in range(SC.PAIRS):
            assert np.array_equal(d.fixed[f"scale{j}"][row: row + 8], d.fixed[f"scale{j}"][:8]), (row, j)


def test_the_copies_of_an_xor_plan_stand_behind_the_old_ones_in_order(described):
    plan, d, _, _, _ = described
    strip = lambda s: SS.PRIVATE if isinstance(s, SS.Xor) else s
    old = SS.describe(11, SS.Plan(tuple(seg._replace(sources=tuple(strip(s) for s in seg.sources)) for seg in plan.segments), plan.public))
    assert d.copies[: len(old.copies)] == old.copies
    tail = d.copies[len(old.copies):]
    X, const = d.advice[2 * SC.PAIRS], d.fixed_columns["const"]
    e = lambda u, second: (X, XM.unit_rows(plan, u)[second] + XM.ROW["E"])
    w = lambda u: (X, XM.unit_rows(plan, u)[1] + XM.ROW["W"])
    digest5 = (X, SC.REGION_ROWS * (68 + 3 - 5 % 4) + XM.ROW["E"])  # digest word 5 of segment 0: tail region 2, E row
    state2 = (X, SC.REGION_ROWS * (72 + 3 - 2) + XM.ROW["A"])  # initial word 2 of segment 1
    want = [((const, e(0, 1)[1]), e(0, 1)), ((const, e(1, 1)[1]), e(1, 1)), (digest5, e(2, 0)),  # (1) constants and digests, unit by unit
            (e(0, 0), e(3, 0)), (e(0, 0), e(3, 1)),  # (2) var 0 has cells in units only: its first is unit 0's x
            (state2, e(2, 1))]  # var 1: its state cell comes first; var 2 has one cell and needs no copy
    assert tail[:6] == want
    readers = [(w(0), (X, SM.w_cell(plan, 0, 3)[0])), (w(0), (X, SM.w_cell(plan, 1, 0)[0])), (w(1), (X, SM.w_cell(plan, 1, 8)[0])),
               (w(2), (X, SM.w_cell(plan, 1, 9)[0])), (w(3), (X, SM.w_cell(plan, 1, 15)[0]))]
    assert tail[6:] == readers  # (3) every reader to its unit, by (segment, word); var 2 has one cell and needs no copy
    assert int(d.fixed["const"][e(0, 1)[1]]) == 0xFFFF0000 and int(d.fixed["const"][e(1, 1)[1]]) == 7


def test_plans_without_an_xor_are_described_as_before():
    a = SC.describe(10, 1)
    b = SS.describe(10, SS.batch([1]))
    for d in (a, b):
        h = hashlib.sha256(b"".join(d.fixed[name].tobytes() for name in SC.FIXED) + repr(d.copies).encode())
        assert h.hexdigest() == DESCRIBED_FIXED_AND_COPIES[10, 1]
    assert description_hash(SS.describe(12, SS.merkle_path(2, leaf_blocks=1, public_leaf=True))) == DESCRIBED["choice"]
    assert description_hash(SS.describe(12, SS.merkle_tree(2))) == DESCRIBED["segments"]
    assert description_hash(SS.describe(11, SS.midstate(2))) == MIDSTATE_11_2
    low = SS.lower(SS.merkle_path(2))
    assert low.xors.shape == (0, 4) and low.xors.dtype == np.uint32


# ---- 4. the model's witness against the description ---------------------------------------------------------------------------

def _gate(name, row):
    return ("gate", SC.GATES_XOR.index(name), row)


def _copies_touching(d, cell):
    return {i for i, (a, b) in enumerate(d.copies) if cell in (a, b)}


def test_the_model_witness_satisfies_the_description(described):
    plan, d, cols, digests, operands = described
    _, _, shared = xor_case()
    assert operands == [(shared[0], 0xFFFF0000), (shared[2], 7), (digests[0][5], shared[1]), (shared[0], shared[0])]
    assert XM.findings(d, cols, digests[1]) == []


@pytest.mark.parametrize("table_bits", [11, 12])
def test_the_hmac_plan_with_a_committed_key_is_satisfied_by_the_model(table_bits):
    key, message = CASES["rfc4231_1"]
    plan = SS.hmac_sha256(len(key), len(message), commit_key=True)
    d = SS.describe(12, plan, table_bits)
    values, shared = hmac_inputs(plan, key, message)
    cols, digests, _ = XM.plan_witness(plan, values, shared, table_bits, 1 << 12)
    instance = words_of(hmac.new(key, message, "sha256").digest() + hashlib.sha256(key).digest())
    assert digests[1] + digests[2] == instance and SS.rows_for(plan) == 2240 + 160 + 576
    assert XM.findings(d, cols, instance) == []
    wrong = list(instance)
    wrong[3] ^= 1
    assert [f[0] for f in XM.findings(d, cols, wrong)] == ["copy"]


def _set_word(cols, table_bits, row0, kind, value):
    """The X cell of word `kind` (A, E or W) of the region at row0 and the dense / spread pieces it decomposes into."""
    for c in SC.layout():
        if c.kind != SC.SRC[kind] or c.form == SC.FORM_SPREAD:
            continue
        field = (value >> c.offset) & ((1 << c.len) - 1)
        cols[c.column][row0 + c.row] = field
        if c.form == SC.FORM_PAIR:
            cols[c.column + 1][row0 + c.row] = XM.M.spread(field)
    if kind == "E":
        cols[XM.Y][row0 + XM.ROW["E"]] = XM.M.spread(value)


def test_a_changed_result_word_is_the_gate_and_the_copies(described):
    """Unit 0 (read twice): W of u1 replaced by another 32-bit word with its row-2 pieces, so `w_word` holds; the sigma
    cells of the old W stay, so the two sigma decompositions fail with `xor_word`, and both readers' copies."""
    plan, d, cols, digests, _ = described
    cols = [list(c) for c in cols]
    row0 = XM.unit_rows(plan, 0)[1]
    _set_word(cols, d.table_bits, row0, "W", cols[XM.X][row0 + XM.ROW["W"]] ^ 0x00010000)
    found = set(XM.findings(d, cols, digests[1]))
    ties = _copies_touching(d, (d.advice[XM.X], row0 + XM.ROW["W"]))
    assert len(ties) == 2
    assert found == {_gate("xor_word", row0), _gate("sigma0_even_odd", row0), _gate("sigma1_even_odd", row0)} | {("copy", i, row0 + XM.ROW["W"]) for i in ties}


def test_a_changed_operand_is_the_ch_decomposition_and_its_copy(described):
    """Unit 2's x (digest word 5 of segment 0), E of u0 and its pieces and spread form replaced: `e_word` / `e_spread`
    hold; `chp_even_odd` of u1 fails (its chunks are the old x's), Sigma1's decomposition in u0, and the copy to the tail."""
    plan, d, cols, digests, _ = described
    cols = [list(c) for c in cols]
    u0, u1 = XM.unit_rows(plan, 2)
    _set_word(cols, d.table_bits, u0, "E", cols[XM.X][u0 + XM.ROW["E"]] ^ 0x4)
    found = set(XM.findings(d, cols, digests[1]))
    (tie,) = _copies_touching(d, (d.advice[XM.X], u0 + XM.ROW["E"]))
    # u1 of unit 3 looks two regions back onto this region? no: two back from unit 3's u1 is unit 2's u1
    assert found == {_gate("chp_even_odd", u1), _gate("Sigma1_even_odd", u0), ("copy", tie, d.copies[tie][0][1])}
