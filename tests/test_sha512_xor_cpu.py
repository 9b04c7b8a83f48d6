"""CPU: XOR-wired message words on the 64-bit circuit and HMAC-SHA-512 / HMAC-SHA-384 (sha512_xor.py; no device, the built
library for cq_sha512_layout only) -- what the XOR variant adds to the constraint system and what it leaves as it was, the
plans that are refused, the lowering, and the model's witness against every gate, lookup and copy of the description
through tests/witness_check_model.py: clean as it is, with Python's hmac / hashlib tags, and named where a cell is changed."""
import hashlib
import hmac
import random
import struct

import numpy as np
import pytest

from oracle import cq_prover as CP
from oracle import plonk as PL
from sha2_on_cq_halo2_amd import api
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from sha2_on_cq_halo2_amd import sha512_xor as SX
from sha2_on_cq_halo2_amd.sha2_segments import Choice, Xor
from tests import sha512_segments_model as SM
from tests import sha512_xor_model as XM
from tests import witness_check_model as WM
from tests.sha2_model import spread, words_of
from tests.sha_oracle import KINDS, oracle_circuit

P16 = (SS.PRIVATE,) * 16
ONES = (1 << 64) - 1
Var, Const, DW = SS.Var, SS.Const, SS.DigestWord
EDGES = [(0, 0), (ONES, 0), (0x6A09E667F3BCC908, 0x6A09E667F3BCC908), (0x8000000000000001, 0x7FFFFFFFFFFFFFFE)]
KEY = bytes(range(1, 129))
MESSAGE = bytes((11 * i + 3) % 256 for i in range(112))


def one_unit_plan():
    return SS.Plan((SS.Segment(1, P16[:3] + (Xor(Var(0), Var(1)),) + P16[4:]),), ((0, 8),))


def same_var_plan():
    """One Var as both operands of a unit, and the same Var beside a constant."""
    return SS.Plan((SS.Segment(1, (Xor(Var(0), Var(0)), Xor(Const(ONES), Var(0))) + P16[2:]),), ((0, 8),))


def edges_plan():
    """Four units over eight Vars: the edge pairs stand in `shared`."""
    return SS.Plan((SS.Segment(1, tuple(Xor(Var(2 * i), Var(2 * i + 1)) for i in range(4)) + P16[4:]),), ((0, 8),))


def two_segment_plan():
    """Unit 0 = digest word 7 of segment 0 ^ Var 0, read by words 0 and 5 of segment 1, a SHA-384 segment; unit 1 =
    Const ^ Var 0 (word 9): Var 0 stands in operand cells only, unit 0's y first, unit 1's y second."""
    a, b = Xor(DW(0, 7), Var(0)), Xor(Const(0x5C5C5C5C5C5C5C5C), Var(0))
    return SS.Plan((SS.Segment(1, P16), SS.Segment(1, (a,) + P16[1:5] + (a,) + P16[6:9] + (b,) + P16[10:], None, SC.VARIANT_384)), ((1, 6),))


def hmac_inputs(plan, key, message):
    return [words_of(message, XM.W)] + [[]] * (len(plan.segments) - 1), words_of(key, XM.W)


# ---- 1. the variant of the constraint system ---------------------------------------------------------------------------------

def test_a_plan_without_an_xor_is_described_as_sha512_segments_describes_it():
    for k, plan in ((12, SS.double_sha512(1)), (11, SS.sha512_256(1)), (13, SM.mixed_plan())):
        a, b = SX.describe(k, plan), SS.describe(k, plan)
        assert a.fixed_names == b.fixed_names == SC.FIXED and tuple(a.fixed) == tuple(b.fixed) and a.copies == b.copies
        assert all(np.array_equal(a.fixed[name], b.fixed[name]) for name in SC.FIXED)
        assert [g for g in a.cs.gates] and len(a.cs.gates) == len(b.cs.gates) == len(SC.GATES)
        assert a.cs.advice_queries == b.cs.advice_queries and a.cs.fixed_queries == b.cs.fixed_queries
        assert a.cs.permutation_columns == [a.advice[XM.X], a.fixed_columns["const"], a.instance]
        assert (a.blocks_list, a.variants) == (b.blocks_list, b.variants)
        la, lb = SX.lower(plan), SS.lower(plan)
        assert all(np.array_equal(x, y) for x, y in zip(la[:7], lb[:7])) and la[7:] == lb[7:]
        assert SX.rows_for(plan) == SS.rows_for(plan) and SX.first_regions(plan) == SS.first_regions(plan)


def test_sha512_segments_still_refuses_an_xor():
    assert SS.WIDTH.gated == () and SX.WIDTH.gated == (Xor,) and SX.Segment is SS.Segment and SX.Plan is SS.Plan
    for f in (SS.describe, SS.lower):
        with pytest.raises(ValueError, match="segment 0, word 3: Xor words are not built on the 64-bit circuit yet"):
            f(*((11,) if f is SS.describe else ()), one_unit_plan())


@pytest.mark.parametrize("table_bits", [11, 12, 13, 16])
def test_the_variant_adds_one_column_one_gate_and_no_blinding_row(table_bits):
    base = SC._constraint_system(table_bits, "dense", "spread")[0]
    d = SX.describe(11, one_unit_plan(), table_bits)
    assert (d.cs.blinding_factors(), d.cs.degree()) == (base.blinding_factors(), base.degree()) == (20, 4)
    assert SC.usable_rows(11, table_bits) == 2048 - 21 and SC.max_blocks(13, table_bits) == 6
    assert d.fixed_names == SC.FIXED_XOR == SC.FIXED + ("q_xor",) and tuple(d.fixed) == SC.FIXED_XOR
    assert SC.GATES_XOR == SC.GATES + ("xor_word",) and len(d.cs.gates) == len(SC.GATES_XOR) == len(base.gates) + 1
    assert d.cs.permutation_columns == [d.advice[XM.X], d.fixed_columns["const"], d.instance]  # no equality on Y
    assert (SC.XOR_REGIONS, SC.XOR_WORDS) == (XM.XOR_REGIONS, 4)
    # the new queries: the dense cell of every CHP_EVEN chunk that starts below bit 64, in the region's own rows, and q_xor
    chunks = [c for c, name in XM.M2.layout(XM.W) if name == "CHP_EVEN" and c.form == SC.FORM_PAIR and not c.len]
    assert len(chunks) == SC.CHUNKS
    want = sorted((c.column, c.row) for c in chunks if c.per_table_bits * table_bits < 64)
    assert len(want) == -(-64 // table_bits) and set(want) <= set(d.cs.advice_queries)
    assert sorted(set(d.cs.advice_queries) - set(base.advice_queries)) == [q for q in want if q not in base.advice_queries]
    assert len(d.cs.fixed_queries) == len(base.fixed_queries) + 1


def test_the_fixed_cells_of_the_units():
    plan = two_segment_plan()
    d = SX.describe(12, plan)
    units = SX.xor_units(plan)
    assert units == XM.xor_units(plan) and len(units) == 2 and units[0].x == DW(0, 7)
    assert SX.rows_for(plan) == 2 * 1408 + 2 * 32 and SX.xor_first_region(plan) == 176 == XM.first_regions(plan)[-1]
    u0, u1 = ([XM.unit_rows(plan, u)[i] for u in range(2)] for i in range(2))
    assert np.nonzero(d.fixed["q_xor"])[0].tolist() == u1
    assert [r for r in np.nonzero(d.fixed["q_all"])[0].tolist() if r >= 2816] == sorted(u0 + u1)
    assert [r for r in np.nonzero(d.fixed["q_f3"])[0].tolist() if r >= 2816] == u1
    assert not any(d.fixed[name][2816:].any() for name in ("q_round", "q_sched", "q_chain"))
    for row in u0 + u1:  # scales as in a segment's region
        for j in range(SC.PAIRS):
            assert np.array_equal(d.fixed[f"scale{j}"][row: row + 16], d.fixed[f"scale{j}"][:16]), (row, j)
    # the copies stand behind those of the plan with the Xor words Private
    strip = lambda s: SS.PRIVATE if isinstance(s, Xor) else s
    old = SS.describe(12, SS.Plan(tuple(seg._replace(sources=tuple(strip(s) for s in seg.sources)) for seg in plan.segments), plan.public))
    assert d.copies[: len(old.copies)] == old.copies
    Xc, const = d.advice[XM.X], d.fixed_columns["const"]
    e = lambda u, second: (Xc, XM.unit_rows(plan, u)[second] + XM.ROW["E"])
    w = lambda u: (Xc, XM.unit_rows(plan, u)[1] + XM.ROW["W"])
    assert d.copies[len(old.copies):] == [
        ((Xc, SM.tail_row(0, 1, 7)), e(0, 0)), ((const, e(1, 0)[1]), e(1, 0)),   # (1) digests and constants, unit by unit
        (e(0, 1), e(1, 1)),                                                       # (2) Var 0: its first cell is unit 0's y
        (w(0), (Xc, SM.message_row(88, 0))), (w(0), (Xc, SM.message_row(88, 5))), (w(1), (Xc, SM.message_row(88, 9)))]  # (3) the readers
    assert int(d.fixed["const"][e(1, 0)[1]]) == 0x5C5C5C5C5C5C5C5C


# ---- 2. refusals, lowering, the HMAC plans -----------------------------------------------------------------------------------

def test_plans_that_are_refused():
    var = tuple(Var(t) for t in range(16))
    first = SS.Segment(1, P16)

    def plan(word, at=2):
        return SS.Plan((first, SS.Segment(1, var[:at] + (word,) + var[at + 1:])), ((1, 8),))

    for good in (Xor(var[0], Const(5)), Xor(DW(0, 7), var[3]), Xor(Const(1), Const(ONES)), Xor(var[0], var[0])):
        SX.describe(12, plan(good))
        SX.lower(plan(good))
    for bad in (Xor(Xor(var[0], var[1]), var[1]), Xor(var[0], Choice(0, var[0], var[1])), Xor(SS.PRIVATE, var[1]), Xor(var[0], SS.PRIVATE),
                Xor(var[0], 7), Xor(Var(-1), var[1]), Xor(var[0], Const(1 << 64)), Xor(DW(1, 0), var[1]), Xor(var[0], DW(2, 0)),
                Xor(var[0], DW(0, 8))):
        with pytest.raises(ValueError, match="segment 1, word 2"):
            SX.describe(12, plan(bad))
        with pytest.raises(ValueError, match="segment 1, word 2"):
            SX.lower(plan(bad))
    with pytest.raises(ValueError, match="the x operand of an xor is a Const, a Var or a DigestWord"):
        SX._check_plan(plan(Xor(SS.PRIVATE, var[1])))
    # a shared unit: every reader must come behind the unit's digest operand
    shared = Xor(DW(0, 0), var[0])
    with pytest.raises(ValueError, match="segment 0, word 5"):
        SX.describe(12, SS.Plan((SS.Segment(1, P16[:5] + (shared,) + P16[6:]), SS.Segment(1, (shared,) + P16[1:])), ((1, 8),)))
    # an Xor as an initial word
    with pytest.raises(ValueError, match="segment 1, initial word 3: an initial word is Private, Const, DigestWord or Var"):
        SX.describe(12, SS.Plan((first, SS.Segment(1, P16, (SS.PRIVATE,) * 3 + (Xor(var[0], var[1]),) + (SS.PRIVATE,) * 4)), ((1, 8),)))
    # a Choice anywhere: as a word, beside an Xor, as an initial word
    choice = Choice(0, var[0], var[1])
    for segs, where in (((first, SS.Segment(1, P16[:4] + (choice,) + P16[5:])), "segment 1, word 4"),
                        ((first, SS.Segment(1, (Xor(var[0], var[1]),) + P16[1:4] + (choice,) + P16[5:])), "segment 1, word 4"),
                        ((SS.Segment(1, P16, (choice,) + (SS.PRIVATE,) * 7),), "segment 0, initial word 0")):
        with pytest.raises(ValueError, match=where + ": Choice words are not built on the 64-bit circuit yet"):
            SX.describe(12, SS.Plan(segs, ((0, 8),)))
    # the area counts: five one-block segments and 35 units are 8160 rows, 2^13 has 8171 usable; 36 units are 8192
    def area(units):
        xs = tuple(Xor(Var(t), Const(t)) for t in range(units)) + (SS.PRIVATE,) * (80 - units)
        return SS.Plan(tuple(SS.Segment(1, xs[16 * j: 16 * j + 16]) for j in range(5)), ((4, 8),))

    assert SX.rows_for(area(35)) == 5 * 1408 + 35 * 32 == 8160
    SX.describe(13, area(35))
    with pytest.raises(ValueError, match="5 segments and 36 xor units need 8192 rows"):
        SX.describe(13, area(36))


def test_bad_hmac_lengths_are_refused():
    for args in ((136, 0), (0, 8), (12, 0), (16, 4), (-8, 0), (8, -8), (7, 8)):
        with pytest.raises(ValueError, match="multiples of 8, the key from 8 to 128 bytes"):
            SX.hmac_sha512(*args)
    with pytest.raises(ValueError, match="variant"):
        SX.hmac_sha512(16, 8, variant=2)
    for name in ("HmacSha512Circuit", "HmacSha384Circuit", "Sha512XorSegmentsCircuit", "hmac_sha512"):
        assert getattr(api, name) is getattr(SX, name)


def test_lower_gives_the_units_and_their_readers():
    plan = two_segment_plan()
    low = SX.lower(plan)
    assert low.xors.dtype == np.uint32 and low.xors.shape == (2, 4) == (2, SC.XOR_WORDS)
    D = SS.SOURCE_DIGEST
    assert D == XM.SOURCE_DIGEST and SS.SOURCE_IV == XM.SOURCE_IV
    first_var = low.words_len - 1
    assert low.consts.tolist() == [0x5C5C5C5C5C5C5C5C] and low.shared_counts == (1, 0) and low.private_counts == [16, 13]
    assert low.xors.tolist() == [[D + 7, first_var, 0, 0], [0, first_var, 0, 0]]
    assert [low.sources[16 + t] for t in (0, 5, 9)] == [D + 8 * 2 + 0, D + 8 * 2 + 0, D + 8 * 2 + 1]
    assert low.seg_variant.tolist() == [SC.VARIANT_512, SC.VARIANT_384]
    none = SX.lower(SS.double_sha512(1))
    assert none.xors.shape == (0, 4) and none.xors.dtype == np.uint32


def test_the_hmac_plan_word_for_word():
    p = SX.hmac_sha512(16, 120, commit_key=True, variant=SC.VARIANT_384)
    inner, outer, commit = p.segments
    assert (inner.blocks, outer.blocks, commit.blocks) == (1 + 2, 2, 1) and SS.shared_counts(p) == (2, 0)
    assert {s.variant for s in p.segments} == {SC.VARIANT_384} and p.public == ((1, 6), (2, 6))
    assert inner.sources[:16] == (Xor(Var(0), Const(XM.IPAD)), Xor(Var(1), Const(XM.IPAD))) + (Const(XM.IPAD),) * 14
    assert inner.sources[16:31] == (SS.PRIVATE,) * 15 and [s.value for s in inner.sources[31:]] == SC.pad(bytes(248))[31:]
    assert outer.sources[:16] == (Xor(Var(0), Const(XM.OPAD)), Xor(Var(1), Const(XM.OPAD))) + (Const(XM.OPAD),) * 14
    assert outer.sources[16:22] == tuple(DW(0, i) for i in range(6)) and [s.value for s in outer.sources[22:]] == SC.pad(bytes(176))[22:]
    assert commit.sources[:2] == (Var(0), Var(1)) and [s.value for s in commit.sources[2:]] == SC.pad(bytes(16))[2:]
    q = SX.hmac_sha512(128, 0)
    assert q.public == ((1, 8),) and [s.value for s in q.segments[1].sources[24:]] == SC.pad(bytes(192))[24:] and q.segments[0].blocks == 2
    assert (SX.HMAC_IPAD, SX.HMAC_OPAD) == (XM.IPAD, XM.OPAD)


def test_the_rows_of_the_hmac_plans():
    """1344 rows per block, 64 per tail, 32 per unit: an HMAC whose message fits one block has 2 + 2 blocks, two tails and
    two units per key word."""
    for key_words in (1, 2, 8, 13, 16):
        assert SX.rows_for(SX.hmac_sha512(8 * key_words, 104)) == 4 * 1344 + 2 * 64 + 64 * key_words == 5504 + 2 * 32 * key_words
    assert SX.rows_for(SX.hmac_sha512(8, 112)) == 5504 + 64 + 1344  # 112 + 17 bytes no longer fit the second block
    assert SX.rows_for(SX.hmac_sha512(128, 104)) == 6528 <= SC.usable_rows(13)
    for key_bytes, more in ((8, 1408), (104, 1408), (112, 2752), (120, 2752), (128, 2752)):
        assert SX.rows_for(SX.hmac_sha512(key_bytes, 0, commit_key=True)) - SX.rows_for(SX.hmac_sha512(key_bytes, 0)) == more
    assert SX.rows_for(SX.hmac_sha512(104, 104, commit_key=True)) == 5504 + 64 * 13 + 1408 == 7744 <= SC.usable_rows(13)
    assert SC.usable_rows(13) < SX.rows_for(SX.hmac_sha512(128, 0, commit_key=True)) == 9280 <= SC.usable_rows(14)


@pytest.mark.parametrize("variant, name", [(SC.VARIANT_512, "sha512"), (SC.VARIANT_384, "sha384")])
@pytest.mark.parametrize("key_bytes, message_bytes", [(8, 0), (16, 8), (128, 112), (64, 240)])
def test_a_lowered_hmac_plan_gives_pythons_tag(variant, name, key_bytes, message_bytes):
    key, message = KEY[:key_bytes], (MESSAGE * 3)[:message_bytes]
    want = hmac.new(key, message, name).digest()
    plan = SX.hmac_sha512(key_bytes, message_bytes, True, variant)
    low = SX.lower(plan)
    values, shared = hmac_inputs(plan, key, message)
    states, results = XM.run_lowered(low, SS.word_buffer(low, values, shared))
    words = SC.DIGEST_WORDS[variant]
    assert SM.digest_bytes(states[1], words) == want and SM.digest_bytes(states[2], words) == hashlib.new(name, key).digest()
    assert len(low.xors) == 2 * (key_bytes // 8) == len(results)
    assert results == [w ^ pad for pad in (XM.IPAD, XM.OPAD) for w in words_of(key, XM.W)]
    assert plan.segments[0].blocks == 1 + -(-(message_bytes + 17) // 128)


# ---- 3. the model's witness against the description --------------------------------------------------------------------------

class Checked:
    """A plan, one witness of the model's for it, and what tests/witness_check_model.py needs."""

    def __init__(self, k, plan, values, shared, table_bits=12):
        self.k, self.plan, self.n, self.table_bits = k, plan, 1 << k, table_bits
        self.desc = d = SX.describe(k, plan, table_bits)
        self.cols, self.states, self.operands = XM.plan_witness(plan, values, shared, table_bits, self.n)
        self.instance = XM.instance_of(plan, self.states)
        self.circ = oracle_circuit(d.cs, k, lambda t: t)
        self.fixed = [[int(v) for v in d.fixed[name]] for name in d.fixed_names]
        N = 1 << table_bits
        self.tables = {"dense": list(range(N)), "spread": [spread(i) for i in range(N)]}
        perm = list(d.cs.permutation_columns)
        asm = PL.Assembly(self.n, perm)
        for (lc, lr), (rc, rr) in d.copies:
            asm.copy(lc, lr, rc, rr)
        self.mapping = asm.mapping
        self.x_perm = next(i for i, col in enumerate(perm) if KINDS[col.kind] == PL.ADVICE and col.index == XM.X)
        self.copies_only = CP.CqCircuit(k, d.cs.num_advice_columns, [], d.cs.num_fixed_columns, 1, [], self.circ.perm_columns,
                                        {PL.ADVICE: list(d.cs.advice_queries), PL.FIXED: list(d.cs.fixed_queries), PL.INSTANCE: list(d.cs.instance_queries)})

    def findings(self, cols=None):
        return WM.check_witness(self.circ, self.fixed, self.cols if cols is None else cols, [self.instance], self.mapping, self.tables)[1]

    def cycle(self, c, row):
        out, at = set(), (c, row)
        while at not in out:
            out.add(at)
            at = (int(self.mapping[at[0]][at[1]][0]), int(self.mapping[at[0]][at[1]][1]))
        return out

    def assert_names(self, row):
        """Bit 5 of column X at `row` flipped: a permutation finding at that cell and none outside its copy cycle."""
        cols = [list(c) if i == XM.X else c for i, c in enumerate(self.cols)]
        cols[XM.X][row] ^= 32
        found = WM.check_witness(self.copies_only, self.fixed, cols, [self.instance], self.mapping, self.tables)[1]
        assert all(kind == WM.PERMUTATION for kind, _, _, _ in found)
        found, cycle = {(c, r) for _, c, r, _ in found}, self.cycle(self.x_perm, row)
        assert (self.x_perm, row) in found and found <= cycle and len(cycle) > 1, (row, found)


def random_values(plan, seed):
    rng = random.Random(seed)
    return [[rng.getrandbits(64) for _ in range(count)] for count in SX.lower(plan).private_counts]


def test_one_unit_of_two_vars_is_satisfied():
    plan = one_unit_plan()
    x, y = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    case = Checked(11, plan, random_values(plan, 1), [x, y])
    assert case.operands == [(x, y)] and SX.rows_for(plan) == 1408 + 32 <= SC.usable_rows(11) < SX.rows_for(two_segment_plan())
    assert case.cols[XM.X][SM.message_row(0, 3)] == x ^ y == case.cols[XM.X][XM.unit_rows(plan, 0)[1] + XM.ROW["W"]]
    assert case.findings() == []
    # one bit of the unit's W cell: the gate is named, beside the word's own decomposition and the reader's copy
    u1 = XM.unit_rows(plan, 0)[1]
    cols = [list(c) if i == XM.X else c for i, c in enumerate(case.cols)]
    cols[XM.X][u1 + XM.ROW["W"]] ^= 1 << 40
    found = case.findings(cols)
    assert (WM.GATE, SC.GATES_XOR.index("xor_word"), u1, 0) in found
    assert {f[:3] for f in found} == {(WM.GATE, SC.GATES_XOR.index("xor_word"), u1), (WM.GATE, SC.GATES_XOR.index("w_word"), u1),
                                      (WM.PERMUTATION, case.x_perm, u1 + XM.ROW["W"]), (WM.PERMUTATION, case.x_perm, SM.message_row(0, 3))}


def test_one_var_as_both_operands_and_beside_a_constant_is_satisfied():
    plan = same_var_plan()
    case = Checked(11, plan, random_values(plan, 2), [0xDEADBEEF00C0FFEE])
    assert case.operands == [(0xDEADBEEF00C0FFEE,) * 2, (ONES, 0xDEADBEEF00C0FFEE)]
    assert case.cols[XM.X][SM.message_row(0, 0)] == 0 and case.cols[XM.X][SM.message_row(0, 1)] == ONES ^ 0xDEADBEEF00C0FFEE
    assert case.findings() == []


@pytest.mark.parametrize("table_bits", [11, 12, 16])
def test_edge_words_through_the_gate(table_bits):
    """At width 11 the sixth chunk holds the top 9 bits of the word; at width 16 chunks 4 and 5 start at or past bit 64."""
    plan = edges_plan()
    case = Checked(11, plan, random_values(plan, table_bits), [w for pair in EDGES for w in pair], table_bits)
    assert case.operands == EDGES
    for u, (x, y) in enumerate(EDGES):
        assert case.cols[XM.X][XM.unit_rows(plan, u)[1] + XM.ROW["W"]] == x ^ y == case.cols[XM.X][SM.message_row(0, u)]
    chunks = sorted((c for c, name in XM.M2.layout(XM.W) if name == "CHP_EVEN" and c.form == SC.FORM_PAIR and not c.len), key=lambda c: c.per_table_bits)
    u1 = XM.unit_rows(plan, 1)[1]  # ONES ^ 0: every chunk is full as far as the word reaches
    assert [case.cols[c.column][u1 + c.row] for c in chunks] == [(ONES >> (table_bits * i)) & ((1 << table_bits) - 1) for i in range(6)]
    assert case.cols[chunks[5].column][u1 + chunks[5].row] == {11: 0x1FF, 12: 0xF, 16: 0}[table_bits]
    assert case.findings() == []


@pytest.fixture(scope="module")
def two():
    plan = two_segment_plan()
    return Checked(12, plan, random_values(plan, 4), [0x0F0F0F0F12345678])


def test_a_digest_operand_read_twice_by_a_sha384_segment_is_satisfied(two):
    assert two.findings() == []
    assert two.operands == [(two.states[0][7], 0x0F0F0F0F12345678), (0x5C5C5C5C5C5C5C5C, 0x0F0F0F0F12345678)]
    assert XM.M2.levels(two.plan) == [0, 1] and len(two.instance) == 6
    values = random_values(two.plan, 4)
    words = [two.states[0][7] ^ 0x0F0F0F0F12345678] + values[1][:4] + [two.states[0][7] ^ 0x0F0F0F0F12345678] + values[1][4:7] + \
        [0x5C5C5C5C5C5C5C5C ^ 0x0F0F0F0F12345678] + values[1][7:]
    assert two.states[1] == SM.compress(words, 1, XM.M.IV[SC.VARIANT_384])[1][-1]


def test_a_changed_wired_cell_of_a_unit_is_a_permutation_finding_at_that_cell(two):
    plan = two.plan
    two.assert_names(SM.message_row(88, 5))                            # a reader's W cell
    two.assert_names(XM.unit_rows(plan, 0)[1] + XM.ROW["W"])           # ... and its unit's
    two.assert_names(XM.unit_rows(plan, 1)[0] + XM.ROW["E"])           # a Const operand's E cell
    two.assert_names(XM.unit_rows(plan, 0)[0] + XM.ROW["E"])           # a DigestWord operand's E cell
    two.assert_names(SM.tail_row(0, 1, 7))                             # ... and its producer
    two.assert_names(XM.unit_rows(plan, 1)[1] + XM.ROW["E"])           # the second operand cell of a Var
    two.assert_names(XM.unit_rows(plan, 0)[1] + XM.ROW["E"])           # ... and its first


@pytest.mark.parametrize("key_bytes, message_bytes, commit, variant, name", [
    (16, 8, False, SC.VARIANT_512, "sha512"), (128, 112, False, SC.VARIANT_384, "sha384"), (16, 8, True, SC.VARIANT_512, "sha512")])
def test_the_hmac_plans_are_satisfied_by_the_model_with_pythons_tag(key_bytes, message_bytes, commit, variant, name):
    key, message = KEY[:key_bytes], MESSAGE[:message_bytes]
    plan = SX.hmac_sha512(key_bytes, message_bytes, commit, variant)
    assert SC.usable_rows(12) < SX.rows_for(plan) <= SC.usable_rows(13)
    values, shared = hmac_inputs(plan, key, message)
    case = Checked(13, plan, values, shared)
    words = SC.DIGEST_WORDS[variant]
    want = hmac.new(key, message, name).digest() + (hashlib.new(name, key).digest() if commit else b"")
    assert struct.pack(f">{len(case.instance)}Q", *case.instance) == want and len(case.instance) == words * (2 if commit else 1)
    assert SM.digest_bytes(case.states[0], words) == hashlib.new(name, bytes(b ^ 0x36 for b in key.ljust(128, b"\0")) + message).digest()
    assert case.findings() == []
    case.instance[3] ^= 1
    assert [f[0] for f in case.findings()] == [WM.PERMUTATION] * 2  # the instance cell and the tail cell it is copied to
