"""CPU: wired SHA-512 segments -- the plan types, their descriptions and lowering (no device; the built library for
cq_sha512_layout only), the model against hashlib, and the model's witness against the constraint system through
tests/witness_check_model.py: clean as it is, a permutation finding at every wired cell that is changed."""
import hashlib
import random
import struct

import numpy as np
import pytest

from oracle import cq_prover as CP
from oracle import plonk as PL
from sha2_on_cq_halo2_amd import api
from sha2_on_cq_halo2_amd import sha256_segments as S256
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from tests import sha512_circuit_model as M
from tests import sha512_segments_model as SM
from tests import witness_check_model as WM
from tests.sha_oracle import KINDS, oracle_circuit

P16 = (SS.PRIVATE,) * 16
ROWS_1, ROWS_2 = 1408, 2752


def rand_words(rng, count):
    return [rng.getrandbits(64) for _ in range(count)]


def same_description(a, b):
    assert a.copies == b.copies and a.fixed_names == b.fixed_names and a.blocks_list == b.blocks_list and a.variants == b.variants
    assert all(np.array_equal(a.fixed[name], b.fixed[name]) for name in a.fixed_names)


# ---- 1. descriptions do not move ---------------------------------------------------------------------------------------------

def test_the_batch_plan_is_describe_batch():
    variants = [SC.VARIANT_512, SC.VARIANT_384]
    same_description(SS.describe(13, SS.batch([1, 2], variants)), SC.describe_batch(13, [1, 2], variants))
    same_description(SS.describe(13, SS.batch([1, 2])), SC.describe_batch(13, [1, 2]))


def test_a_pinned_sha384_initial_value_is_the_sha384_description():
    plan = SS.Plan((SS.Segment(1, P16, tuple(SS.Const(v) for v in SC.IV384)),), ((0, 6),))
    got, want = SS.describe(11, plan), SC.describe(11, 1, variant=SC.VARIANT_384)
    assert got.copies == want.copies and all(np.array_equal(got.fixed[name], want.fixed[name]) for name in want.fixed_names)


def test_sizes():
    assert SC.rows_for(1) == ROWS_1 and SC.rows_for(2) == ROWS_2 and SC.usable_rows(12) == (1 << 12) - 21
    cs = SS.describe(12, SS.double_sha512(1)).cs
    assert len(cs.gates) == 23 and len(cs.static_lookups) == 16 and cs.blinding_factors() == 20
    SS.describe(12, SS.double_sha512(1)), SS.describe(14, SS.merkle_tree(2)), SS.describe(11, SS.midstate(1)), SS.describe(11, SS.sha512_256(1))
    for k, plan in ((11, SS.double_sha512(1)), (13, SS.merkle_tree(2)), (10, SS.midstate(1)), (10, SS.sha512_256(1))):
        with pytest.raises(ValueError, match="usable"):
            SS.describe(k, plan)


def test_builders_and_exports():
    d = SS.double_sha512(2)
    assert d.public == ((1, 8),) and d.segments[1].sources == tuple(SS.DigestWord(0, i) for i in range(8)) + (SS.Const(1 << 63),) + (SS.Const(0),) * 6 + (SS.Const(512),)
    t = SS.merkle_tree(2)
    assert [s.blocks for s in t.segments] == [2, 2, 2] and t.public == ((2, 8),)
    assert t.segments[2].sources[:16] == tuple(SS.DigestWord(s, w) for s in (0, 1) for w in range(8))
    assert t.segments[0].sources[16:] == (SS.Const(1 << 63),) + (SS.Const(0),) * 14 + (SS.Const(1024),)
    assert [len(SS.merkle_tree(d).segments) for d in (1, 3)] == [1, 7] and SS.merkle_tree(3).segments[6].sources[0] == SS.DigestWord(4, 0)
    m = SS.midstate(2)
    assert m.public == ((0, 8),) and m.public_init == (0,) and m.segments[0].init == (SS.PRIVATE,) * 8
    s = SS.sha512_256(1)
    assert s.public == ((0, 4),) and s.segments[0].variant == SC.VARIANT_512
    assert (SS.Private, SS.Const, SS.DigestWord, SS.Var) == (S256.Private, S256.Const, S256.DigestWord, S256.Var)
    for name in ("batch", "double_sha512", "merkle_tree", "midstate", "sha512_256", "Sha512SegmentsCircuit", "Sha512dCircuit",
                 "Sha512MerkleCircuit", "Sha512MidstateCircuit", "Sha512_256Circuit"):
        assert getattr(api, name) is getattr(SS, name)


def test_the_sha512_256_initial_value_is_generated():
    """FIPS 180-4, 5.3.6: the package's constant is what the model generates, and the model's SHA-512 is hashlib's."""
    assert list(SS.IV512_256) == SM.IV512_256 == [c.value for c in SS.sha512_256(1).segments[0].init]
    assert SM.compress(SC.pad(b"SHA-512/256", 1), 1, M.IV[SC.VARIANT_512])[1][-1] == list(struct.unpack(">8Q", hashlib.sha512(b"SHA-512/256").digest()))
    abc = SM.compress(SC.pad(b"abc", 1), 1, SM.IV512_256)[1][-1]
    assert SM.digest_bytes(abc, 4).hex() == "53048e2681941ef99b2e29b76b4c7dabe4c2d0c634fc6d46e0e2f13107e7af23" == hashlib.new("sha512_256", b"abc").hexdigest()


# ---- 2. _check_plan, lower, word_buffer --------------------------------------------------------------------------------------

D0 = SS.DigestWord(0, 0)


@pytest.mark.parametrize("plan, names", [
    (SS.Plan((), ((0, 8),)), ("at least one segment",)),
    (SS.Plan((SS.Segment(0, ()),), ((0, 8),)), ("segment 0", "0 blocks")),
    (SS.Plan((SS.Segment(1, P16[:15]),), ((0, 8),)), ("segment 0", "15 word sources")),
    (SS.Plan((SS.Segment(1, P16, None, 2),), ((0, 8),)), ("segment 0", "variant")),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 7),), ((0, 8),)), ("segment 0", "8 words")),
    (SS.Plan((SS.Segment(1, (D0,) + P16[1:]),), ((0, 8),)), ("segment 0, word 0", "does not come before")),
    (SS.Plan((SS.Segment(1, P16), SS.Segment(1, P16[:5] + (SS.DigestWord(1, 0),) + P16[6:])), ((0, 8),)), ("segment 1, word 5", "does not come before")),
    (SS.Plan((SS.Segment(1, P16), SS.Segment(1, P16[:5] + (SS.DigestWord(0, 8),) + P16[6:])), ((0, 8),)), ("segment 1, word 5", "words 0 .. 7")),
    (SS.Plan((SS.Segment(1, P16), SS.Segment(1, P16, (SS.PRIVATE,) * 3 + (SS.DigestWord(1, 0),) + (SS.PRIVATE,) * 4)), ((0, 8),)),
     ("segment 1, initial word 3", "does not come before")),
    (SS.Plan((SS.Segment(1, P16[:3] + (SS.Var(-1),) + P16[4:]),), ((0, 8),)), ("segment 0, word 3", "negative")),
    (SS.Plan((SS.Segment(1, P16, (SS.Var(-2),) + (SS.PRIVATE,) * 7),), ((0, 8),)), ("segment 0, initial word 0", "negative")),
    (SS.Plan((SS.Segment(1, P16[:3] + (SS.Const(1 << 64),) + P16[4:]),), ((0, 8),)), ("segment 0, word 3", "64-bit")),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 7 + (SS.Const(-1),)),), ((0, 8),)), ("segment 0, initial word 7", "64-bit")),
    (SS.Plan((SS.Segment(1, P16[:9] + (S256.Choice(0, SS.Var(0), SS.Var(1)),) + P16[10:]),), ((0, 8),)), ("segment 0, word 9", "Choice", "not built on the 64-bit circuit yet")),
    (SS.Plan((SS.Segment(1, P16[:9] + (S256.Xor(SS.Var(0), SS.Const(1)),) + P16[10:]),), ((0, 8),)), ("segment 0, word 9", "Xor", "not built on the 64-bit circuit yet")),
    (SS.Plan((SS.Segment(1, P16, (S256.Xor(SS.Var(0), SS.Const(1)),) + (SS.PRIVATE,) * 7),), ((0, 8),)), ("segment 0, initial word 0", "not built")),
    (SS.Plan((SS.Segment(1, P16[:9] + (7,) + P16[10:]),), ((0, 8),)), ("segment 0, word 9", "a source is")),
    (SS.Plan((SS.Segment(1, P16),), ()), ("public", "at least one")),
    (SS.Plan((SS.Segment(1, P16),), (0,)), ("public", "(segment, words)")),
    (SS.Plan((SS.Segment(1, P16),), ((1, 8),)), ("public", "below 1")),
    (SS.Plan((SS.Segment(1, P16),), ((0, 8), (0, 4))), ("public", "none twice")),
    (SS.Plan((SS.Segment(1, P16),), ((0, 0),)), ("public", "1 .. 8")),
    (SS.Plan((SS.Segment(1, P16),), ((0, 9),)), ("public", "1 .. 8")),
    (SS.Plan((SS.Segment(1, P16),), ((0, 8),), (0,)), ("public_init",)),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 8),), ((0, 8),), (0, 0)), ("public_init",)),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 8),), ((0, 8),), (1,)), ("public_init",)),
])
def test_check_plan_names_what_is_wrong(plan, names):
    with pytest.raises(ValueError) as e:
        SS.describe(13, plan)
    assert all(name in str(e.value) for name in names), str(e.value)
    with pytest.raises(ValueError):
        SS.lower(plan)


def test_describe_rejects_a_table_width_out_of_range():
    for tb in (SC.MIN_TABLE_BITS - 1, SC.MAX_TABLE_BITS + 1):
        with pytest.raises(ValueError, match="table_bits"):
            SS.describe(13, SS.sha512_256(1), tb)


mixed_plan = SM.mixed_plan


def test_lower_and_word_buffer_round_trip():
    plan = mixed_plan()
    low = SS.lower(plan)
    assert low.consts.dtype == np.uint64 and low.consts.tolist() == [5, 1 << 63, (1 << 64) - 1]
    assert low.seg_blocks.tolist() == [1, 1, 2] and low.seg_variant.tolist() == [SC.VARIANT_512, SC.VARIANT_384, SC.VARIANT_512]
    assert low.private_counts == [14, 16, 1 + 13 + 15] and low.var_count == 2 and low.words_len == 3 + 59 + 2
    first_var = 3 + 59
    assert low.sources[:3].tolist() == [first_var + 1, 0, 3] and low.sources[3:16].tolist() == list(range(4, 17))
    assert low.init_sources[:16].tolist() == [SS.SOURCE_IV] * 16 and SS.SOURCE_IV == 0xFFFFFFFF and SS.SOURCE_DIGEST == 1 << 31
    D = SS.SOURCE_DIGEST
    assert low.init_sources[16:].tolist() == [D + 7, D + 8 + 6, first_var, 1, 33, D + 8, first_var + 1, 0]  # its Private initial word first
    assert low.sources[32:35].tolist() == [D + 15, first_var + 1, 2] and low.sources[35] == 34 and low.sources[-1] == D + 3
    rng = random.Random(1)
    values, shared = [rand_words(rng, c) for c in low.private_counts], rand_words(rng, 2)
    buf = SS.word_buffer(low, values, shared)
    assert buf.dtype == np.uint64 and len(buf) == low.words_len
    # the round trip: every source that is no digest reads the word the plan says
    want = {}
    for j, seg in enumerate(plan.segments):
        private = iter(values[j])
        for src, s in zip(tuple(seg.init or ()) + tuple(seg.sources),
                          (low.init_sources[8 * j: 8 * j + 8].tolist() if seg.init else []) + low.sources[16 * sum(low.seg_blocks[:j].tolist()):].tolist()):
            if isinstance(src, SS.DigestWord):
                assert s == D + 8 * src.segment + src.word
            else:
                value = next(private) if isinstance(src, SS.Private) else src.value if isinstance(src, SS.Const) else shared[src.index]
                assert int(buf[s]) == value
                assert want.setdefault(s, value) == value
    assert sorted(want) == list(range(low.words_len))
    for bad_values, bad_shared in ((values[:2], shared), (values, shared[:1]), ([v[:-1] for v in values], shared), (values, [1 << 64, 0])):
        with pytest.raises(ValueError):
            SS.word_buffer(low, bad_values, bad_shared)
    assert SS.lower(SS.double_sha512(1)).init_sources.tolist() == [SS.SOURCE_IV] * 16


def test_copies_of_the_mixed_plan():
    plan = mixed_plan()
    d = SS.describe(13, plan)
    Xc, inst, const = d.advice[SM.X], d.instance, d.fixed_columns["const"]
    f = SS.first_regions(plan)
    assert f == [0, 88, 176]
    own = SC.describe_batch(13, [1, 1, 2], [0, 1, 0]).copies
    # every segment's round-constant copies and the initial hash values of segments 0 and 1 stay; the instance rows are the plan's
    in_order = lambda words: [h for i in range(4) for h in (3 - i, 7 - i) if h < words]  # region after region, A row then E row
    assert [c for c in d.copies if c[0][0] == inst] == (
        [((inst, 5 + 6 + 0), (Xc, SM.tail_row(f[0], 1, 0)))]
        + [((inst, 5 + h), (Xc, SM.tail_row(f[1], 1, h))) for h in in_order(6)]
        + [((inst, h), (Xc, SM.tail_row(f[2], 2, h))) for h in in_order(5)]
        + [((inst, 12 + i), (Xc, SM.state_row(f[2], i))) for i in range(8)])
    # segment 2's pinned initial words are copies of the cells an initial hash value is pinned to; its other six are gone
    gone = [c for c in own if c not in d.copies and c[0][0] != inst]
    assert gone == [((const, SM.state_row(f[2], h)), (Xc, SM.state_row(f[2], h))) for h in in_order(8) if h not in (3, 7)]
    tail = [c for c in d.copies if c not in own and c[0][0] != inst]
    assert tail == [
        ((const, SM.message_row(f[0], 1)), (Xc, SM.message_row(f[0], 1))),
        ((Xc, SM.tail_row(f[1], 1, 7)), (Xc, SM.message_row(f[2], 0))),
        ((const, SM.message_row(f[2], 2)), (Xc, SM.message_row(f[2], 2))),
        ((Xc, SM.tail_row(f[0], 1, 3)), (Xc, SM.message_row(f[2], 31))),
        ((Xc, SM.message_row(f[0], 0)), (Xc, SM.message_row(f[2], 1))),                      # Var 1: its later message cell
        ((Xc, SM.tail_row(f[0], 1, 7)), (Xc, SM.state_row(f[2], 0))), ((Xc, SM.tail_row(f[1], 1, 6)), (Xc, SM.state_row(f[2], 1))),
        ((Xc, SM.tail_row(f[1], 1, 0)), (Xc, SM.state_row(f[2], 5))),
        ((Xc, SM.message_row(f[0], 0)), (Xc, SM.state_row(f[2], 6))),                        # Var 1: its state cell; Var 0 stands once
    ]
    assert int(d.fixed["const"][SM.state_row(f[2], 3)]) == 1 << 63 and int(d.fixed["const"][SM.message_row(f[2], 2)]) == (1 << 64) - 1


# ---- 3. the model's witness and the constraint system ------------------------------------------------------------------------

class Checked:
    """A plan, one witness of the model's for it at the smallest k, and what tests/witness_check_model.py needs."""

    def __init__(self, k, plan, seed, values=None, shared=()):
        rng = random.Random(seed)
        self.k, self.plan, self.n, self.shared = k, plan, 1 << k, list(shared)
        self.desc = d = SS.describe(k, plan)
        low = SS.lower(plan)
        self.values = [rand_words(rng, c) for c in low.private_counts] if values is None else values
        self.cols, self.states, self.inits, self.instance = SM.plan_witness(plan, self.values, self.shared, 12, self.n)
        self.circ = oracle_circuit(d.cs, k, lambda t: t)
        self.fixed = [[int(v) for v in d.fixed[name]] for name in d.fixed_names]
        N = 1 << 12
        self.tables = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
        perm = list(d.cs.permutation_columns)
        asm = PL.Assembly(self.n, perm)
        for (lc, lr), (rc, rr) in d.copies:
            asm.copy(lc, lr, rc, rr)
        self.mapping = asm.mapping
        self.x_perm = next(i for i, col in enumerate(perm) if KINDS[col.kind] == PL.ADVICE and col.index == SM.X)
        self.inst_perm = next(i for i, col in enumerate(perm) if KINDS[col.kind] == PL.INSTANCE)
        # the same circuit without gates and lookups: what a changed cell does to the copies alone
        self.copies_only = CP.CqCircuit(k, d.cs.num_advice_columns, [], d.cs.num_fixed_columns, 1, [], self.circ.perm_columns,
                                        {PL.ADVICE: list(d.cs.advice_queries), PL.FIXED: list(d.cs.fixed_queries), PL.INSTANCE: list(d.cs.instance_queries)})
        assert self.copies_only.blinding_factors() == self.circ.blinding_factors()

    def findings(self):
        return WM.check_witness(self.circ, self.fixed, self.cols, [self.instance], self.mapping, self.tables)[1]

    def cycle(self, c, row):
        out, at = set(), (c, row)
        while at not in out:
            out.add(at)
            at = (int(self.mapping[at[0]][at[1]][0]), int(self.mapping[at[0]][at[1]][1]))
        return out

    def copy_findings(self, row=None, instance_row=None):
        """The permutation findings with bit 5 of one cell flipped: column X at `row`, or the instance at `instance_row`."""
        cols, instance = [list(c) if i == SM.X else c for i, c in enumerate(self.cols)], list(self.instance)
        if row is not None:
            cols[SM.X][row] ^= 32
        else:
            instance[instance_row] ^= 32
        found = WM.check_witness(self.copies_only, self.fixed, cols, [instance], self.mapping, self.tables)[1]
        assert all(kind == WM.PERMUTATION for kind, _, _, _ in found)
        return {(c, r) for _, c, r, _ in found}


def hash_words(name, data):
    d = hashlib.new(name, data).digest()
    return list(struct.unpack(f">{len(d) // 8}Q", d))


LEAVES = [bytes((37 * i + 11 * j) % 256 for j in range(64)) for i in range(4)]
DOUBLE_MSG, S256_MSG = b"the quick brown fox", bytes(range(111))
MID_DATA = bytes((5 * i + 1) % 256 for i in range(128))


@pytest.fixture(scope="module")
def double():
    return Checked(12, SS.double_sha512(1), 1, [SC.pad(DOUBLE_MSG, 1), []])


@pytest.fixture(scope="module")
def merkle():
    return Checked(14, SS.merkle_tree(2), 2, [list(struct.unpack(">16Q", LEAVES[0] + LEAVES[1])), list(struct.unpack(">16Q", LEAVES[2] + LEAVES[3])), []])


@pytest.fixture(scope="module")
def mid():
    h_in = SM.compress(SC.pad(b"x" * 128, 2)[:16], 1, M.IV[SC.VARIANT_512])[1][-1]
    return Checked(11, SS.midstate(1), 3, [h_in + list(struct.unpack(">16Q", MID_DATA))])


@pytest.fixture(scope="module")
def s256():
    return Checked(11, SS.sha512_256(1), 4, [SC.pad(S256_MSG, 1)])


@pytest.fixture(scope="module")
def mixed():
    return Checked(13, mixed_plan(), 5, None, [0x0123456789ABCDEF, (1 << 64) - 2])


def test_double_sha512_is_satisfied_and_is_hashlib(double):
    assert double.findings() == []
    assert double.instance == hash_words("sha512", hashlib.sha512(DOUBLE_MSG).digest()) and len(double.instance) == 8
    assert double.states[0] == hash_words("sha512", DOUBLE_MSG) and SM.levels(double.plan) == [0, 1]


def test_merkle_tree_is_satisfied_and_is_hashlib(merkle):
    assert merkle.findings() == []
    node = lambda a, b: hashlib.sha512(a + b).digest()
    assert SM.digest_bytes(merkle.instance) == node(node(LEAVES[0], LEAVES[1]), node(LEAVES[2], LEAVES[3]))
    assert SM.levels(merkle.plan) == [0, 0, 1] and SM.levels(SS.merkle_tree(3)) == [0] * 4 + [1] * 2 + [2]


def test_midstate_is_satisfied_and_continues_hashlib(mid):
    assert mid.findings() == []
    assert mid.instance[8:] == mid.values[0][:8] and len(mid.instance) == 16
    # the state after the first block of a 2-block message, then its second block: hashlib's digest of the whole
    msg = b"x" * 128 + MID_DATA[:100]
    words = SC.pad(msg, 2)
    out = SM.compress(words[16:], 1, mid.values[0][:8])[1][-1]
    assert out == hash_words("sha512", msg)
    assert mid.instance[:8] == SM.compress(list(struct.unpack(">16Q", MID_DATA)), 1, mid.values[0][:8])[1][-1]


def test_sha512_256_is_satisfied_and_is_hashlib(s256):
    assert s256.findings() == []
    assert s256.instance == hash_words("sha512_256", S256_MSG) and len(s256.instance) == 4


def test_word_4_of_a_sha512_256_digest_is_on_no_instance_copy(s256):
    inst = s256.desc.instance
    assert sorted(c[0][1] for c in s256.desc.copies if c[0][0] == inst) == [0, 1, 2, 3]
    for word in range(4, 8):
        row = SM.tail_row(0, 1, word)
        assert s256.cycle(s256.x_perm, row) == {(s256.x_perm, row)} and s256.copy_findings(row=row) == set()
    assert (s256.x_perm, SM.tail_row(0, 1, 3)) in s256.copy_findings(row=SM.tail_row(0, 1, 3))


def test_the_mixed_plan_is_satisfied(mixed):
    assert mixed.findings() == []
    assert SM.levels(mixed.plan) == [0, 0, 1] and len(mixed.instance) == 5 + 6 + 1 + 8


def assert_names(case, row=None, instance_row=None):
    """Changing the cell gives a permutation finding at that cell and none outside its copy cycle."""
    cell = (case.x_perm, row) if row is not None else (case.inst_perm, instance_row)
    found = case.copy_findings(row, instance_row)
    assert cell in found and found <= case.cycle(*cell) and len(case.cycle(*cell)) > 1, (cell, found)


def test_a_changed_wired_cell_is_a_permutation_finding_at_that_cell(double, merkle, mid, s256, mixed):
    f = SS.first_regions(mixed.plan)
    assert_names(mixed, row=SM.message_row(f[2], 0))        # a DigestWord message word
    assert_names(mixed, row=SM.tail_row(f[1], 1, 7))        # ... and its producer, word 7 of a SHA-384 segment
    assert_names(mixed, row=SM.message_row(f[2], 2))        # a Const word
    assert_names(mixed, row=SM.message_row(f[2], 1))        # the second cell of a Var
    assert_names(mixed, row=SM.state_row(f[2], 6))          # ... and its third, an initial word
    assert_names(mixed, row=SM.state_row(f[2], 0))          # a digest-wired initial word
    assert_names(mixed, row=SM.state_row(f[2], 3))          # a Const initial word
    assert_names(mixed, row=SM.tail_row(f[2], 2, 4))        # a public word
    assert_names(mixed, instance_row=4)
    assert_names(mixed, instance_row=12 + 4)                # a public initial word that is Private otherwise
    assert_names(double, row=SM.message_row(88, 3)), assert_names(double, row=SM.message_row(88, 15)), assert_names(double, instance_row=7)
    assert_names(merkle, row=SM.message_row(2 * 172, 9)), assert_names(merkle, row=SM.message_row(172, 16))
    assert_names(mid, row=SM.state_row(0, 5)), assert_names(mid, instance_row=0)
    assert_names(s256, row=SM.state_row(0, 2)), assert_names(s256, instance_row=3)


def test_a_changed_private_word_is_no_permutation_finding(double, mixed):
    f = SS.first_regions(mixed.plan)
    for case, row in ((double, SM.message_row(0, 4)), (mixed, SM.message_row(f[0], 2)), (mixed, SM.message_row(f[2], 20)),
                      (mixed, SM.tail_row(f[2], 2, 5)), (mixed, SM.tail_row(f[0], 1, 1))):
        assert case.cycle(case.x_perm, row) == {(case.x_perm, row)} and case.copy_findings(row=row) == set()
