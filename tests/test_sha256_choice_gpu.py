"""GPU: choice-wired message words -- Sha256MerklePathCircuit's device chains and choice cells give the pure-Python model's
witness cell for cell and hashlib's roots, the witness checker accepts them and names a bit that is not boolean and a cut
operand, proofs verify against the path's own root only, a bad choice table is refused before anything is launched, and
the new entry point without choices is the old one byte for byte."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import cq_verifier as CV
from oracle import plonk as PL
from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd._lib import constants
from sha2_on_cq_halo2_amd.api import FAIL_GATE, FAIL_PERMUTATION, Sha256MerklePathCircuit, Sha256SegmentsCircuit, fr_to_mont
from tests import sha256_choice_model as CM
from tests import sha256_circuit_model as M
from tests import sha256_segments_model as SM
from tests.sha2_model import words_of
from tests.sha_oracle import mont_column as _mont

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
ERR_ARG = constants()["CQ_ERR_ARG"]
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1


def node(i, salt=0):
    return hashlib.sha256(bytes([i, salt])).digest()


LEAF_MESSAGE = bytes((5 * i + 3) % 256 for i in range(41))
# name -> (constructor, depth, leaf_blocks, [per path (leaf, index, siblings)]); paths2: two lanes of one wave whose bits
# differ at every level
MAKE = {
    "path1": (lambda ctx: Sha256MerklePathCircuit(ctx, 11, 1, seed=SEED), 1, None, [(node(0), 0, [node(1)])]),
    "path1_right": (None, 1, None, [(node(0), 1, [node(1)])]),  # the same key, the other index
    "path3": (lambda ctx: Sha256MerklePathCircuit(ctx, 12, 3, seed=SEED), 3, None, [(node(0), 0b101, [node(i) for i in (1, 2, 3)])]),
    "path3_leaf": (lambda ctx: Sha256MerklePathCircuit(ctx, 12, 3, leaf_blocks=1, public_leaf=True, seed=SEED), 3, 1,
                   [(LEAF_MESSAGE, 0b011, [node(i, 1) for i in (1, 2, 3)])]),
    "paths2": (lambda ctx: Sha256MerklePathCircuit(ctx, 13, 3, paths=2, seed=SEED), 3, None,
               [(node(0, 2), 0b010, [node(i, 2) for i in (1, 2, 3)]), (node(0, 3), 0b101, [node(i, 3) for i in (1, 2, 3)])]),
}
KEY = {"path1_right": "path1"}


def leaf_of(name, item):
    return hashlib.sha256(item[0]).digest() if MAKE[name][2] else item[0]


def roots_of(name, items=None):
    return [CM.path_root(leaf_of(name, it), it[1], it[2]) for it in (items or MAKE[name][3])]


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(name):
        name = KEY.get(name, name)
        if name not in made:
            made[name] = MAKE[name][0](ctx)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", ["path1", "path1_right", "path3", "path3_leaf", "paths2"])
def test_synthesis_equals_the_model_and_roots_equal_hashlib(circuits, name):
    c, (_, depth, leaf_blocks, items) = circuits(name), MAKE[name]
    assert c.rows == {"path1": 1120, "path3": 3360, "path3_leaf": 3936, "paths2": 6720}[KEY.get(name, name)]
    assert SC.usable_rows(c.k - 1) < c.rows <= SC.usable_rows(c.k)  # the smallest k that holds the plan
    cols, inst = c.synthesize(items)
    values, shared, bits = CM.path_inputs(depth, items, leaf_blocks)
    assert c._inputs(items) == (values, [int(x) for x in shared], bits)
    want = CM.witness(c.plan, values, shared, bits, c.table_bits, c.n)
    assert any(want[Y][r] for r in range(c.n) if r % SC.REGION_ROWS in (SC.CHOICE_ROW_ZERO, SC.CHOICE_ROW_ONE, SC.CHOICE_ROW_BIT))
    for i, (got, exp) in enumerate(zip(cols, want)):
        assert np.array_equal(got.download((c.n, 4)), _mont(exp)), f"advice column {i}"
    assert c.digest_words == CM.digests(c.plan, values, shared, bits)
    assert c.roots == roots_of(name)
    public = ([leaf_of(name, it) for it in items] if leaf_blocks else [None] * len(items))
    expected = [w for leaf, root in zip(public, roots_of(name)) for d in (leaf, root) if d is not None for w in words_of(d)]
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(inst[0]))] == expected
    assert c.check(items) == (0, [])
    c.assert_satisfied(items)


def _oracle_expr(e):
    if e.op == "const":
        return PL.const(e.a)
    if e.op == "query":
        return (PL.adv, PL.fix, PL.inst)[e.a.kind](e.a.index, e.b)
    if e.op == "neg":
        return PL.neg(_oracle_expr(e.a))
    if e.op == "scale":
        return PL.scale(_oracle_expr(e.a), e.b)
    return (PL.add if e.op == "add" else PL.mul)(_oracle_expr(e.a), _oracle_expr(e.b))


def _verifier(c, seed):
    """The circuit's constraint system restated for the oracle's verifier -> verify(proof, instance words)."""
    cs = c.cs
    kinds = {GP.COL_ADVICE: PL.ADVICE, GP.COL_FIXED: PL.FIXED, GP.COL_INSTANCE: PL.INSTANCE}
    names = {id(c.dense): "dense", id(c.spread): "spread"}
    exprs = iter(cs._lookup_exprs)
    lookups = [[(_oracle_expr(next(exprs)), names[id(t)]) for _, t in lk] for lk in cs.static_lookups]
    queries = {PL.ADVICE: list(cs.advice_queries), PL.FIXED: list(cs.fixed_queries), PL.INSTANCE: list(cs.instance_queries)}
    circ = CP.CqCircuit(c.k, cs.num_advice_columns, lookups, cs.num_fixed_columns, 1, [_oracle_expr(g) for g in cs.gates],
                        [(kinds[col.kind], col.index) for col in cs.permutation_columns], queries)
    assert circ.degree() == cs.degree() and circ.blinding_factors() == cs.blinding_factors()
    assert cs.num_fixed_columns == len(SC.FIXED_CHOICE) and len(cs.gates) == len(SC.GATES_CHOICE) and len(cs.permutation_columns) == 4
    s = (seed * 0x9E3779B97F4A7C15 + 12345) % B.R_MOD
    N = 1 << c.table_bits
    tv = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
    fcm, pcm = c.pk.vk_commitments()

    def verify(proof, instance_words):
        return CV.verify_proof(proof, circ, c.vk_repr, s, tv, N, 1 << c.k, instances=[list(instance_words)],
                               fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))

    return verify


@pytest.mark.parametrize("name", ["path1", "path3_leaf"])
def test_proofs_verify_against_the_root_of_their_own_index_only(circuits, name):
    c, items = circuits(name), MAKE[name][3]
    proof, roots = c.prove(items, seed=7)
    assert len(proof) == c.pk.proof_size and roots == roots_of(name)
    assert c.prove(items, seed=7) == (proof, roots)
    verify = _verifier(c, SEED)
    leaf = words_of(leaf_of(name, items[0])) if MAKE[name][2] else []
    assert verify(proof, leaf + words_of(roots[0]))
    (message, index, siblings), = items
    (other,) = roots_of(name, [(message, index ^ 1, siblings)])  # the same leaf and siblings under another index
    assert other != roots[0] and not verify(proof, leaf + words_of(other))


def _write(c, column, row, value):
    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[column].ptr + 32 * row, v.ctypes.data, 32))


def _found(c):
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert total == len(fails) == len(found)
    return found


def _gate(name, row):
    return (FAIL_GATE, SC.GATES_CHOICE.index(name), row)


def test_a_bit_that_is_not_boolean_is_named(circuits):
    """path3, level 1 (bit 0), word 3: the bit cell overwritten with 2.  `choice_bit` at that region's row 0, and `choice`,
    which no longer holds (x != y there); the permutation findings are cells of that bit in column Y (permutation column
    3): the checker names a cell whose value differs from the cell it is mapped to, so on the bit's cycle of 16 cells it
    names the overwritten one and the one mapped to it."""
    c = circuits("path3")
    c.synthesize(MAKE["path3"][3])
    _, _, rb, base = CM.choice_cells(c.plan, 1, 3)
    _write(c, Y, rb, 2)
    found = _found(c)
    cycle = {(FAIL_PERMUTATION, 3, CM.choice_cells(c.plan, 1, t)[2]) for t in range(16)}
    assert {f for f in found if f[0] == FAIL_GATE} == {_gate("choice_bit", base), _gate("choice", base)}
    permutation = found - {_gate("choice_bit", base), _gate("choice", base)}
    assert (FAIL_PERMUTATION, 3, rb) in permutation and permutation <= cycle and len(permutation) == 2


def test_a_cut_digest_operand_is_named(circuits):
    """path3, level 2 (bit 1), word 13 = Choice(bit, sib_5, cur_5): the one operand -- digest word 5 of level 1, the operand
    taken -- changed in column Y.  Digest word 5 is read twice (word 5's zero operand too), so the wire is a cycle of three
    cells: the tail cell in X and the two operand cells in Y.  Named: the changed cell and the cell mapped to it, and
    `choice` at the region."""
    c = circuits("path3")
    c.synthesize(MAKE["path3"][3])
    assert c.plan.segments[2].sources[13].one == SS.DigestWord(1, 5)
    _, r1, _, base = CM.choice_cells(c.plan, 2, 13)
    tail = SC.REGION_ROWS * (SS.first_regions(c.plan)[1] + SC.BLOCK_REGIONS * 2 + 3 - 5 % 4) + 1  # digest word 5: tail region 2, E row
    _write(c, Y, r1, c.digest_words[1][5] ^ 1)
    found = _found(c)
    cycle = {(FAIL_PERMUTATION, 0, tail), (FAIL_PERMUTATION, 3, CM.choice_cells(c.plan, 2, 5)[0]), (FAIL_PERMUTATION, 3, r1)}
    permutation = found - {_gate("choice", base)}
    assert _gate("choice", base) in found and (FAIL_PERMUTATION, 3, r1) in permutation and permutation <= cycle and len(permutation) == 2


def test_a_bad_choice_table_is_refused_and_nothing_is_written(ctx, circuits):
    c = circuits("path3")
    n = c.n
    pattern = np.arange(4 * n, dtype=np.uint64).reshape(n, 4)
    c.cols[0].upload(pattern)
    c.cols[SC.ADVICE_COLUMNS - 1].upload(pattern)
    words = ctx.to_device(np.array(list(range(16)) + [0, 1], dtype=np.uint32))  # 16 words and two bits
    digests = ctx.alloc(64)
    arr = (C.c_void_p * SC.ADVICE_COLUMNS)(*[x.ptr for x in c.cols])
    blocks = np.array([1, 1], dtype=np.uint32)
    private, D, CH = list(range(16)), SS.SOURCE_DIGEST, SS.SOURCE_CHOICE
    good = [16, D + 3, 5, 0]

    def call(second, entries):
        sources = np.array(private + second, dtype=np.uint32)
        table = np.array(entries, dtype=np.uint32).reshape(-1, 4)
        return ctx.lib.cq_sha256_synthesize_choices_dev(ctx.h, c.table_bits, blocks.ctypes.data, 2, sources.ctypes.data, table.ctypes.data,
                                                        len(table), words.ptr, 18, n, arr, digests.ptr)

    one = private[:2] + [CH + 0] + private[3:]
    try:
        for second, entries, what in (
                (private[:2] + [CH + 1] + private[3:], [good], "segment 1, word 2"),          # a choice index >= n_choices
                (private[:2] + [CH + 0, CH + 0] + private[4:], [good], "segment 1, word 3"),  # an entry referenced twice
                (one, [good, good], "choice 1"),                                             # an entry referenced never
                (one, [[18, 0, 1, 0]], "segment 1, word 2"),                                  # the bit outside the buffer
                (one, [[16, 18, 1, 0]], "segment 1, word 2"),                                 # an operand outside the buffer
                (one, [[16, 0, CH + 0, 0]], "segment 1, word 2"),                             # an operand that is a choice: outside too
                (one, [[16, D + 8 * 1, 1, 0]], "segment 1, word 2"),                          # the digest of the segment itself
                (one, [[16, 1, D + 8 * 2 + 7, 0]], "segment 1, word 2")):                     # the digest of a later segment
            assert call(second, entries) == ERR_ARG
            assert what in ctx.lib.cq_last_error(ctx.h).decode()
        # the old entry point: a CHOICE-flagged source is a word index outside the buffer
        sources = np.array(private + one, dtype=np.uint32)
        assert ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, c.table_bits, blocks.ctypes.data, 2, sources.ctypes.data, words.ptr, 18, n, arr,
                                                         digests.ptr) == ERR_ARG
        assert "segment 1, word 2" in ctx.lib.cq_last_error(ctx.h).decode()
        ctx.sync()
        for i in (0, SC.ADVICE_COLUMNS - 1):
            assert np.array_equal(c.cols[i].download((n, 4)), pattern)
        assert call(one, [[17, D + 3, 5, 0]]) == 0  # and a good table goes through: bit 1 takes word 5
        ctx.sync()
        assert not np.array_equal(c.cols[0].download((n, 4)), pattern)
        _, base = SM.w_cell(SS.batch([1, 1]), 1, 2)
        y = c.cols[Y].download((n, 4))
        got_digests = digests.download((2, 8), np.uint32).tolist()
        cells = _mont([got_digests[0][3], 5, 1])  # the zero operand, the one operand, the bit
        assert np.array_equal(y[base + SC.CHOICE_ROW_ZERO: base + SC.CHOICE_ROW_BIT + 1], cells)
        assert np.array_equal(c.cols[X].download((n, 4))[base + 2], _mont([5])[0])
    finally:
        words.close()
        digests.close()


def test_no_choices_through_the_new_entry_point_is_the_old_one(ctx):
    """A one-segment all-Private plan: cq_sha256_synthesize_choices_dev with n_choices = 0 gives the columns and the proof
    bytes of cq_sha256_synthesize_segments_dev."""
    c = Sha256SegmentsCircuit(ctx, 11, SS.batch([2]), seed=SEED)
    try:
        message = bytes((7 * i + 40) % 256 for i in range(119))
        proof, digests = c.prove([SC.pad(message, 2)], seed=7)
        assert digests == [hashlib.sha256(message).digest()]
        old = [col.download((c.n, 4)) for col in c.cols]
        for col in c.cols:
            col.upload(np.zeros((c.n, 4), dtype=np.uint64))
        arr = (C.c_void_p * SC.ADVICE_COLUMNS)(*[col.ptr for col in c.cols])
        ctx._chk(ctx.lib.cq_sha256_synthesize_choices_dev(ctx.h, c.table_bits, c._seg_blocks.ctypes.data, 1, c._sources.ctypes.data, None, 0,
                                                          c._words.ptr, c._words_len, c.n, arr, c._digests.ptr))
        for i, (col, exp) in enumerate(zip(c.cols, old)):
            assert np.array_equal(col.download((c.n, 4)), exp), f"advice column {i}"
        assert c.pk.create_proof_dev([col.ptr for col in c.cols], seed=7, instances=c.instances) == proof
    finally:
        c.close()
