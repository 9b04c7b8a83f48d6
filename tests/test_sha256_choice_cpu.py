"""CPU: choice-wired message words -- merkle_path's description against the pure-Python model's witness for every leaf
position (every gate, lookup and copy) and its instance against hashlib's root of the full tree, what a broken bit, operand
or chosen word is reported as, what the choice variant of the constraint system must leave as it was, and the plans that
must be refused."""
import hashlib
import struct

import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_choice_model as CM
from tests import sha256_segments_model as SM
from tests.sha2_model import words_of

DEPTH, K = 3, 12
LEAF_MESSAGE = bytes((5 * i + 3) % 256 for i in range(41))
LEAVES = [hashlib.sha256(bytes([i])).digest() for i in range(1 << DEPTH)]


def tree_levels(leaves):
    """[leaves, their parents, ..., [root]] from hashlib."""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([hashlib.sha256(below[i] + below[i + 1]).digest() for i in range(0, len(below), 2)])
    return levels


def siblings_of(levels, index):
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


@pytest.fixture(scope="module")
def plain():
    """merkle_path(3): the description, and the full tree's root as merkle_tree(3)'s model gives it."""
    values = [words_of(LEAVES[2 * i] + LEAVES[2 * i + 1]) for i in range(4)] + [[]] * 3
    root = SM.instance_words(SS.merkle_tree(DEPTH), values)
    levels = tree_levels(LEAVES)
    assert root == words_of(levels[-1][0])
    plan = SS.merkle_path(DEPTH)
    return plan, SS.describe(K, plan), levels, root


@pytest.fixture(scope="module")
def honest(plain):
    """index 0b101 of merkle_path(3): inputs, the model witness and the instance."""
    plan, d, levels, root = plain
    values, shared, bits = CM.path_inputs(DEPTH, [(LEAVES[5], 5, siblings_of(levels, 5))])
    return values, shared, bits, CM.witness(plan, values, shared, bits, d.table_bits, 1 << K)


@pytest.mark.parametrize("index", range(1 << DEPTH))
def test_model_witness_satisfies_the_path_and_the_instance_is_the_trees_root(plain, index):
    plan, d, levels, root = plain
    item = (LEAVES[index], index, siblings_of(levels, index))
    assert words_of(CM.path_root(*item)) == root
    values, shared, bits = CM.path_inputs(DEPTH, [item])
    assert (len(shared), len(bits)) == SS.shared_counts(plan) == (8 * (DEPTH + 1), DEPTH)
    inst = CM.instance_words(plan, values, shared, bits)
    assert inst == root
    assert CM.findings(d, CM.witness(plan, values, shared, bits, d.table_bits, 1 << K), inst) == []


@pytest.mark.parametrize("index", range(1 << DEPTH))
def test_model_witness_with_a_hashed_public_leaf(index):
    leaves = list(LEAVES)
    leaves[index] = hashlib.sha256(LEAF_MESSAGE).digest()
    levels = tree_levels(leaves)
    plan = SS.merkle_path(DEPTH, leaf_blocks=1, public_leaf=True)
    assert SS.rows_for(plan) == 3936 and plan.public == (0, DEPTH)
    d = SS.describe(K, plan)
    values, shared, bits = CM.path_inputs(DEPTH, [(LEAF_MESSAGE, index, siblings_of(levels, index))], leaf_blocks=1)
    inst = CM.instance_words(plan, values, shared, bits)
    assert inst == words_of(leaves[index]) + words_of(levels[-1][0])
    assert CM.findings(d, CM.witness(plan, values, shared, bits, d.table_bits, 1 << K), inst) == []


def _copies_touching(d, column, row):
    return {i for i, (a, b) in enumerate(d.copies) if (column, row) in (a, b)}


def _gate(name, row):
    return ("gate", SC.GATES_CHOICE.index(name), row)


def test_a_bit_that_is_not_boolean(plain, honest):
    """Level 1, word 3: the bit cell set to 2.  x != y there, so W - x - 2 (y - x) is not zero either: `choice_bit` and
    `choice` at that region's row 0 and nothing else among the gates; the bit's first cell is word 0's, so the one copy
    that ties this cell to it."""
    plan, d, _, root = plain
    cols = [list(c) for c in honest[3]]
    Y = d.advice[2 * SC.PAIRS + 1]
    r0, r1, rb, base = CM.choice_cells(plan, 1, 3)
    first = CM.choice_cells(plan, 1, 0)[2]
    assert cols[Y.index][rb] == 0 and cols[Y.index][r0] != cols[Y.index][r1]
    cols[Y.index][rb] = 2
    (tie,) = _copies_touching(d, Y, rb)
    assert d.copies[tie] == ((Y, first), (Y, rb))
    assert set(CM.findings(d, cols, root)) == {_gate("choice_bit", base), _gate("choice", base), ("copy", tie, first)}
    # the bit's first cell: every other cell of the bit hangs on it
    cols[Y.index][rb] = 0
    cols[Y.index][first] = 2
    ties = _copies_touching(d, Y, first)
    assert len(ties) == 15 and all(d.copies[i][0] == (Y, first) for i in ties)
    base0 = CM.choice_cells(plan, 1, 0)[3]
    assert set(CM.findings(d, cols, root)) == {_gate("choice_bit", base0), _gate("choice", base0)} | {("copy", i, first) for i in ties}


def test_a_changed_sibling_operand(plain, honest):
    """Level 1, word 11 = Choice(bit, sib_3, cur_3) under bit 0: the zero operand is the sibling's word 3 and is the one
    taken.  Changed: the copy to the var's first cell (word 3's one operand) and `choice` at this region only."""
    plan, d, _, root = plain
    cols = [list(c) for c in honest[3]]
    Y = d.advice[2 * SC.PAIRS + 1]
    assert plan.segments[1].sources[11] == SS.Choice(1, SS.Var(16 + 3), SS.DigestWord(0, 3))
    r0, _, _, base = CM.choice_cells(plan, 1, 11)
    first = CM.choice_cells(plan, 1, 3)[1]
    cols[Y.index][r0] ^= 0x100
    (tie,) = _copies_touching(d, Y, r0)
    assert d.copies[tie] == ((Y, first), (Y, r0))
    assert set(CM.findings(d, cols, root)) == {("copy", tie, first), _gate("choice", base)}


def test_a_changed_chosen_word(plain, honest):
    """The W cell of level 2, word 5 (the sibling's word, taken under bit 1): `choice`, and the gates that read W."""
    plan, d, _, root = plain
    cols = [list(c) for c in honest[3]]
    X = d.advice[2 * SC.PAIRS]
    row, base = SM.w_cell(plan, 2, 5)
    assert _copies_touching(d, X, row) == set()  # a chosen word is wired through its operands only
    cols[X.index][row] ^= 0x10
    assert set(CM.findings(d, cols, root)) == {_gate("choice", base)} | SM.gates_reading_w(base, 5)


def test_a_cut_digest_operand(plain, honest):
    """Level 2, word 13 = Choice(bit, sib_5, cur_5) under bit 1: the one operand, digest word 5 of level 1, is the one taken
    and is tied to that segment's tail cell in X."""
    plan, d, _, root = plain
    cols = [list(c) for c in honest[3]]
    X, Y = d.advice[2 * SC.PAIRS], d.advice[2 * SC.PAIRS + 1]
    assert plan.segments[2].sources[13].one == SS.DigestWord(1, 5) and honest[2][2] == 1
    _, r1, _, base = CM.choice_cells(plan, 2, 13)
    cols[Y.index][r1] ^= 1
    (wire,) = _copies_touching(d, Y, r1)
    tail = SC.REGION_ROWS * (SS.first_regions(plan)[1] + SC.BLOCK_REGIONS * 2 + 3 - 5 % 4) + 1  # digest word 5: tail region 2, E row
    assert d.copies[wire] == ((X, tail), (Y, r1))
    assert set(CM.findings(d, cols, root)) == {("copy", wire, tail), _gate("choice", base)}


def test_what_the_choice_variant_leaves_as_it_was(plain):
    _, d, _, _ = plain
    base = SC._constraint_system(12, "dense", "spread")[0]
    assert (d.cs.blinding_factors(), d.cs.degree()) == (base.blinding_factors(), base.degree()) == (20, 4)
    assert SC.usable_rows(K) == (1 << K) - 21 and SC.max_blocks(K) == 7 and SC.rows_for(2) == 1120
    X, Y = d.advice[2 * SC.PAIRS], d.advice[2 * SC.PAIRS + 1]
    assert d.cs.permutation_columns == [X, d.fixed_columns["const"], d.instance, Y]
    assert d.fixed_names == SC.FIXED_CHOICE == SC.FIXED + ("q_choice",) and tuple(d.fixed) == SC.FIXED_CHOICE
    assert [c.index for c in d.fixed_columns.values()] == list(range(len(SC.FIXED_CHOICE)))
    assert SC.GATES_CHOICE == SC.GATES + ("choice", "choice_bit") and len(d.cs.gates) == len(SC.GATES_CHOICE)
    assert (SC.CHOICE_ROW_ZERO, SC.CHOICE_ROW_ONE, SC.CHOICE_ROW_BIT) == (4, 5, 6)
    # the choice gates read their own region only: no rotation of X the plain system lacks, Y stays below X
    per = lambda cs, col: sorted(r for c, r in cs.advice_queries if c == col.index)
    assert per(d.cs, X) == per(base, X) and len(per(d.cs, X)) == 18 and len(per(d.cs, Y)) < 18
    assert set(per(d.cs, Y)) - set(per(base, Y)) == {4, 5, 6}
    # one selected row per chosen word
    assert int(d.fixed["q_choice"].sum()) == 16 * DEPTH
    # a plan without a choice: the plain system, whatever else it holds
    for plan in (SS.merkle_tree(2), SS.Plan((SS.Segment(1, (SS.Var(0), SS.Var(0)) + (SS.PRIVATE,) * 14),), (0,))):
        p = SS.describe(K, plan)
        assert set(p.fixed) == set(SC.FIXED) and p.fixed_names == SC.FIXED and len(p.cs.gates) == len(SC.GATES)
        assert p.cs.permutation_columns == [X, p.fixed_columns["const"], p.instance]
    assert p.copies[-1] == ((X, SM.w_cell(plan, 0, 0)[0]), (X, SM.w_cell(plan, 0, 1)[0]))
    assert SC.describe(11, 2).fixed_names == SC.FIXED


def test_a_shared_word_as_a_message_word():
    """Var as a plain source beside a Choice that reads it: its W cell in X and the operand cell in Y are one var."""
    cur = tuple(SS.Var(t) for t in range(8))
    words = tuple(SS.Choice(0, SS.Var(t), SS.Var(8 + t)) for t in range(8)) + cur[::-1]
    plan = SS.Plan((SS.Segment(2, words + SS.PAD_64_BYTES),), (0,))
    d = SS.describe(11, plan)
    shared = list(range(100, 116))
    for bit in (0, 1):
        cols = CM.witness(plan, [[]], shared, [bit], d.table_bits, 1 << 11)
        inst = CM.instance_words(plan, [[]], shared, [bit])
        taken = shared[8:] if bit else shared[:8]
        assert inst == words_of(hashlib.sha256(struct.pack(">16I", *(taken + shared[7::-1]))).digest())
        assert CM.findings(d, cols, inst) == []
    X, Y = d.advice[2 * SC.PAIRS], d.advice[2 * SC.PAIRS + 1]
    assert ((Y, CM.choice_cells(plan, 0, 0)[0]), (X, SM.w_cell(plan, 0, 15)[0])) in d.copies


def test_plans_that_are_refused():
    var = tuple(SS.Var(t) for t in range(16))
    first = SS.Segment(1, (SS.PRIVATE,) * 16)

    def plan(word, at=2):
        return SS.Plan((first, SS.Segment(1, var[:at] + (word,) + var[at + 1:])), (1,))

    SS.describe(K, plan(SS.Choice(0, SS.Var(0), SS.DigestWord(0, 7))))
    for bad in (SS.Var(-1), SS.Choice(-1, var[0], var[1]), SS.Choice(0, SS.Var(-2), var[1]), SS.Choice(0, var[0], SS.Var(-2)),
                SS.Choice(0, SS.PRIVATE, var[1]), SS.Choice(0, var[0], SS.Const(1)), SS.Choice(0, var[0], SS.Choice(0, var[0], var[1])),
                SS.Choice(0, 7, var[1]), SS.Choice(0, SS.DigestWord(1, 0), var[1]), SS.Choice(0, var[0], SS.DigestWord(2, 0)),
                SS.Choice(0, var[0], SS.DigestWord(-1, 0)), SS.Choice(0, var[0], SS.DigestWord(0, 8))):
        with pytest.raises(ValueError, match="segment 1, word 2"):
            SS.describe(K, plan(bad))
    for args in ((0,), (3, 0)):
        with pytest.raises(ValueError):
            SS.merkle_path(*args)
    with pytest.raises(ValueError):
        SS.merkle_path(2, public_leaf=True)
    with pytest.raises(ValueError, match="3360 rows"):
        SS.describe(11, SS.merkle_path(DEPTH))


def test_the_path_builder():
    p = SS.merkle_path(2, paths=2, leaf_blocks=3, public_leaf=True)
    assert [s.blocks for s in p.segments] == [3, 2, 2, 3, 2, 2] and p.public == (0, 2, 3, 5)
    assert SS.shared_counts(p) == (32, 4)
    second = p.segments[4].sources  # path 1, level 0: bit 2, the leaf segment's digest against vars 16 .. 23
    assert second[:8] == tuple(SS.Choice(2, SS.DigestWord(3, t), SS.Var(16 + t)) for t in range(8))
    assert second[8:16] == tuple(SS.Choice(2, SS.Var(16 + t), SS.DigestWord(3, t)) for t in range(8))
    assert second[16:] == SS.PAD_64_BYTES
    top = p.segments[5].sources
    assert top[3] == SS.Choice(3, SS.DigestWord(4, 3), SS.Var(24 + 3)) and top[8 + 3] == SS.Choice(3, SS.Var(24 + 3), SS.DigestWord(4, 3))
    q = SS.merkle_path(1)
    assert q.public == (0,) and q.segments[0].sources[0] == SS.Choice(0, SS.Var(0), SS.Var(8))
