"""CPU: plans of wired SHA-256 segments -- their descriptions against the pure-Python model's witness (every gate, lookup
and copy), the instance against hashlib, what a broken wire is reported as, and the plans that must be refused."""
import hashlib

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha256_circuit_model as M
from tests import sha256_segments_model as SM
from tests.sha2_model import message, words_of


LEAVES = [hashlib.sha256(bytes([i])).digest() for i in range(4)]
BATCH_MESSAGES = [b"", message(119, 3), b"\xff" * 55]
D_MESSAGE = message(55, 1)


def _case(name):
    """(k, plan, values, expected public digests) of the three plans the GPU tests use too."""
    if name == "batch":
        plan = SS.batch([1, 2, 1])
        values = [SC.pad(m, b) for m, b in zip(BATCH_MESSAGES, (1, 2, 1))]
        return 12, plan, values, [hashlib.sha256(m).digest() for m in BATCH_MESSAGES]
    if name == "double":
        return 11, SS.double_sha256(1), [SC.pad(D_MESSAGE, 1), []], [hashlib.sha256(hashlib.sha256(D_MESSAGE).digest()).digest()]
    left, right = hashlib.sha256(LEAVES[0] + LEAVES[1]).digest(), hashlib.sha256(LEAVES[2] + LEAVES[3]).digest()
    values = [words_of(LEAVES[0] + LEAVES[1]), words_of(LEAVES[2] + LEAVES[3]), []]
    return 12, SS.merkle_tree(2), values, [hashlib.sha256(left + right).digest()]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in ("batch", "double", "merkle"):
        k, plan, values, public = _case(name)
        d = SS.describe(k, plan)
        out[name] = (d, plan, values, public, SM.witness(plan, values, d.table_bits, 1 << k), SM.instance_words(plan, values))
    return out


@pytest.mark.parametrize("name", ["batch", "double", "merkle"])
def test_model_witness_satisfies_the_plan_and_the_instance_is_hashlib(cases, name):
    d, plan, values, public, cols, inst = cases[name]
    assert inst == [w for digest in public for w in words_of(digest)]
    assert M.findings(d, cols, inst) == []
    assert SS.rows_for(plan) == sum(544 * s.blocks + 32 for s in plan.segments)
    assert d.blocks == tuple(s.blocks for s in plan.segments)


def _copy_index(d, left, right):
    (i,) = [i for i, (a, b) in enumerate(d.copies) if (a, b) == (left, right)]
    return i


def test_a_broken_wire_is_a_copy_finding_and_the_gates_that_read_the_cell(cases):
    d, plan, values, _, cols, inst = cases["merkle"]
    X, root = d.advice[2 * SC.PAIRS], len(plan.segments) - 1
    cols = [list(c) for c in cols]

    # the root's W_3, wired to digest word 3 of the left child: another value in the word column
    row, base = SM.w_cell(plan, root, 3)
    src = plan.segments[root].sources[3]
    assert src == SS.DigestWord(0, 3)
    tail = SC.REGION_ROWS * (SS.first_regions(plan)[0] + SC.BLOCK_REGIONS * 2 + 0)  # digest word 3: tail region 0, A row
    wire = _copy_index(d, (X, tail + 0), (X, row))
    assert cols[X.index][tail] == cols[X.index][row]
    cols[X.index][row] ^= 0x10
    assert set(M.findings(d, cols, inst)) == {("copy", wire, tail)} | SM.gates_reading_w(base, 3)
    cols[X.index][row] ^= 0x10

    # the witness copy of a pinned padding word (the root's second block, W_0 = 0x80000000)
    row, base = SM.w_cell(plan, root, 16)
    assert cols[X.index][row] == 0x80000000 == int(d.fixed["const"][row])
    pin = _copy_index(d, (d.fixed_columns["const"], row), (X, row))
    cols[X.index][row] = 0
    assert set(M.findings(d, cols, inst)) == {("copy", pin, row)} | SM.gates_reading_w(base, 0)
    cols[X.index][row] = 0x80000000

    # one public digest word flipped in the instance
    assert M.findings(d, cols, inst) == []
    bad = list(inst)
    bad[5] ^= 1
    found = M.findings(d, cols, bad)
    assert [f[0] for f in found] == ["copy"] and d.copies[found[0][1]][0] == (d.instance, 5)


def test_plans_that_are_refused():
    one = (SS.PRIVATE,) * 16
    for ref in (1, 2):  # the segment itself, a later one
        plan = SS.Plan((SS.Segment(1, one), SS.Segment(1, (SS.DigestWord(ref, 0),) + one[1:]), SS.Segment(1, one)), (2,))
        with pytest.raises(ValueError, match="segment 1, word 0"):
            SS.describe(12, plan)
    with pytest.raises(ValueError):
        SS.describe(12, SS.Plan((SS.Segment(1, one), SS.Segment(1, (SS.DigestWord(0, 8),) + one[1:])), (1,)))
    with pytest.raises(ValueError):
        SS.describe(12, SS.Plan((SS.Segment(1, one[1:]),), (0,)))
    with pytest.raises(ValueError):
        SS.describe(12, SS.Plan((SS.Segment(1, one),), (1,)))
    # merkle_tree(2): three two-block segments, 3 * 1120 rows, more than 2^11 has
    assert SS.rows_for(SS.merkle_tree(2)) == 3 * 1120
    with pytest.raises(ValueError, match="3360 rows"):
        SS.describe(11, SS.merkle_tree(2))
    SS.describe(12, SS.merkle_tree(2))
    with pytest.raises(ValueError):
        SS.describe(12, SS.batch([1]), table_bits=10)
    with pytest.raises(ValueError):
        SS.merkle_tree(0)


def test_plan_builders():
    t = SS.merkle_tree(3)
    assert len(t.segments) == 7 and t.public == (6,) and all(s.blocks == 2 for s in t.segments)
    assert all(s.sources[:16] == (SS.PRIVATE,) * 16 for s in t.segments[:4])
    assert t.segments[4].sources[:16] == tuple(SS.DigestWord(c, w) for c in (0, 1) for w in range(8))
    assert t.segments[6].sources[:16] == tuple(SS.DigestWord(c, w) for c in (4, 5) for w in range(8))
    assert [s.value for s in t.segments[6].sources[16:]] == SC.pad(b"\x00" * 64)[16:]
    dd = SS.double_sha256(2)
    assert [s.blocks for s in dd.segments] == [2, 1] and dd.public == (1,)
    assert [s.value for s in dd.segments[1].sources[8:]] == SC.pad(b"\x00" * 32)[8:]
    assert SS.batch([1, 3]).public == (0, 1)


# SHA-256 over the fixed columns' bytes (uint64, FIXED order) and repr(copies) of sha256_circuit.describe(k, blocks), recorded
# from the commit before _assign_fixed was split into a per-segment helper
DESCRIBED = {(10, 1): "d667a8a549f4a3485e5b9912e1abb7a379c4f20f173c688ab0bc86a3598bd933",
             (11, 2): "752578c1cf37be6880f56f660e77f94e9da88b5ad8b7dd0082a7f8e65072b1b0"}


@pytest.mark.parametrize("k,blocks", sorted(DESCRIBED))
def test_a_one_segment_private_public_plan_is_the_single_message_circuit(k, blocks):
    """Pins the refactor of sha256_circuit._assign_fixed: describe() returns what it returned before, and a one-segment
    plan gives the same fixed columns and the same copies in the same order."""
    a = SC.describe(k, blocks)
    h = hashlib.sha256(b"".join(a.fixed[name].tobytes() for name in SC.FIXED) + repr(a.copies).encode())
    assert h.hexdigest() == DESCRIBED[k, blocks]
    b = SS.describe(k, SS.batch([blocks]))
    assert set(a.fixed) == set(b.fixed) == set(SC.FIXED)
    for name in SC.FIXED:
        assert np.array_equal(a.fixed[name], b.fixed[name]), name
    assert a.copies == b.copies
    assert b.blocks == (blocks,) and a.blocks == blocks
