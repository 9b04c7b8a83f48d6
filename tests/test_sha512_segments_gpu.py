"""GPU: wired SHA-512 segments under a proving key -- the synthesised witness equals the pure-Python model cell for cell,
the witness checker accepts it and names a changed wired cell of every kind, proofs verify against the oracle's verifier
with the public words alone, and the `batch` plan is Sha512BatchCircuit byte for byte."""
import hashlib
import random
import struct

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from sha2_on_cq_halo2_amd.api import (FAIL_GATE, FAIL_PERMUTATION, Sha512_256Circuit, Sha512BatchCircuit, Sha512dCircuit, Sha512MerkleCircuit,
                                      Sha512MidstateCircuit, Sha512SegmentsCircuit)
from tests import sha512_circuit_model as M
from tests import sha512_segments_model as SM
from tests.sha512_direct import mont_column
from tests.sha_oracle import verifier as _verifier
from tests.sha_oracle import write_cell as _write

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
X, PERM_X, PERM_CONST, PERM_INST = SM.X, 0, 1, 2  # the word column is the first column of the permutation, then `const`, then the instance

LEAVES = [bytes((41 * i + 7 * j + 3) % 256 for j in range(64)) for i in range(4)]
MSG = bytes((7 * i + 1) % 256 for i in range(111))
MID_DATA = bytes((5 * i + 1) % 256 for i in range(128))
H_IN = SM.compress(SC.pad(b"y" * 128, 2)[:16], 1, M.IV[SC.VARIANT_512])[1][-1]


def words_of(data):
    return list(struct.unpack(f">{len(data) // 8}Q", data))


def node(a, b):
    return hashlib.sha512(a + b).digest()


# name -> (class, k, its argument, what the methods take, the plan's values, the public words hashlib gives)
CASES = {
    "double": (Sha512dCircuit, 12, 1, MSG, [SC.pad(MSG, 1), []], words_of(hashlib.sha512(hashlib.sha512(MSG).digest()).digest())),
    "merkle": (Sha512MerkleCircuit, 14, 2, LEAVES, [words_of(LEAVES[0] + LEAVES[1]), words_of(LEAVES[2] + LEAVES[3]), []],
               words_of(node(node(LEAVES[0], LEAVES[1]), node(LEAVES[2], LEAVES[3])))),
    "midstate": (Sha512MidstateCircuit, 11, 1, (H_IN, MID_DATA), [H_IN + words_of(MID_DATA)], None),
    "sha512_256": (Sha512_256Circuit, 11, 1, MSG, [SC.pad(MSG, 1)], words_of(hashlib.new("sha512_256", MSG).digest())),
}


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(name):
        if name not in made:
            cls, k, arg = CASES[name][:3]
            made[name] = cls(ctx, k, arg, seed=SEED)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def mixed(ctx):
    c = Sha512SegmentsCircuit(ctx, 13, SM.mixed_plan(), seed=SEED)
    rng = random.Random(11)
    c.values = [[rng.getrandbits(64) for _ in range(count)] for count in SS.lower(c.plan).private_counts]
    c.shared = [0x0123456789ABCDEF, (1 << 64) - 2]
    yield c
    c.close()


def assert_model(c, values, shared=()):
    """The device columns of the last synthesis are the model's, cell for cell over all n rows; -> the model's instance."""
    want, states, _, instance = SM.plan_witness(c.plan, values, shared, c.table_bits, c.n)
    for i, (got, exp) in enumerate(zip(c.cols, want)):
        assert np.array_equal(got.download((c.n, 4)), mont_column(exp)), f"advice column {i}"
    assert c.state_words == states and c.instance_words == instance
    return instance


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthesis_equals_the_model_and_is_accepted(circuits, name):
    _, _, _, item, values, public = CASES[name]
    c = circuits(name)
    c.synthesize(item)
    instance = assert_model(c, values)
    if public is not None:
        assert instance == public and b"".join(c.digests) == struct.pack(f">{len(public)}Q", *public)
    else:  # the midstate: H_out of this block, then H_in
        assert instance == SM.compress(words_of(MID_DATA), 1, H_IN)[1][-1] + H_IN and c.h_out == instance[:8]
    assert c.check(item) == (0, [])
    c.assert_satisfied(item)


def test_the_mixed_plan_equals_the_model_and_is_accepted(mixed):
    mixed.synthesize(mixed.values, mixed.shared)
    instance = assert_model(mixed, mixed.values, mixed.shared)
    assert len(instance) == 5 + 6 + 1 + 8 and mixed.check(mixed.values, mixed.shared) == (0, [])


def _findings(c, instances=None):
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=instances if instances is not None else c.instances, max_failures=256)
    assert total == len(fails) and total > 0
    return {(f.kind, f.index, f.row) for f in fails}


def test_a_changed_wired_cell_is_named(mixed):
    """Each change starts from the honest witness.  The findings: a permutation finding at the changed cell, permutation
    findings nowhere but on the cells it is tied to, and otherwise only the gates that read the word."""
    c = mixed
    f = SS.first_regions(c.plan)
    want, _, _, instance = SM.plan_witness(c.plan, c.values, c.shared, c.table_bits, c.n)
    cases = [  # the changed row of column X, and the cells it is tied to
        ("a DigestWord message word", SM.message_row(f[2], 0), {(PERM_X, SM.tail_row(f[1], 1, 7))}),
        ("a Const word", SM.message_row(f[2], 2), {(PERM_CONST, SM.message_row(f[2], 2))}),
        # the Var's third cell is initial word 6 of segment 2, whose initial state is public: instance row 12 + 6 is on the cycle
        ("the second cell of a Var", SM.message_row(f[2], 1), {(PERM_X, SM.message_row(f[0], 0)), (PERM_X, SM.state_row(f[2], 6)), (PERM_INST, 18)}),
        ("a digest-wired initial word", SM.state_row(f[2], 0), {(PERM_X, SM.tail_row(f[0], 1, 7)), (PERM_INST, 12)}),
        ("a public word", SM.tail_row(f[2], 2, 4), {(PERM_INST, 4)}),
    ]
    for what, row, tied in cases:
        c.synthesize(c.values, c.shared)
        _write(c, X, row, want[X][row] ^ 32)
        found = _findings(c)
        perm = {(index, r) for kind, index, r in found if kind == FAIL_PERMUTATION}
        assert (PERM_X, row) in perm and perm <= tied | {(PERM_X, row)}, (what, found)
        assert all(kind in (FAIL_PERMUTATION, FAIL_GATE) for kind, _, _ in found), (what, found)
    # a public word changed in the instance
    c.synthesize(c.values, c.shared)
    inst = [c.instances[0].copy()]
    inst[0][4] = SS._words_to_mont([instance[4] ^ 32])[0]
    assert _findings(c, inst) == {(FAIL_PERMUTATION, PERM_INST, 4), (FAIL_PERMUTATION, PERM_X, SM.tail_row(f[2], 2, 4))}
    # a private word: the gates that read it, no copy
    c.synthesize(c.values, c.shared)
    row = SM.message_row(f[2], 20)
    _write(c, X, row, want[X][row] ^ 32)
    found = _findings(c)
    assert found and all(kind == FAIL_GATE for kind, _, _ in found)


@pytest.mark.parametrize("name", sorted(CASES))
def test_proofs_verify_against_the_public_words_only(circuits, name):
    item = CASES[name][3]
    c = circuits(name)
    proof, _ = c.prove(item, seed=7)
    assert len(proof) == c.pk.proof_size
    words = list(c.instance_words)
    assert len(words) == {"double": 8, "merkle": 8, "midstate": 16, "sha512_256": 4}[name]
    verify = _verifier(c, SEED)
    assert verify(proof, words)
    for at in (0, len(words) - 1):
        changed = list(words)
        changed[at] ^= 1 << 40
        assert not verify(proof, changed)


def test_the_batch_plan_is_sha512_batch_circuit_byte_for_byte(ctx):
    msgs, blocks, variants = [bytes(range(100)), b"abc"], [1, 1], [SC.VARIANT_512, SC.VARIANT_384]
    a = Sha512BatchCircuit(ctx, 12, blocks, variants, seed=SEED)
    b = Sha512SegmentsCircuit(ctx, 12, SS.batch(blocks, variants), seed=SEED)
    try:
        proof_a, digests = a.prove(msgs, seed=5)
        proof_b, digests_b = b.prove([SC.pad(m, 1) for m in msgs], seed=5)
        assert proof_a == proof_b and digests == digests_b == [hashlib.sha512(msgs[0]).digest(), hashlib.sha384(msgs[1]).digest()]
        assert a.digest_words == b.instance_words and len(b.instance_words) == 14
    finally:
        a.close()
        b.close()
