"""GPU: wired SHA-256 segments -- the device compression chains give the pure-Python model's witness cell for cell and
hashlib's digests, the witness checker accepts them and names a cut wire, proofs verify against the right root or
double digest only, a one-segment plan is the single-message circuit byte for byte, and a bad description is refused
before anything is launched."""
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
from sha2_on_cq_halo2_amd.api import (FAIL_GATE, FAIL_PERMUTATION, Sha256BatchCircuit, Sha256Circuit, Sha256dCircuit, Sha256MerkleCircuit,
                                      Sha256SegmentsCircuit, fr_to_mont)
from tests import sha256_circuit_model as M
from tests import sha256_segments_model as SM
from tests.sha2_model import message, words_of
from tests.sha_oracle import mont_column as _mont

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
ERR_ARG = constants()["CQ_ERR_ARG"]


LEAVES = [hashlib.sha256(bytes([i])).digest() for i in range(4)]
# name -> (constructor, what the front end takes); the batch: three lanes of one level with unequal block counts
MAKE = {
    "batch": (lambda ctx: Sha256BatchCircuit(ctx, 12, [1, 2, 1], seed=SEED), [b"", message(119, 3), b"\xff" * 55]),
    "double": (lambda ctx: Sha256dCircuit(ctx, 11, 1, seed=SEED), message(55, 1)),
    "merkle2": (lambda ctx: Sha256MerkleCircuit(ctx, 12, 2, seed=SEED), LEAVES),
    "merkle1": (lambda ctx: Sha256MerkleCircuit(ctx, 11, 1, seed=SEED), LEAVES[:2]),
    "single": (lambda ctx: Sha256SegmentsCircuit(ctx, 11, SS.batch([2]), seed=SEED), [SC.pad(message(119, 3), 2)]),
}


def merkle_root(leaves):
    level = list(leaves)
    while len(level) > 1:
        level = [hashlib.sha256(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    return level[0]


def sha256d(msg):
    return hashlib.sha256(hashlib.sha256(msg).digest()).digest()


EXPECTED = {"batch": lambda ms: [hashlib.sha256(m).digest() for m in ms], "double": lambda m: [sha256d(m)],
            "merkle2": lambda ls: [merkle_root(ls)], "merkle1": lambda ls: [merkle_root(ls)]}


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = MAKE[name][0](ctx)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", ["batch", "double", "merkle2"])
def test_synthesis_equals_the_model_and_digests_equal_hashlib(circuits, name):
    c, arg = circuits(name), MAKE[name][1]
    cols, inst = c.synthesize(arg)
    values = c._values(arg)
    want = SM.witness(c.plan, values, c.table_bits, c.n)
    for i, (got, exp) in enumerate(zip(cols, want)):
        assert np.array_equal(got.download((c.n, 4)), _mont(exp)), f"advice column {i}"
    assert c.digest_words == SM.digests(c.plan, values)
    assert c.digests == EXPECTED[name](arg)
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(inst[0]))] == [w for d in EXPECTED[name](arg) for w in words_of(d)]
    assert c.check(arg) == (0, [])
    c.assert_satisfied(arg)


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
    """The circuit's constraint system restated for the oracle's verifier -> verify(proof, digest words)."""
    cs = c.cs
    kinds = {GP.COL_ADVICE: PL.ADVICE, GP.COL_FIXED: PL.FIXED, GP.COL_INSTANCE: PL.INSTANCE}
    names = {id(c.dense): "dense", id(c.spread): "spread"}
    exprs = iter(cs._lookup_exprs)
    lookups = [[(_oracle_expr(next(exprs)), names[id(t)]) for _, t in lk] for lk in cs.static_lookups]
    queries = {PL.ADVICE: list(cs.advice_queries), PL.FIXED: list(cs.fixed_queries), PL.INSTANCE: list(cs.instance_queries)}
    circ = CP.CqCircuit(c.k, cs.num_advice_columns, lookups, cs.num_fixed_columns, 1, [_oracle_expr(g) for g in cs.gates],
                        [(kinds[col.kind], col.index) for col in cs.permutation_columns], queries)
    assert circ.degree() == cs.degree() and circ.blinding_factors() == cs.blinding_factors()
    s = (seed * 0x9E3779B97F4A7C15 + 12345) % B.R_MOD
    N = 1 << c.table_bits
    tv = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
    fcm, pcm = c.pk.vk_commitments()

    def verify(proof, digest_words):
        return CV.verify_proof(proof, circ, c.vk_repr, s, tv, N, 1 << c.k, instances=[list(digest_words)],
                               fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))

    return verify


@pytest.mark.parametrize("name", ["merkle1", "double"])
def test_proofs_verify_against_their_root_or_double_digest_only(circuits, name):
    c, arg = circuits(name), MAKE[name][1]
    proof, digest = c.prove(arg, seed=7)
    (expected,) = EXPECTED[name](arg)
    assert len(proof) == c.pk.proof_size and digest == expected
    assert c.prove(arg, seed=7) == (proof, digest)
    verify = _verifier(c, SEED)
    assert verify(proof, words_of(expected))
    if name == "merkle1":  # one leaf byte changed
        (other,) = EXPECTED[name]([arg[0], arg[1][:-1] + bytes([arg[1][-1] ^ 1])])
    else:
        (other,) = EXPECTED[name](arg[:-1] + bytes([arg[-1] ^ 1]))
    assert other != expected and not verify(proof, words_of(other))


def _write(c, column, row, value):
    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[column].ptr + 32 * row, v.ctypes.data, 32))


def test_a_cut_wire_is_named(circuits):
    """merkle_tree(2), the root's W_3 (wired to digest word 3 of the left child) overwritten in the word column: the
    permutation finding at that cell and at the wire's other end -- the checker names every cell whose value differs from
    the cell it is mapped to, so the child's tail cell is named too, the one finding outside the root -- and the gates
    that read the cell: the word's recomposition, its round's two additions, the schedule addition of round 19."""
    c = circuits("merkle2")
    c.synthesize(LEAVES)
    root = len(c.plan.segments) - 1
    row, base = SM.w_cell(c.plan, root, 3)
    honest = c.digest_words[0][3]
    _write(c, 2 * SC.PAIRS, row, honest ^ 0x10)
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert total == len(fails) == len(found)
    tail = SC.REGION_ROWS * (SS.first_regions(c.plan)[0] + SC.BLOCK_REGIONS * 2)  # digest word 3: tail region 0, A row (row 0)
    gates = {(FAIL_GATE, index, r) for _, index, r in SM.gates_reading_w(base, 3)}
    assert (FAIL_PERMUTATION, 0, row) in found and (FAIL_GATE, SC.GATES.index("w_word"), base) in found
    assert found == gates | {(FAIL_PERMUTATION, 0, row), (FAIL_PERMUTATION, 0, tail)}
    first_root_row = SC.REGION_ROWS * SS.first_regions(c.plan)[root]
    assert all(r >= first_root_row for kind, _, r in found if kind != FAIL_PERMUTATION)


def test_a_one_segment_plan_is_the_single_message_circuit(ctx, circuits):
    """The device chain against the host chain: the same 18 columns, the same digest, the same proof bytes."""
    msg = message(119, 3)
    seg = circuits("single")
    one = Sha256Circuit(ctx, 11, 2, seed=SEED)
    try:
        proof, digest = one.prove(msg, seed=7)
        got = seg.prove([SC.pad(msg, 2)], seed=7)
        for i, (a, b) in enumerate(zip(one.cols, seg.cols)):
            assert np.array_equal(a.download((one.n, 4)), b.download((seg.n, 4))), f"advice column {i}"
        assert got == (proof, [digest]) and digest == hashlib.sha256(msg).digest()
    finally:
        one.close()


def test_a_bad_description_is_refused_and_nothing_is_written(ctx, circuits):
    c = circuits("double")
    n = c.n
    pattern = np.arange(4 * n, dtype=np.uint64).reshape(n, 4)
    c.cols[0].upload(pattern)
    c.cols[SC.ADVICE_COLUMNS - 1].upload(pattern)
    words = ctx.to_device(np.arange(16, dtype=np.uint32))
    arr = (C.c_void_p * SC.ADVICE_COLUMNS)(*[x.ptr for x in c.cols])
    blocks = np.array([1, 1], dtype=np.uint32)
    private = list(range(16))

    def call(second):
        sources = np.array(private + second, dtype=np.uint32)
        return ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, c.table_bits, blocks.ctypes.data, 2, sources.ctypes.data, words.ptr, 16, n, arr,
                                                         c._digests.ptr)

    try:
        for bad, what in ((SS.SOURCE_DIGEST + 8 * 1 + 0, "segment 1, word 2"), (SS.SOURCE_DIGEST + 8 * 2 + 7, "segment 1, word 2"),
                          (16, "segment 1, word 2")):
            second = private[:2] + [bad] + private[3:]
            assert call(second) == ERR_ARG
            assert what in ctx.lib.cq_last_error(ctx.h).decode()
        blocks[1] = 3  # 1 + 3 blocks do not fit 2^11 rows
        assert call(private * 3) == ERR_ARG
        blocks[1] = 0
        assert call([]) == ERR_ARG
        ctx.sync()
        for i in (0, SC.ADVICE_COLUMNS - 1):
            assert np.array_equal(c.cols[i].download((n, 4)), pattern)
        blocks[1] = 1  # and the same call with a good description goes through
        assert call([SS.SOURCE_DIGEST + i for i in range(8)] + private[8:]) == 0
        ctx.sync()
        assert not np.array_equal(c.cols[0].download((n, 4)), pattern)
    finally:
        words.close()
