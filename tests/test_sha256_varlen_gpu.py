"""GPU: SHA-256 of variable-length messages -- under ONE key of three blocks, every length that moves the boundary word, the
spill into the next block or the final block: the device's padding, chains and cells give the pure-Python model's witness
cell for cell and hashlib's digest, the witness checker accepts them and names each forged padding by its gate, proofs
verify against their own digest (and length) only, and a bad description is refused before anything is launched."""
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
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from sha2_on_cq_halo2_amd._lib import constants
from sha2_on_cq_halo2_amd.api import FAIL_GATE, FAIL_STATIC_LOOKUP, Sha256VarCircuit, fr_to_mont
from tests import sha256_circuit_model as M
from tests import sha256_varlen_model as VM
from tests.sha2_model import nonzero_message as message, words_of
from tests.sha_oracle import mont_column as _mont

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
ERR_ARG = constants()["CQ_ERR_ARG"]
X, Y = VM.X, VM.Y
VAR = SC.VAR
K, MAX_BLOCKS = 11, 3
# r = 0 .. 3; the boundary in words 13, 14 and 15; padding that spills into the next block (56 .. 63, 120); the final block
# 0, 1 or 2; the empty message and the longest
LENGTHS = [0, 1, 3, 4, 5, 52, 55, 56, 59, 60, 63, 64, 119, 120, 183]


@pytest.fixture(scope="module")
def circuits(ctx):
    make = {"one": lambda: Sha256VarCircuit(ctx, K, [MAX_BLOCKS], seed=SEED),
            "public": lambda: Sha256VarCircuit(ctx, K, [MAX_BLOCKS], public_length=True, seed=SEED),
            "two": lambda: Sha256VarCircuit(ctx, 12, [1, 3], seed=SEED)}
    made = {}

    def get(name):
        if name not in made:
            made[name] = make[name]()
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _same_cells(c, messages):
    want, digests = VM.witness(messages, c.max_blocks_list, c.table_bits, c.n)
    for i, (got, exp) in enumerate(zip(c.cols, want)):
        assert np.array_equal(got.download((c.n, 4)), _mont(exp)), f"advice column {i}"
    assert c.digest_words == digests
    assert c.digests == [hashlib.sha256(m).digest() for m in messages]


@pytest.mark.parametrize("length", LENGTHS)
def test_synthesis_equals_the_model_and_the_digest_is_hashlibs(circuits, length):
    c, m = circuits("one"), message(length, salt=length)
    assert c.rows == SC.rows_for(MAX_BLOCKS) and SC.max_blocks(K) == MAX_BLOCKS
    cols, inst = c.synthesize([m])
    _same_cells(c, [m])
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(inst[0]))] == words_of(hashlib.sha256(m).digest())
    assert c.pk.check_witness([x.ptr for x in cols], instances=inst) == (0, [])


def test_every_length_is_satisfied_under_the_one_key(circuits):
    c = circuits("one")
    for length in LENGTHS:
        c.assert_satisfied([message(length)])
    with pytest.raises(ValueError, match="184 bytes"):
        c.synthesize([message(184)])


def test_a_batch_of_two_messages_of_different_block_counts(circuits):
    c, messages = circuits("two"), [message(55, 1), message(120, 2)]
    assert SC.usable_rows(11) < c.rows <= SC.usable_rows(12)
    cols, inst = c.synthesize(messages)
    _same_cells(c, messages)
    assert [B.from_mont_limbs(inst[0])[i] for i in range(16)] == [w for m in messages for w in words_of(hashlib.sha256(m).digest())]
    c.assert_satisfied(messages)
    c.assert_satisfied([b"", message(183)])
    with pytest.raises(ValueError, match="message 0"):
        c.synthesize([message(56), b""])


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
    assert circ.degree() == cs.degree() == 4 and circ.blinding_factors() == cs.blinding_factors() == 20
    assert cs.num_fixed_columns == len(SC.FIXED_VARLEN) and len(cs.gates) == len(SC.GATES_VARLEN) and len(cs.permutation_columns) == 4
    s = (seed * 0x9E3779B97F4A7C15 + 12345) % B.R_MOD
    N = 1 << c.table_bits
    tv = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
    fcm, pcm = c.pk.vk_commitments()

    def verify(proof, instance_words):
        return CV.verify_proof(proof, circ, c.vk_repr, s, tv, N, 1 << c.k, instances=[list(instance_words)],
                               fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))

    return verify


@pytest.mark.parametrize("length", [0, 55, 56, 183])
def test_a_proof_verifies_against_its_own_digest_only(circuits, length):
    c, m = circuits("one"), message(length, salt=3)
    proof, digests = c.create_proof([m], seed=7)
    assert len(proof) == c.pk.proof_size and digests == [hashlib.sha256(m).digest()]
    assert c.create_proof([m], seed=7) == (proof, digests)
    verify = _verifier(c, SEED)
    assert verify(proof, words_of(digests[0]))
    assert not verify(proof, words_of(hashlib.sha256(message(length + 1, salt=3)).digest()))  # the message one byte longer


@pytest.mark.parametrize("length", [0, 55, 56, 183])
def test_a_public_length_is_the_messages_own(circuits, length):
    c, m = circuits("public"), message(length, salt=4)
    proof, digests = c.create_proof([m], seed=7)
    digest = words_of(hashlib.sha256(m).digest())
    assert words_of(digests[0]) == digest
    verify = _verifier(c, SEED)
    assert verify(proof, digest + [length])
    assert not verify(proof, digest + [length + 1]) and not verify(proof, digest + [(length - 1) % B.R_MOD])


def _write(c, column, row, value):
    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[column].ptr + 32 * row, v.ctypes.data, 32))


def region(block, which):
    return SV.region_row(0, block, which)


def word(block, t):
    return region(block, 4 + t)


W13 = VM.pad_words(message(53), MAX_BLOCKS)[0][13]  # L = 53: one byte of the message, 0x80, two zero bytes
FINAL, CARRY = VAR["REGION_FINAL"], VAR["REGION_CARRY"]
# name -> (length, [(column, row, value)] written behind the synthesis, the finding that must be among the checker's)
FORGERIES = {
    "a non-zero byte behind 0x80": (53, [(X, word(0, 13) + 2, W13 | 0x0100)], ("var_boundary", word(0, 13))),
    "0x80 missing": (53, [(X, word(0, 13) + 2, W13 & ~0x800000)], ("var_boundary", word(0, 13))),
    "a non-zero pad word": (3, [(X, word(0, 5) + 2, 1)], ("var_pad_zero", word(0, 5))),
    "a wrong length word": (53, [(X, word(0, 15) + 2, 8 * 53 + 8)], ("var_length_word", word(0, 15))),
    "the length in word 14": (53, [(X, word(0, 14) + 2, 8 * 53), (X, word(0, 15) + 2, 0)], ("var_pad_zero", word(0, 14))),
    # word 13 of block 0 called a message word, block 1 (all zero) called final: word 14 is then the boundary word
    "a final flag one block late": (53, [(Y, word(0, 13) + VAR["ROW_M"], 1), (Y, region(0, FINAL) + VAR["ROW_FLAG"], 1),
                                         (Y, region(0, FINAL) + VAR["ROW_VALUE"], 0), (Y, region(1, FINAL) + VAR["ROW_IN"], 1),
                                         (Y, region(1, FINAL) + VAR["ROW_VALUE"], 1), (Y, region(1, CARRY) + VAR["ROW_OUT"], 1)],
                                    ("var_boundary", word(0, 14))),
    "two final blocks": (53, [(Y, region(1, FINAL) + VAR["ROW_VALUE"], 1)], ("var_final", region(1, FINAL))),
    "no final block": (183, [(Y, word(2, 13) + VAR["ROW_M"], 1)], ("var_last_final", word(2, 13))),
    "an m that rises again": (3, [(Y, word(0, 9) + VAR["ROW_M"], 1)], ("var_b_bool", word(0, 9))),
    "c0 = 2": (53, [(Y, word(0, 13) + VAR["ROW_C0"], 2)], ("var_c0_bool", word(0, 13))),
}


@pytest.mark.parametrize("name", sorted(FORGERIES))
def test_a_forged_padding_is_named_by_its_gate(circuits, name):
    length, edits, (gate, row) = FORGERIES[name]
    c = circuits("one")
    c.synthesize([message(length)])
    for column, at, value in edits:
        _write(c, column, at, value)
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert total == len(fails) == len(found)
    assert (FAIL_GATE, SC.GATES_VARLEN.index(gate), row) in found
    # and the model names the same gates
    cols, _ = VM.witness([message(length)], [MAX_BLOCKS], c.table_bits, c.n)
    for column, at, value in edits:
        cols[column][at] = value
    model = VM.findings(SV.describe(K, [MAX_BLOCKS]), cols, VM.instance_words([message(length)], [MAX_BLOCKS]))
    assert {(i, r) for kind, i, r in model if kind == "gate"} == {(i, r) for kind, i, r in found if kind == FAIL_GATE}


def test_a_data_half_of_thirteen_bits_is_named_by_its_lookups(circuits):
    """d1 = 2^12 is no row of the dense table: the finding is the pair and the length lookup of slot 7 (lookups 7 and 15),
    which is where the 12-bit bound lives -- no gate reads it."""
    c = circuits("one")
    c.synthesize([message(53)])
    _write(c, 2 * VAR["SLOT_DATA"], word(0, 13) + 1, 1 << 12)
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert {(FAIL_STATIC_LOOKUP, VAR["SLOT_DATA"], word(0, 13) + 1), (FAIL_STATIC_LOOKUP, SC.PAIRS + VAR["SLOT_DATA"], word(0, 13) + 1)} <= found


def test_a_bad_description_is_refused_and_nothing_is_written(ctx, circuits):
    c = circuits("one")
    n = c.n
    pattern = np.arange(4 * n, dtype=np.uint64).reshape(n, 4)
    c.cols[0].upload(pattern)
    c.cols[SC.ADVICE_COLUMNS - 1].upload(pattern)
    data = ctx.to_device(np.frombuffer(message(200), dtype=np.uint8))
    digests = ctx.alloc(32)
    arr = (C.c_void_p * SC.ADVICE_COLUMNS)(*[x.ptr for x in c.cols])

    def call(blocks, offset, length, table_bits=12, rows=n):
        b, o, ln = np.array([blocks], dtype=np.uint32), np.array([offset], dtype=np.uint64), np.array([length], dtype=np.uint64)
        return ctx.lib.cq_sha256_synthesize_varlen_dev(ctx.h, table_bits, b.ctypes.data, 1, data.ptr, 200, o.ctypes.data, ln.ctypes.data,
                                                       rows, arr, digests.ptr)

    try:
        for args, what in (((3, 0, 184), "segment 0"),            # one byte more than three blocks hold
                           ((3, 201, 0), "segment 0"),            # an offset behind the buffer
                           ((3, 100, 101), "segment 0"),          # a length that leaves the buffer
                           ((0, 0, 0), "segment 0"),              # no block
                           ((4, 0, 10), "segment 0"),             # rows that do not fit n
                           ((3, 0, 10, 11), "table_bits")):       # 12-bit halves need a table of 2^12
            assert call(*args) == ERR_ARG
            assert what in ctx.lib.cq_last_error(ctx.h).decode()
        ctx.sync()
        for i in (0, SC.ADVICE_COLUMNS - 1):
            assert np.array_equal(c.cols[i].download((n, 4)), pattern)
        assert call(3, 17, 183) == 0  # and a good one goes through, at an odd offset
        ctx.sync()
        assert not np.array_equal(c.cols[0].download((n, 4)), pattern)
        assert digests.download((8,), np.uint32).tolist() == words_of(hashlib.sha256(message(200)[17:]).digest())
    finally:
        data.close()
        digests.close()
