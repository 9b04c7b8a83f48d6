"""CPU: SHA-256 of variable-length messages -- the model's padding against hashlib at every length a three-block segment
holds, the variable-length description against the model's witness (every gate, lookup and copy), what each forged padding
is reported as, and what the variant must leave as it was: the descriptions of the plain, segment and choice plans, the
degree and the blinding factors."""
import hashlib

import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha256_varlen_model as VM
from tests.sha2_model import nonzero_message as message, words_of

K, MAX_BLOCKS = 11, 3
X, Y = VM.X, VM.Y
VAR = SC.VAR


def test_the_models_padding_gives_hashlibs_digest_at_every_length():
    for length in range(64 * MAX_BLOCKS - 8):
        m = message(length)
        words, final = VM.pad_words(m, MAX_BLOCKS)
        assert len(words) == 16 * MAX_BLOCKS and final == (length + 8) // 64
        assert words[: 16 * (final + 1)] == SC.pad(m) and not any(words[16 * (final + 1):])
        assert VM.digest_of(m, MAX_BLOCKS) == words_of(hashlib.sha256(m).digest())
    with pytest.raises(AssertionError):
        VM.pad_words(message(64 * MAX_BLOCKS - 8), MAX_BLOCKS)


def description_hash(d):
    """SHA-256 over everything a key is made from: the fixed columns' bytes in allocation order, the copies, the queries and
    permutation columns in registration order, and every gate and lookup input compiled for the gate interpreter."""
    cs, constants = d.cs, []
    programs = [g.compile(constants) for g in cs.gates] + [e.compile(constants) for e in cs._lookup_exprs]
    text = repr((d.copies, cs.advice_queries, cs.fixed_queries, cs.instance_queries, cs.permutation_columns, programs, constants,
                 [[c for c, _ in lk] for lk in cs.static_lookups], d.fixed_names, d.blocks, d.k, d.table_bits))
    return hashlib.sha256(b"".join(d.fixed[name].tobytes() for name in d.fixed_names) + text.encode()).hexdigest()


# description_hash of a plain (9c), a segment (9d) and a choice (9e) plan, recorded on the commit before the variable-length
# variant was added to _constraint_system
DESCRIBED = {"plain": "91d4217c86cd71729fc59653a5a5743ef13dac9b388810a0ff5dad37d2876880",
             "segments": "1949213ab67fd97fd040543fcac43ce3a33511ee5e149c47e7a612b720c313a5",
             "choice": "8efe63266ea8fddabd017bd0394af97e5b48466d05cbba0f2651a260e8ddcf8a"}


def test_the_other_variants_are_described_as_before():
    assert description_hash(SC.describe(11, 2)) == DESCRIBED["plain"]
    assert description_hash(SS.describe(12, SS.merkle_tree(2))) == DESCRIBED["segments"]
    assert description_hash(SS.describe(12, SS.merkle_path(2, leaf_blocks=1, public_leaf=True))) == DESCRIBED["choice"]


@pytest.fixture(scope="module")
def description():
    return SV.describe(K, [MAX_BLOCKS], public_length=True)


def test_degree_blinding_factors_and_shape(description):
    cs = description.cs
    assert cs.degree() == 4 and cs.blinding_factors() == 20
    plain = SC.describe(K, MAX_BLOCKS).cs
    assert (plain.degree(), plain.blinding_factors()) == (4, 20)
    per_column = [sum(1 for c, _ in cs.advice_queries if c == i) for i in range(SC.ADVICE_COLUMNS)]
    assert per_column[X] == 18 and per_column[Y] == 17 and max(per_column) == 18
    assert description.fixed_names == SC.FIXED_VARLEN and len(cs.gates) == len(SC.GATES_VARLEN) == len(SC.GATES) + 13
    assert [(c.kind, c.index) for c in cs.permutation_columns] == [(0, X), (1, len(SC.FIXED) - 1), (2, 0), (0, Y)]
    assert max(g.degree() for g in cs.gates) == 4
    assert SC.usable_rows(K) >= SC.rows_for(MAX_BLOCKS) and SC.max_blocks(K) == MAX_BLOCKS
    # everything the plain system has is there unchanged, in front
    assert set(plain.advice_queries) <= set(cs.advice_queries) and set(plain.fixed_queries) <= set(cs.fixed_queries)
    constants = []
    assert [g.compile(constants) for g in cs.gates[: len(SC.GATES)]] == [g.compile(constants) for g in plain.gates]
    with pytest.raises(ValueError, match="does not combine"):
        SC._constraint_system(12, "dense", "spread", choice=True, varlen=True)
    with pytest.raises(ValueError, match="table_bits"):
        SV.describe(K, [MAX_BLOCKS], table_bits=11)
    with pytest.raises(ValueError, match="usable"):
        SV.describe(K, [MAX_BLOCKS + 1])


def gate(name, row):
    return ("gate", SC.GATES_VARLEN.index(name), row)


def honest(length):
    m = message(length, salt=length)
    cols, digests = VM.witness([m], [MAX_BLOCKS], 12, 1 << K)
    assert digests == [words_of(hashlib.sha256(m).digest())]
    return cols, digests[0] + [length]


@pytest.mark.parametrize("length", [0, 3, 55, 56, 63, 64, 120, 183])
def test_the_models_witness_satisfies_the_description(description, length):
    cols, inst = honest(length)
    assert VM.findings(description, cols, inst) == []


def test_a_wrong_digest_or_length_is_a_broken_copy(description):
    cols, inst = honest(56)
    for i in (0, 7, 8):
        bad = list(inst)
        bad[i] ^= 1
        found = VM.findings(description, cols, bad)
        assert len(found) == 1 and found[0][0] == "copy"


def region(block, which):
    return SV.region_row(0, block, which)


def word(block, t):
    return region(block, 4 + t)


def new_gates(description, cols, inst):
    """The findings among the variable-length gates: {(name, row)}."""
    first = len(SC.GATES)
    return {(SC.GATES_VARLEN[i], r) for kind, i, r in VM.findings(description, cols, inst) if kind == "gate" and i >= first}


def test_forged_paddings_are_named(description):
    M_, LEN, C0 = VAR["ROW_M"], VAR["ROW_LEN"], VAR["ROW_C0"]
    FLAG, VALUE = VAR["ROW_FLAG"], VAR["ROW_VALUE"]
    wrow = 2
    data = 2 * VAR["SLOT_DATA"]

    def forged(length, edits):
        cols, inst = honest(length)
        for column, row, value in edits:
            cols[column][row] = value
        return new_gates(description, cols, inst)

    # L = 53: word 13 is the boundary word, one byte of the message, 0x80, two zero bytes
    w13 = VM.pad_words(message(53, salt=53), MAX_BLOCKS)[0][13]
    assert w13 & 0xFFFFFF == 0x800000
    # a non-zero byte behind 0x80
    assert ("var_boundary", word(0, 13)) in forged(53, [(X, word(0, 13) + wrow, w13 | 0x0100)])
    # 0x80 missing
    assert ("var_boundary", word(0, 13)) in forged(53, [(X, word(0, 13) + wrow, w13 & ~0x800000)])
    # a non-zero pad word: L = 3, word 5 of the final block
    assert forged(3, [(X, word(0, 5) + wrow, 1)]) == {("var_pad_zero", word(0, 5))}
    # a wrong length word
    assert forged(53, [(X, word(0, 15) + wrow, 8 * 53 + 8)]) == {("var_length_word", word(0, 15))}
    # the length in word 14
    assert forged(53, [(X, word(0, 14) + wrow, 8 * 53), (X, word(0, 15) + wrow, 0)]) == {("var_pad_zero", word(0, 14)), ("var_length_word", word(0, 15))}
    # a final flag one block late, with an all-zero extra block: L = 53 claims block 1 as final by calling word 13 of block
    # 0 a message word -- then word 14 is the boundary word and holds no 0x80
    late = [(Y, word(0, 13) + M_, 1), (Y, region(0, VAR["REGION_FINAL"]) + FLAG, 1), (Y, region(0, VAR["REGION_FINAL"]) + VALUE, 0),
            (Y, region(1, VAR["REGION_FINAL"]) + VAR["ROW_IN"], 1), (Y, region(1, VAR["REGION_FINAL"]) + VALUE, 1),
            (Y, region(1, VAR["REGION_CARRY"]) + VAR["ROW_OUT"], 1)]
    found = forged(53, late)
    assert ("var_boundary", word(0, 14)) in found and ("var_final", region(0, VAR["REGION_FINAL"])) not in found
    # two final blocks: block 1's flag set beside block 0's
    assert ("var_final", region(1, VAR["REGION_FINAL"])) in forged(53, [(Y, region(1, VAR["REGION_FINAL"]) + VALUE, 1)])
    # no final block: L = 183 ends in block 2, whose word 13 is called a message word
    assert ("var_last_final", word(2, 13)) in forged(183, [(Y, word(2, 13) + M_, 1)])
    # an m that rises again behind the boundary
    assert ("var_b_bool", word(0, 9)) in forged(3, [(Y, word(0, 9) + M_, 1)])
    # c0 = 2 in the boundary word
    assert ("var_c0_bool", word(0, 13)) in forged(53, [(Y, word(0, 13) + C0, 2)])
    # d1 = 2^12: outside the table -- the lookups of pair slot 7, no gate's business
    cols, inst = honest(53)
    cols[data][word(0, 13) + 1] = 1 << 12
    found = VM.findings(description, cols, inst)
    assert ("lookup", VAR["SLOT_DATA"], word(0, 13) + 1) in found and ("lookup", SC.PAIRS + VAR["SLOT_DATA"], word(0, 13) + 1) in found
    # a length that is not the sum: len of a message word raised by one
    assert ("var_len", word(0, 2)) in forged(53, [(Y, word(0, 2) + LEN, 13)])
