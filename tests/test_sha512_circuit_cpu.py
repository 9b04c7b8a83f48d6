"""CPU: the SHA-512 / SHA-384 compression circuit's padding, its constraint-system description against the library's
limits, its layout table, and the pure-Python model's witness against every gate, lookup and copy -- and against hashlib."""
import hashlib
import os
import re

import pytest

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from tests import sha512_circuit_model as M
from tests.sha2_model import message

MESSAGES = {0: 1, 1: 1, 111: 1, 112: 2, 127: 2, 128: 2, 239: 2}
HASH = {SC.VARIANT_512: hashlib.sha512, SC.VARIANT_384: hashlib.sha384}
K_FOR = {1: 11, 2: 12}  # the smallest k that holds the block count


@pytest.mark.parametrize("length,blocks", sorted(MESSAGES.items()))
def test_pad_gives_the_standard_padding(length, blocks):
    msg = message(length)
    words = SC.pad(msg)
    raw = b"".join(w.to_bytes(8, "big") for w in words)
    assert len(raw) == 128 * blocks
    assert raw[:length] == msg and raw[length] == 0x80
    assert raw[length + 1:-16] == b"\x00" * (128 * blocks - length - 17)
    assert int.from_bytes(raw[-16:], "big") == 8 * length
    assert SC.pad(msg, blocks) == words
    with pytest.raises(ValueError):
        SC.pad(msg, blocks + 1)


def test_constants_are_the_roots_of_the_primes():
    """The package's round constants and initial hash values against FIPS 180-4's definition, computed by the model."""
    assert SC.K512 == M.K and SC.IV512 == M.IV[SC.VARIANT_512] and SC.IV384 == M.IV[SC.VARIANT_384]


def _postfix_effects(prog):
    """+1 for every push, -1 for every binary operator of a compiled gate program"""
    i = 0
    while i < len(prog):
        op = prog[i] & 0xFF
        if op in (GP.GATE_ADVICE, GP.GATE_FIXED, GP.GATE_INSTANCE):
            i += 1
            yield 1
        elif op in (GP.GATE_CONST, GP.GATE_CHALLENGE):
            yield 1
        elif op in (GP.GATE_ADD, GP.GATE_MUL):
            yield -1
        i += 1


@pytest.mark.parametrize("table_bits", [11, 12, 16])
def test_description_stays_inside_the_library_limits(table_bits):
    """At most CQ_MAX_LOOKUPS lookups of at most CQ_MAX_WIDTH table columns, at most PERM_MAX_COLUMNS permutation
    columns (the constants of csrc/poly.hpp, cq.hpp and plonk.hpp), a gate degree of at most 5, and an expression depth
    the gate interpreter's operand stack holds."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(SC.__file__)), "csrc")
    limit = lambda f, name: int(re.search(name + r"\s*=\s*(\d+)", open(os.path.join(csrc, f)).read()).group(1))
    cs = SC.describe(11, 1, table_bits).cs
    assert len(cs.static_lookups) == 2 * SC.PAIRS <= limit("poly.hpp", "CQ_MAX_LOOKUPS")
    assert max(len(lk) for lk in cs.static_lookups) <= limit("cq.hpp", "CQ_MAX_WIDTH")
    assert len(cs.permutation_columns) <= limit("plonk.hpp", "PERM_MAX_COLUMNS")
    assert cs.degree() <= 5
    assert cs.num_advice_columns == SC.ADVICE_COLUMNS == 18 and cs.num_instance_columns == 1 and len(cs.gates) == len(SC.GATES) == 23
    stack = limit("plonk.hpp", "GATE_STACK")
    for e in cs.gates + cs._lookup_exprs:
        depth = best = 0
        for word in _postfix_effects(e.compile([])):
            depth += word
            best = max(best, depth)
        assert best <= stack


def test_description_rejects_what_does_not_fit():
    with pytest.raises(ValueError):
        SC.describe(11, 2)
    with pytest.raises(ValueError):
        SC.describe(11, 1, table_bits=10)
    with pytest.raises(ValueError):
        SC.describe(11, 1, table_bits=17)
    with pytest.raises(ValueError):
        SC.describe(11, 1, variant=2)
    with pytest.raises(ValueError):
        SC.describe_batch(12, [1, 0])
    with pytest.raises(ValueError):
        SC.describe_batch(12, [1, 1], [SC.VARIANT_512])


@pytest.mark.parametrize("k", [11, 12, 14])
def test_rows_of_the_largest_block_count_fit(k):
    usable = (1 << k) - (SC.describe(11, 1).cs.blinding_factors() + 1)
    b = SC.max_blocks(k)
    assert b >= 1 and SC.usable_rows(k) == usable and SC.rows_for(b) <= usable < SC.rows_for(b + 1)
    assert SC.describe(k, b).blocks == b
    with pytest.raises(ValueError):
        SC.describe(k, b + 1)


def test_layout_table_is_consistent():
    """Every word's pieces tile its 64 bits, no piece is wider than the smallest table, no two cells share a place, and
    every even / odd word has chunks 0 .. 5, which cover 64 bits at the smallest table."""
    cells = SC.layout()
    places = [(c.column + d, c.row) for c in cells for d in ((0, 1) if c.form == SC.FORM_PAIR else (0,))]
    assert len(places) == len(set(places))
    assert all(c.row < SC.REGION_ROWS and c.column + (c.form == SC.FORM_PAIR) < SC.ADVICE_COLUMNS for c in cells)
    assert all(c.column % 2 == 0 and c.column < 2 * SC.PAIRS for c in cells if c.form == SC.FORM_PAIR)
    assert all(c.column >= 2 * SC.PAIRS and (c.offset, c.per_table_bits, c.len) == (0, 0, 64) for c in cells if c.form != SC.FORM_PAIR)
    for name in ("A", "E", "W"):
        ps = sorted((c.offset, c.len) for c in cells if c.kind == SC.SRC[name] and c.form == SC.FORM_PAIR)
        assert ps[0][0] == 0 and all(a + l == b for (a, l), (b, _) in zip(ps, ps[1:])) and sum(ps[-1]) == 64
        assert max(l for _, l in ps) <= SC.MIN_TABLE_BITS
    for name in ("CARRY_A", "CARRY_E", "CARRY_W"):
        assert [(c.offset, c.len) for c in cells if c.kind == SC.SRC[name]] == [(0, 3)]
    for name, v in SC.SRC.items():
        if name.endswith(("_EVEN", "_ODD")):
            assert sorted(c.per_table_bits for c in cells if c.kind == v and c.form == SC.FORM_PAIR) == list(range(SC.CHUNKS)) == [0, 1, 2, 3, 4, 5]
    assert SC.CHUNKS * SC.MIN_TABLE_BITS >= 64
    assert SC.REGION_ROWS * SC.PAIRS >= sum(c.form == SC.FORM_PAIR for c in cells) == 30 + 7 * 12


@pytest.fixture(scope="module")
def descriptions():
    made = {}

    def get(blocks, variant=SC.VARIANT_512, table_bits=12):
        key = (blocks, variant, table_bits)
        if key not in made:
            made[key] = SC.describe(K_FOR[blocks], blocks, table_bits, variant=variant)
        return made[key]

    return get


CASES = [(length, variant, 12) for variant in (SC.VARIANT_512, SC.VARIANT_384) for length in (0, 111, 112, 239)] + \
        [(111, SC.VARIANT_512, 11), (111, SC.VARIANT_384, 16)]


@pytest.mark.parametrize("length,variant,table_bits", CASES)
def test_model_witness_satisfies_the_circuit_and_gives_the_digest(descriptions, length, variant, table_bits):
    msg = message(length, salt=length + variant)
    d = descriptions(MESSAGES[length], variant, table_bits)
    cols, instance, (state,) = M.witness([msg], [d.blocks], [variant], table_bits, 1 << d.k)
    assert M.digest_bytes(state, variant) == HASH[variant](msg).digest()
    assert len(instance) == SC.DIGEST_WORDS[variant] and instance == state[:len(instance)]
    assert M.findings(d, cols, instance) == []


def test_model_witness_of_a_batch_satisfies_the_circuit():
    """Two messages of different variants in one description: the second segment's rows, constants and instance rows."""
    msgs, blocks_list, variants = [message(5, 1), message(200, 2)], [1, 2], [SC.VARIANT_384, SC.VARIANT_512]
    d = SC.describe_batch(13, blocks_list, variants)
    cols, instance, states = M.witness(msgs, blocks_list, variants, d.table_bits, 1 << d.k)
    assert [M.digest_bytes(s, v) for s, v in zip(states, variants)] == [hashlib.sha384(msgs[0]).digest(), hashlib.sha512(msgs[1]).digest()]
    assert len(instance) == 14 and M.findings(d, cols, instance) == []
    swapped = instance[6:] + instance[:6]
    assert {f[0] for f in M.findings(d, cols, swapped)} == {"copy"}


def _set(cols, cell, row, value):
    cols[cell.column][row], cols[cell.column + 1][row] = value, M.spread(value)


def test_model_names_a_broken_witness(descriptions):
    """The evaluator is not vacuous: a flipped message bit, a wrong digest word, an over-long piece that recomposes to the
    same word and a set bit in a chunk above bit 63 are each found."""
    d = descriptions(1, SC.VARIANT_512, 16)  # at 16 bits the chunks 4 and 5 of every even / odd word start above bit 63
    msg = message(111)
    cols, digest = M.witness_one(msg, 1, d.table_bits, 1 << d.k)
    assert M.findings(d, cols, digest) == []
    piece = next(c for c in d.cells if c.kind == SC.SRC["W"] and c.form == SC.FORM_PAIR and c.offset == 8)
    base = SC.REGION_ROWS * (4 + 3)
    row = base + piece.row
    # a flipped message bit (W_3, bit 8): the word no longer recomposes; no lookup objects
    _set(cols, piece, row, cols[piece.column][row] ^ 1)
    kinds = {(kind, index) for kind, index, _ in M.findings(d, cols, digest)}
    assert ("gate", SC.GATES.index("w_word")) in kinds and not any(k == "lookup" for k, _ in kinds)
    _set(cols, piece, row, cols[piece.column][row] ^ 1)
    # a wrong digest word
    assert [f[0] for f in M.findings(d, cols, [digest[0] ^ 1] + digest[1:])] == ["copy"]
    assert [f[0] for f in M.findings(d, cols, digest[:7] + [digest[7] ^ (1 << 63)])] == ["copy"]
    # piece + 2^len with the next piece one less: the word is the same, the length lookup objects
    nxt = next(c for c in d.cells if c.kind == SC.SRC["W"] and c.form == SC.FORM_PAIR and c.offset == piece.offset + piece.len)
    assert nxt.row == piece.row and cols[nxt.column][row] > 0
    saved = cols[piece.column][row], cols[nxt.column][row]
    _set(cols, piece, row, saved[0] + (1 << piece.len))
    _set(cols, nxt, row, saved[1] - 1)
    found = M.findings(d, cols, digest)
    assert ("lookup", SC.PAIRS + piece.column // 2, row) in found and ("gate", SC.GATES.index("w_word"), base) not in found
    _set(cols, piece, row, saved[0])
    _set(cols, nxt, row, saved[1])
    assert M.findings(d, cols, digest) == []
    # a set bit in a chunk above bit 63 (chunk 4 of Sigma0's even word at 16 bits): no gate reads the cell, its length
    # lookup is the only constraint on it, and names it
    chunk = next(c for c in d.cells if c.kind == SC.SRC["S0_EVEN"] and c.form == SC.FORM_PAIR and not c.len and c.per_table_bits == 4)
    assert chunk.per_table_bits * d.table_bits >= 64 and cols[chunk.column][base + chunk.row] == 0
    _set(cols, chunk, base + chunk.row, 1)
    assert M.findings(d, cols, digest) == [("lookup", SC.PAIRS + chunk.column // 2, base + chunk.row)]
