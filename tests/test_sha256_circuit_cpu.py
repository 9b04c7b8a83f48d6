"""CPU: the SHA-256 compression circuit's padding, its constraint-system description against the library's limits, and
the pure-Python model's witness against every gate, lookup and copy -- and against hashlib."""
import hashlib
import re
import struct

import pytest

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from tests import sha256_circuit_model as M
from tests.sha2_model import message

MESSAGES = {0: 1, 1: 1, 55: 1, 56: 2, 63: 2, 64: 2, 119: 2}


@pytest.mark.parametrize("length,blocks", sorted(MESSAGES.items()))
def test_pad_gives_the_standard_padding(length, blocks):
    msg = message(length)
    words = SC.pad(msg)
    raw = struct.pack(f">{len(words)}I", *words)
    assert len(raw) == 64 * blocks
    assert raw[:length] == msg and raw[length] == 0x80
    assert raw[length + 1:-8] == b"\x00" * (64 * blocks - length - 9)
    assert int.from_bytes(raw[-8:], "big") == 8 * length
    assert SC.pad(msg, blocks) == words
    with pytest.raises(ValueError):
        SC.pad(msg, blocks + 1)


def test_description_stays_inside_the_library_limits():
    """At most CQ_MAX_LOOKUPS lookups of at most CQ_MAX_WIDTH table columns, at most PERM_MAX_COLUMNS permutation
    columns (the constants of csrc/poly.hpp, cq.hpp and plonk.hpp), a gate degree the fixtures reach (5), and an
    expression depth the gate interpreter's operand stack holds."""
    import os

    csrc = os.path.join(os.path.dirname(os.path.abspath(SC.__file__)), "csrc")
    limit = lambda f, name: int(re.search(name + r"\s*=\s*(\d+)", open(os.path.join(csrc, f)).read()).group(1))
    d = SC.describe(10, 1)
    cs = d.cs
    assert len(cs.static_lookups) <= limit("poly.hpp", "CQ_MAX_LOOKUPS")
    assert max(len(lk) for lk in cs.static_lookups) <= limit("cq.hpp", "CQ_MAX_WIDTH")
    assert len(cs.permutation_columns) <= limit("plonk.hpp", "PERM_MAX_COLUMNS")
    assert cs.degree() <= 5
    assert cs.num_advice_columns == SC.ADVICE_COLUMNS and cs.num_instance_columns == 1 and len(cs.gates) == len(SC.GATES)
    stack = limit("plonk.hpp", "GATE_STACK")
    for e in cs.gates + cs._lookup_exprs:
        depth = best = 0
        for word in _postfix_effects(e.compile([])):
            depth += word
            best = max(best, depth)
        assert best <= stack
    # both tables have one size, and the rows of the largest block count fit
    for k in (10, 11, 14):
        b = SC.max_blocks(k)
        assert b >= 1 and SC.rows_for(b) <= (1 << k) - (cs.blinding_factors() + 1) < SC.rows_for(b + 1)
    with pytest.raises(ValueError):
        SC.describe(10, 2)
    with pytest.raises(ValueError):
        SC.describe(10, 1, table_bits=10)


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


def test_layout_table_is_consistent():
    """Every word's pieces tile its 32 bits, no two cells share a place, and no piece is wider than the smallest table."""
    cells = SC.layout()
    places = [(c.column + d, c.row) for c in cells for d in ((0, 1) if c.form == SC.FORM_PAIR else (0,))]
    assert len(places) == len(set(places))
    assert all(c.row < SC.REGION_ROWS and c.column < SC.ADVICE_COLUMNS for c in cells)
    for name in ("A", "E", "W"):
        ps = sorted((c.offset, c.len) for c in cells if c.kind == SC.SRC[name] and c.form == SC.FORM_PAIR)
        assert ps[0][0] == 0 and all(a + l == b for (a, l), (b, _) in zip(ps, ps[1:])) and sum(ps[-1]) == 32
        assert max(l for _, l in ps) <= SC.MIN_TABLE_BITS
    for name, v in SC.SRC.items():
        if name.endswith(("_EVEN", "_ODD")):
            assert sorted(c.per_table_bits for c in cells if c.kind == v and c.form == SC.FORM_PAIR) == [0, 1, 2]
    assert 3 * SC.MIN_TABLE_BITS >= 32


@pytest.fixture(scope="module")
def descriptions():
    return {b: SC.describe(10 if b == 1 else 11, b) for b in (1, 2)}


@pytest.mark.parametrize("length", sorted(MESSAGES))
def test_model_witness_satisfies_the_circuit_and_gives_the_digest(descriptions, length):
    msg = message(length, salt=length)
    d = descriptions[MESSAGES[length]]
    cols, digest = M.witness(msg, d.blocks, d.table_bits, 1 << d.k)
    assert M.digest_bytes(digest) == hashlib.sha256(msg).digest()
    assert M.findings(d, cols, digest) == []


def test_model_names_a_broken_witness(descriptions):
    """The evaluator is not vacuous: a flipped message bit, a wrong digest word and an over-long piece are each found."""
    d = descriptions[1]
    msg = message(55)
    cols, digest = M.witness(msg, 1, d.table_bits, 1 << d.k)
    piece = next(c for c in d.cells if c.kind == SC.SRC["W"] and c.form == SC.FORM_PAIR and c.offset == 0)
    row = SC.REGION_ROWS * (4 + 3) + piece.row
    cols[piece.column][row] ^= 1
    cols[piece.column + 1][row] ^= 1
    kinds = {(kind, index) for kind, index, _ in M.findings(d, cols, digest)}
    assert ("gate", SC.GATES.index("w_word")) in kinds and not any(k == "lookup" for k, _ in kinds)
    cols[piece.column][row] ^= 1
    cols[piece.column + 1][row] ^= 1
    assert [f[0] for f in M.findings(d, cols, [digest[0] ^ 1] + digest[1:])] == ["copy"]
    # piece + 2^len with the next piece one less: the word is the same, the length lookup objects
    nxt = next(c for c in d.cells if c.kind == SC.SRC["W"] and c.form == SC.FORM_PAIR and c.offset == piece.offset + piece.len)
    assert cols[nxt.column][row] > 0
    for c, v in ((piece, cols[piece.column][row] + (1 << piece.len)), (nxt, cols[nxt.column][row] - 1)):
        cols[c.column][row], cols[c.column + 1][row] = v, M.spread(v)
    found = M.findings(d, cols, digest)
    assert ("lookup", SC.PAIRS + piece.column // 2, row) in found and ("gate", SC.GATES.index("w_word"), row - piece.row) not in found
