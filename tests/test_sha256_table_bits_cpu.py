"""CPU: the SHA-256 circuits at table widths other than 12.  Chunk c of an even / odd word holds bits
[c * table_bits, (c + 1) * table_bits) as far as the word goes: at 11 the top chunk has 10 bits, at 13 it has 6, at 16 it
starts at bit 32 and is always zero.  The models' witnesses satisfy every description at these widths, and the models
name a tampered top chunk at the two edges."""
import hashlib
import struct

import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha256_choice_model as CM
from tests import sha256_circuit_model as M
from tests import sha256_segments_model as SM
from tests import sha256_varlen_model as VM

WIDTHS = [11, 13, 16]


def message(length, salt=0):
    return bytes((151 * i + 13 * salt) % 256 for i in range(length))


@pytest.mark.parametrize("table_bits", WIDTHS)
@pytest.mark.parametrize("blocks,k,length", [(1, 10, 55), (2, 11, 119)])
def test_single_message_witness_satisfies_the_description(table_bits, blocks, k, length):
    msg = message(length, table_bits)
    d = SC.describe(k, blocks, table_bits=table_bits)
    cols, digest = M.witness(msg, blocks, table_bits, 1 << k)
    assert M.digest_bytes(digest) == hashlib.sha256(msg).digest()
    assert M.findings(d, cols, digest) == []


@pytest.mark.parametrize("table_bits", WIDTHS)
def test_wired_plan_witness_satisfies_the_description(table_bits):
    plan, values = SS.double_sha256(1), [SC.pad(message(55, table_bits), 1), []]
    d = SS.describe(11, plan, table_bits=table_bits)
    cols = SM.witness(plan, values, table_bits, 1 << 11)
    assert M.findings(d, cols, SM.instance_words(plan, values)) == []


@pytest.mark.parametrize("table_bits", WIDTHS)
def test_choice_plan_witness_satisfies_the_description(table_bits):
    plan = SS.merkle_path(1)
    leaf, sibling = hashlib.sha256(b"leaf").digest(), hashlib.sha256(b"sibling").digest()
    values, shared, bits = CM.path_inputs(1, [(leaf, 1, [sibling])])
    d = SS.describe(11, plan, table_bits=table_bits)
    cols = CM.witness(plan, values, shared, bits, table_bits, 1 << 11)
    instance = CM.instance_words(plan, values, shared, bits)
    assert instance == list(struct.unpack(">8I", CM.path_root(leaf, 1, [sibling])))
    assert CM.findings(d, cols, instance) == []


@pytest.mark.parametrize("table_bits", [tb for tb in WIDTHS if tb >= SV.MIN_TABLE_BITS])
def test_varlen_witness_satisfies_the_description(table_bits):
    messages, max_blocks = [message(53, table_bits)], [1]
    d = SV.describe(10, max_blocks, table_bits=table_bits)
    cols, digests = VM.witness(messages, max_blocks, table_bits, 1 << 10)
    assert M.digest_bytes(digests[0]) == hashlib.sha256(messages[0]).digest()
    assert VM.findings(d, cols, VM.instance_words(messages, max_blocks)) == []


def test_varlen_is_refused_below_twelve_bits():
    with pytest.raises(ValueError, match="table_bits"):
        SV.describe(10, [1], table_bits=11)


@pytest.mark.parametrize("table_bits,value", [(11, 1 << 10), (16, 1)])
def test_a_tampered_top_chunk_is_named(table_bits, value):
    """The top chunk of Sigma0's even word in round 5, its dense and spread cell changed together so that the pair stays a
    row of the tables.  At 11 bits the chunk's field is bits 22 .. 31: bit 10 of the cell would be bit 32 of the word.  At
    16 the field starts at bit 32: anything but zero is wrong.  No lookup objects -- the value is below 2^table_bits --
    and the two gates that read the chunk both do: its weight 2^(2 * table_bits), or 4^(2 * table_bits) in the spread
    form, is not zero in the field."""
    msg = message(55, 1)
    d = SC.describe(10, 1, table_bits=table_bits)
    cols, digest = M.witness(msg, 1, table_bits, 1 << 10)
    cell = next(c for c in d.cells if c.kind == SC.SRC["S0_EVEN"] and c.form == SC.FORM_PAIR and c.per_table_bits == 2)
    base = SC.REGION_ROWS * (4 + 5)
    row = base + cell.row
    honest = cols[cell.column][row]
    assert honest < value and (honest == 0) == (table_bits == 16)
    assert SC._field_of(cell, table_bits) == ((22, 10) if table_bits == 11 else (32, 0))
    cols[cell.column][row], cols[cell.column + 1][row] = honest | value, M.spread(honest | value)
    gates = {("gate", SC.GATES.index(name), base) for name in ("Sigma0_even_odd", "Sigma0_word")}
    assert set(M.findings(d, cols, digest)) == gates
