"""GPU: the SHA-512 / SHA-384 compression circuit -- the synthesised witness equals the pure-Python model cell for cell,
the witness checker accepts it and names every kind of tampering, and proofs verify against the right digests only."""
import hashlib

import numpy as np
import pytest

from oracle import bn254 as B
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd.api import (FAIL_GATE, FAIL_PERMUTATION, FAIL_STATIC_LOOKUP, Sha384Circuit, Sha512BatchCircuit, Sha512Circuit,
                                      fr_to_mont)
from tests import sha512_circuit_model as M
from tests.sha512_direct import mont_column
from tests.sha_oracle import verifier as _verifier
from tests.sha_oracle import write_cell as _write
from tests.sha2_model import message

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
K_FOR = {1: 11, 2: 12}  # the smallest k that holds the block count
V512, V384 = SC.VARIANT_512, SC.VARIANT_384
CLASS = {V512: Sha512Circuit, V384: Sha384Circuit}
HASH = {V512: hashlib.sha512, V384: hashlib.sha384}


MESSAGES = {"empty": (1, b""), "111": (1, message(111, 1)), "112": (2, message(112, 2)), "239": (2, message(239, 3)),
            "ones": (2, b"\xff" * 128), "zeros": (2, b"\x00" * 128)}
CASES = [(name, V512) for name in sorted(MESSAGES)] + [("111", V384), ("239", V384)]


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(blocks, variant=V512):
        if (blocks, variant) not in made:
            made[blocks, variant] = CLASS[variant](ctx, K_FOR[blocks], blocks, seed=SEED)
        return made[blocks, variant]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("case,variant", CASES)
def test_synthesis_equals_the_model_and_is_accepted(circuits, case, variant):
    blocks, msg = MESSAGES[case]
    c = circuits(blocks, variant)
    cols, inst = c.synthesize(msg)
    want, instance, (state,) = M.witness([msg], [blocks], [variant], c.table_bits, c.n)
    for i, (got, exp) in enumerate(zip(cols, want)):
        assert np.array_equal(got.download((c.n, 4)), mont_column(exp)), f"advice column {i}"
    assert c.digest == HASH[variant](msg).digest() == M.digest_bytes(state, variant)
    assert c.digest_words == instance and len(instance) == SC.DIGEST_WORDS[variant]
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(instance))] == instance
    assert c.check(msg) == (0, [])
    c.assert_satisfied(msg)


def _region_row(blocks_before, round_):
    return SC.REGION_ROWS * (SC.BLOCK_REGIONS * blocks_before + 4 + round_)


def _cell(c, name, form=SC.FORM_PAIR, **where):
    return next(x for x in c.description.cells if x.kind == SC.SRC[name] and x.form == form and all(getattr(x, k) == v for k, v in where.items()))


def _read(c, column, row):
    return B.from_mont_limbs(c.cols[column].download((c.n, 4))[row: row + 1])[0]


def _findings(c, instances=None):
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=instances if instances is not None else c.instances, max_failures=256)
    assert total == len(fails) and total > 0
    return {(f.kind, f.index, f.row) for f in fails}


def _gate(name, base):
    return (FAIL_GATE, SC.GATES.index(name), base)


def test_a_wrong_witness_is_named(circuits):
    """Each tampering starts from the honest witness of a two-block message; the kind, the constraint and the region
    of the findings are the ones the layout predicts."""
    c = circuits(2)
    msg = MESSAGES["239"][1]
    X, perm_x = 2 * SC.PAIRS, 0  # the word column: advice column 16, first column of the permutation

    # one bit of a message-word piece (block 1, W_5): the word no longer recomposes, sigma0 / sigma1 no longer decompose
    c.synthesize(msg)
    base = _region_row(1, 5)
    p = _cell(c, "W", offset=19)
    v = _read(c, p.column, base + p.row) ^ 4
    _write(c, p.column, base + p.row, v)
    _write(c, p.column + 1, base + p.row, M.spread(v))
    assert _findings(c) == {_gate("w_word", base), _gate("sigma0_even_odd", base), _gate("sigma1_even_odd", base)}

    # one carry incremented (block 0, round 20, the carry of e): only that addition fails, the carry is still in range
    c.synthesize(msg)
    base = _region_row(0, 20)
    p = _cell(c, "CARRY_E")
    v = _read(c, p.column, base + p.row) + 1
    assert v < 8
    _write(c, p.column, base + p.row, v)
    _write(c, p.column + 1, base + p.row, M.spread(v))
    assert _findings(c) == {_gate("e_add", base)}

    # an even chunk of Maj swapped with its odd chunk (block 1, round 9)
    c.synthesize(msg)
    base = _region_row(1, 9)
    ev, od = _cell(c, "MAJ_EVEN", per_table_bits=0), _cell(c, "MAJ_ODD", per_table_bits=0)
    a, b = _read(c, ev.column, base + ev.row), _read(c, od.column, base + od.row)
    assert a != b
    for cell, v in ((ev, b), (od, a)):
        _write(c, cell.column, base + cell.row, v)
        _write(c, cell.column + 1, base + cell.row, M.spread(v))
    assert _findings(c) == {_gate("maj_even_odd", base), _gate("maj_word", base)}

    # one digest word changed in the instance, in its upper half: the copy from the last regions no longer holds
    c.synthesize(msg)
    inst = [c.instances[0].copy()]
    inst[0][2] = fr_to_mont(c.digest_words[2] ^ (1 << 47))
    tail = SC.REGION_ROWS * (SC.BLOCK_REGIONS * 2 + 3 - 2)
    found = _findings(c, inst)
    assert {f[0] for f in found} == {FAIL_PERMUTATION}
    assert (FAIL_PERMUTATION, perm_x, tail + _cell(c, "A", SC.FORM_WORD).row) in found and (FAIL_PERMUTATION, 2, 2) in found

    # a round-constant use detached: the witness copy of K_70 changed, the fixed cell untouched
    c.synthesize(msg)
    base = _region_row(0, 70)
    kc = _cell(c, "K", SC.FORM_WORD)
    assert kc.column == X
    _write(c, kc.column, base + kc.row, SC.K512[70] + 1)
    found = _findings(c)
    assert {(FAIL_PERMUTATION, perm_x, base + kc.row), (FAIL_PERMUTATION, 1, base + kc.row), _gate("e_add", base), _gate("a_add", base)} == found

    # a piece one bit too long that recomposes to the same word (block 0, e_40: piece + 2^len, the next piece one less):
    # the (dense, spread) lookup still holds, the length lookup does not
    c.synthesize(msg)
    base = _region_row(0, 40)
    p, nxt = _cell(c, "E", offset=7), _cell(c, "E", offset=14)
    assert p.offset + p.len == nxt.offset and p.row == nxt.row
    lo, hi = _read(c, p.column, base + p.row), _read(c, nxt.column, base + nxt.row)
    assert hi > 0
    for cell, v in ((p, lo + (1 << p.len)), (nxt, hi - 1)):
        _write(c, cell.column, base + cell.row, v)
        _write(c, cell.column + 1, base + cell.row, M.spread(v))
    found = _findings(c)
    assert (FAIL_STATIC_LOOKUP, SC.PAIRS + p.column // 2, base + p.row) in found
    assert _gate("e_word", base) not in found and not any(f[0] == FAIL_STATIC_LOOKUP and f[1] < SC.PAIRS for f in found)
    assert all(f[2] in (base, base + p.row) for f in found)


def _words(digest):
    return [int.from_bytes(digest[8 * i: 8 * i + 8], "big") for i in range(len(digest) // 8)]


@pytest.mark.parametrize("blocks,variant", [(1, V512), (2, V384)])
def test_proofs_verify_against_their_digest_only(circuits, blocks, variant):
    c = circuits(blocks, variant)
    msg = MESSAGES["111" if blocks == 1 else "239"][1]
    proof, digest = c.prove(msg, seed=7)
    assert len(proof) == c.pk.proof_size and digest == HASH[variant](msg).digest()
    assert c.prove(msg, seed=7) == (proof, digest)
    assert c.prove(msg, seed=8)[0] != proof
    verify = _verifier(c, SEED)
    assert c.digest_words == _words(digest)
    assert verify(proof, c.digest_words)
    assert not verify(proof, _words(HASH[variant](msg[:-1] + b"\x00").digest()))


def test_a_batch_proof_verifies_against_its_22_words(ctx):
    """Three independent messages of 1, 2 and 1 blocks, the last SHA-384, in one proof."""
    msgs, variants = [message(100, 5), message(239, 6), message(3, 7)], [V512, V512, V384]
    c = Sha512BatchCircuit(ctx, 13, [1, 2, 1], variants, seed=SEED)
    try:
        assert c.check(msgs) == (0, [])
        want, instance, _ = M.witness(msgs, [1, 2, 1], variants, c.table_bits, c.n)
        for i, (got, exp) in enumerate(zip(c.cols, want)):
            assert np.array_equal(got.download((c.n, 4)), mont_column(exp)), f"advice column {i}"
        proof, digests = c.prove(msgs, seed=3)
        assert digests == [hashlib.sha512(msgs[0]).digest(), hashlib.sha512(msgs[1]).digest(), hashlib.sha384(msgs[2]).digest()]
        words = [w for d in digests for w in _words(d)]
        assert len(words) == 22 and words == c.digest_words == instance
        verify = _verifier(c, SEED)
        assert verify(proof, words)
        assert not verify(proof, words[8:16] + words[:8] + words[16:])
    finally:
        c.close()


def test_powers_setup_gives_the_same_proof(ctx, circuits):
    msg = MESSAGES["111"][1]
    toxic = circuits(1).prove(msg, seed=7)
    c = Sha512Circuit(ctx, K_FOR[1], 1, seed=SEED, setup="powers")
    try:
        assert c.prove(msg, seed=7) == toxic
    finally:
        c.close()


def test_block_count_and_rows(ctx, circuits):
    c = circuits(1)
    assert c.rows_per_block == SC.BLOCK_REGIONS * SC.REGION_ROWS and c.rows == SC.rows_for(1) <= c.pk.usable_rows
    assert SC.max_blocks(11) == 1 and SC.max_blocks(12) == 2 and SC.max_blocks(10) == 0
    with pytest.raises(ValueError):
        c.synthesize(message(112))
    with pytest.raises(ValueError):
        Sha512Circuit(ctx, 10)
