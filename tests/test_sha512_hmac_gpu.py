"""GPU: HMAC-SHA-512 and HMAC-SHA-384 through XOR-wired message words -- HmacSha512Circuit / HmacSha384Circuit at k = 13
(k = 14 for a 128-byte key with commit_key) give Python's hmac tag (and, with commit_key, hashlib's hash of the key), the
columns are the model's, the witness checker accepts the synthesis and the oracle's verifier the proof, and a changed result
word or operand of any unit is named: the gate at the unit's second region and the copy that ties the cell."""
import hashlib
import hmac

import numpy as np
import pytest

from oracle import bn254 as B
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from sha2_on_cq_halo2_amd import sha512_xor as SX
from sha2_on_cq_halo2_amd.api import FAIL_GATE, FAIL_PERMUTATION, HmacSha384Circuit, HmacSha512Circuit, Sha512BatchCircuit, Sha512XorSegmentsCircuit
from sha2_on_cq_halo2_amd.sha2_segments import Xor
from tests import sha512_xor_model as XM
from tests.sha2_model import spread, words_of
from tests.sha_oracle import mont_column, verifier, write_cell

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
P16 = (SS.PRIVATE,) * 16
KEY = bytes((29 * i + 7) % 256 for i in range(128))
MESSAGE = bytes((13 * i + 5) % 256 for i in range(120))
# name: (circuit, hash, k, key bytes, message bytes, commit_key, table_bits): an 8-byte key with an empty message, a committed
# key at table width 11, a 128-byte key, a message of two blocks, and the one shape that needs k = 14
CASES = {"key8_empty": (HmacSha512Circuit, "sha512", 13, 8, 0, False, 12),
         "key16_commit": (HmacSha512Circuit, "sha512", 13, 16, 8, True, 11),
         "key128_sha384": (HmacSha384Circuit, "sha384", 13, 128, 104, False, 12),
         "two_blocks_sha384": (HmacSha384Circuit, "sha384", 13, 64, 120, False, 12),
         "key128_commit": (HmacSha512Circuit, "sha512", 14, 128, 8, True, 12)}


def three_unit_plan():
    """Unit 0 = Var 0 ^ Const, unit 1 = Var 1 ^ Var 2 (segment 0, which also holds Vars 1 and 2 as words), unit 2 = word 1
    of segment 0's final state ^ Var 0 (segment 1, SHA-384): every operand cell has a copy."""
    first = SS.Segment(1, (Xor(SS.Var(0), SS.Const(XM.OPAD)), Xor(SS.Var(1), SS.Var(2)), SS.Var(1), SS.Var(2)) + P16[4:])
    second = SS.Segment(1, P16[:9] + (Xor(SS.DigestWord(0, 1), SS.Var(0)),) + P16[10:], None, SC.VARIANT_384)
    return SS.Plan((first, second), ((1, 6),))


THREE_VALUES = ([list(range(1, 13)), list(range(101, 116))], [0xA5A5A5A5A5A5A5A5, 0x0123456789ABCDEF, 0x8000000000000001])


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(name):
        if name not in made:
            if name == "three":
                made[name] = Sha512XorSegmentsCircuit(ctx, 12, three_unit_plan(), table_bits=11, seed=SEED)
            elif name == "batch":
                made[name] = Sha512BatchCircuit(ctx, 13, [2, 2], seed=SEED)
            else:
                cls, _, k, key_bytes, message_bytes, commit, table_bits = CASES[name]
                made[name] = cls(ctx, k, key_bytes, message_bytes, commit_key=commit, table_bits=table_bits, seed=SEED)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hmac_is_satisfied_proved_and_pythons_tag(circuits, name):
    cls, hash_name, k, key_bytes, message_bytes, commit, table_bits = CASES[name]
    key, message = KEY[:key_bytes], MESSAGE[:message_bytes]
    c = circuits(name)
    want = hmac.new(key, message, hash_name).digest()
    assert c.rows == SX.rows_for(c.plan) <= SC.usable_rows(k) and (k == 13 or c.rows > SC.usable_rows(13)) and c.table_bits == table_bits
    assert c.rows == 1344 * (3 + -(-(message_bytes + 17) // 128)) + 128 + 64 * (key_bytes // 8) + (SC.rows_for(1 + (key_bytes > 104)) if commit else 0)
    cols, inst = c.synthesize(key, message)
    values, shared, _ = c._inputs((key, message))
    model, states, _ = XM.plan_witness(c.plan, values, shared, table_bits, c.n)
    for i, (got, exp) in enumerate(zip(cols, model)):
        assert np.array_equal(got.download((c.n, 4)), mont_column(exp)), f"advice column {i}"
    assert c.state_words == states
    assert c.tag() == want and len(want) == 8 * SC.DIGEST_WORDS[c.variant]
    instance = words_of(want, XM.W)
    if commit:
        assert c.key_commitment() == hashlib.new(hash_name, key).digest()
        instance += words_of(hashlib.new(hash_name, key).digest(), XM.W)
    else:
        with pytest.raises(ValueError):
            c.key_commitment()
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(inst[0]))] == instance == XM.instance_of(c.plan, states)
    assert c.check(key, message) == (0, [])
    c.assert_satisfied(key, message)
    proof, tag = c.prove(key, message, seed=7)
    assert tag == want and len(proof) == c.pk.proof_size
    assert c.cs.num_fixed_columns == len(SC.FIXED_XOR) and len(c.cs.gates) == len(SC.GATES_XOR) and len(c.cs.permutation_columns) == 3
    verify = verifier(c, SEED)
    assert verify(proof, instance)
    wrong = list(instance)
    wrong[3] ^= 1
    assert not verify(proof, wrong)
    with pytest.raises(ValueError):
        c.synthesize(key + b"\x00" * 8, message)


def test_an_xor_key_is_not_a_batch_key(circuits):
    """The XOR variant has one fixed column more, so its key is another key; the batch circuit's key and proof stay what the
    existing tests pin."""
    x, b = circuits("key8_empty"), circuits("batch")
    assert x.k == b.k and b.description.fixed_names == SC.FIXED and x.description.fixed_names == SC.FIXED_XOR
    fx, fb = x.pk.vk_commitments()[0], b.pk.vk_commitments()[0]
    assert len(fx) == len(fb) + 1 and not np.array_equal(np.asarray(fx)[: len(fb)], np.asarray(fb))
    proof_x, _ = x.prove(KEY[:8], b"", seed=7)
    proof_b, _ = b.prove([bytes(200), bytes(200)], seed=7)
    assert proof_x != proof_b


# ---- a changed cell of a unit is named ------------------------------------------------------------------------------------------

def _set_word(c, row0, kind, value):
    """The X cell of word `kind` (E or W) of the region at row0, the dense / spread pieces it decomposes into and, for E, its
    spread form in Y: the word's own recomposition gates and lookups still hold."""
    for cell in SC.layout():
        if cell.kind != SC.SRC[kind]:
            continue
        field = (value >> cell.offset) & ((1 << cell.len) - 1)
        write_cell(c, cell.column, row0 + cell.row, spread(field) if cell.form == SC.FORM_SPREAD else field)
        if cell.form == SC.FORM_PAIR:
            write_cell(c, cell.column + 1, row0 + cell.row, spread(field))


def _found(c):
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert total == len(fails) == len(found)
    return found


def _gate(name, row):
    return (FAIL_GATE, SC.GATES_XOR.index(name), row)


def _cycle(c, cell):
    """Every cell the description's copies tie to `cell`, as the checker names them: (FAIL_PERMUTATION, index of the column
    among the permutation columns, row)."""
    tied, grew = {cell}, True
    while grew:
        grew = False
        for a, b in c.description.copies:
            if (a in tied) != (b in tied):
                tied |= {a, b}
                grew = True
    return {(FAIL_PERMUTATION, c.cs.permutation_columns.index(col), row) for col, row in tied}


@pytest.mark.parametrize("what", ["W", "x", "y"])
@pytest.mark.parametrize("unit", range(3))
def test_a_changed_cell_of_every_unit_is_named(circuits, unit, what):
    c = circuits("three")
    values, shared = THREE_VALUES
    c.synthesize(values, shared)
    assert len(SX.xor_units(c.plan)) == 3 and _found(c) == set()
    X = c.description.advice[XM.X]
    u0, u1 = XM.unit_rows(c.plan, unit)
    x_cols = c.cols[XM.X].download((c.n, 4))
    if what == "W":
        # another 64-bit word in the W cell with its pieces: `w_word` holds, the sigma cells are the old word's
        row0, cell = u1, u1 + XM.ROW["W"]
        old = B.from_mont_limbs(x_cols[cell: cell + 1])[0]
        _set_word(c, row0, "W", old ^ (1 << 48))
        gates = {_gate("xor_word", u1), _gate("sigma0_even_odd", u1), _gate("sigma1_even_odd", u1)}
    else:
        # another 64-bit word in an operand's E cell with its pieces and spread form: `e_word` and `e_spread` hold
        row0 = u0 if what == "x" else u1
        cell = row0 + XM.ROW["E"]
        old = B.from_mont_limbs(x_cols[cell: cell + 1])[0]
        _set_word(c, row0, "E", old ^ (1 << 35))
        gates = {_gate("chp_even_odd", u1), _gate("Sigma1_even_odd", row0)}
        if what == "y":  # ~e of this region, and e two regions back of the next unit's second region
            gates |= {_gate("chq_even_odd", u1)} | ({_gate("chq_even_odd", XM.unit_rows(c.plan, unit + 1)[1])} if unit < 2 else set())
    found = _found(c)
    assert {f for f in found if f[0] == FAIL_GATE} == gates
    assert _gate("xor_word", u1) in found or _gate("chp_even_odd", u1) in found
    cycle = _cycle(c, (X, cell))
    permutation = found - gates
    assert len(cycle) >= 2 and (FAIL_PERMUTATION, 0, cell) in permutation and permutation <= cycle and len(permutation) == 2
