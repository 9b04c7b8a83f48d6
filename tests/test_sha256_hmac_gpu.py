"""GPU: HMAC-SHA-256 through XOR-wired message words -- HmacSha256Circuit at k = 12 gives Python's hmac tag (and, with
commit_key, hashlib's SHA-256 of the key) for RFC 4231 cases 1 and 2, the witness checker accepts the synthesis and the
oracle's verifier the proof, and a changed result word or operand of any unit is named: the gate at the unit's second
region and the copy that ties the cell."""
import hashlib
import hmac

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import cq_verifier as CV
from oracle import plonk as PL
from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd.api import FAIL_GATE, FAIL_PERMUTATION, HmacSha256Circuit, Sha256BatchCircuit, Sha256SegmentsCircuit, fr_to_mont
from tests import sha256_circuit_model as M
from tests import sha256_xor_model as XM
from tests.test_sha256_choice_gpu import _oracle_expr
from tests.sha2_model import words_of
from tests.sha_oracle import mont_column as _mont

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
P16 = (SS.PRIVATE,) * 16
# RFC 4231 test cases 1 and 2; the second at table_bits 11
CASES = {"rfc1": (b"\x0b" * 20, b"Hi There", 12, "b0344c61d8db38535ca8afceaf0bf12b881dc200c9833da726e9376c2e32cff7"),
         "rfc2": (b"Jefe", b"what do ya want for nothing?", 11, "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843")}


def three_unit_plan():
    """Unit 0 = Var 0 ^ Const, unit 1 = Var 1 ^ Var 2 (segment 0, which also holds Vars 1 and 2 as words), unit 2 = digest
    word 1 of segment 0 ^ Var 0 (segment 1): every operand cell has a copy."""
    first = SS.Segment(1, (SS.Xor(SS.Var(0), SS.Const(0x5C5C5C5C)), SS.Xor(SS.Var(1), SS.Var(2)), SS.Var(1), SS.Var(2)) + P16[4:])
    second = SS.Segment(1, P16[:9] + (SS.Xor(SS.DigestWord(0, 1), SS.Var(0)),) + P16[10:])
    return SS.Plan((first, second), (1,))


THREE_VALUES = ([list(range(1, 13)), list(range(101, 116))], [0xA5A5A5A5, 0x01234567, 0x89ABCDEF])


@pytest.fixture(scope="module")
def circuits(ctx):
    made = {}

    def get(name, commit=False):
        if (name, commit) not in made:
            if name == "three":
                made[name, commit] = Sha256SegmentsCircuit(ctx, 11, three_unit_plan(), table_bits=11, seed=SEED)
            elif name == "batch":
                made[name, commit] = Sha256BatchCircuit(ctx, 12, [2, 2], seed=SEED)
            else:
                key, message, table_bits, _ = CASES[name]
                made[name, commit] = HmacSha256Circuit(ctx, 12, len(key), len(message), commit_key=commit, table_bits=table_bits, seed=SEED)
        return made[name, commit]

    yield get
    for c in made.values():
        c.close()


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
    assert cs.num_fixed_columns == len(SC.FIXED_XOR) and len(cs.gates) == len(SC.GATES_XOR) and len(cs.permutation_columns) == 3
    s = (seed * 0x9E3779B97F4A7C15 + 12345) % B.R_MOD
    N = 1 << c.table_bits
    tv = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
    fcm, pcm = c.pk.vk_commitments()

    def verify(proof, instance_words):
        return CV.verify_proof(proof, circ, c.vk_repr, s, tv, N, 1 << c.k, instances=[list(instance_words)],
                               fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))

    return verify


@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hmac_is_satisfied_proved_and_pythons_tag(circuits, name, commit):
    key, message, table_bits, rfc = CASES[name]
    c = circuits(name, commit)
    want = hmac.new(key, message, "sha256").digest()
    assert want.hex() == rfc
    assert c.rows == 2240 + 32 * (len(key) // 4) + (576 if commit else 0) <= SC.usable_rows(12) and c.table_bits == table_bits
    cols, inst = c.synthesize(key, message)
    values, shared, _ = c._inputs((key, message))
    model, digests, _ = XM.plan_witness(c.plan, values, shared, table_bits, c.n)
    for i, (got, exp) in enumerate(zip(cols, model)):
        assert np.array_equal(got.download((c.n, 4)), _mont(exp)), f"advice column {i}"
    assert c.digest_words == digests
    assert c.tag() == want
    instance = words_of(want)
    if commit:
        assert c.key_commitment() == hashlib.sha256(key).digest()
        instance += words_of(hashlib.sha256(key).digest())
    else:
        with pytest.raises(ValueError):
            c.key_commitment()
    assert [B.from_mont_limbs(inst[0])[i] for i in range(len(inst[0]))] == instance
    assert c.check(key, message) == (0, [])
    c.assert_satisfied(key, message)
    proof, tag = c.prove(key, message, seed=7)
    assert tag == want and len(proof) == c.pk.proof_size
    verify = _verifier(c, SEED)
    assert verify(proof, instance)
    wrong = list(instance)
    wrong[-1] ^= 1
    assert not verify(proof, wrong)
    with pytest.raises(ValueError):
        c.synthesize(key + b"\x00" * 4, message)


def test_an_xor_key_is_not_a_batch_key(circuits):
    """The XOR variant has one fixed column more, so its key is another key; the batch plan's key and proof stay what the
    existing tests pin."""
    x, b = circuits("rfc1"), circuits("batch")
    assert x.k == b.k and b.description.fixed_names == SC.FIXED and x.description.fixed_names == SC.FIXED_XOR
    fx, fb = x.pk.vk_commitments()[0], b.pk.vk_commitments()[0]
    assert len(fx) == len(fb) + 1 and not np.array_equal(np.asarray(fx)[: len(fb)], np.asarray(fb))
    key, message, _, _ = CASES["rfc1"]
    proof_x, _ = x.prove(key, message, seed=7)
    proof_b, _ = b.prove([bytes(100), bytes(100)], seed=7)
    assert proof_x != proof_b


# ---- a changed cell of a unit is named ------------------------------------------------------------------------------------------

def _write(c, column, row, value):
    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[column].ptr + 32 * row, v.ctypes.data, 32))


def _set_word(c, row0, kind, value):
    """The X cell of word `kind` (E or W) of the region at row0, the dense / spread pieces it decomposes into and, for E, its
    spread form in Y: the word's own recomposition gates and lookups still hold."""
    for cell in SC.layout():
        if cell.kind != SC.SRC[kind]:
            continue
        field = (value >> cell.offset) & ((1 << cell.len) - 1)
        _write(c, cell.column, row0 + cell.row, M.spread(field) if cell.form == SC.FORM_SPREAD else field)
        if cell.form == SC.FORM_PAIR:
            _write(c, cell.column + 1, row0 + cell.row, M.spread(field))


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
    assert len(SS.xor_units(c.plan)) == 3 and _found(c) == set()
    X = c.description.advice[XM.X]
    u0, u1 = XM.unit_rows(c.plan, unit)
    x_cols = c.cols[XM.X].download((c.n, 4))
    if what == "W":
        # another 32-bit word in the W cell with its row-2 pieces: `w_word` holds, the sigma cells are the old word's
        row0, cell = u1, u1 + XM.ROW["W"]
        old = B.from_mont_limbs(x_cols[cell: cell + 1])[0]
        _set_word(c, row0, "W", old ^ 0x00010000)
        gates = {_gate("xor_word", u1), _gate("sigma0_even_odd", u1), _gate("sigma1_even_odd", u1)}
    else:
        # another 32-bit word in an operand's E cell with its pieces and spread form: `e_word` and `e_spread` hold
        row0 = u0 if what == "x" else u1
        cell = row0 + XM.ROW["E"]
        old = B.from_mont_limbs(x_cols[cell: cell + 1])[0]
        _set_word(c, row0, "E", old ^ 0x4)
        gates = {_gate("chp_even_odd", u1), _gate("Sigma1_even_odd", row0)}
        if what == "y":  # ~e of this region, and e two regions back of the next unit's second region
            gates |= {_gate("chq_even_odd", u1)} | ({_gate("chq_even_odd", XM.unit_rows(c.plan, unit + 1)[1])} if unit < 2 else set())
    found = _found(c)
    assert {f for f in found if f[0] == FAIL_GATE} == gates
    assert _gate("xor_word", u1) in found or _gate("chp_even_odd", u1) in found
    cycle = _cycle(c, (X, cell))
    permutation = found - gates
    assert len(cycle) >= 2 and (FAIL_PERMUTATION, 0, cell) in permutation and permutation <= cycle and len(permutation) == 2
