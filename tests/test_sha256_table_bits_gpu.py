"""GPU: the SHA-256 compression circuit under keys whose tables have 2^11 rows -- the narrowest the pieces fit, where the
top chunk of every even / odd word has 10 bits -- and 2^13 rows, where it has 6: the witness checker accepts the synthesis
and names a tampered top chunk by its lookup, and a proof verifies against its own digest only.  (Every width is compared
cell for cell, without a key, in test_sha256_launch_shapes_gpu.py; 2^16 rows only there.)"""
import hashlib

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd.api import FAIL_STATIC_LOOKUP, Sha256Circuit, fr_to_mont
from tests import sha256_circuit_model as M
from tests.test_sha256_circuit_gpu import SEED, _verifier

pytestmark = pytest.mark.gpu
K = 10
MESSAGE = bytes((151 * i + 7) % 256 for i in range(55))


@pytest.fixture(scope="module", params=[11, 13])
def circuit(ctx, request):
    c = Sha256Circuit(ctx, K, 1, table_bits=request.param, seed=SEED)
    yield c
    c.close()


def test_the_synthesis_is_the_models_and_is_accepted(circuit):
    c = circuit
    assert c.check(MESSAGE) == (0, [])
    want, digest = M.witness(MESSAGE, 1, c.table_bits, c.n)
    for i, (got, exp) in enumerate(zip(c.cols, want)):
        assert np.array_equal(got.download((c.n, 4)), SC._mont_column(np.array(exp, dtype=np.uint64))), f"advice column {i}"
    assert c.digest == hashlib.sha256(MESSAGE).digest() == M.digest_bytes(digest)


def test_a_tampered_top_chunk_is_named_by_its_lookup(circuit):
    """The dense cell of the top chunk of Sigma1's odd word in round 9 set to 2^table_bits, its spread cell left alone: no row of
    the tables.  The pair lookup and the length lookup of the cell's slot name the row, and nothing else does: no gate
    reads the dense cell of a chunk of Sigma1's odd word (the even / odd gate reads the spread cell)."""
    c = circuit
    c.synthesize(MESSAGE)
    cell = next(x for x in c.description.cells if x.kind == SC.SRC["S1_ODD"] and x.form == SC.FORM_PAIR and x.per_table_bits == 2)
    assert SC._field_of(cell, c.table_bits) == {11: (22, 10), 13: (26, 6)}[c.table_bits]
    row = SC.REGION_ROWS * (4 + 9) + cell.row
    v = np.ascontiguousarray(fr_to_mont(1 << c.table_bits), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[cell.column].ptr + 32 * row, v.ctypes.data, 32))
    total, fails = c.pk.check_witness([x.ptr for x in c.cols], instances=c.instances, max_failures=256)
    found = {(f.kind, f.index, f.row) for f in fails}
    assert total == len(fails) == len(found)
    slot = cell.column // 2
    assert found == {(FAIL_STATIC_LOOKUP, slot, row), (FAIL_STATIC_LOOKUP, SC.PAIRS + slot, row)}


def test_a_proof_verifies_against_its_digest_only(circuit):
    c = circuit
    proof, digest = c.prove(MESSAGE, seed=7)
    assert len(proof) == c.pk.proof_size and digest == hashlib.sha256(MESSAGE).digest()
    verify = _verifier(c, SEED)
    assert verify(proof, list(c.digest_words))
    other = hashlib.sha256(MESSAGE[:-1] + b"\x00").digest()
    assert not verify(proof, [int.from_bytes(other[4 * i: 4 * i + 4], "big") for i in range(8)])
