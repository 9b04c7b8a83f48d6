"""CPU: what the SHA-2 test models compute, pinned.  Every entry of tests/golden/sha2_model_pins.json is the SHA-256 digest of the
canonical JSON of one model call's whole result -- all 18 columns, the instance or digest words, the chaining values, or a list of
findings -- at both word widths and through every model module, at the smallest n that holds the case.  The fixture was generated
from the per-width models, before they were written once over a width record in tests/sha2_model.py; regenerate it
(`python -m tests.test_sha2_model_pins_cpu`; its "constants" entry then reads the names the bindings export) only for a change
that means to alter what a model computes.  The second test holds the
round constants and initial hash values the models derive from the primes to the package's tables.  Needs the built library's
host entry points (the layout tables), no GPU."""
import hashlib
import json
import os
import random

import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as S256
from sha2_on_cq_halo2_amd import sha256_segments as G256
from sha2_on_cq_halo2_amd import sha256_varlen as V256
from sha2_on_cq_halo2_amd import sha512_circuit as S512
from sha2_on_cq_halo2_amd import sha512_segments as G512
from tests import sha2_model as M2
from tests import sha256_choice_model as CM
from tests import sha256_circuit_model as M256
from tests import sha256_segments_model as SM256
from tests import sha256_states_model as IM
from tests import sha256_varlen_model as VM
from tests import sha256_xor_model as XM
from tests import sha512_circuit_model as M512
from tests import sha512_segments_model as SM512
from tests.sha2_model import message, words_of

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sha2_model_pins.json")
SOURCE = "source"  # the fixture's first key: where its digests come from
V512, V384 = S512.VARIANT_512, S512.VARIANT_384


def words(count, bits, seed):
    rng = random.Random(seed)
    return [rng.getrandbits(bits) for _ in range(count)]


def size(circuit, rows, table_bits=12):
    """The smallest n = 2^k whose usable rows hold `rows`"""
    return 1 << next(k for k in range(8, 20) if rows <= circuit.usable_rows(k, table_bits))


def inputs(module, plan, bits, seed):
    """(values, shared, choice bits) of the plan's sizes, from a seeded generator"""
    low, rng = module.lower(plan), random.Random(seed)
    values = [[rng.getrandbits(bits) for _ in range(count)] for count in low.private_counts]
    var_count, bit_count = low.shared_counts
    return values, [rng.getrandbits(bits) for _ in range(var_count)], [rng.getrandbits(1) for _ in range(bit_count)]


def described(describe):
    """The description at the smallest k that holds it"""
    for k in range(8, 20):
        try:
            return describe(k)
        except ValueError:
            continue
    raise AssertionError("no k up to 19 holds the circuit")


def word_row(circuit, region):
    """The row of region `region`'s W cell in the word column"""
    return circuit.REGION_ROWS * region + next(c.row for c in circuit.layout() if c.kind == circuit.SRC["W"] and c.form == circuit.FORM_WORD)


def valid_and_flipped(find, d, cols, instance, column, row):
    """[the findings of the witness (none), the findings with one bit of one cell flipped]"""
    clean = find(d, cols, instance)
    assert clean == [] and cols[column][row] is not None
    cols[column][row] ^= 1
    found = find(d, cols, instance)
    assert found
    return [clean, [list(f) for f in found]]


def findings_256():
    d = described(lambda k: S256.describe(k, 1, 12))
    cols, digest = M256.witness(message(55), 1, 12, 1 << d.k)
    return valid_and_flipped(M256.findings, d, cols, digest, 2 * S256.PAIRS, word_row(S256, 4 + 9))


def findings_512():
    d = described(lambda k: S512.describe(k, 1, 12, variant=V384))
    cols, instance = M512.witness_one(message(111), 1, 12, 1 << d.k, V384)
    return valid_and_flipped(M512.findings, d, cols, instance, 2 * S512.PAIRS, word_row(S512, 4 + 9))


def path_case():
    leaf, siblings = hashlib.sha256(b"leaf").digest(), [hashlib.sha256(bytes([i])).digest() for i in range(2)]
    return G256.merkle_path(2), CM.path_inputs(2, [(leaf, 2, siblings)])


def findings_choice():
    plan, (values, shared, bits) = path_case()
    d = described(lambda k: G256.describe(k, plan))
    cols = CM.witness(plan, values, shared, bits, d.table_bits, 1 << d.k)
    return valid_and_flipped(CM.findings, d, cols, CM.instance_words(plan, values, shared, bits), 2 * S256.PAIRS + 1, CM.choice_cells(plan, 1, 3)[2])


def findings_varlen():
    d = described(lambda k: V256.describe(k, [2], public_length=True))
    cols, _ = VM.witness([message(56)], [2], d.table_bits, 1 << d.k)
    row = VM.word_row([2], 0, 14) + S256.VAR["ROW_M"]
    return valid_and_flipped(VM.findings, d, cols, VM.instance_words([message(56)], [2], True), 2 * S256.PAIRS + 1, row)


VARLEN = ([message(n, n) for n in (0, 3, 55, 56, 64, 119, 3)], [1, 1, 1, 2, 2, 2, 2])
VARLEN_BASES = [64, 128, 0, 192, 64, 128, 64]
HMAC_KEY, HMAC_MESSAGE = message(8, 2), message(4, 3)


def hmac_case():
    plan = G256.hmac_sha256(len(HMAC_KEY), len(HMAC_MESSAGE), commit_key=True)
    return plan, [words_of(HMAC_MESSAGE)] + [[]] * (len(plan.segments) - 1), words_of(HMAC_KEY)


def run_lowered():
    plan, values, shared = hmac_case()
    low = G256.lower(plan)
    return XM.run_lowered(low, G256.word_buffer(low, values, shared))


def entries():
    """{name: a call that gives the model's result} of everything pinned"""
    out = {}
    for blocks, length in ((1, 55), (2, 119)):
        out[f"sha256_circuit_model/region_words/blocks={blocks}"] = lambda b=blocks, l=length: M256.region_words(message(l), b)
        for tb in (S256.MIN_TABLE_BITS, 12, S256.MAX_TABLE_BITS):
            out[f"sha256_circuit_model/witness/blocks={blocks}/table_bits={tb}"] = lambda b=blocks, l=length, tb=tb: M256.witness(
                message(l), b, tb, size(S256, S256.rows_for(b), tb))
    out["sha512_circuit_model/region_words/blocks=2/sha384"] = lambda: M512.region_words(message(150, 1), 2, V384)
    out["sha512_circuit_model/witness/blocks=[1,2]/variants=[512,384]"] = lambda: M512.witness(
        [message(111), message(150, 1)], [1, 2], [V512, V384], 12, size(S512, S512.rows_for(1) + S512.rows_for(2)))
    for tb in (S512.MIN_TABLE_BITS, S512.MAX_TABLE_BITS):
        out[f"sha512_circuit_model/witness_one/sha384/table_bits={tb}"] = lambda tb=tb: M512.witness_one(
            message(3), 1, tb, size(S512, S512.rows_for(1), tb), V384)
    out["sha256_states_model/cells_of/iv"] = lambda: IM.cells_of(words(32, 32, 1), 2, 12)
    out["sha256_states_model/cells_of/state"] = lambda: IM.cells_of(words(32, 32, 1), 2, 12, words(8, 32, 2))
    out["sha256_states_model/state_after"] = lambda: [IM.state_after(message(128)), IM.state_after(message(64, 1), words(8, 32, 2))]
    out["sha512_segments_model/cells_of/iv"] = lambda: SM512.cells_of(words(16, 64, 3), 1, 12, M512.IV[V512])
    out["sha512_segments_model/cells_of/state"] = lambda: SM512.cells_of(words(32, 64, 3), 2, 11, words(8, 64, 4))
    out["sha512_segments_model/constants"] = lambda: [M512.K, M512.IV[V512], M512.IV[V384], SM512.IV512_256]
    for name, plan in (("merkle_tree(2)", G256.merkle_tree(2)), ("midstate(1)", G256.midstate(1)), ("double_sha256(1)", G256.double_sha256(1)),
                       ("merkle_path(2)", G256.merkle_path(2))):
        out[f"sha256_states_model/plan_witness/{name}"] = lambda plan=plan: IM.plan_witness(
            plan, *inputs(G256, plan, 32, 5), 12, size(S256, G256.rows_for(plan)))
    leaves = [hashlib.sha256(bytes([i])).digest() for i in range(4)]
    batch = (G256.batch([1, 2, 1]), [S256.pad(m, b) for m, b in zip((b"", message(119, 3), b"\xff" * 55), (1, 2, 1))])
    merkle = (G256.merkle_tree(2), [words_of(leaves[0] + leaves[1]), words_of(leaves[2] + leaves[3]), []])
    for name, (plan, values) in (("batch([1,2,1])", batch), ("merkle_tree(2)", merkle)):
        out[f"sha256_segments_model/witness/{name}"] = lambda plan=plan, values=values: [
            SM256.witness(plan, values, 12, size(S256, G256.rows_for(plan))), SM256.instance_words(plan, values)]
    out["sha256_choice_model/witness/merkle_path(2)"] = lambda: (lambda plan, given: [
        CM.witness(plan, *given, 12, size(S256, G256.rows_for(plan))), CM.instance_words(plan, *given)])(*path_case())
    out["sha256_xor_model/plan_witness/hmac_sha256(8,4,commit_key=True)"] = lambda: (lambda plan, values, shared: XM.plan_witness(
        plan, values, shared, 12, size(S256, G256.rows_for(plan))))(*hmac_case())
    out["sha256_xor_model/run_lowered/hmac_sha256(8,4,commit_key=True)"] = run_lowered
    rows = sum(S256.rows_for(b) for b in VARLEN[1])
    out["sha256_varlen_model/witness/lengths=0,3,55,56,64,119,3"] = lambda: [
        VM.witness(*VARLEN, 12, size(S256, rows)), VM.instance_words(*VARLEN, public_length=True)]
    out["sha256_states_model/varlen_witness/lengths=0,3,55,56,64,119,3/bases"] = lambda: IM.varlen_witness(
        *VARLEN, 12, size(S256, rows), [IM.state_after(message(base, 5)) for base in VARLEN_BASES], VARLEN_BASES)
    for name, plan in (("merkle_tree(2)", G512.merkle_tree(2)), ("midstate(1)", G512.midstate(1)), ("double_sha512(1)", G512.double_sha512(1)),
                       ("sha512_256(1)", G512.sha512_256(1)), ("mixed_plan()", SM512.mixed_plan())):
        out[f"sha512_segments_model/plan_witness/{name}"] = lambda plan=plan: SM512.plan_witness(
            plan, *inputs(G512, plan, 64, 6)[:2], 12, size(S512, G512.rows_for(plan)))
    out.update({"sha256_circuit_model/findings": findings_256, "sha512_circuit_model/findings": findings_512,
                "sha256_choice_model/findings": findings_choice, "sha256_varlen_model/findings": findings_varlen})
    return out


def digest(result) -> str:
    return hashlib.sha256(json.dumps(result, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


PINS = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}


@pytest.mark.parametrize("name", sorted(entries()))
def test_model_result_is_the_pinned_one(name):
    assert next(iter(PINS)) == SOURCE and sorted(PINS) == sorted([SOURCE] + list(entries()))
    assert digest(entries()[name]()) == PINS[name]


def test_the_constants_from_the_primes_are_the_packages():
    """FIPS 180-4, 4.2.2, 4.2.3 and 5.3.2 to 5.3.6: what the models derive against what the package tabulates."""
    assert M2.W32.K == S256.K256 and M2.W32.iv["sha256"] == S256.IV256 and M2.W32.iv["sha224"] == list(G256.IV224)
    assert M2.W64.K == S512.K512 and M2.W64.iv["sha512"] == S512.IV[V512] and M2.W64.iv["sha384"] == S512.IV[V384]
    assert M2.W64.iv["sha512/256"] == list(G512.IV512_256)
    assert (len(M2.W32.K), len(M2.W64.K)) == (64, 80) and all(len(iv) == 8 for w in (M2.W32, M2.W64) for iv in w.iv.values())
    assert (M256.K, M256.IV, M512.K, M512.IV, SM512.IV512_256) == (
        M2.W32.K, M2.W32.iv["sha256"], M2.W64.K, {V512: M2.W64.iv["sha512"], V384: M2.W64.iv["sha384"]}, M2.W64.iv["sha512/256"])


if __name__ == "__main__":
    import subprocess

    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    pins = {SOURCE: f"generated by tests/test_sha2_model_pins_cpu.py's entries() and digest() from the tree of commit {commit}, the parent of the "
                    "commit that wrote the test models once over a width record (tests/sha2_model.py)"}
    pins.update({name: digest(entry()) for name, entry in entries().items()})
    with open(FIXTURE, "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    print(f"wrote {len(pins) - 1} digests to {FIXTURE}")
