"""GPU: the device witness checker against the mutations of tests/sha_mutations.py, through the real keys.

One `Sha512BatchCircuit` at k = 13 holds a SHA-512 and a SHA-384 message of two blocks each (one key for both variants, a
segment boundary between them), one `Sha256Circuit` a two-block message.  Every single-cell and compound mutation of every
chosen region is uploaded, checked by `ProvingKey.check_witness` and taken back; the findings must be the set the CPU
evaluator expects (tests/test_sha_soundness_cpu.py checks that evaluator against the whole model)."""
import time

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import CqError
from sha2_on_cq_halo2_amd import sha256_circuit as S256
from sha2_on_cq_halo2_amd import sha512_circuit as S512
from sha2_on_cq_halo2_amd.api import Sha256Circuit, Sha512BatchCircuit
from tests import sha256_circuit_model as M256
from tests import sha512_circuit_model as M512
from tests.sha512_direct import mont_column
from tests.sha_mutations import Sweep, check_compound, message
from tests.sha_oracle import verifier, write_cell

pytestmark = pytest.mark.gpu
SEED = 0x5348413243515F
VARIANTS = [S512.VARIANT_512, S512.VARIANT_384]
MESSAGES_512 = [message(239, 1), message(200, 2)]
MESSAGE_256 = message(119, 3)
K_512 = 13
K_256 = next(k for k in range(8, 20) if S256.max_blocks(k) >= 2)
CQ_ERR_LOOKUP = -4


def _sweep_512():
    desc = S512.describe_batch(K_512, [2, 2], VARIANTS)
    cols, inst, _ = M512.witness(MESSAGES_512, [2, 2], VARIANTS, desc.table_bits, 1 << K_512)
    return Sweep(S512, M512, desc, cols, inst)


def _sweep_256():
    desc = S256.describe(K_256, 2)
    cols, inst = M256.witness(MESSAGE_256, 2, desc.table_bits, 1 << K_256)
    return Sweep(S256, M256, desc, cols, inst)


# the descriptions need no device: the chosen regions are known when the tests are collected
SWEEPS = {"sha512_384": _sweep_512(), "sha256": _sweep_256()}
GROUPS = [(name, g) for name, sw in SWEEPS.items() for g in sw.chosen]


class Rig:
    """A circuit with its honest witness on the device, and the same witness as Montgomery limbs on the host."""

    def __init__(self, circuit, sweep, synthesize):
        self.c, self.sw = circuit, sweep
        synthesize()
        self.ptrs = [x.ptr for x in circuit.cols]
        self.instances = circuit.instances
        self.honest = [mont_column(list(col)) for col in sweep.honest]
        self.assert_intact()

    def check(self):
        total, fails = self.c.pk.check_witness(self.ptrs, instances=self.instances, max_failures=256)
        assert total == len(fails)
        return sorted((f.kind, f.index, f.row) for f in fails)

    def write(self, writes):
        for col, row, value in writes:
            write_cell(self.c, col, row, value)

    def restore(self, writes):
        self.write([(col, row, self.sw.honest[col][row]) for col, row, _ in writes])

    def assert_intact(self):
        for i, (dev, want) in enumerate(zip(self.c.cols, self.honest)):
            assert np.array_equal(dev.download((self.c.n, 4)), want), f"advice column {i} is not the honest witness"
        assert self.c.pk.check_witness(self.ptrs, instances=self.instances, max_failures=256) == (0, [])


@pytest.fixture(scope="module")
def rigs(ctx):
    made = {}

    def get(name):
        if name not in made:
            if name == "sha256":
                c = Sha256Circuit(ctx, K_256, 2, seed=SEED)
                made[name] = Rig(c, SWEEPS[name], lambda: c.synthesize(MESSAGE_256))
            else:
                c = Sha512BatchCircuit(ctx, K_512, [2, 2], VARIANTS, seed=SEED)
                made[name] = Rig(c, SWEEPS[name], lambda: c.synthesize(MESSAGES_512))
        return made[name]

    yield get
    for rig in made.values():
        rig.c.close()


def test_the_batch_has_both_variants_and_a_segment_boundary():
    sw = SWEEPS["sha512_384"]
    per_segment = 2 * S512.BLOCK_REGIONS + S512.TAIL_REGIONS
    assert sw.region_count == 2 * per_segment
    # the last tail region of the SHA-512 segment and the first region of the SHA-384 segment are both swept
    assert {per_segment - 1, per_segment} <= set(sw.chosen)
    public = [len([1 for (_, kind) in sw.class_of[g][1] if kind == "instance"]) for g in range(sw.region_count)]
    assert sum(public[:per_segment]) == 8 and sum(public[per_segment:]) == 6


@pytest.mark.parametrize("name,region", GROUPS, ids=[f"{name}-r{g}" for name, g in GROUPS])
def test_the_checker_finds_what_the_model_finds(rigs, name, region):
    """Every mutation of one region: the checker's (kind, index, row) set is the evaluator's, and the witness is intact
    afterwards."""
    rig = rigs(name)
    sw = rig.sw
    single, compound, _ = sw.mutations([region])
    start = time.perf_counter()
    for m in single + compound:
        want = sw.expected(m)
        rig.write(m.writes)
        try:
            got = rig.check()
        finally:
            rig.restore(m.writes)
        assert got == want, m.ident
        if m.kind != "cell":
            check_compound(sw, m, got)
    spent = time.perf_counter() - start
    print(f"{name} region {region} ({sw.label(region)}): {len(single) + len(compound)} checks in {spent:.2f} s")
    rig.assert_intact()


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_the_checker_verdict_is_the_proof_systems(rigs, name):
    """One representative mutation per way the proof system can object, in the first scheduled round of the last block.  A
    piece one bit too long (kind c) fails only lookups and gates the checker names -- and the prover, as the reference's,
    refuses a witness whose lookup input is not in its table: no proof exists to verify.  A carry one too large (kind d)
    passes every lookup, so the prover does prove it: the oracle's verifier rejects that proof and accepts the honest one."""
    rig = rigs(name)
    sw, c = rig.sw, rig.c
    region = sw.region_count - sw.SC.TAIL_REGIONS - sw.SC.BLOCK_REGIONS + 20
    assert sw.label(region) == "all+f3+round+sched"
    compound = sw.mutations([region])[1]
    long_piece = next(m for m in compound if m.kind == "c" and m.word == "E")
    carry = next(m for m in compound if m.kind == "d" and m.word == "CARRY_E" and m.variant == "+1")
    verify = verifier(c, SEED)
    words = list(sw.instances[0])

    def prove():
        return c.pk.create_proof_dev(rig.ptrs, seed=5, instances=rig.instances)

    rig.write(long_piece.writes)
    try:
        assert set(long_piece.must_find) <= set(rig.check())
        with pytest.raises(CqError) as e:
            prove()
        assert e.value.code == CQ_ERR_LOOKUP
    finally:
        rig.restore(long_piece.writes)
    rig.write(carry.writes)
    try:
        found = rig.check()
        assert found == sw.expected(carry) and {f[0] for f in found} == {1}  # gates only: every lookup holds
        bad = prove()
    finally:
        rig.restore(carry.writes)
    assert len(bad) == c.pk.proof_size and not verify(bad, words)
    rig.assert_intact()
    assert verify(prove(), words)
