"""CPU: the constraint systems of the SHA-2 circuits, pinned bit for bit.  Every entry of tests/golden/sha2_description_pins.json
is the SHA-256 digest of one description -- gates, queries, equality columns, lookups, fixed columns and copies -- taken at
the smallest k that holds it.  A change to a gate, a rotation, a scale or the order of anything shows up here as a changed
digest; regenerate the fixture (`python -m tests.test_sha2_description_pins_cpu`) only for a change that means to alter a
circuit.  Needs the built library's host entry points (the layout tables), no GPU."""
import contextlib
import hashlib
import json
import os

import pytest

from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd import sha256_circuit as S256
from sha2_on_cq_halo2_amd import sha256_segments as G256
from sha2_on_cq_halo2_amd import sha256_varlen as V256
from sha2_on_cq_halo2_amd import sha512_circuit as S512
from sha2_on_cq_halo2_amd import sha512_segments as G512

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sha2_description_pins.json")
SOURCE = "source"  # the fixture's first key: where its digests come from


@contextlib.contextmanager
def recorded_names():
    """While it is open, every constraint system keeps the names its gates and lookups are created under (the class
    itself drops them): `names[id(cs)]` = ([gate name per polynomial], [lookup name])."""
    names = {}
    create_gate, lookup_static = GP.ConstraintSystem.create_gate, GP.ConstraintSystem.lookup_static

    def gate(self, name, polys):
        polys = list(polys)
        names.setdefault(id(self), ([], []))[0].extend([name] * len(polys))
        return create_gate(self, name, polys)

    def lookup(self, name, table_map):
        names.setdefault(id(self), ([], []))[1].append(name)
        return lookup_static(self, name, table_map)

    GP.ConstraintSystem.create_gate, GP.ConstraintSystem.lookup_static = gate, lookup
    try:
        yield names
    finally:
        GP.ConstraintSystem.create_gate, GP.ConstraintSystem.lookup_static = create_gate, lookup_static


def smallest(describe):
    """(k, description, recorded names) at the smallest k whose rows hold the circuit (`describe(k)` raises ValueError below it)"""
    for k in range(8, 20):
        with recorded_names() as names:
            try:
                d = describe(k)
            except ValueError:
                continue
        return k, d, names[id(d.cs)]
    raise AssertionError("no k up to 19 holds the circuit")


def digest(describe) -> str:
    k, d, (gate_names, lookup_names) = smallest(describe)
    cs, h = d.cs, hashlib.sha256()

    def put(label, obj):
        h.update((label + "=" + json.dumps(obj, separators=(",", ":")) + "\n").encode())

    assert len(gate_names) == len(cs.gates) and len(lookup_names) == len(cs.static_lookups)
    constants = []
    put("k", k)
    put("gates", [[name, g.compile(constants)] for name, g in zip(gate_names, cs.gates)])
    put("advice_queries", [list(q) for q in cs.advice_queries])
    put("fixed_queries", [list(q) for q in cs.fixed_queries])
    put("instance_queries", [list(q) for q in cs.instance_queries])
    put("equality", [[c.kind, c.index] for c in cs.permutation_columns])
    put("lookups", [[name, [[col, str(table)] for col, table in row]] for name, row in zip(lookup_names, cs.static_lookups)])
    put("lookup_inputs", [e.compile(constants) for e in cs._lookup_exprs])
    put("constants", [int(c) for c in constants])
    put("fixed_names", list(d.fixed_names))
    for name in d.fixed_names:
        h.update(name.encode() + b":" + d.fixed[name].astype("<u8").tobytes())
    put("copies", [[lc.kind, lc.index, int(lr), rc.kind, rc.index, int(rr)] for (lc, lr), (rc, rr) in d.copies])
    return h.hexdigest()


def entries():
    """{name: describe(k)} of every pinned description"""
    out = {}
    for tb in (S256.MIN_TABLE_BITS, 12, S256.MAX_TABLE_BITS):
        out[f"sha256_circuit/blocks=1/table_bits={tb}"] = lambda k, tb=tb: S256.describe(k, 1, tb)
    out["sha256_segments/merkle_path(1)"] = lambda k: G256.describe(k, G256.merkle_path(1))
    out["sha256_segments/hmac_sha256(4,0)"] = lambda k: G256.describe(k, G256.hmac_sha256(4, 0))
    out["sha256_segments/midstate(1)"] = lambda k: G256.describe(k, G256.midstate(1))
    for public_length in (False, True):
        out[f"sha256_varlen/max_blocks=2/public_length={public_length}"] = lambda k, p=public_length: V256.describe(k, [2], public_length=p)
    for tb in (S512.MIN_TABLE_BITS, 12, S512.MAX_TABLE_BITS):
        out[f"sha512_circuit/blocks=[1,2]/variants=[512,384]/table_bits={tb}"] = lambda k, tb=tb: S512.describe_batch(
            k, [1, 2], [S512.VARIANT_512, S512.VARIANT_384], tb)
    for name in ("double_sha512", "midstate", "sha512_256"):
        out[f"sha512_segments/{name}(1)"] = lambda k, name=name: G512.describe(k, getattr(G512, name)(1))
    return out


PINS = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}


def test_the_fixture_pins_every_entry_and_nothing_else():
    assert next(iter(PINS)) == SOURCE and sorted(PINS) == sorted([SOURCE] + list(entries()))


@pytest.mark.parametrize("name", sorted(entries()))
def test_description_is_the_pinned_one(name):
    assert digest(entries()[name]) == PINS[name]


if __name__ == "__main__":
    import subprocess

    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    pins = {SOURCE: f"generated by tests/test_sha2_description_pins_cpu.py's digest() from the tree of commit {commit}, the parent of the "
                    "commit that moved both circuits onto sha2_family.py"}
    pins.update({name: digest(describe) for name, describe in entries().items()})
    with open(FIXTURE, "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    print(f"wrote {len(pins) - 1} digests to {FIXTURE}")
