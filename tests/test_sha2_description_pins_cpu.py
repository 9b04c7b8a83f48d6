"""CPU: the constraint systems of the SHA-2 circuits, pinned bit for bit.  Every entry of tests/golden/sha2_description_pins.json
is the SHA-256 digest of one description -- gates, queries, equality columns, lookups, fixed columns and copies -- taken at
the smallest k that holds it -- or, under `<module>/lower/<plan>`, of one plan's lowering: the arrays the synthesis entry
points take.  A change to a gate, a rotation, a scale or the order of anything shows up here as a changed digest; regenerate the fixture (`python -m tests.test_sha2_description_pins_cpu`) only for a change that means to alter a
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
from tests import sha512_segments_model as M512

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


def hand_plan(a, b, c):
    """Three 32-bit segments that reach every branch of the copy order; a, b, c are Xor or Choice words.  Var 0 stands
    first as a message word, then as an operand and as an initial word; Var 1 as an operand only; Var 2 first as an initial
    word, then as an operand.  `a` is read twice.  The last segment's `init` mixes Const, Private, Var and DigestWord, and
    its initial words are public."""
    P, V, D, K = G256.PRIVATE, G256.Var, G256.DigestWord, G256.Const
    init = (K(7), P, V(0), D(1, 3), V(2), K(5), P, D(0, 5))
    segs = (G256.Segment(1, (V(0), K(5)) + (P,) * 14), G256.Segment(1, (P, a, b, a) + (P,) * 11 + (D(0, 2),)),
            G256.Segment(1, (c, V(0)) + (P,) * 14, init))
    return G256.Plan(segs, (2, 0), (2,))


def plans():
    """{name: (module, plan)} of every pinned plan"""
    V, D = G256.Var, G256.DigestWord
    out = {
        "merkle_path(1)": G256.merkle_path(1), "hmac_sha256(4,0)": G256.hmac_sha256(4, 0), "midstate(1)": G256.midstate(1),
        "batch([1,2])": G256.batch([1, 2]), "double_sha256(1)": G256.double_sha256(1), "merkle_tree(2)": G256.merkle_tree(2),
        "sha224(1)": G256.sha224(1), "merkle_path(2,paths=2,leaf_blocks=1,public_leaf=True)": G256.merkle_path(2, paths=2, leaf_blocks=1, public_leaf=True),
        "hmac_sha256(8,4,commit_key=True)": G256.hmac_sha256(8, 4, commit_key=True),
        "hand_plan(xor)": hand_plan(G256.Xor(V(0), G256.Const(0x36363636)), G256.Xor(D(0, 1), V(1)), G256.Xor(V(2), V(1))),
        "hand_plan(choice)": hand_plan(G256.Choice(0, V(0), D(0, 1)), G256.Choice(1, D(0, 1), V(1)), G256.Choice(0, V(2), D(1, 0))),
    }
    out = {"sha256_segments/" + name: (G256, plan) for name, plan in out.items()}
    for name in ("double_sha512", "midstate", "sha512_256"):
        out[f"sha512_segments/{name}(1)"] = (G512, getattr(G512, name)(1))
    out["sha512_segments/batch([1,2],[512,384])"] = (G512, G512.batch([1, 2], [S512.VARIANT_512, S512.VARIANT_384]))
    out["sha512_segments/merkle_tree(2)"] = (G512, G512.merkle_tree(2))
    out["sha512_segments/mixed_plan()"] = (G512, M512.mixed_plan())
    return out


def lower_digest(module, plan) -> str:
    """The digest of `module.lower(plan)`: every array's dtype and bytes (an array the width does not have counts as an
    empty one), the word buffer's length, the Private words per segment and the (var, bit) counts."""
    low, h = module.lower(plan), hashlib.sha256()

    def put(label, obj):
        h.update((label + "=" + json.dumps(obj, separators=(",", ":")) + "\n").encode())

    for name in ("seg_blocks", "seg_variant", "sources", "choices", "init_sources", "xors", "consts"):
        a = getattr(low, name, None)
        put(name, ["absent"] if a is None or not a.size else [a.dtype.str, a.tobytes().hex()])
    put("words_len", int(low.words_len))
    put("private_counts", [int(c) for c in low.private_counts])
    put("shared_counts", list(low.shared_counts) if hasattr(low, "shared_counts") else [low.var_count, 0])
    return h.hexdigest()


def entries():
    """{name: a call that gives the digest} of everything pinned: descriptions, then lowerings"""
    describes = {}
    for tb in (S256.MIN_TABLE_BITS, 12, S256.MAX_TABLE_BITS):
        describes[f"sha256_circuit/blocks=1/table_bits={tb}"] = lambda k, tb=tb: S256.describe(k, 1, tb)
    for public_length in (False, True):
        describes[f"sha256_varlen/max_blocks=2/public_length={public_length}"] = lambda k, p=public_length: V256.describe(k, [2], public_length=p)
    for tb in (S512.MIN_TABLE_BITS, 12, S512.MAX_TABLE_BITS):
        describes[f"sha512_circuit/blocks=[1,2]/variants=[512,384]/table_bits={tb}"] = lambda k, tb=tb: S512.describe_batch(
            k, [1, 2], [S512.VARIANT_512, S512.VARIANT_384], tb)
    for name, (module, plan) in plans().items():
        describes[name] = lambda k, module=module, plan=plan: module.describe(k, plan)
    out = {name: (lambda describe=describe: digest(describe)) for name, describe in describes.items()}
    for name, (module, plan) in plans().items():
        out[name.replace("/", "/lower/", 1)] = lambda module=module, plan=plan: lower_digest(module, plan)
    return out


PINS = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}


def test_the_fixture_pins_every_entry_and_nothing_else():
    assert next(iter(PINS)) == SOURCE and sorted(PINS) == sorted([SOURCE] + list(entries()))


@pytest.mark.parametrize("name", sorted(entries()))
def test_description_is_the_pinned_one(name):
    assert entries()[name]() == PINS[name]


if __name__ == "__main__":
    import subprocess

    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    pins = {SOURCE: f"generated by tests/test_sha2_description_pins_cpu.py's digest() and lower_digest() from the tree of commit {commit}, the "
                    "parent of the commit that moved the wired segments onto sha2_segments.py; the 14 descriptions pinned before it came out as they "
                    "did from the parent of the commit that moved both circuits onto sha2_family.py"}
    pins.update({name: entry() for name, entry in entries().items()})
    with open(FIXTURE, "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    print(f"wrote {len(pins) - 1} digests to {FIXTURE}")
