"""CPU: every cell of the SHA-256 and SHA-512 / SHA-384 circuits is constrained, or is on a pinned list with its reason.

tests/sha_mutations.py enumerates the layout: every cell of one region per region class (and of the first and last region of
every selector run), mutated in and out of range, and the compound mutations that keep part of the circuit consistent.  The
findings come from a local evaluator that is itself checked against the whole of tests/witness_check_model.py."""
import random
from collections import Counter

import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as S256
from sha2_on_cq_halo2_amd import sha512_circuit as S512
from tests import sha256_circuit_model as M256
from tests import sha512_circuit_model as M512
from tests.sha_mutations import Sweep, check_compound, message

CIRCUITS = ("sha512", "sha384", "sha256")

# (word, form, the selectors that are on in the region): the cells a single-cell mutation of which has NO finding.  Form
# "word" is a cell of X; "pair" is a pair cell whose dense half is changed and whose spread half follows (a change of one
# half alone always fails the `pair` lookup).  Every entry is read off the gates of `_constraint_system` and DESIGN.md 9c /
# 9j ("Not constrained, and not read by anything: W, K and the carries of regions whose selectors are off").  The
# evaluator evaluates EVERY gate that queries the cell, at every row it is queried from, and every copy cycle it is on: a
# cell listed here enters no active equation, in its own region or a later one, so no value in it can reach a public word.
_NOT_ROUND = ("all", "all+f3", "all+chain", "all+f3+chain")
_F3_OFF = ("all", "all+chain")  # regions 0 and 1 of a block and of the tail
FREE = {}
FREE.update({("K", "word", c): "no round: only e_add / a_add read the K cell, at their own region, under q_round; the copy to `const` exists "
             "in rounds only" for c in _NOT_ROUND})
FREE.update({(w, "word", c): "q_f3 is off: ch_word / maj_word are off, and the other readers, e_add / a_add of the NEXT region, are off "
             "too, since region 1 or 2 of a block or of the tail is no round" for w in ("CH", "MAJ_ODD") for c in _F3_OFF})
FREE.update({(w + h, "pair", c): "q_f3 is off: only the region's own maj / chp / chq gates read the chunk; `pair` and `length` still "
             "bound it" for w in ("MAJ", "CHP", "CHQ") for h in ("_EVEN", "_ODD") for c in _F3_OFF})
FREE.update({(w, "pair", c): "state regions of a segment's first block: only the region's own e_add / a_add (q_round) and chain_a / "
             "chain_e (q_chain) read the carry, all off; in [0, 8) by `length`" for w in ("CARRY_A", "CARRY_E") for c in ("all", "all+f3")})
FREE.update({("CARRY_W", "pair", c): "no round from 16 on: only the region's own w_add reads the carry, under q_sched; in [0, 8) by "
             "`length`" for c in _NOT_ROUND + ("all+f3+round",)})
SKIP_CAP = 0.10


def _sweep(name, table_bits=12):
    if name == "sha256":
        k = next(k for k in range(8, 20) if S256.max_blocks(k) >= 2)
        desc = S256.describe(k, 2, table_bits)
        cols, inst = M256.witness(message(119, 3), 2, table_bits, 1 << k)
        return Sweep(S256, M256, desc, cols, inst)
    variant = S512.VARIANT_512 if name == "sha512" else S512.VARIANT_384
    desc = S512.describe(12, 2, table_bits, variant=variant)
    cols, inst = M512.witness_one(message(239, 1 if name == "sha512" else 2), 2, table_bits, 1 << 12, variant)
    return Sweep(S512, M512, desc, cols, inst)


_MADE = {}


def swept(name):
    """(sweep, single-cell mutations, compound mutations, what was left out, {ident: findings}) at the default width"""
    if name not in _MADE:
        sw = _sweep(name)
        single, compound, skipped = sw.mutations()
        _MADE[name] = sw, single, compound, skipped, {m.ident: sw.expected(m) for m in single + compound}
    return _MADE[name]


@pytest.mark.parametrize("name", CIRCUITS)
def test_chosen_regions_cover_every_class(name):
    sw = swept(name)[0]
    SC = sw.SC
    B, T = SC.BLOCK_REGIONS, SC.TAIL_REGIONS
    assert sw.region_count == 2 * B + T
    assert {sw.class_of[g] for g in sw.chosen} == set(sw.class_of)
    # what the layout says must be there: the state regions, the first rounds with and without the schedule gate and the last
    # round of block 0; the chained state, the first round and the first scheduled round of block 1; every tail region
    want = {0, 1, 2, 3, 4, 19, 20, B - 1} | {B + 0, B + 2, B + 4, B + 20} | {2 * B + i for i in range(T)}
    assert want <= set(sw.chosen), sorted(want - set(sw.chosen))
    # and the selectors each of them must have on: the names the pinned list of free cells goes by.  A selector that starts a
    # region late or ends one early changes a name here
    state = ("all", "all", "all+f3", "all+f3")
    names = {i: state[i] for i in range(4)}
    names.update({B + i: state[i] + "+chain" for i in range(4)})
    names.update({2 * B + i: state[i] + "+chain" for i in range(T)})
    names.update({4: "all+f3+round", 19: "all+f3+round", B + 4: "all+f3+round"})
    names.update({20: "all+f3+round+sched", B - 1: "all+f3+round+sched", B + 20: "all+f3+round+sched"})
    assert want <= set(names) <= set(sw.chosen) and {g: sw.label(g) for g in names} == names
    for selector, first, last in sw.runs:
        assert first in sw.chosen and last in sw.chosen, (selector, first, last)


@pytest.mark.parametrize("name", CIRCUITS)
def test_the_local_evaluator_is_the_full_model(name):
    """The honest witness has no finding; for a fixed sample -- one mutation per cell form, per region class and per compound
    kind -- the whole model over all rows gives exactly the local set."""
    sw, single, compound, _, expected = swept(name)
    assert sw.full() == []
    rng = random.Random(0x5EED)
    sample = {}
    for form in sorted({m.form for m in single}):
        m = rng.choice([m for m in single if m.form == form])
        sample[m.ident] = m
    for g in sorted(sw.classes.values()):
        m = rng.choice([m for m in single + compound if m.region == g])
        sample[m.ident] = m
    for kind in "abcd":
        m = rng.choice([m for m in compound if m.kind == kind])
        sample[m.ident] = m
    assert len(sample) >= 25
    for ident, m in sample.items():
        assert sw.full(m) == expected[ident], ident
    assert sw.full() == []


@pytest.mark.parametrize("name", CIRCUITS)
def test_no_cell_is_free_unless_pinned(name):
    sw, single, _, _, expected = swept(name)
    free = Counter((m.word, m.form, sw.label(m.region)) for m in single if not expected[m.ident])
    unexplained = sorted(set(free) - set(FREE))
    print(f"{name}: {sum(free.values())} single-cell mutations without a finding in {len(free)} (word, form, class) entries, "
          f"{len(unexplained)} unexplained")
    assert not unexplained, [m.ident for m in single if not expected[m.ident] and (m.word, m.form, sw.label(m.region)) in unexplained]
    assert set(free) == set(FREE), sorted(set(FREE) - set(free))
    # a change of one half of a pair, or a value out of range, is always found
    assert all(expected[m.ident] for m in single if m.form in ("dense", "spread_half", "spread"))
    assert all(expected[m.ident] for m in single if m.variant == "out_of_range" and (m.word, m.form, sw.label(m.region)) not in FREE)


@pytest.mark.parametrize("name", CIRCUITS)
def test_compound_mutations_are_found(name):
    sw, _, compound, _, expected = swept(name)
    assert {m.kind for m in compound} == set("abcd")
    for m in compound:
        check_compound(sw, m, expected[m.ident])
    # (d) ran where the carry's addition is on and where it is off, for every carry
    assert {(m.word, m.gate_on) for m in compound if m.kind == "d"} == {(w, on) for w in ("CARRY_A", "CARRY_E", "CARRY_W") for on in (True, False)}
    for m in compound:
        if m.kind == "d" and not m.gate_on:
            assert (m.word, "pair", sw.label(m.region)) in FREE


@pytest.mark.parametrize("name", CIRCUITS)
def test_no_exclusion_is_silent(name):
    """The counts of the sweep, and the share of compound cases the message's bytes did not allow."""
    sw, single, compound, skipped, _ = swept(name)
    cells = len(sw.desc.cells)
    per_region = Counter(m.region for m in single)
    assert set(per_region) == set(sw.chosen) and len(set(per_region.values())) == 1
    pairs = sum(c.form == sw.SC.FORM_PAIR for c in sw.desc.cells)
    assert per_region[sw.chosen[0]] == 5 * pairs + 2 * (cells - pairs)
    print(f"{name}: {cells} cells ({pairs} pairs x 5 variants, {cells - pairs} words x 2) x {len(sw.chosen)} regions of "
          f"{sw.region_count} = {len(single)} single-cell mutations; compound: {dict(Counter(m.kind for m in compound))}")
    for (kind, reason), count in sorted(skipped.items()):
        print(f"  ({kind}) {reason}: {count}")
    assert all(reason.startswith(("skipped: ", "not applicable: ", "not defined: ")) for _, reason in skipped)
    for kind in "abcd":
        built = sum(m.kind == kind for m in compound)
        left = sum(v for (k, reason), v in skipped.items() if k == kind and reason.startswith("skipped: "))
        print(f"  ({kind}) skip share {left} / {built + left} = {left / (built + left):.3f}")
        assert left <= SKIP_CAP * (built + left), (kind, left, built)


WIDTHS = [("sha512", S512.MAX_TABLE_BITS), ("sha384", S512.MAX_TABLE_BITS), ("sha256", S256.MAX_TABLE_BITS), ("sha256", S256.MIN_TABLE_BITS)]


@pytest.mark.parametrize("name,table_bits", WIDTHS)
def test_a_round_region_at_the_table_width_limits(name, table_bits):
    """The first scheduled round of block 1 at the widest table (chunks past the word exist: the gates leave them out and
    the length lookup pins them to zero) and, for SHA-256, at the narrowest."""
    sw = _sweep(name, table_bits)
    region = sw.SC.BLOCK_REGIONS + 20
    assert sw.label(region) == "all+f3+round+sched"
    single, compound, skipped = sw.mutations([region])
    if table_bits == sw.SC.MAX_TABLE_BITS:
        past = [c for c in sw.desc.cells if c.form == sw.SC.FORM_PAIR and not c.len and c.per_table_bits * table_bits >= sw.word_bits]
        assert past, "no chunk starts at or above the word width"
        assert all(sw.honest[c.column][region * sw.SC.REGION_ROWS + c.row] == 0 for c in past)
    expected = {m.ident: sw.expected(m) for m in single + compound}
    free = {(m.word, m.form, sw.label(m.region)) for m in single if not expected[m.ident]}
    assert free == {key for key in FREE if key[2] == "all+f3+round+sched"} == set()
    for m in compound:
        check_compound(sw, m, expected[m.ident])
    assert sw.full() == []
    rng = random.Random(table_bits)
    for m in rng.sample(single, 3) + rng.sample(compound, 2):
        assert sw.full(m) == expected[m.ident], m.ident
    print(f"{name} at {table_bits} bits: {len(single)} single-cell and {len(compound)} compound mutations, left out {dict(skipped)}")
