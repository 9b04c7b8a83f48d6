"""Mutations of an honest SHA-256 / SHA-512 / SHA-384 circuit witness and the findings each must produce, without a device.

`Sweep(SC, M, desc, cols, instance)` takes a circuit module (sha256_circuit or sha512_circuit), its model (for `spread`), a
`Description` and the model's honest witness.  It derives the region classes from the description's fixed columns and copies,
enumerates single-cell and compound mutations of the chosen regions from `layout()`, and computes the findings of a mutation
with a local evaluator: tests/witness_check_model.py's `evaluate` on the gates and lookups that read a mutated cell -- which
ones, and at which rows, comes from the queries of the constraint system's expressions -- and the copy cycles the cell is on.
`full()` runs the whole model over all rows for comparison.

A finding is (kind, index, row) with the kinds of the C ABI (gate 1, static lookup 4, permutation 5).
"""
from collections import Counter
from typing import NamedTuple

from oracle import plonk as PL
from tests import witness_check_model as WM
from tests.sha_oracle import KINDS, oracle_circuit

SELECTORS = ("q_all", "q_f3", "q_round", "q_sched", "q_chain")
WORDS = ("A", "E", "W")
CARRIES = ("CARRY_A", "CARRY_E", "CARRY_W")
# the seven even / odd decompositions: the prefix of their two source words -> the prefix of their `*_even_odd` gate
DECOMPOSITIONS = {"S0": "Sigma0", "S1": "Sigma1", "G0": "sigma0", "G1": "sigma1", "MAJ": "maj", "CHP": "chp", "CHQ": "chq"}


class Mutation(NamedTuple):
    """`writes`: ((advice column, row, value), ...).  `kind`: "cell" or "a" .. "d"; `word`: the source word's name (for a
    decomposition its prefix); `form`: "word" / "spread" (a cell of X or Y), "dense" / "spread_half" / "pair" (the halves of a
    pair cell, and both written consistently); `variant`: what was done to the value."""

    ident: str
    kind: str
    region: int
    word: str
    form: str
    variant: str
    writes: tuple
    # what a compound mutation's findings must or must not hold (see test_sha_soundness_cpu.py)
    must_find: tuple = ()
    must_not_find: tuple = ()
    gate_on: bool = True


class Sweep:
    def __init__(self, SC, M, desc, cols, instance):
        self.SC, self.M, self.desc = SC, M, desc
        self.n = 1 << desc.k
        self.advice = [list(c) for c in cols]
        self.honest = [tuple(c) for c in self.advice]
        self.instances = [list(instance)]
        self.fixed = [[int(v) for v in desc.fixed[name]] for name in desc.fixed_names]
        self.circ = oracle_circuit(desc.cs, desc.k, lambda t: t)
        self.usable = self.n - (self.circ.blinding_factors() + 1)
        self.tb = desc.table_bits
        N = 1 << self.tb
        self.tables = {"dense": list(range(N)), "spread": [M.spread(i) for i in range(N)]}
        self._index = {name: {v: i for i, v in enumerate(vals)} for name, vals in self.tables.items()}
        self.names = {v: name for name, v in SC.SRC.items()}
        word_cells = [c for c in desc.cells if c.form == SC.FORM_WORD]
        self.word_bits = word_cells[0].len
        assert all(c.len == self.word_bits for c in word_cells)
        # copy constraints as the oracle's Assembly builds its mapping
        perm = list(desc.cs.permutation_columns)
        asm = PL.Assembly(self.n, perm)
        for (lc, lr), (rc, rr) in desc.copies:
            asm.copy(lc, lr, rc, rr)
        self.mapping = asm.mapping
        self._perm_of = {col.index: i for i, col in enumerate(perm) if KINDS[col.kind] == PL.ADVICE}
        # which gates and lookup inputs read which advice column, at which rotation: from the expressions' queries
        self._gate_reads, self._lookup_reads = {}, {}
        for g, poly in enumerate(self.circ.gates):
            qs = []
            PL.expr_queries(poly, qs)
            for kind, col, rot in qs:
                if kind == PL.ADVICE:
                    self._gate_reads.setdefault(col, set()).add((g, rot))
        for l, lk in enumerate(self.circ.lookups):
            for inp, _ in lk:
                qs = []
                PL.expr_queries(inp, qs)
                for kind, col, rot in qs:
                    if kind == PL.ADVICE:
                        self._lookup_reads.setdefault(col, set()).add((l, rot))
        self._regions()

    # ---- cells -----------------------------------------------------------------------------------------------------------
    def _cell(self, kind, col, row):
        if kind == PL.ADVICE:
            return WM.POISON if row >= self.usable else self.advice[col][row] % WM.P
        if kind == PL.FIXED:
            return self.fixed[col][row] % WM.P
        return self.instances[col][row] % WM.P if row < len(self.instances[col]) else 0

    def _fixed_column(self, name):
        return self.fixed[self.desc.fixed_names.index(name)]

    # ---- regions and their classes ---------------------------------------------------------------------------------------
    def _regions(self):
        SC, R = self.SC, self.SC.REGION_ROWS
        q_all = self._fixed_column("q_all")
        count = sum(1 for v in q_all if v)
        assert [r for r, v in enumerate(q_all) if v] == [g * R for g in range(count)], "q_all marks row 0 of every region"
        self.region_count = count
        self.selectors = [tuple(int(self._fixed_column(s)[g * R]) for s in SELECTORS) for g in range(count)]
        on_copy = [set() for _ in range(count)]
        for left, right in self.desc.copies:
            for (col, row), (other, _) in ((left, right), (right, left)):
                if KINDS[col.kind] == PL.ADVICE:
                    assert col.index == 2 * SC.PAIRS and row // R < count
                    on_copy[row // R].add((row % R, KINDS[other.kind]))
        self.runs = []  # (selector, first region, last region) of every maximal run of one value
        edge = [[] for _ in range(count)]
        for s, name in enumerate(SELECTORS):
            first = 0
            for g in range(count):
                if g + 1 == count or self.selectors[g + 1][s] != self.selectors[g][s]:
                    self.runs.append((name, first, g))
                    edge[first].append((name, "first"))
                    edge[g].append((name, "last"))
                    first = g + 1
        self.class_of = [(self.selectors[g], frozenset(on_copy[g]), tuple(sorted(edge[g]))) for g in range(count)]
        representatives = {}
        for g in range(count):
            representatives.setdefault(self.class_of[g], g)
        self.classes = representatives
        self.chosen = sorted(set(representatives.values()) | {g for _, first, last in self.runs for g in (first, last)})
        assert {self.class_of[g] for g in self.chosen} == set(self.class_of), "the chosen regions cover every class"

    def label(self, region):
        """The selectors that are on in the region: the name of its class in the pinned list of free cells."""
        return "+".join(name[2:] for name, v in zip(SELECTORS, self.selectors[region]) if v)

    # ---- mutations -------------------------------------------------------------------------------------------------------
    def _field_len(self, cell):
        return self.SC._field_of(cell, self.tb)[1]

    def _pair_writes(self, cell, row, dense):
        return ((cell.column, row, dense), (cell.column + 1, row, self.M.spread(dense)))

    def single_cell(self, region):
        """Every layout cell of the region: the value XOR 1 and a value out of range, the halves of a pair separately, and
        -- what alone can show a pair cell that nothing reads -- a pair's dense half XOR 1 with its spread half following."""
        SC, base = self.SC, region * self.SC.REGION_ROWS
        out = []
        seen = Counter()
        for cell in self.desc.cells:
            word, row = self.names[cell.kind], base + cell.row
            v = self.honest[cell.column][row]
            seen[word, cell.form] += 1
            tag = f"r{region}:{word}.{seen[word, cell.form] - 1}"
            if cell.form == SC.FORM_PAIR:
                s = self.honest[cell.column + 1][row]
                assert s == self.M.spread(v)
                cases = (("dense", "xor1", ((cell.column, row, v ^ 1),)),
                         ("dense", "out_of_range", ((cell.column, row, v + (1 << self._field_len(cell))),)),
                         ("spread_half", "xor1", ((cell.column + 1, row, s ^ 1),)),
                         ("spread_half", "out_of_range", ((cell.column + 1, row, s ^ 2),)),
                         ("pair", "xor1", self._pair_writes(cell, row, v ^ 1)))
            elif cell.form == SC.FORM_SPREAD:
                cases = (("spread", "xor1", ((cell.column, row, v ^ 1),)), ("spread", "out_of_range", ((cell.column, row, v ^ 2),)))
            else:
                cases = (("word", "xor1", ((cell.column, row, v ^ 1),)),
                         ("word", "out_of_range", ((cell.column, row, v + (1 << self.word_bits)),)))
            out += [Mutation(f"{tag}:{form}:{variant}", "cell", region, word, form, variant, writes) for form, variant, writes in cases]
        return out

    def _cells_of(self, word, form=None):
        SC = self.SC
        return [c for c in self.desc.cells if c.kind == SC.SRC[word] and (form is None or c.form == form)]

    def _pieces(self, word):
        return sorted((c for c in self._cells_of(word, self.SC.FORM_PAIR) if c.len), key=lambda c: c.offset)

    def _chunks(self, word):
        return sorted((c for c in self._cells_of(word, self.SC.FORM_PAIR) if not c.len), key=lambda c: c.per_table_bits)

    def _gate(self, name):
        return self.SC.GATES.index(name)

    def _selector_of_gate(self, g, row):
        poly = self.circ.gates[g]
        assert poly[0] == "mul" and poly[1][0] == PL.FIXED, "a gate is a selector times a linear form"
        return self._cell(PL.FIXED, poly[1][1], (row + poly[1][2]) % self.n)

    def _read_by_an_active_gate(self, col, row):
        return any(self._selector_of_gate(g, (row - rot) % self.n) for g, rot in self._gate_reads.get(col, ()))

    def compound(self, region, skipped):
        """The compound mutations (a) .. (d) of the region; what could not be built is counted in `skipped`
        (Counter of (kind, reason))."""
        SC, R = self.SC, self.SC.REGION_ROWS
        base = region * R
        wb = self.word_bits
        sel = dict(zip(SELECTORS, self.selectors[region]))
        out = []
        # (a) a word replaced with its pieces and its spread form: its own recomposition holds, what consumes it fails
        for word in WORDS:
            (wc,) = self._cells_of(word, SC.FORM_WORD)
            old = self.honest[wc.column][base + wc.row]
            for flip in (0, wb - 1):
                new = old ^ (1 << flip)
                writes = []
                for c in self._cells_of(word):
                    field = (new >> c.offset) & ((1 << c.len) - 1)
                    writes += list(self._pair_writes(c, base + c.row, field)) if c.form == SC.FORM_PAIR else \
                        [(c.column, base + c.row, self.M.spread(field) if c.form == SC.FORM_SPREAD else field)]
                writes = tuple(w for w in writes if self.honest[w[0]][w[1]] != w[2])
                own = tuple((WM.GATE, self._gate(word.lower() + s), base) for s in ("_word", "_spread") if word.lower() + s in SC.GATES)
                out.append(Mutation(f"r{region}:a:{word}:bit{flip}", "a", region, word, "word_set", f"bit{flip}", writes, (), own))
        # (b) an even chunk swapped with its odd chunk
        for dec, gate in DECOMPOSITIONS.items():
            on = self._selector_of_gate(self._gate(gate + "_even_odd"), base)
            for ev, od in zip(self._chunks(dec + "_EVEN"), self._chunks(dec + "_ODD")):
                assert ev.per_table_bits == od.per_table_bits
                a, b = self.honest[ev.column][base + ev.row], self.honest[od.column][base + od.row]
                if not on:
                    skipped["b", "not applicable: the decomposition's selector is off"] += 1
                elif dec in ("G0", "G1") and not sel["q_round"]:
                    assert a == b == 0
                    skipped["b", "not applicable: W is zero outside the rounds"] += 1
                elif ev.per_table_bits * self.tb >= wb:
                    skipped["b", "not applicable: the chunk lies past the word"] += 1
                elif a == b:
                    skipped["b", "skipped: chunks equal"] += 1
                else:
                    writes = self._pair_writes(ev, base + ev.row, b) + self._pair_writes(od, base + od.row, a)
                    out.append(Mutation(f"r{region}:b:{dec}:chunk{ev.per_table_bits}", "b", region, dec, "pair", "swap", writes))
        # (c) a piece one bit too long, the next piece one less: the word recomposes, the length lookup objects
        for word in WORDS:
            pieces = self._pieces(word)
            for lo, hi in zip(pieces, pieces[1:]):
                assert lo.offset + lo.len == hi.offset
                a, b = self.honest[lo.column][base + lo.row], self.honest[hi.column][base + hi.row]
                if word == "W" and not sel["q_round"]:
                    assert b == 0
                    skipped["c", "not applicable: W is zero outside the rounds"] += 1
                elif b == 0:
                    skipped["c", "skipped: upper piece is zero"] += 1
                else:
                    writes = self._pair_writes(lo, base + lo.row, a + (1 << lo.len)) + self._pair_writes(hi, base + hi.row, b - 1)
                    out.append(Mutation(f"r{region}:c:{word}:bit{hi.offset}", "c", region, word, "pair", "long_piece", writes,
                                        ((WM.STATIC_LOOKUP, SC.PAIRS + lo.column // 2, base + lo.row),),
                                        ((WM.GATE, self._gate(word.lower() + "_word"), base),)))
        # (d) a carry one more and, where it is positive, one less
        for word in CARRIES:
            (c,) = self._pieces(word)
            v = self.honest[c.column][base + c.row]
            on = self._read_by_an_active_gate(c.column, base + c.row)
            for delta in (1, -1):
                if v + delta < 0:
                    skipped["d", "not defined: the carry is zero" + (", its gates are off" if not on else "")] += 1
                    continue
                out.append(Mutation(f"r{region}:d:{word}:{delta:+d}", "d", region, word, "pair", f"{delta:+d}",
                                    self._pair_writes(c, base + c.row, v + delta), gate_on=bool(on)))
        return out

    # ---- findings --------------------------------------------------------------------------------------------------------
    def _apply(self, writes):
        for col, row, v in writes:
            self.advice[col][row] = v

    def _restore(self, writes):
        for col, row, _ in writes:
            self.advice[col][row] = self.honest[col][row]

    def _gate_value(self, poly, row):
        """The gate polynomial on one row; a leading factor that is zero makes it zero, whatever the rest holds (the model
        treats poison times zero as zero)."""
        if poly[0] == "mul" and WM.evaluate(poly[1], row, self.n, self._cell, ()) == 0:
            return 0
        return WM.evaluate(poly, row, self.n, self._cell, ())

    def _lookup_fails(self, l, row):
        first = None
        for j, (inp, table) in enumerate(self.circ.lookups[l]):
            v = WM.evaluate(inp, row, self.n, self._cell, ())
            at = None if v is WM.POISON else self._index[table].get(v)
            if at is None or (j and at != first):
                return True
            first = at
        return False

    def _plain(self, c, row):
        kind, idx = self.circ.perm_columns[c]
        v = self._cell(kind, idx, row)
        return ("blinding", c, row) if v is WM.POISON else v

    def expected(self, m):
        """The sorted findings of the mutation: every gate on every row from which one of its queries reads a written cell,
        the static lookups that read it, and the cells of the copy cycles it is on."""
        gates, lookups, cells = set(), set(), set()
        for col, row, _ in m.writes:
            gates |= {(g, (row - rot) % self.n) for g, rot in self._gate_reads.get(col, ())}
            lookups |= {(l, (row - rot) % self.n) for l, rot in self._lookup_reads.get(col, ())}
            if col in self._perm_of:
                at = start = (self._perm_of[col], row)
                while True:
                    cells.add(at)
                    at = tuple(self.mapping[at[0]][at[1]])
                    if at == start:
                        break
        self._apply(m.writes)
        try:
            out = []
            for g, row in gates:
                v = self._gate_value(self.circ.gates[g], row)
                if v is WM.POISON:
                    out.append((WM.GATE_POISONED, g, row))
                elif v != 0:
                    out.append((WM.GATE, g, row))
            out += [(WM.STATIC_LOOKUP, l, row) for l, row in lookups if row < self.usable and self._lookup_fails(l, row)]
            out += [(WM.PERMUTATION, c, row) for c, row in cells if self._plain(c, row) != self._plain(*self.mapping[c][row])]
        finally:
            self._restore(m.writes)
        return sorted(out)

    def full(self, m=None):
        """The whole model over all rows on the mutated witness (the honest one for None)."""
        writes = m.writes if m is not None else ()
        self._apply(writes)
        try:
            total, found = WM.check_witness(self.circ, self.fixed, self.advice, self.instances, self.mapping, self.tables)
        finally:
            self._restore(writes)
        assert total == len(found)
        return sorted(f[:3] for f in found)

    def mutations(self, regions=None):
        """-> (single-cell mutations, compound mutations, Counter of (kind, reason) for what was left out)"""
        skipped = Counter()
        regions = self.chosen if regions is None else regions
        single = [m for g in regions for m in self.single_cell(g)]
        compound = [m for g in regions for m in self.compound(g, skipped)]
        return single, compound, skipped


def message(length, seed):
    """Fixed bytes among which runs of 0x00 and 0xFF are common (carries of every size, few equal chunks)."""
    import random

    rng = random.Random(seed)
    return bytes(rng.choice((0x00, 0x80, 0xFF)) if rng.random() < 0.5 else rng.randrange(256) for _ in range(length))


def check_compound(sweep, m, found):
    """What the findings of a compound mutation must hold; `found`: the sorted (kind, index, row) list."""
    found = set(found)
    if m.kind == "d" and not m.gate_on:  # a carry whose additions are all off: in range and read by nothing
        assert not found, (m.ident, sorted(found))
        return
    assert found, f"{m.ident}: no finding"
    assert set(m.must_find) <= found, (m.ident, sorted(found))
    assert not set(m.must_not_find) & found, (m.ident, sorted(found))
    if m.kind == "a":  # something outside the word's own recomposition gates
        assert found - set(m.must_not_find), m.ident
