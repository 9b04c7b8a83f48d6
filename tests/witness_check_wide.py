"""Circuits for the check_witness tests at size: wide enough that the verdict bitmap spans several 256-block scan tiles,
and simple enough that the findings of a planted witness are WRITTEN DOWN from the planted positions -- the Python
model (tests/witness_check_model.py) walks expression trees per row and is not run above k = 11;
tests/test_witness_check_wide_cpu.py holds the analytic lists against it at k = 6 and 7.

`wide_circuit(k, gates)`:  fixed 0 = q (1 on the usable rows, 0 on the blinding rows), fixed 1 + j = f[j] with
f[j][row] = (7 row + j) % 13 + 1, fixed 1 + advice = kc (the same pattern as f[0]; no gate reads it).  Gate polynomial g is
q (a[g % advice] - f[g % advice]) at Rotation::cur(); the valid witness is a[j] = f[j] on the usable rows.  Permutation
columns: 0 .. advice - 1 = the advice columns, advice = the instance column, advice + 1 = kc.  `copies` copy constraints
between cells of equal value, spread over the row range: within one advice column (f[j] has period 13), between two
advice columns, from kc and from the instance column (whose cell i holds f[1][13 i + 5]) into advice columns; some of
them chain into cycles longer than two.

legacy=True adds advice columns p0 = advice, p1 = advice + 1 and two width-2 legacy lookups over 8 distinct table tuples
T[i] = (10 + i, 20 + i), repeated over all usable rows: lookup 0 reads (p0, p1) against (t0, t1)[row] = T[row % 8];
lookup 1 reads (p0 @ Rotation::next(), p1) against (t2, t3)[row] = (T[s(row + 1)][0], T[s(row)][1]), where the valid
witness is (p0, p1)[row] = T[s(row)], s(row) = (5 row + 3) % 8.  On the last usable row lookup 1 reads a blinding-row
cell: its tuple has a poisoned component, which is no table tuple -- one finding even on the valid witness.
"""
from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import plonk as PL

GATE, GATE_POISONED, LOOKUP, STATIC_LOOKUP, PERMUTATION = 1, 2, 3, 4, 5
A, F, I = PL.ADVICE, PL.FIXED, PL.INSTANCE
PERIOD = 13
# The large case of the GPU tests: 2^14 rows are 256 words = one block per check, 320 gate polynomials make 646 checks
# and blocks, three spine tiles: failed gates 0 .. 255 | failed gates 256 .. 319 and poisoned gates 0 .. 191 | the
# other poisoned gates and the permutation.  (With 256 polynomials tile 1 would hold poisoned-gate checks alone,
# which a witness cannot reach.)
LARGE_K, LARGE_GATES = 14, 320
TUPLES = [(10 + i, 20 + i) for i in range(8)]


def pattern(j, row):
    return (7 * row + j) % PERIOD + 1


def tuple_of(row):
    return (5 * row + 3) % 8


def wrong_value(col, row):
    """What `overwrite` plants: above every pattern and table value, and different for every cell."""
    return (1 << 20) + 8 * row + col


def usable(fx):
    return (1 << fx["circuit"].k) - (fx["circuit"].blinding_factors() + 1)


def wide_circuit(k, gates, advice=4, copies=None, legacy=False):
    """-> dict(circuit, fixed, advice, instances, mapping, tables) as plonk_fixtures builds them, plus `gates_of` (the
    advice columns the gates read), `copy_cells` (the (permutation column, row) cells the copy constraints name, in
    the order they were made)."""
    n = 1 << k
    q, kc = 0, 1 + advice
    num_fixed, num_advice = 2 + advice, advice
    polys = [PL.mul(PL.fix(q), PL.sub(PL.adv(g % advice), PL.fix(1 + g % advice))) for g in range(gates)]
    plookups = []
    if legacy:
        p0, p1 = advice, advice + 1
        t0 = num_fixed
        num_advice, num_fixed = advice + 2, num_fixed + 4
        plookups = [([PL.adv(p0), PL.adv(p1)], [PL.fix(t0), PL.fix(t0 + 1)]),
                    ([PL.adv(p0, 1), PL.adv(p1)], [PL.fix(t0 + 2), PL.fix(t0 + 3)])]
    perm_columns = [(A, j) for j in range(advice)] + [(I, 0), (F, kc)]
    circuit = CP.CqCircuit(k, num_advice, [], num_fixed, 1, polys, perm_columns, None, plookups)
    u = n - (circuit.blinding_factors() + 1)
    fixed = [[0] * n for _ in range(num_fixed)]
    for row in range(n):
        fixed[q][row] = 1 if row < u else 0
        for j in range(advice):
            fixed[1 + j][row] = pattern(j, row)
        fixed[kc][row] = pattern(0, row)
    adv = [[pattern(j, row) for row in range(u)] for j in range(advice)]
    instances = [[pattern(1, PERIOD * i + 5) for i in range(max(1, min(16, u // PERIOD - 1)))]]
    if legacy:
        adv += [[TUPLES[tuple_of(row)][0] for row in range(u)], [TUPLES[tuple_of(row)][1] for row in range(u)]]
        for row in range(u):
            fixed[t0][row], fixed[t0 + 1][row] = TUPLES[row % 8]
            fixed[t0 + 2][row], fixed[t0 + 3][row] = TUPLES[tuple_of(row + 1)][0], TUPLES[tuple_of(row)][1]

    asm = PL.Assembly(n, perm_columns)
    rng = B.Xoshiro256ss(0xC0B1E5 + k)
    rnd = lambda m: rng.next_u64() % m
    copy_cells = []

    def value(c, row):
        kind, idx = perm_columns[c]
        return adv[idx][row] if kind == A else (fixed[idx][row] if kind == F else instances[idx][row])

    def partner_row(j, want, near):
        """a usable row of advice column j among the 13 from `near` on (or the last 13) that holds `want`"""
        near = min(near, u - PERIOD)
        for row in range(near, near + PERIOD):
            if adv[j][row] == want:
                return row
        raise AssertionError("every value of the pattern occurs in any 13 consecutive rows")

    copies = min(384, 2 * u) if copies is None else copies
    for i in range(copies):
        j = i % advice
        row = (i * u) // copies  # spread over the whole row range; the partner is drawn
        kind = rnd(8)
        if kind == 0:  # from kc
            left = (advice + 1, rnd(u))
        elif kind == 1:  # from the instance column
            left = (advice, rnd(len(instances[0])))
        elif kind < 5:  # within the column
            left = (j, partner_row(j, adv[j][row], rnd(u)))
        else:  # from another advice column
            j2 = (j + 1 + rnd(advice - 1)) % advice
            left = (j2, partner_row(j2, adv[j][row], rnd(u)))
        right = (j, row) if kind >= 2 else (j, partner_row(j, value(*left), row))
        assert value(*left) == value(*right)
        asm.copy(perm_columns[left[0]], left[1], perm_columns[right[0]], right[1])
        copy_cells += [left, right]
    return dict(circuit=circuit, fixed=fixed, advice=adv, instances=instances, mapping=asm.mapping, tables={},
                gates_of=[g % advice for g in range(gates)], copy_cells=copy_cells)


def fresh(fx):
    """The fixture with value columns of its own (the circuit, the mapping and the cell lists are shared)."""
    return dict(fx, fixed=[list(c) for c in fx["fixed"]], advice=[list(c) for c in fx["advice"]],
                instances=[list(c) for c in fx["instances"]])


def overwrite(fx, cells):
    u = usable(fx)
    for col, row in cells:
        assert row < u and fx["advice"][col][row] != wrong_value(col, row)
        fx["advice"][col][row] = wrong_value(col, row)


def gate_findings(fx, cells):
    """Every gate polynomial that reads a planted cell's column fails on its row, and nothing else does: q = 1 there,
    a - f != 0, and the polynomials read Rotation::cur() only."""
    reading = {col: [g for g, j in enumerate(fx["gates_of"]) if j == col] for col in {c for c, _ in cells}}
    return [(GATE, g, row, 0) for col, row in cells for g in reading[col]]


def perm_findings(fx):
    """The cells of the copy constraints whose mapped partner holds another value (cells no copy names map to themselves)."""
    cols = fx["circuit"].perm_columns

    def value(c, row):
        kind, idx = cols[c]
        col = fx["advice"][idx] if kind == A else (fx["fixed"][idx] if kind == F else fx["instances"][idx])
        return col[row] if row < len(col) else 0

    out = []
    for c, row in sorted(set(fx["copy_cells"])):
        c2, r2 = fx["mapping"][c][row]
        if value(c, row) != value(int(c2), int(r2)):
            out.append((PERMUTATION, c, row, 0))
    return out


def findings(fx, cells):
    """The sorted findings of a fixture whose advice cells `cells` were overwritten."""
    return sorted(gate_findings(fx, sorted(set(cells))) + perm_findings(fx))


def plant(fx, cells):
    """Overwrites the (advice column, row) cells with `wrong_value` and returns the sorted findings that must follow."""
    overwrite(fx, sorted(set(cells)))
    return findings(fx, cells)


def break_cycles(fx, count):
    """Changes about `count` of the cells the copy constraints name, taken evenly from the list and so from every
    permutation column: an advice cell as `plant` does (its gates fail too), an instance or kc cell by adding 100 (no
    gate reads either).  Call it before the key is built: kc is part of the key.  -> the sorted findings."""
    adv = len(set(fx["gates_of"]))
    named = sorted(set(fx["copy_cells"]))
    picked = sorted({named[(i * len(named)) // count] for i in range(count)} | {c for c in named if c[0] >= adv and c[1] % 2})
    kinds = {c for c, _ in picked}
    assert kinds == set(range(adv + 2)), "cells of every permutation column"
    for c, row in picked:
        if c == adv:
            fx["instances"][0][row] += 100
        elif c == adv + 1:
            fx["fixed"][1 + adv][row] += 100
    return plant(fx, [cell for cell in picked if cell[0] < adv])


def sparse_cells(fx):
    """One cell per advice column: row 5 of column 0 (the first word of check 0), the last usable row of the last
    column (the last word of the last failed-gate check), and for the columns between them (and once more for column
    0) a cell that a copy constraint names, so that the permutation section has findings too."""
    adv = len(set(fx["gates_of"]))
    u = usable(fx)
    named = {}
    for c, row in fx["copy_cells"]:
        if c < adv and row not in (5, u - 1):
            named.setdefault(c, row)
    return [(0, 5), (adv - 1, u - 1)] + [(j, named[j]) for j in range(adv - 1)]


# ---- where a finding sits in the verdict bitmap (csrc/check.hip: checks ordered failed gates | poisoned gates | legacy |
#      static | permutation, `words` 64-row words per check, 256 words per block, 256 blocks per spine tile) ----------------
def num_checks(fx):
    c = fx["circuit"]
    return 2 * len(c.gates) + len(c.plookups) + len(c.lookups) + len(c.perm_columns)


def geometry(k, checks):
    """-> (words per check, words of the bitmap, blocks of the count / emit kernels, 256-block tiles of the spine)"""
    words = ((1 << k) + 63) // 64
    nwords = checks * words
    nblocks = (nwords + 255) // 256
    return words, nwords, nblocks, (nblocks + 255) // 256


def place(fx, finding):
    """-> (word, block, tile) of a finding's bit"""
    c = fx["circuit"]
    kind, index, row, _ = finding
    first = {GATE: 0, GATE_POISONED: len(c.gates), LOOKUP: 2 * len(c.gates), STATIC_LOOKUP: 2 * len(c.gates) + len(c.plookups),
             PERMUTATION: 2 * len(c.gates) + len(c.plookups) + len(c.lookups)}[kind]
    word = (first + index) * geometry(c.k, 1)[0] + row // 64
    return word, word // 256, word // 65536


# ---- the legacy lookups ------------------------------------------------------------------------------------------------------
def plant_half_matching_tuples(fx, count=50):
    """About `count` rows spread over the row range get an input tuple that matches the table in one component only:
    on even picks p1 becomes the second component of another tuple, on odd picks p0 the first of another.  Lookup 0
    fails on exactly those rows; lookup 1 reads (p0[row + 1], p1[row]), so it fails on the row of a changed p1, on the
    row before a changed p0, and on the last usable row (poisoned, see the module's head).  -> the sorted findings."""
    u = usable(fx)
    p0, p1 = fx["circuit"].num_advice - 2, fx["circuit"].num_advice - 1
    rows = sorted({3 + (i * (u - 8)) // count for i in range(count)})
    assert all(b - a > 1 for a, b in zip(rows, rows[1:])), "no two planted rows may share a tuple of lookup 1"
    second = {u - 1}
    for i, row in enumerate(rows):
        other = TUPLES[(tuple_of(row) + 1 + i % 7) % 8]
        if i % 2 == 0:
            fx["advice"][p1][row] = other[1]
            second.add(row)
        else:
            fx["advice"][p0][row] = other[0]
            second.add(row - 1)
    return [(LOOKUP, 0, row, 0) for row in rows] + [(LOOKUP, 1, row, 0) for row in sorted(second)]
