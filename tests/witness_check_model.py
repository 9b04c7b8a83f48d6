"""What `ProvingKey.check_witness` must answer, on Python integers: `MockProver::verify` (halo2_proofs/src/dev.rs:601-958)
restated over the structures tests/plonk_fixtures.py produces (`CqCircuit`, fixed, advice, instances, mapping, tables),
extended to static lookups as `static_lookup::Argument::commit` walks them (plonk/static_lookup/prover.rs:122-160).

It shares no code with the library: expressions are walked as trees (the library runs postfix programs), membership
is a Python set, and the copy constraints come from the caller's `mapping` (the library inverts the key's sigma values).

A finding is (kind, index, row, detail); the list is sorted, which is the (kind, index, row) order of the C ABI.
"""
from oracle import bn254 as B
from oracle import plonk as PL

P = B.R_MOD
GATE, GATE_POISONED, LOOKUP, STATIC_LOOKUP, PERMUTATION = 1, 2, 3, 4, 5
NOT_IN_TABLE, DIFFERENT_ROWS, INPUT_POISONED = 0, 1, 2


class _Poison:
    """`Value::Poison` (dev.rs:109-124): equal to itself and to nothing else (`Value` derives Eq)."""

    def __repr__(self):
        return "Poison"


POISON = _Poison()


# ---- `Value` arithmetic, dev.rs:126-178 ------------------------------------------------------------------------------
def v_neg(a):
    return POISON if a is POISON else (-a) % P


def v_add(a, b):
    return POISON if (a is POISON or b is POISON) else (a + b) % P


def v_mul(a, b):
    if a is POISON and b is POISON:
        return POISON
    if a is POISON:
        return 0 if b % P == 0 else POISON  # "If poison is multiplied by zero, then we treat the poison as unconstrained"
    if b is POISON:
        return 0 if a % P == 0 else POISON
    return a * b % P


def v_scale(a, k):
    if a is POISON:
        return 0 if k % P == 0 else POISON
    return a * k % P


def evaluate(e, row, n, cell, challenges):
    """`Expression::evaluate` over `Value`s on one row (dev.rs:702-750); `cell(kind, column, row)` resolves a query."""
    t = e[0]
    if t == "const":
        return e[1] % P
    if t == "challenge":
        return challenges[e[1]] % P
    if t in (PL.ADVICE, PL.FIXED, PL.INSTANCE):
        return cell(t, e[1], (row + e[2]) % n)
    if t == "neg":
        return v_neg(evaluate(e[1], row, n, cell, challenges))
    if t == "add":
        return v_add(evaluate(e[1], row, n, cell, challenges), evaluate(e[2], row, n, cell, challenges))
    if t == "mul":
        a = evaluate(e[1], row, n, cell, challenges)
        if a is not POISON and a == 0:  # zero times anything, poison included, is zero: a gate whose selector is off costs one query
            return 0
        return v_mul(a, evaluate(e[2], row, n, cell, challenges))
    if t == "scale":
        return v_scale(evaluate(e[1], row, n, cell, challenges), e[2])
    raise ValueError(t)


def check_witness(circuit, fixed, advice, instances, mapping, tables, challenges=(), cap=None):
    """-> (total, findings[:cap]).  `advice`: one list per column; rows >= usable rows, if present, are ignored."""
    n = 1 << circuit.k
    u = n - (circuit.blinding_factors() + 1)

    def cell(kind, col, row):
        if kind == PL.ADVICE:  # blinding rows are poisoned (dev.rs:546-548)
            return POISON if row >= u else (advice[col][row] % P if row < len(advice[col]) else 0)
        if kind == PL.FIXED:
            return fixed[col][row] % P
        return instances[col][row] % P if row < len(instances[col]) else 0

    out = []
    # gates (dev.rs:694-766): every polynomial on every row, blinding rows included
    for g, poly in enumerate(circuit.gates):
        for row in range(n):
            v = evaluate(poly, row, n, cell, challenges)
            if v is POISON:
                out.append((GATE_POISONED, g, row, 0))
            elif v != 0:
                out.append((GATE, g, row, 0))
    # legacy lookups (dev.rs:768-906): the input tuple of a usable row must be the table tuple of some usable row
    for l, (ins, tabs) in enumerate(circuit.plookups):
        tup = lambda exprs, row: tuple(evaluate(e, row, n, cell, challenges) for e in exprs)
        rows_of_table = {tup(tabs, row) for row in range(u)}
        for row in range(u):
            if tup(ins, row) not in rows_of_table:
                out.append((LOOKUP, l, row, 0))
    # static lookups (static_lookup/prover.rs:132-161): every input in its table column, all on one table index
    for l, lk in enumerate(circuit.lookups):
        index_of = [{v % P: i for i, v in enumerate(tables[name])} for _, name in lk]
        for row in range(u):
            first = None
            for j, (inp, _) in enumerate(lk):
                v = cell(PL.ADVICE, inp, row) if isinstance(inp, int) else evaluate(inp, row, n, cell, challenges)
                if v is POISON:
                    out.append((STATIC_LOOKUP, l, row, INPUT_POISONED))
                    break
                if v not in index_of[j]:
                    out.append((STATIC_LOOKUP, l, row, NOT_IN_TABLE))
                    break
                if j and index_of[j][v] != first:
                    out.append((STATIC_LOOKUP, l, row, DIFFERENT_ROWS))
                    break
                first = index_of[j][v]
    # permutation (dev.rs:908-951): every cell equals the cell the mapping sends it to.  Copy constraints name usable rows
    # only (dev.rs:457), so a blinding-row cell maps to itself, whatever it holds.
    def plain(c, row):
        kind, idx = circuit.perm_columns[c]
        v = cell(kind, idx, row)
        return ("blinding", c, row) if v is POISON else v

    for c in range(len(circuit.perm_columns)):
        for row in range(n):
            c2, r2 = mapping[c][row]
            if plain(c, row) != plain(int(c2), int(r2)):
                out.append((PERMUTATION, c, row, 0))
    out.sort()
    return len(out), (out if cap is None else out[:cap])
