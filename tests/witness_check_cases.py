"""The witness mutations of the check_witness tests, one per kind of finding, over `chain_circuit`
(tests/plonk_fixtures.py), with the findings each must produce at k = 5 WRITTEN OUT from the circuit's definition:
n = 32, 5 blinding factors, usable rows 0 .. 25, chain rows 0 .. 23 (even rows add, odd rows multiply).

Gate polynomials: 0 q_add (a + b - c), 1 q_mul (a b - c), 2 q_next (a@next - c), 3 q_prev (a - c@prev),
4 q_fix (3 a - kc - 5).  Permutation columns: 0 a, 1 b, 2 c, 3 instance, 4 the fixed column kc.
"""
from oracle import bn254 as B
from oracle import plonk as PL
from tests.plonk_fixtures import chain_circuit

P = B.R_MOD
GATE, GATE_POISONED, LOOKUP, STATIC_LOOKUP, PERMUTATION = 1, 2, 3, 4, 5


def _fx(k, **kw):
    fx = chain_circuit(k, **kw)
    fx["advice"] = [list(c) if not callable(c) else c for c in fx["advice"]]
    fx["fixed"] = [list(c) for c in fx["fixed"]]
    fx["instances"] = [list(c) for c in fx["instances"]]
    return fx


def usable(fx):
    return (1 << fx["circuit"].k) - (fx["circuit"].blinding_factors() + 1)


def wrong_c(k):
    """c of the add row 10 is off by one: the add gate and q_next fail there, q_prev on the next row; c is copied nowhere."""
    fx = _fx(k)
    fx["advice"][2][10] = (fx["advice"][2][10] + 1) % P
    return fx, [(GATE, 0, 10, 0), (GATE, 2, 10, 0), (GATE, 3, 11, 0)]


def wrong_instance(k):
    """Public input 1 is copied from c on the last chain row: both cells of that 2-cycle fail, no gate reads the instance."""
    fx = _fx(k)
    fx["instances"][0][1] = (fx["instances"][0][1] + 1) % P
    last = usable(fx) - 3
    return fx, [(PERMUTATION, 2, last, 0), (PERMUTATION, 3, 1, 0)]


def wrong_fixed_copy(k):
    """kc[1] is the constant b[0] is copied from (q_fix is off on row 1, so no gate reads it): the 2-cycle fails."""
    fx = _fx(k)
    kc = 5
    fx["fixed"][kc][1] = (fx["fixed"][kc][1] + 1) % P
    return fx, [(PERMUTATION, 1, 0, 0), (PERMUTATION, 4, 1, 0)]


def static_outside_table(k):
    fx = _fx(k, with_lookup=True)
    fx["advice"][3][7] = 5  # TABLE holds 0, 1 and the even numbers 6 .. 32
    return fx, [(STATIC_LOOKUP, 0, 7, 0)]


def legacy_not_a_row(k):
    """p = 4 on the selected row 0 looks up (4, 9): no table row."""
    fx = _fx(k, plookup=True)
    fx["advice"][3][0] = 4
    return fx, [(LOOKUP, 0, 0, 0)]


def legacy_table_pair(k):
    """The table row of p = 3 becomes (3, 2 * 3 + 2): every selected row whose p is 3 looks up (3, 7) in vain.  p =
    vals[(5 r + 2) % 7] = 3 on rows r = 1 (mod 7); rows r = 3 (mod 4) are not selected.  Written out for k = 5."""
    fx = _fx(k, plookup=True)
    t1 = fx["circuit"].num_fixed - 1
    assert fx["fixed"][t1][1] == 7
    fx["fixed"][t1][1] = 8
    return fx, [(LOOKUP, 0, 1, 0), (LOOKUP, 0, 8, 0), (LOOKUP, 0, 22, 0)]


def poisoned_gates(k):
    """q_add set on the blinding row u + 1: a + b - c is poisoned there.  And a sixth gate without a selector, a - a:
    real zero on the usable rows, poisoned on every blinding row (-P = P, P + P = P)."""
    fx = _fx(k)
    u = usable(fx)
    fx["fixed"][0][u + 1] = 1
    fx["circuit"].gates.append(PL.sub(PL.adv(0), PL.adv(0)))
    n = 1 << k
    return fx, [(GATE_POISONED, 0, u + 1, 0)] + [(GATE_POISONED, 5, r, 0) for r in range(u, n)]


def blinding_row_garbage(k):
    """The caller leaves non-zero values in blinding rows of a, b and c: ignored, as the prover ignores them."""
    fx = _fx(k)
    n, u = 1 << k, usable(fx)
    for col in range(3):
        fx["advice"][col] = fx["advice"][col] + [0] * (n - u)
        fx["advice"][col][u + 2] = 7 + col
        fx["advice"][col][n - 1] = 11
    return fx, []


def two_at_once(k):
    fx, e1 = wrong_c(k)
    fx["instances"][0][1] = (fx["instances"][0][1] + 1) % P
    return fx, e1 + [(PERMUTATION, 2, usable(fx) - 3, 0), (PERMUTATION, 3, 1, 0)]


MUTATIONS = {f.__name__: f for f in (wrong_c, wrong_instance, wrong_fixed_copy, static_outside_table, legacy_not_a_row,
                                    legacy_table_pair, poisoned_gates, blinding_row_garbage, two_at_once)}
# whose expected lists hold for every k (the others name rows of the k = 5 layout)
ANY_K = ("wrong_c", "wrong_instance", "wrong_fixed_copy", "static_outside_table", "legacy_not_a_row", "poisoned_gates",
         "blinding_row_garbage", "two_at_once")


def phase_challenges():
    return [0x1234567, 0x89ABCDEF01]


def resolve_phases(fx, challenges):
    """Synthesises the later-phase columns of `chain_circuit(phases=True)` with the given challenges."""
    fx["advice"] = [c(challenges) if callable(c) else c for c in fx["advice"]]
    return fx


def wrong_challenges(k):
    """The witness was synthesised with (c0, c1), the checker is told (c0 + 1, c1 + 1): gate 5 (ph1 - c0 a) and gate 6
    (ph2 - ph1 - c1) fail on every q_add row -- the even chain rows -- and nothing else does."""
    fx = resolve_phases(_fx(k, phases=True), phase_challenges())
    told = [c + 1 for c in phase_challenges()]
    rows = range(0, usable(fx) - 2, 2)
    return fx, told, [(GATE, 5, r, 0) for r in rows] + [(GATE, 6, r, 0) for r in rows]
