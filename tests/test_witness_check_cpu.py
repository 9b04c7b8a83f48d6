"""CPU: pins tests/witness_check_model.py -- the yardstick the GPU witness checker is compared with -- before any GPU is
involved: valid fixtures have no findings, every mutation of tests/witness_check_cases.py gives the list written out
there by hand for k = 5, and the poison algebra is the table of dev.rs:126-178."""
import pytest

from tests import witness_check_cases as WC
from tests import witness_check_model as M
from tests.plonk_fixtures import chain_circuit, plonk_api_circuit, random_circuit


def _check(fx, challenges=(), cap=None):
    return M.check_witness(fx["circuit"], fx["fixed"], fx["advice"], fx["instances"], fx["mapping"], fx["tables"], challenges, cap)


@pytest.mark.parametrize("kw", [dict(), dict(degree5=True), dict(with_lookup=True), dict(lookup_expr=True), dict(plookup=True),
                                dict(phases=True)], ids=["deg3", "degree5", "with_lookup", "lookup_expr", "plookup", "phases"])
def test_model_accepts_the_valid_chain_circuits(kw):
    fx = chain_circuit(5, **kw)
    ch = WC.phase_challenges() if kw.get("phases") else ()
    WC.resolve_phases(fx, ch)
    assert _check(fx, ch) == (0, [])


def test_model_accepts_the_plonk_api_circuit():
    assert _check(plonk_api_circuit(5)) == (0, [])


@pytest.mark.parametrize("name", sorted(WC.MUTATIONS))
def test_model_gives_the_hand_written_findings(name):
    fx, expected = WC.MUTATIONS[name](5)
    assert _check(fx) == (len(expected), expected)


def test_model_hand_written_rows_at_k5():
    """The same lists with their row numbers spelled out, so that a slip in the helpers' arithmetic cannot hide."""
    assert WC.wrong_instance(5)[1] == [(5, 2, 23, 0), (5, 3, 1, 0)]
    assert WC.poisoned_gates(5)[1] == [(2, 0, 27, 0)] + [(2, 5, r, 0) for r in (26, 27, 28, 29, 30, 31)]
    assert WC.two_at_once(5)[1] == [(1, 0, 10, 0), (1, 2, 10, 0), (1, 3, 11, 0), (5, 2, 23, 0), (5, 3, 1, 0)]
    assert WC.wrong_challenges(5)[2] == [(1, g, r, 0) for g in (5, 6) for r in range(0, 24, 2)]


def test_model_wrong_challenges_fail_the_two_phase_gates():
    fx, told, expected = WC.wrong_challenges(5)
    assert _check(fx, WC.phase_challenges()) == (0, [])
    assert _check(fx, told) == (len(expected), expected)


def test_model_cap_keeps_the_total_and_the_prefix():
    fx = random_circuit(5, 3)
    total, everything = _check(fx)
    assert total == len(everything) > 8 and everything == sorted(everything)
    assert _check(fx, cap=5) == (total, everything[:5])
    assert _check(fx, cap=0) == (total, [])


def test_poison_algebra():
    """dev.rs:126-178: -P = P; P + x = P; P * 0 = 0; 0 * P = 0; P * x = P; P * P = P; P scaled by 0 = 0, by k = P."""
    Pn = M.POISON
    assert M.v_neg(Pn) is Pn and M.v_neg(3) == M.P - 3
    assert M.v_add(Pn, 0) is Pn and M.v_add(0, Pn) is Pn and M.v_add(Pn, Pn) is Pn and M.v_add(2, 3) == 5
    assert M.v_mul(Pn, 0) == 0 and M.v_mul(0, Pn) == 0
    assert M.v_mul(Pn, 7) is Pn and M.v_mul(7, Pn) is Pn and M.v_mul(Pn, Pn) is Pn and M.v_mul(2, 3) == 6
    assert M.v_scale(Pn, 0) == 0 and M.v_scale(Pn, M.P) == 0 and M.v_scale(Pn, 5) is Pn and M.v_scale(4, 5) == 20
    # a poisoned tuple entry equals a poisoned entry and nothing else (`Value` derives Eq, dev.rs:109)
    assert (Pn, 1) == (Pn, 1) and (Pn, 1) != (0, 1) and (Pn, 1) in {(Pn, 1)}
