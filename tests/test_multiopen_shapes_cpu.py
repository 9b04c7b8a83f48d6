"""CPU: the multi-open oracles (oracle.shplonk.shplonk_prove, stages_helpers.gwc_prove) pinned from the verifier side on
every case table of tests/multiopen_cases.py, before tests/test_multiopen_shapes_gpu.py compares the device with them
there.  With the scalar "commitment" commit(p) = p(s) the pairing checks become identities in Fr:

  SHPLONK (shplonk/verifier.rs:88-138, oracle.shplonk.shplonk_verifier_terms):
      s h2 = sum_i scalar_i p_i(s) - r_outer - z_0 h1 + u h2
  GWC (gwc/verifier.rs:76-128), per distinct point x with witness w:
      w (s - x) = sum_i v^i (p_i(s) - e_i)   over the point's queries in order

The provers see only polynomials and evaluations, the verifier side only commitments and evaluations, and neither
identity holds for a wrong quotient except with negligible probability.  The mutation tests show that they do fail."""
import pytest

from oracle import bn254 as B
from oracle import kzg
from oracle.poly import eval_polynomial, msm_affine
from oracle.shplonk import shplonk_prove, shplonk_verifier_terms

from .multiopen_cases import ALL, DUPLICATE, SET_LIMITS, THRESHOLD, build, case_name, key_secret
from .stages_helpers import ScriptedTranscript, gwc_prove, trapdoor_commit

P = B.R_MOD


def _shplonk_sides(case, s, queries=None, commit=None):
    """(left, right) of the SHPLONK identity, for the proof of the case's own queries read against `queries`."""
    n = 1 << case.k
    commit = commit or (lambda poly: eval_polynomial(poly, s))
    tr = ScriptedTranscript(case.script)
    assert shplonk_prove(tr, n, case.queries, case.polys, commit) == case.script
    h1, h2 = tr.points
    y, v, u = case.script
    terms, r_outer, z_0 = shplonk_verifier_terms(queries or case.queries, y, v, u)
    at_s = {key: eval_polynomial(poly, s) for key, poly in case.polys.items()}
    right = (sum(scalar * at_s[key] for scalar, key in terms) - r_outer - z_0 * h1 + u * h2) % P
    return s * h2 % P, right, (h1, h2)


def _gwc_sides(case, s, queries=None):
    """[(left, right)] of the GWC identity per distinct point, and the witnesses."""
    n = 1 << case.k
    tr = ScriptedTranscript(case.script[1:2])
    v = gwc_prove(tr, n, case.queries, case.polys, None, commit=lambda poly: eval_polynomial(poly, s))
    points = list(dict.fromkeys(pt for _, pt, _ in case.queries))
    assert len(tr.points) == len(points)
    at_s = {key: eval_polynomial(poly, s) for key, poly in case.polys.items()}
    sides = []
    for w, x in zip(tr.points, points):
        right, pv = 0, 1
        for key, pt, ev in queries or case.queries:
            if pt == x:
                right, pv = (right + pv * (at_s[key] - ev)) % P, pv * v % P
        sides.append((w * (s - x) % P, right))
    return sides, tr.points


@pytest.mark.parametrize("case_id", ALL, ids=case_name)
def test_the_oracles_satisfy_the_verifier_identities_on_every_case_table(case_id):
    """Also: no commitment of any case is the identity (p(s) = 0), which cq_multiopen_dev may refuse (CQ_ERR_TRANSCRIPT)."""
    case = build(case_id)
    s = key_secret(case.k)
    left, right, commitments = _shplonk_sides(case, s)
    assert left == right
    assert all(c != 0 for c in commitments)
    sides, witnesses = _gwc_sides(case, s)
    assert all(l == r for l, r in sides)
    assert all(w != 0 for w in witnesses)


@pytest.mark.parametrize("case_id", [THRESHOLD[0], SET_LIMITS[0], DUPLICATE[0]], ids=case_name)
def test_the_identities_fail_for_a_wrong_evaluation_and_a_wrong_quotient(case_id):
    case = build(case_id)
    s = key_secret(case.k)
    for at in (0, len(case.queries) // 2, len(case.queries) - 1):  # one evaluation off by one, on the verifier's side
        key, pt, ev = case.queries[at]
        wrong = case.queries[:at] + [(key, pt, (ev + 1) % P)] + case.queries[at + 1:]
        if case_id == DUPLICATE[0]:  # a repeated query: SHPLONK reads the first of the two, GWC both
            wrong = [(k_, p_, (ev + 1) % P if (k_, p_) == (key, pt) else e_) for k_, p_, e_ in case.queries]
        left, right, _ = _shplonk_sides(case, s, queries=wrong)
        assert left != right
        assert any(l != r for l, r in _gwc_sides(case, s, queries=wrong)[0])
    calls = []

    def h1_off_by_one_coefficient(poly):  # the first polynomial committed is h1's
        calls.append(len(poly))
        if len(calls) == 1:
            poly = poly[:3] + [(poly[3] + 1) % P] + poly[4:]
        return eval_polynomial(poly, s)

    left, right, _ = _shplonk_sides(case, s, commit=h1_off_by_one_coefficient)
    assert len(calls) == 2 and left != right


def test_the_trapdoor_commitment_is_the_msm_over_the_srs():
    k = 5
    n, s = 1 << k, key_secret(k)
    poly = build(THRESHOLD[0]).polys[0][:n]
    g = kzg.ParamsKZG(k, s).g
    assert trapdoor_commit(s)(poly) == msm_affine(poly, g[:n])
    assert trapdoor_commit(s)(poly[: n - 1]) == msm_affine(poly[: n - 1], g[: n - 1])
