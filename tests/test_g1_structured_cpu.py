"""The scalar model of tests/g1_structured.py against the point-wise oracle, and the properties its input families are
built for.  This guards the families and the model, not the kernels: no GPU."""
import pytest

from oracle import bn254 as B
from oracle import kzg
from tests import g1_structured as S

P = B.R_MOD


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_lagrange_model_equals_pointwise_oracle(k):
    """e_i G from the scalar model == `g_to_lagrange` (oracle/kzg.py) run on the points a_j G, every family."""
    for name, a in S.family_cases(k):
        e = S.lagrange_scalars(a, k)
        assert e == S.lagrange_scalars_direct(a, k), name
        assert S.points_affine(e) == kzg.g_to_lagrange(S.points_affine(a), k), name


@pytest.mark.parametrize("k,n_in,shift", [(2, 3, 1), (3, 5, 2), (3, 7, 1), (3, 1, 7)])
def test_shifted_lagrange_model_equals_pointwise_oracle(k, n_in, shift):
    """The shifted form (the proving key's b_row_bases): the array [identity x shift | g | identity ...]."""
    n = 1 << k
    for name, a in S.family_cases(k):
        a = a[:n_in]
        e = S.lagrange_scalars(a, k, shift)
        assert e == S.lagrange_scalars_direct(a, k, shift), name
        padded = [None] * shift + S.points_affine(a) + [None] * (n - shift - n_in)
        assert S.points_affine(e) == kzg.g_to_lagrange(padded, k), name


def test_lagrange_model_fft_form_equals_direct_sum_k6():
    for name, a in S.family_cases(6):
        assert S.lagrange_scalars(a, 6) == S.lagrange_scalars_direct(a, 6), name


@pytest.mark.parametrize("N", [2, 4, 8])
def test_quotient_model_equals_pointwise_oracle(N):
    """Q_i from the scalar model == `StaticTableValues(values, srs).qs` on the SRS a_j G, every family x value set."""
    k = N.bit_length() - 1
    for vname, vf in S.VALUE_SETS.items():
        values = vf(N)
        assert len(set(values)) == N
        for name, a in S.family_cases(k):
            exp = kzg.StaticTableValues(values, S.points_affine(a)).qs
            assert S.points_affine(S.quotient_scalars(values, a)) == exp, (vname, name)


@pytest.mark.parametrize("N", [4, 16])
def test_quotient_model_equals_closed_form_on_a_real_srs(N):
    s = B.fr_random(B.Xoshiro256ss(N))
    srs = [pow(s, j, P) for j in range(N)]
    for vname, vf in S.VALUE_SETS.items():
        values = vf(N)
        q = S.quotient_scalars(values, srs)
        assert q == S.closed_form_quotient_scalars(values, s), vname
        if N == 4:
            assert S.points_affine(q) == kzg.StaticTableValues.qs_closed_form(values, s), vname


def test_value_sets_are_distinct_and_shaped_as_claimed():
    from oracle.poly import EvaluationDomain

    for N in (2, 4, 32, 64, 128, 256, 1024, 4096):
        for vname, vf in S.VALUE_SETS.items():
            assert len(set(vf(N))) == N, (vname, N)
        assert 0 in S.values_range(N)
    for N in (2, 16, 64):  # T = c X
        c = EvaluationDomain(2, N.bit_length() - 1).lagrange_to_coeff(S.values_monomial(N, False))
        assert c[1] != 0 and all(v == 0 for i, v in enumerate(c) if i != 1)
        c = EvaluationDomain(2, N.bit_length() - 1).lagrange_to_coeff(S.values_monomial(N, True))
        assert N == 2 or sum(1 for v in c if v) > 1


def _flies(a, k):
    return list(S.dit_stages(a, k))


def test_character_butterflies_are_all_degenerate():
    """character(r), k = 4: every butterfly of every stage is identity + identity, an exact doubling or an exact
    cancellation (u = 0 = w t or u = +-w t), all three kinds occur over the parameters, and degenerate pairs carry a
    twiddle (operands with zz != 1)."""
    k = 4
    seen = set()
    for r in S.character_params(k):
        kinds = set()
        twiddled = False
        for stage, flies in _flies(S.fam_character(k, r), k):
            for u, wt, ex in flies:
                assert (u == 0 and wt == 0) or u == wt or u == (-wt) % P, (r, stage)
                kinds.add("zero" if u == 0 else "dbl" if u == wt else "cancel")
                twiddled |= u != 0 and ex != 0
        # u = w t: the sum doubles and the difference cancels; u = -w t: the other way round
        assert "zero" in kinds and kinds & {"dbl", "cancel"}, (r, kinds)
        seen |= kinds
        assert twiddled, r
        e = S.lagrange_scalars(S.fam_character(k, r), k)
        assert e == [1 if i == r else 0 for i in range(1 << k)]
    assert seen == {"zero", "dbl", "cancel"}


def test_same_and_sym_families_double_and_cancel_at_stage_0():
    for k in (1, 4, 6):
        n = 1 << k
        stage0 = _flies(S.fam_same(k), k)[0][1]
        assert all(u == wt == 1 for u, wt, _ in stage0)
        for stage, flies in _flies(S.fam_same(k), k)[1:]:  # afterwards: identity times a twiddle in the odd halves
            assert any(wt == 0 and ex != 0 for _, wt, ex in flies) or k == 1
        assert S.lagrange_scalars(S.fam_same(k), k) == [1] + [0] * (n - 1)
        assert all(u == wt != 0 for u, wt, _ in _flies(S.fam_sym(k), k)[0][1])
        assert all(u == (-wt) % P != 0 for u, wt, _ in _flies(S.fam_antisym(k), k)[0][1])
        e = S.lagrange_scalars(S.fam_sym(k), k)
        assert all(e[i] == 0 for i in range(1, n, 2)) and all(e[i] != 0 for i in range(0, n, 2))
        e = S.lagrange_scalars(S.fam_antisym(k), k)
        assert all(e[i] == 0 for i in range(0, n, 2)) and all(e[i] != 0 for i in range(1, n, 2))


def test_delta_zero_and_mixed_families_reach_what_they_claim():
    for k in (2, 5):
        n = 1 << k
        for j0 in S.delta_params(k):
            a = S.fam_delta(k, j0)
            for stage, flies in _flies(a, k):  # an identity operand in every butterfly
                assert all(u == 0 or wt == 0 for u, wt, _ in flies)
            assert all(v != 0 for v in S.lagrange_scalars(a, k))  # no output is the identity
            if j0 and k > 2:  # a twiddle times the identity, and a twiddle times a live point
                assert any(ex and wt == 0 for _, fl in _flies(a, k) for _, wt, ex in fl)
                assert any(ex and wt != 0 for _, fl in _flies(a, k) for _, wt, ex in fl)
        assert S.lagrange_scalars(S.fam_zero(k), k) == [0] * n
        # two characters: degenerate early stages, then a generic butterfly among identity pairs; G at 1, 3 G at 1 + n/2
        a = S.fam_two_characters(k)
        assert S.lagrange_scalars(a, k) == [1 if i == 1 else 3 if i == 1 + n // 2 else 0 for i in range(n)]
        stages = _flies(a, k)
        assert all(u == wt or u == (-wt) % P for _, fl in stages[:-1] for u, wt, _ in fl)
        assert any(u and u in (wt, (-wt) % P) for _, fl in stages[:-1] for u, wt, _ in fl)
        last = stages[-1][1]
        assert any(u == 0 == wt for u, wt, _ in last) and any(u != 0 and wt != 0 and u not in (wt, (-wt) % P) for u, wt, _ in last)
        # sparse mix: zeros, repeats and generic values
        a = S.fam_sparse_mix(5)
        assert a.count(0) >= 5 and len(set(a)) < len(a) - a.count(0) + 1 and len(set(a)) > 8


def test_families_cover_every_size_of_the_gpu_tests():
    for k in (0, 1, 2, 5, 7, 8, 9, 12):
        cases = S.family_cases(k)
        assert {i.split("(")[0] for i, _ in cases} == set(S.FAMILY_IDS)
        assert all(len(a) == 1 << k and all(0 <= v < P for v in a) for _, a in cases)


def test_point_bytes_match_the_python_oracle():
    import numpy as np

    e = [0, 1, 2, P - 1, B.fr_random(B.Xoshiro256ss(9))]
    assert np.array_equal(S.point_bytes(e), B.points_to_mont_limbs(S.points_affine(e)))
