"""GPU: cq_multiopen_dev (GWC and SHPLONK) against its oracles at the sizes, counts and point sets of
tests/multiopen_cases.py -- poly_kate_division on both sides of its 4096 threshold within one division chain,
block_eval_kernel at a second level with mixed lengths, eval_many / lincomb_many across their batches of 40 and
lincomb_kernel's groups of 6, SHPLONK's 64 sets of 8 points, challenges 0, 1 and p - 1 against coefficients p - 1, and a
repeated query.  Under scripted challenges (no hash) every written commitment must equal the oracle's, point for point;
tests/test_multiopen_shapes_cpu.py pins the oracles on the same tables.  The oracle commits with the key's trapdoor
(p(s) G), which is what keeps k = 12 and 13 to well under a second on the host."""
import pytest

from oracle import bn254 as B
from oracle.shplonk import shplonk_prove

from .multiopen_cases import COUNTS, DUPLICATE, EDGES, SET_LIMITS, SMALL, THRESHOLD, build, case_name, key_secret
from .stages_helpers import ScriptedTranscript, gwc_prove, trapdoor_commit

pytestmark = pytest.mark.gpu
OPENERS = ["gwc", "shplonk"]


@pytest.fixture(scope="module")
def key_for(ctx):
    """k -> the key of test_stages_gpu._cq_env(ctx, k) (one static lookup into range(2^k), SRS of 2^k powers), device side
    only: b0_g1_bound = [s^1 .. s^(n-1)]_1 is read from the params' own powers.  One key per k for the module."""
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey, StaticTable, TableConfig

    keys = {}

    def get(k):
        if k not in keys:
            n = 1 << k
            sm = B.to_mont_limbs([key_secret(k)])[0]
            params = ParamsKZG.setup_from_toxic_waste(ctx, k, sm)
            cfg = TableConfig.setup_from_toxic_waste(ctx, n, sm)
            table = StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(list(range(n))), sm)
            keys[k] = ProvingKey(ctx, params, k, 1, [[(0, table)]], cfg, params.g_dev + 64, B.to_mont_limbs([0x1234567 + k])[0])
        return keys[k]

    yield get
    for gpk in keys.values():
        gpk.close()


def _oracle_points(case, opener):
    n, commit = 1 << case.k, trapdoor_commit(key_secret(case.k))
    if opener == "shplonk":
        tr = ScriptedTranscript(case.script)
        shplonk_prove(tr, n, case.queries, case.polys, commit)
    else:
        tr = ScriptedTranscript(case.script[1:2])
        gwc_prove(tr, n, case.queries, case.polys, None, commit=commit)
    return tr


def _device(ctx, gpk, case, opener, tr=None):
    """The device's transcript (`tr`, or a new one) after cq_multiopen_dev on the case; the opener is GWC again afterwards."""
    limbs, dev = {}, {}
    for key, poly in case.polys.items():  # equal contents (one list object) are converted once and uploaded per key
        if id(poly) not in limbs:
            limbs[id(poly)] = B.to_mont_limbs(poly)
        dev[key] = ctx.to_device(limbs[id(poly)])
    tr = tr or ScriptedTranscript(case.script if opener == "shplonk" else case.script[1:2])
    gpk.set_opener(opener)
    try:
        gpk.multiopen([(dev[key].ptr, len(case.polys[key]), B.to_mont_limbs([pt])[0]) for key, pt, _ in case.queries], tr.squeeze, tr.write)
    finally:
        gpk.set_opener("gwc")
    return tr


def _matches_the_oracle(ctx, gpk, case, opener):
    ref = _oracle_points(case, opener)
    got = _device(ctx, gpk, case, opener)
    assert got.challenges == ref.challenges
    assert len(got.points) == (2 if opener == "shplonk" else len({pt for _, pt, _ in case.queries}))
    assert got.points == ref.points


@pytest.mark.parametrize("opener", OPENERS)
@pytest.mark.parametrize("case_id", THRESHOLD, ids=case_name)
def test_division_chains_across_the_threshold_and_second_level_evaluations(ctx, key_for, case_id, opener):
    case = build(case_id)
    _matches_the_oracle(ctx, key_for(case.k), case, opener)


@pytest.mark.parametrize("opener", OPENERS)
@pytest.mark.parametrize("case_id", COUNTS, ids=case_name)
def test_query_counts_around_the_batch_and_group_sizes(ctx, key_for, case_id, opener):
    case = build(case_id)
    _matches_the_oracle(ctx, key_for(case.k), case, opener)


@pytest.mark.parametrize("opener", OPENERS)
@pytest.mark.parametrize("case_id", EDGES, ids=case_name)
def test_challenges_zero_one_and_minus_one_against_coefficients_minus_one(ctx, key_for, case_id, opener):
    case = build(case_id)
    _matches_the_oracle(ctx, key_for(case.k), case, opener)


@pytest.mark.parametrize("opener", OPENERS)
def test_a_repeated_query_counts_twice_for_gwc_and_once_for_shplonk(ctx, key_for, opener):
    case = build(DUPLICATE[0])
    _matches_the_oracle(ctx, key_for(case.k), case, opener)


@pytest.mark.parametrize("opener", OPENERS)
def test_64_rotation_sets_with_8_points_in_the_last(ctx, key_for, opener):
    """SHPLONK's legal maximum: the last set's remainder takes the last 8 of the scratch's 5 n + 64 * 8 elements."""
    case = build(SET_LIMITS[0])
    _matches_the_oracle(ctx, key_for(case.k), case, opener)


@pytest.mark.parametrize("case_id", SET_LIMITS[1:], ids=case_name)
def test_shplonk_refuses_a_65th_set_and_a_9th_point_and_the_key_stays_usable(ctx, key_for, case_id):
    """Both are argument errors that open_shplonk_queries (prover_open.hip) returns while it still builds the rotation
    sets on the host: "too many rotation sets" after the first squeeze, "rotation set too large" after the second, each
    before the remainders are copied to the scratch and before any lincomb, division or commitment is launched (the
    queries' evaluations, which stage_multiopen computes first, have run).  Nothing is written to the transcript.  GWC has
    no such limits and opens the same queries."""
    from sha2_on_cq_halo2_amd import CqError

    case = build(case_id)
    assert case.shplonk_refuses
    gpk = key_for(case.k)
    tr = ScriptedTranscript(case.script)
    with pytest.raises(CqError) as e:
        _device(ctx, gpk, case, "shplonk", tr)
    assert e.value.code == -1 and len(str(e.value).split(": ", 1)[1]) > 0, e.value  # CQ_ERR_ARG, cq_last_error set
    assert tr.points == [] and tr.challenges == list(case.script[: 1 if case_id == SET_LIMITS[1] else 2])
    for opener in OPENERS:
        _matches_the_oracle(ctx, gpk, build(SMALL), opener)
    _matches_the_oracle(ctx, gpk, case, "gwc")
