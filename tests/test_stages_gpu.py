"""GPU: the stages of create_proof as stand-alone calls (cq_permutation_commit_dev, cq_lookup_commit_product_dev,
cq_evaluate_h_dev, cq_multiopen_dev) against the oracle's restatement of each stage -- oracle.plonk.permutation_commit /
lookup_product, the `h_ext` of oracle.cq_prover.create_proof's trace, oracle.shplonk.shplonk_prove and the GWC restatement
of tests/stages_helpers.py -- byte for byte, for the same challenges and the same position in the RNG stream."""
import ctypes as C

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import plonk as PL
from oracle.poly import msm_affine
from oracle.shplonk import shplonk_prove
from tests.plonk_fixtures import oracle_env, plonk_api_circuit

from .stages_helpers import RecordingTranscript, evaluations, gwc_prove, reference_transcript
from .test_plonk_gpu import _advice_cols, _backend_pk
from .test_prover_gpu import _prove_both, _setup

pytestmark = pytest.mark.gpu
P = B.R_MOD


def _mont(v):
    return B.to_mont_limbs([v])[0]


def _up(ctx, values):
    return ctx.to_device(B.to_mont_limbs(list(values)))


def test_stages_match_the_oracle_on_the_plonk_api_circuit(ctx):
    """plonk_api.rs `MyCircuit` at k = 5: gates with rotations, 12 permutation columns of three kinds in 6 chained sets
    (cs_degree 4), one legacy lookup.  Challenges from the oracle's trace; the RNG stream is replayed up to where the
    reference calls permutation::Argument::commit."""
    k, seed = 5, 3
    n = 1 << k
    fx = oracle_env(k, builder=plonk_api_circuit)
    gpk, _ = _backend_pk(ctx, fx, k, fx["s"])
    tr = CP.create_proof(fx["params"], fx["pk"], fx["advice"], B.Xoshiro256ss(seed), instances=fx["instances"])
    cs, opk, dom = fx["circuit"], fx["pk"], fx["pk"].domain
    bf = cs.blinding_factors()
    u = n - (bf + 1)
    beta, gamma, theta, y = (tr.challenges[c] for c in ("beta", "gamma", "theta", "y"))
    rng = B.BufferRng(B.Xoshiro256ss(seed).words(8 * 400))
    # prover.rs:346-355: blinding rows of every advice column, then one blind per column
    advice = [list(c) + [0] * (u - len(c)) for c in fx["advice"]]
    for col in advice:
        col += [B.fr_random(rng) for _ in range(bf + 1)]
    for _ in advice:
        B.fr_random(rng)
    instance = [list(i) + [0] * (n - len(i)) for i in fx["instances"]]
    # commit_permuted of the one legacy lookup: input = advice a (column 1), table = fixed sl (column 6) (single expressions: theta drops out)
    ci, ct = advice[1], opk.fixed_values[6]
    pi, pt = PL.permute_expression_pair(n, bf, ci, ct, rng)
    B.fr_random(rng)
    B.fr_random(rng)
    pos = rng.pos
    words = np.array(rng.words[pos:], dtype=np.uint64)
    rng_state = gpk._rng(rng_words=words)

    # ---- permutation::Argument::commit
    values = {CP.ADVICE: advice, CP.FIXED: opk.fixed_values, CP.INSTANCE: instance}
    sets = PL.permutation_commit(dom, cs.degree(), bf, cs.perm_columns, lambda col: values[col[0]][col[1]], opk.permutations, beta,
                                 gamma, rng)
    assert len(sets) == 6
    adv_dev = [_up(ctx, c) for c in advice]
    inst_dev = [_up(ctx, c) for c in instance]
    z, cm = gpk.permutation_commit([d.ptr for d in adv_dev], _mont(beta), _mont(gamma), instance_ptrs=[d.ptr for d in inst_dev], rng=rng_state)
    assert np.array_equal(cm, B.points_to_mont_limbs(tr.points["perm_z"])), "permutation product commitments"
    zh = z.download((len(sets), n, 4))
    for st, (z_lag, _blind) in enumerate(sets):
        assert np.array_equal(zh[st], B.to_mont_limbs(dom.lagrange_to_coeff(z_lag))), f"z of set {st}"

    # ---- lookup::Permuted::commit_product, drawing on from the same stream
    lz = PL.lookup_product(n, bf, ci, ct, pi, pt, beta, gamma, rng)
    B.fr_random(rng)
    lk_dev = [_up(ctx, v) for v in (ci, ct, pi, pt)]
    zl, cml = gpk.lookup_commit_product([lk_dev[0].ptr], [lk_dev[1].ptr], [lk_dev[2].ptr], [lk_dev[3].ptr], _mont(beta), _mont(gamma),
                                        rng=rng_state)
    assert np.array_equal(cml, B.points_to_mont_limbs(B.batch_to_affine([fx["params"].commit_lagrange(lz)]))), "lookup product commitment"
    assert np.array_equal(zl.download((n, 4)), B.to_mont_limbs(dom.lagrange_to_coeff(lz)))
    assert gpk._rng_keep[1].pos == rng.pos - pos  # both sides drew the same number of words

    # ---- evaluate_h, then cq_quotient_dev's division: the trace's h (no static lookup: h_ext holds exactly these terms)
    ext = dom.extended_len
    coeff = lambda cols: [_up(ctx, dom.lagrange_to_coeff(c)) for c in cols]
    adv_c, inst_c, perm_c = coeff(advice), coeff(instance), coeff([pi, pt])
    h = gpk.evaluate_h([d.ptr for d in adv_c], _mont(beta), _mont(gamma), _mont(theta), _mont(y), ext, instance_coeff_ptrs=[d.ptr for d in inst_c],
                       perm_z=z, permuted_input_coeff_ptrs=[perm_c[0].ptr], permuted_table_coeff_ptrs=[perm_c[1].ptr], lookup_z=zl)
    assert np.array_equal(h.download((ext, 4)), B.to_mont_limbs(tr.polys["h_ext"])), "h on the extended coset"
    none = ctx.alloc(32)
    hd = gpk.cq_quotient(none, none, _mont(y), _mont(beta), h_in=h, divide=True, ext=ext)
    assert np.array_equal(hd.download((ext, 4)), B.to_mont_limbs(dom.divide_by_vanishing_poly(list(tr.polys["h_ext"]))))
    # and a whole proof with the key afterwards gives its usual bytes
    proof = gpk.create_proof(_advice_cols(fx, n), seed=seed, instances=[B.to_mont_limbs(i) for i in fx["instances"]])
    assert proof == tr.proof


def _cq_env(ctx, k=5):
    N = 1 << k
    return _setup(ctx, k, {"t": list(range(N))}, [[(0, "t")]], 1, 700 + k, srs_len=N)


def test_evaluate_h_of_a_cq_only_key_is_zero_and_the_quotient_agrees_with_null(ctx):
    env = _cq_env(ctx)
    gpk, n = env["gpk"], 32
    tr, proof = _prove_both(env, [[3, 1, 4, 1, 5]], 11)
    assert proof == tr.proof
    ext = env["opk"].domain.extended_len
    beta, y = _mont(tr.challenges["beta"]), _mont(tr.challenges["y"])
    h0 = gpk.evaluate_h([ctx.alloc(n * 32).ptr], beta, beta, beta, y, ext)
    assert not h0.download((ext, 4)).any()
    b, f = _up(ctx, tr.polys["b0"]), _up(ctx, tr.polys["f0"])
    with_zero = gpk.cq_quotient(b, f, y, beta, h_in=h0, divide=True, ext=ext).download((ext, 4))
    with_null = gpk.cq_quotient(b, f, y, beta, divide=True, ext=ext).download((ext, 4))
    assert np.array_equal(with_zero, with_null)
    assert np.array_equal(with_null, B.to_mont_limbs(env["opk"].domain.divide_by_vanishing_poly(list(tr.polys["h_ext"]))))


def _open_case(n, shape):
    """Polynomials of lengths n, n, n - 1, 7, 1 and three points: two polynomials at two points each, one point with a
    single query; or the degenerate shapes."""
    rng = B.Xoshiro256ss(n + len(shape))
    polys = {i: [B.fr_random(rng) for _ in range(ln)] for i, ln in enumerate((n, n, n - 1, 7, 1))}
    x0, x1, x2 = (B.fr_random(rng) for _ in range(3))
    kp = {"mixed": [(0, x0), (0, x1), (1, x0), (1, x1), (2, x0), (4, x0), (3, x2)],
          "single": [(3, x1)],
          "one-point": [(0, x2), (2, x2), (4, x2), (3, x2)]}[shape]
    return polys, evaluations(kp, polys)


@pytest.mark.parametrize("k", [5, 6])
@pytest.mark.parametrize("shape", ["mixed", "single", "one-point"])
@pytest.mark.parametrize("opener", ["gwc", "shplonk"])
def test_multiopen_on_its_own(ctx, k, shape, opener):
    n = 1 << k
    env = _cq_env(ctx, k)
    gpk, g = env["gpk"], env["oparams"].g
    polys, queries = _open_case(n, shape)
    ref = reference_transcript()
    if opener == "shplonk":
        exp_ch = list(shplonk_prove(ref, n, queries, polys, lambda p_: msm_affine(p_, g[: len(p_)])))
    else:
        exp_ch = [gwc_prove(ref, n, queries, polys, g)]
    dev = {key: _up(ctx, c) for key, c in polys.items()}
    rec = RecordingTranscript()
    gpk.set_opener(opener)
    try:
        gpk.multiopen([(dev[key].ptr, len(polys[key]), _mont(pt)) for key, pt, _ in queries], rec.squeeze, rec.write)
    finally:
        gpk.set_opener("gwc")
    assert rec.challenges == exp_ch
    assert bytes(rec.tr.proof) == bytes(ref.proof) and len(rec.points) == (2 if opener == "shplonk" else len({q[1] for q in queries}))


def test_stage_calls_refuse_what_they_cannot_do_and_leave_the_key_usable(ctx):
    from sha2_on_cq_halo2_amd import CqError
    from sha2_on_cq_halo2_amd.api import _ALLGATHER_T

    env = _cq_env(ctx)
    gpk, n = env["gpk"], 32
    tr, proof = _prove_both(env, [[3, 1, 4, 1, 5]], 11)
    one = _mont(1)
    col = ctx.alloc(n * 32)
    poly = _up(ctx, range(1, n + 1))
    rec = RecordingTranscript()

    def refused(call):
        with pytest.raises(CqError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value).split(": ", 1)[1]) > 0, e.value  # CQ_ERR_ARG, cq_last_error set

    refused(lambda: gpk.permutation_commit([col.ptr], one, one, seed=1))  # a key without a permutation argument
    refused(lambda: gpk.multiopen([(poly.ptr, n + 1, one)], rec.squeeze, rec.write))  # a query longer than n
    refused(lambda: gpk.multiopen([(poly.ptr, n, one)], RecordingTranscript(fail_squeeze_at=0).squeeze, rec.write))
    refused(lambda: gpk.multiopen([(poly.ptr, n, one)], rec.squeeze, RecordingTranscript(fail_write_at=0).write))
    never = _ALLGATHER_T(lambda *_: -1)
    ctx._chk(ctx.lib.cq_pk_set_sharding(gpk.h, 0, 2, C.cast(never, C.c_void_p), None))  # a sharded key
    try:
        refused(lambda: gpk.permutation_commit([col.ptr], one, one, seed=1))
        refused(lambda: gpk.lookup_commit_product([col.ptr], [col.ptr], [col.ptr], [col.ptr], one, one, seed=1))
        refused(lambda: gpk.evaluate_h([col.ptr], one, one, one, one, env["opk"].domain.extended_len))
        refused(lambda: gpk.multiopen([(poly.ptr, n, one)], rec.squeeze, rec.write))
    finally:
        ctx._chk(ctx.lib.cq_pk_set_sharding(gpk.h, 0, 1, None, None))
    assert _prove_both(env, [[3, 1, 4, 1, 5]], 11)[1] == proof == tr.proof


@pytest.mark.parametrize("columns", [1, 2, 3, 5])
@pytest.mark.parametrize("degree", [3, 4])
def test_permutation_commit_at_the_set_boundaries(ctx, degree, columns):
    """cs_degree 3 puts one column in a set (1, 2, 3, 5 sets: the single set whose last_z chain is trivial, and the chains);
    cs_degree 4 puts two (one partial set, exactly one full set, a second set of one column, three sets with a partial
    last one).  z of every set and its commitment against oracle.plonk.permutation_commit: last_z chains across the sets
    and the blinding rows are drawn set after set."""
    from oracle import kzg
    from oracle.poly import EvaluationDomain as OracleDomain
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey
    from sha2_on_cq_halo2_amd import plonk as GP

    k = 5
    n = 1 << k
    cs = GP.ConstraintSystem()
    adv = [cs.advice_column() for _ in range(columns)]
    q = cs.fixed_column()
    for a in adv:
        cs.enable_equality(a)
    if degree == 4:
        a0 = cs.query_any(adv[0], 0)
        cs.create_gate("cube", [cs.query_any(q, 0) * a0 * a0 * a0])
    assert cs.degree() == degree
    bf = cs.blinding_factors()
    u = n - (bf + 1)
    rng = B.Xoshiro256ss(40 + 10 * degree + columns)
    cols = [(PL.ADVICE, i) for i in range(columns)]
    asm = PL.Assembly(n, cols)
    for _ in range(6):  # a few cycles, within and across columns
        asm.copy(cols[rng.next_u64() % columns], rng.next_u64() % u, cols[rng.next_u64() % columns], rng.next_u64() % u)
    s = B.fr_random(rng)
    gparams = ParamsKZG.setup_from_toxic_waste(ctx, k, _mont(s))
    gpk = ProvingKey(ctx, gparams, k, 0, [], None, None, _mont(99), cs=cs, fixed=[B.to_mont_limbs([0] * n)],
                     permutation=np.array(asm.mapping, dtype=np.uint32))
    dom = OracleDomain(degree, k)
    perms, _, _ = PL.build_permutation_pk(dom, asm.mapping)
    advice = [[B.fr_random(rng) for _ in range(n)] for _ in range(columns)]
    beta, gamma = B.fr_random(rng), B.fr_random(rng)
    seed = 500 + columns
    sets = PL.permutation_commit(dom, degree, bf, cols, lambda col: advice[col[1]], perms, beta, gamma, B.Xoshiro256ss(seed))
    assert len(sets) == -(-columns // (degree - 2))
    dev = [_up(ctx, c) for c in advice]
    z, cm = gpk.permutation_commit([d.ptr for d in dev], _mont(beta), _mont(gamma), seed=seed)
    zh = z.download((len(sets), n, 4))
    oparams = kzg.ParamsKZG(k, s)
    for st, (z_lag, _blind) in enumerate(sets):
        assert np.array_equal(zh[st], B.to_mont_limbs(dom.lagrange_to_coeff(z_lag))), f"z of set {st}"
    assert np.array_equal(cm, B.points_to_mont_limbs(B.batch_to_affine([oparams.commit_lagrange(z_lag) for z_lag, _ in sets])))
    # the stream stands where the reference leaves it: sets x (bf rows + one blind)
    probe, ref = (C.c_uint64 * 4)(*gpk._rng_keep), B.Xoshiro256ss(seed)
    ref.words(8 * len(sets) * (bf + 1))
    assert ctx.lib.cq_xoshiro256ss_next_u64(probe) == ref.next_u64()


@pytest.mark.parametrize("opener", ["gwc", "shplonk"])
@pytest.mark.parametrize("k", [5, 6])
def test_composed_stages_give_the_bytes_of_the_whole_proof(ctx, k, opener):
    """The `_setup` shape (one static lookup of advice column 0) with a gate that reads a rotation and a copy constraint,
    through the ConstraintSystem mirror.  The whole proof driven from Python (tests/stages_helpers.py: advice commits
    through cq_commit_lagrange_dev, cq_cq_round1/2_dev, the four stage calls, cq_quotient_dev; transcript = the oracle's
    Blake2bWrite behind the callbacks) must give the bytes of ProvingKey.create_proof_dev for the same key and RNG stream."""
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey, StaticTable, TableConfig
    from sha2_on_cq_halo2_amd import plonk as GP

    from .stages_helpers import ComposedProver

    n = N = 1 << k
    sm = _mont(B.fr_random(B.Xoshiro256ss(900 + k)))
    gparams = ParamsKZG.setup_from_toxic_waste(ctx, k, sm)
    gcfg = TableConfig.setup_from_toxic_waste(ctx, N, sm)
    table = StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(list(range(N))), sm)
    cs = GP.ConstraintSystem()
    a0, a1, a2 = (cs.advice_column() for _ in range(3))
    q = cs.fixed_column()
    cs.enable_equality(a1)
    cs.enable_equality(a2)
    cs.create_gate("sum", [cs.query_any(q, 0) * (cs.query_any(a0, 0) + cs.query_any(a1, 0) - cs.query_any(a2, 1))])
    cs.lookup_static("t", [(a0, table)])
    u = n - (cs.blinding_factors() + 1)
    rows = u - 1
    rng = B.Xoshiro256ss(k)
    v0 = [rng.next_u64() % N for _ in range(rows)] + [0]
    v1 = [B.fr_random(rng) for _ in range(rows)] + [0]
    v1[3] = (v0[0] + v1[0]) % P  # the copy constraint below: (a1, 3) == (a2, 1)
    v2 = [0] + [(a + b) % P for a, b in zip(v0[:rows], v1[:rows])]
    mapping = np.zeros((2, n, 2), dtype=np.uint32)
    mapping[0, :, 0], mapping[1, :, 0] = 0, 1
    mapping[:, :, 1] = np.arange(n, dtype=np.uint32)
    mapping[0, 3], mapping[1, 1] = (1, 1), (0, 3)
    fixed = [B.to_mont_limbs([1] * rows + [0] * (n - rows))]
    vk_repr = 0xC0DE + k
    gpk = ProvingKey(ctx, gparams, k, 0, [], gcfg, gparams.g_dev + 64, _mont(vk_repr), cs=cs, fixed=fixed, permutation=mapping)
    gpk.assert_satisfied([B.to_mont_limbs(v + [0] * (n - len(v))) for v in (v0, v1, v2)])
    words = B.Xoshiro256ss(77 + k).words(8 * (n + 200))
    columns = lambda: [_up(ctx, v + [0] * (n - len(v))) for v in (v0, v1, v2)]
    gpk.set_opener(opener)
    whole = gpk.create_proof_dev([c.ptr for c in columns()], rng_words=words)
    composed = ComposedProver(ctx, gpk, fixed, mapping).prove(columns(), words, vk_repr, opener)
    assert len(composed) == gpk.proof_size
    assert composed == whole
