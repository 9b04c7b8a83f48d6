"""GPU: the general-circuit prover and the witness checker ON the limits key generation accepts (tests/plonk_limits.py:
degree 3 .. 18 and every extended-domain factor, 1 .. 64 product sets, operand-stack depth 16, far rotations, legacy
lookups 64 wide, the smallest domain) -- proof bytes and key commitments against the oracle, `check_witness` against
tests/witness_check_model.py, a satisfied witness accepted by the restated verifier -- and one step past each limit refused
with its own text.  tests/test_plonk_limits_cpu.py holds the oracle to the verifier at these shapes."""
import functools
import time

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import cq_verifier as CV
from tests import witness_check_model as M
from tests.plonk_fixtures import TABLE, c_msm, oracle_env, to_backend_cs
from tests.plonk_limits import CASES, REJECTED, limit_circuit, permutation_sets

pytestmark = pytest.mark.gpu
P = B.R_MOD
VK_REPR = 424242
CHALLENGES = [0x1234567, 0x89ABCDEF01]  # what the checker is told for the three-phase case


@functools.lru_cache(maxsize=None)
def _env(name):
    """Oracle key, SRS and random witness of one case, shared by its tests (never modified)."""
    k, degree, perm_columns, kw, _ = CASES[name]
    return oracle_env(k, builder=limit_circuit, fast=True, degree=degree, perm_columns=perm_columns, **kw)


@functools.lru_cache(maxsize=None)
def _satisfied(name):
    k, degree, perm_columns, kw, _ = CASES[name]
    return limit_circuit(k, degree, perm_columns, satisfied=True, **kw)


def _backend_pk(ctx, fx, s):
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey

    k = fx["circuit"].k
    gparams = ParamsKZG.setup_from_toxic_waste(ctx, k, B.to_mont_limbs([s])[0])
    return ProvingKey(ctx, gparams, k, 0, [], None, None, B.to_mont_limbs([VK_REPR])[0], cs=to_backend_cs(fx["circuit"], {}),
                      fixed=[B.to_mont_limbs(c) for c in fx["fixed"]], permutation=np.array(fx["mapping"], dtype=np.uint32))


def _padded(values, n):
    return B.to_mont_limbs(list(values) + [0] * (n - len(values)))


def _inst(fx):
    return [B.to_mont_limbs(i) for i in fx["instances"]]


def _prove(ctx, gpk, fx, seed):
    """create_proof; with later phases, through the phase callback that computes their columns from the challenges."""
    cs = fx["circuit"]
    n = 1 << cs.k
    if cs.num_phases() == 1:
        return gpk.create_proof([_padded(c, n) for c in fx["advice"]], seed=seed, instances=_inst(fx))
    bufs = [ctx.to_device(_padded([] if callable(c) else c, n)) for c in fx["advice"]]

    def phase_fn(phase, challenges):
        return {c_: _padded(col(challenges), n) for c_, col in enumerate(fx["advice"]) if callable(col) and cs.phase_of(c_) == phase}

    return gpk.create_proof_phases(bufs, phase_fn, seed=seed, instances=_inst(fx))


def _resolved(fx):
    """The advice with the later-phase columns computed from CHALLENGES."""
    return [c(CHALLENGES) if callable(c) else c for c in fx["advice"]]


def _check(gpk, fx):
    cs = fx["circuit"]
    n = 1 << cs.k
    ch = CHALLENGES if cs.challenge_phases else None
    total, fails = gpk.check_witness([_padded(c, n) for c in _resolved(fx)], _inst(fx), ch, max_failures=1 << 16)
    return total, [tuple(f) for f in fails]


def _model(fx):
    ch = CHALLENGES if fx["circuit"].challenge_phases else ()
    return M.check_witness(fx["circuit"], fx["fixed"], _resolved(fx), fx["instances"], fx["mapping"], fx["tables"], ch)


@pytest.mark.parametrize("name,opener", [(name, opener) for name in CASES for opener in CASES[name][4]])
def test_proof_bytes_and_key_commitments_match_oracle(ctx, name, opener):
    t0 = time.time()
    fx = _env(name)
    cs = fx["circuit"]
    tr = CP.create_proof(fx["params"], fx["pk"], fx["advice"], B.Xoshiro256ss(77), msm=c_msm, instances=fx["instances"], opener=opener)
    t1 = time.time()
    gpk = _backend_pk(ctx, fx, fx["s"])
    fcm, pcm = gpk.vk_commitments()
    commit = lambda cols: B.points_to_mont_limbs(B.batch_to_affine([c_msm(c, fx["params"].g_lagrange) for c in cols]))
    assert np.array_equal(fcm, commit(fx["pk"].fixed_values))
    assert np.array_equal(pcm, commit(fx["pk"].permutations))
    gpk.set_opener(opener)
    proof = _prove(ctx, gpk, fx, 77)
    t2 = time.time()
    print(f"{name} {opener}: k {cs.k} degree {cs.degree()} sets {permutation_sets(len(cs.perm_columns), cs.degree())} "
          f"extended {len(fx['pk'].l0)} proof {len(tr.proof)} B; oracle {t1 - t0:.2f} s, backend key + proof {t2 - t1:.2f} s")
    assert len(proof) == gpk.proof_size == len(tr.proof)
    assert proof == tr.proof
    gpk.close()


@pytest.mark.parametrize("name", list(CASES))
def test_witness_checker_matches_model_and_verifier_accepts(ctx, name):
    t0 = time.time()
    fx, good = _env(name), _satisfied(name)
    cs = fx["circuit"]
    n = 1 << cs.k
    assert good["fixed"] == fx["fixed"] and good["mapping"] == fx["mapping"]  # one key serves both witnesses
    want = _model(fx)
    assert want[0] > 0
    assert _model(good) == (0, [])
    t1 = time.time()
    gpk = _backend_pk(ctx, fx, fx["s"])
    got = _check(gpk, fx)
    print(f"{name}: random witness {got[0]} findings {got[1][:6]}")
    assert got == want
    assert _check(gpk, good) == (0, [])
    proof = _prove(ctx, gpk, good, 9)
    t2 = time.time()
    fcm, pcm = gpk.vk_commitments()
    assert CV.verify_proof(proof, cs, VK_REPR, fx["s"], {}, len(TABLE), n, instances=good["instances"],
                           fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))
    print(f"{name}: models {t1 - t0:.2f} s, backend key + checks + proof {t2 - t1:.2f} s, verifier {time.time() - t2:.2f} s")
    gpk.close()


@functools.lru_cache(maxsize=1)
def _chain():
    from tests.plonk_fixtures import chain_circuit

    fx = oracle_env(5, builder=chain_circuit, fast=True)
    fx["proof"] = CP.create_proof(fx["params"], fx["pk"], fx["advice"], B.Xoshiro256ss(5), msm=c_msm, instances=fx["instances"]).proof
    return fx


@pytest.mark.parametrize("name", list(REJECTED))
def test_one_step_past_each_limit_is_refused(ctx, name):
    """Key creation refuses the shape with the text of the check it trips, and the context goes on proving."""
    from sha2_on_cq_halo2_amd import CqError

    (k, degree, perm_columns, kw), text = REJECTED[name]
    fx = limit_circuit(k, degree, perm_columns, **kw)
    with pytest.raises(CqError) as e:
        _backend_pk(ctx, fx, 12345)
    assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
    chain = _chain()
    gpk = _backend_pk(ctx, chain, chain["s"])
    assert _prove(ctx, gpk, chain, 5) == chain["proof"]
    gpk.close()
