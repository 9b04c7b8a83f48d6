"""CPU: the fixtures of tests/plonk_limits.py mean what they claim -- degree, product sets, extended domain, rows -- and the
oracle, which no reference fixture pins above degree 5, makes VALID proofs at the degree boundaries: the restated verifier
(oracle/cq_verifier.py) accepts the proof of a satisfied witness at degrees 3, 6, 10 and 18, the witness-check model finds
nothing, and one changed cell of a_0 turns both around.  tests/test_plonk_limits_gpu.py compares the GPU with these."""
import functools
import time

import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import cq_verifier as CV
from tests import witness_check_model as M
from tests.plonk_fixtures import TABLE, c_msm, oracle_env
from tests.plonk_limits import CASES, REJECTED, compiled_stack_depth, limit_circuit, permutation_sets

P = B.R_MOD


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_is_the_shape_it_claims(name):
    k, degree, perm_columns, kw, _ = CASES[name]
    n = 1 << k
    for satisfied in (False, True):
        fx = limit_circuit(k, degree, perm_columns, satisfied=satisfied, **kw)
        cs = fx["circuit"]
        assert cs.degree() == degree
        assert len(cs.perm_columns) == perm_columns == len(set(cs.perm_columns)) == len(fx["mapping"])
        sets = permutation_sets(perm_columns, degree)
        assert sets == -(-perm_columns // (degree - 2))
        dom = CP.EvaluationDomain(cs.degree(), k)
        assert dom.extended_k - k == (degree - 2).bit_length()  # ceil(log2(degree - 1))
        assert 1 << (dom.extended_k - k) >= degree - 1 > 1 << (dom.extended_k - k) >> 1
        assert cs.blinding_factors() + 3 <= n
        assert {kind for kind, _ in cs.perm_columns} == ({"advice", "fixed", "instance"} if perm_columns > 2 else {"advice", "fixed"})
        if "depth" in kw:
            assert compiled_stack_depth(cs, 1) == kw["depth"] == 16
        if kw.get("phases"):
            assert cs.num_phases() == 3
        if "legacy_width" in kw:
            assert [len(ins) for ins, _ in cs.plookups] == [kw["legacy_width"]]
        if "rotations" in kw:
            rots = {r for _, r in cs.advice_queries() + cs.fixed_queries()}
            assert set(kw["rotations"]) <= rots and cs.blinding_factors() <= 6
        # copies cross column kinds and the boundaries between product sets
        chunk = degree - 2
        moved = [(c, tuple(fx["mapping"][c][r])) for c in range(perm_columns) for r in range(n) if tuple(fx["mapping"][c][r]) != (c, r)]
        assert len(moved) >= (4 if k == 3 else 12)  # k = 3 has four usable permutation cells in all
        assert any(cs.perm_columns[c][0] != cs.perm_columns[c2][0] for c, (c2, _) in moved)
        if sets > 1:
            assert any(c // chunk != c2 // chunk for c, (c2, _) in moved)
    assert name != "smallest-k3" or (n == 8 and cs.blinding_factors() + 3 == n)


def test_fixtures_one_step_past_each_limit():
    shape = {}
    for name, ((k, degree, perm_columns, kw), _) in REJECTED.items():
        cs = limit_circuit(k, degree, perm_columns, **kw)["circuit"]
        shape[name] = (cs.degree(), len(cs.perm_columns), compiled_stack_depth(cs, 1) if "depth" in kw else None,
                       [len(ins) for ins, _ in cs.plookups])
    assert shape["degree19"][0] == 19 and shape["cols65"][1] == 65 and shape["depth17"][2] == 17 and shape["legacy-width65"][3] == [65]


@functools.lru_cache(maxsize=None)
def _satisfied_env(degree):
    """Oracle key and SRS of the satisfied degree-boundary case (never modified)."""
    k, d, perm_columns, kw, _ = CASES[f"deg{degree}"]
    assert d == degree and k == 5
    return oracle_env(k, builder=limit_circuit, fast=True, degree=degree, perm_columns=perm_columns, satisfied=True, **kw)


def _verify(fx, proof, opener):
    commit = lambda cols: B.batch_to_affine([c_msm(c, fx["params"].g_lagrange) for c in cols])
    if "vk" not in fx:
        fx["vk"] = (commit(fx["pk"].fixed_values), commit(fx["pk"].permutations))
    return CV.verify_proof(proof, fx["circuit"], 424242, fx["s"], fx["tables"], len(TABLE), 1 << fx["circuit"].k, instances=fx["instances"],
                           fixed_commitments=fx["vk"][0], perm_commitments=fx["vk"][1], opener=opener)


def _model(fx, advice):
    return M.check_witness(fx["circuit"], fx["fixed"], advice, fx["instances"], fx["mapping"], fx["tables"])


@pytest.mark.parametrize("degree,opener", [(3, "gwc"), (3, "shplonk"), (6, "gwc"), (10, "gwc"), (18, "gwc"), (18, "shplonk")])
def test_oracle_proof_of_a_satisfied_witness_verifies(degree, opener):
    fx = _satisfied_env(degree)
    t0 = time.time()
    tr = CP.create_proof(fx["params"], fx["pk"], fx["advice"], B.Xoshiro256ss(degree), msm=c_msm, instances=fx["instances"], opener=opener)
    t1 = time.time()
    assert _verify(fx, tr.proof, opener)
    assert _model(fx, fx["advice"]) == (0, [])
    # one cell of a_0, on a row whose gate reads usable cells only and that no copy constraint names
    col0 = fx["circuit"].perm_columns.index(("advice", 0))
    row = next(r for r in fx["gate_rows"] if tuple(fx["mapping"][col0][r]) == (col0, r))
    bad = [list(c) for c in fx["advice"]]
    bad[0][row] = (bad[0][row] + 1) % P
    assert _model(fx, bad) == (1, [(M.GATE, 0, row, 0)])
    tr_bad = CP.create_proof(fx["params"], fx["pk"], bad, B.Xoshiro256ss(degree), msm=c_msm, instances=fx["instances"], opener=opener)
    assert not _verify(fx, tr_bad.proof, opener)
    print(f"degree {degree} {opener}: proof {len(tr.proof)} B in {t1 - t0:.1f} s, verified and mutated in {time.time() - t1:.1f} s")
