"""GPU: `ProvingKey.check_witness` (cq_pk_check_witness, the MockProver role) against tests/witness_check_model.py --
exact equality of (total, list) -- and against lists written out by hand (tests/witness_check_cases.py, the SHA
workloads' definitions)."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_verifier as CV
from tests import witness_check_cases as WC
from tests import witness_check_model as M
from tests.plonk_fixtures import TABLE, chain_circuit, plonk_api_circuit, random_circuit, to_backend_cs

pytestmark = pytest.mark.gpu
P = B.R_MOD
VK_REPR = 424242


def _backend_pk(ctx, fx, raw_of=None):
    """The backend key of a fixture (SRS from toxic waste, b0_g1_bound = g[1..]); raw_of: read it from that key's bytes."""
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey, StaticTable, TableConfig

    k = fx["circuit"].k
    s = B.fr_random(B.Xoshiro256ss(k))
    fx["s"] = s
    if raw_of is not None:
        gparams, gcfg, tabs = raw_of._keep[0], raw_of._keep[1], raw_of._keep[2]
        gtables = {name: t for name, t in zip(fx["tables"], tabs)}
        cs = to_backend_cs(fx["circuit"], gtables)
        return ProvingKey(ctx, gparams, k, 0, [], gcfg, (gparams.g_dev + 64) if fx["tables"] else None,
                          B.to_mont_limbs([VK_REPR])[0], cs=cs, raw=raw_of.to_bytes())
    sm = B.to_mont_limbs([s])[0]
    gparams = ParamsKZG.setup_from_toxic_waste(ctx, k, sm)
    gtables, gcfg, b0 = {}, None, None
    if fx["tables"]:
        gcfg = TableConfig.setup_from_toxic_waste(ctx, len(TABLE), sm)
        gtables = {name: StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(v), sm) for name, v in fx["tables"].items()}
        b0 = gparams.g_dev + 64
    cs = to_backend_cs(fx["circuit"], gtables)
    return ProvingKey(ctx, gparams, k, 0, [], gcfg, b0, B.to_mont_limbs([VK_REPR])[0], cs=cs,
                      fixed=[B.to_mont_limbs(c) for c in fx["fixed"]], permutation=np.array(fx["mapping"], dtype=np.uint32))


def _cols(fx):
    n = 1 << fx["circuit"].k
    return [B.to_mont_limbs(list(c) + [0] * (n - len(c))) for c in fx["advice"]]


def _inst(fx):
    return [B.to_mont_limbs(i) for i in fx["instances"]]


def _gpu(gpk, fx, challenges=None, cap=1 << 16, cols=None):
    total, fails = gpk.check_witness(cols if cols is not None else _cols(fx), _inst(fx), challenges, max_failures=cap)
    got = (total, [tuple(f) for f in fails])
    print("check_witness:", got[0], got[1][:12])
    return got


def _model(fx, challenges=(), cap=None):
    return M.check_witness(fx["circuit"], fx["fixed"], fx["advice"], fx["instances"], fx["mapping"], fx["tables"], challenges, cap)


# ---- 1. valid witnesses; random circuits -------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(degree5=True), dict(with_lookup=True), dict(lookup_expr=True), dict(plookup=True),
                                dict(phases=True)], ids=["deg3", "degree5", "with_lookup", "lookup_expr", "plookup", "phases"])
def test_valid_chain_circuits_have_no_findings(ctx, kw):
    fx = chain_circuit(5, **kw)
    ch = WC.phase_challenges() if kw.get("phases") else None
    WC.resolve_phases(fx, ch)
    assert _model(fx, ch or ()) == (0, [])
    assert _gpu(_backend_pk(ctx, fx), fx, ch) == (0, [])


def test_valid_plonk_api_circuit_has_no_findings(ctx):
    fx = plonk_api_circuit(5)
    assert _model(fx) == (0, [])
    assert _gpu(_backend_pk(ctx, fx), fx) == (0, [])


def test_valid_k11_has_no_findings(ctx):
    """n = 2048: several blocks per kernel, several words per bitmap row, extended domain 4n."""
    fx = chain_circuit(11, degree5=True, with_lookup=True)
    assert _model(fx) == (0, [])
    assert _gpu(_backend_pk(ctx, fx), fx) == (0, [])


@pytest.mark.parametrize("seed", range(10))
def test_random_circuits_match_the_model(ctx, seed):
    """Ungated random gates over a random witness: nearly every row fails or is poisoned, legacy tuples and permutation
    cycles included -- the stress of ordering, counting and poison propagation."""
    fx = random_circuit(5, seed)
    want = _model(fx)
    assert want[0] > 0
    assert _gpu(_backend_pk(ctx, fx), fx) == want


# ---- 2. one mutation per kind ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.MUTATIONS))
def test_mutations_k5(ctx, name):
    fx, expected = WC.MUTATIONS[name](5)
    assert _model(fx) == (len(expected), expected)
    assert _gpu(_backend_pk(ctx, fx), fx) == (len(expected), expected)


@pytest.mark.parametrize("name", WC.ANY_K)
def test_mutations_k11(ctx, name):
    fx, expected = WC.MUTATIONS[name](11)
    assert _model(fx) == (len(expected), expected)
    assert _gpu(_backend_pk(ctx, fx), fx) == (len(expected), expected)


def test_two_column_static_lookup_details(ctx):
    """ShaCqWorkload, pairs = 2: static lookup 0 reads (column 0, dense table) and (column 1, spread table) and needs
    both on one table row.  Another dense value in column 0 -> found, but on a different row than its spread partner
    (detail 1); 2^TABLE_BITS -> not in the dense table (detail 0)."""
    from sha2_on_cq_halo2_amd.api import fr_from_mont, fr_to_mont
    from sha2_on_cq_halo2_amd.sha_circuit import TABLE_BITS, ShaCqWorkload

    wl = ShaCqWorkload(ctx, 10, pairs=2)
    ptrs = [c.ptr for c in wl.cols]
    assert wl.pk.check_witness(ptrs) == (0, [])
    row = 5
    col0 = wl.cols[0].download((wl.n, 4))
    v = fr_from_mont(col0[row])
    assert v < (1 << TABLE_BITS)
    for new, detail in ((v ^ 1, 1), (1 << TABLE_BITS, 0)):
        bad = col0.copy()
        bad[row] = fr_to_mont(new)
        wl.cols[0].upload(bad)
        total, fails = wl.pk.check_witness(ptrs)
        assert (total, [tuple(f) for f in fails]) == (1, [(4, 0, row, detail)])
    wl.cols[0].upload(col0)
    assert wl.pk.check_witness(ptrs) == (0, [])
    wl.close()


# ---- 3. cap, host / device advice, repeatability ---------------------------------------------------------------------------
def test_cap_host_and_device_advice_and_repeat(ctx):
    fx = random_circuit(5, 4)
    gpk = _backend_pk(ctx, fx)
    total, everything = _model(fx)
    assert total > 20
    cols = _cols(fx)
    for cap in (0, 1, 7, total - 1, total, total + 5):
        assert _gpu(gpk, fx, cap=cap, cols=cols) == (total, everything[:cap])
    dev = [ctx.to_device(c) for c in cols]
    for advice in ([d.ptr for d in dev], dev):
        assert _gpu(gpk, fx, cols=advice) == (total, everything)
        assert _gpu(gpk, fx, cols=advice, cap=3) == (total, everything[:3])
    assert _gpu(gpk, fx, cols=cols) == _gpu(gpk, fx, cols=cols) == (total, everything)


def test_argument_errors(ctx):
    from sha2_on_cq_halo2_amd import CqError

    fx = chain_circuit(5, phases=True)
    WC.resolve_phases(fx, WC.phase_challenges())
    gpk = _backend_pk(ctx, fx)
    cols = _cols(fx)
    with pytest.raises(CqError) as e:  # challenges missing
        gpk.check_witness(cols, _inst(fx))
    assert e.value.code == -1
    with pytest.raises(CqError) as e:  # instances missing
        gpk.check_witness(cols, None, WC.phase_challenges())
    assert e.value.code == -1
    with pytest.raises(CqError) as e:  # Error::InstanceTooLarge
        gpk.check_witness(cols, [B.to_mont_limbs([1] * (gpk.usable_rows + 1))], WC.phase_challenges())
    assert e.value.code == -1


def test_assert_satisfied_names_the_findings(ctx):
    from sha2_on_cq_halo2_amd import CqError, WitnessError

    fx, expected = WC.wrong_c(5)
    gpk = _backend_pk(ctx, fx)
    with pytest.raises(CqError) as e:
        gpk.assert_satisfied(_cols(fx), _inst(fx))
    assert isinstance(e.value, WitnessError) and e.value.total == 3 and [tuple(f) for f in e.value.failures] == expected
    assert "gate polynomial 0 is not satisfied on row 10" in str(e.value)
    good = chain_circuit(5)
    gpk.assert_satisfied(_cols(good), _inst(good))


# ---- 4. a key read back from its raw bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrong_instance", "wrong_fixed_copy", "two_at_once", "static_outside_table"])
def test_raw_key_gives_the_same_findings(ctx, name):
    """cq_pk_read_raw never sees the copy-constraint mapping: the findings come from the sigma values alone."""
    fx, expected = WC.MUTATIONS[name](5)
    gpk = _backend_pk(ctx, fx)
    rpk = _backend_pk(ctx, fx, raw_of=gpk)
    assert _gpu(rpk, fx) == _gpu(gpk, fx) == (len(expected), expected)
    rnd = random_circuit(5, 6)
    gpk = _backend_pk(ctx, rnd)
    assert _gpu(_backend_pk(ctx, rnd, raw_of=gpk), rnd) == _gpu(gpk, rnd) == _model(rnd)


# ---- 5. agreement with the prover and the verifier -------------------------------------------------------------------------
def test_checker_verdict_agrees_with_the_verifier(ctx):
    k = 5
    n = 1 << k
    fx = chain_circuit(k)
    gpk = _backend_pk(ctx, fx)
    fcm, pcm = gpk.vk_commitments()
    to_pts = B.points_from_mont_limbs

    def accepted(f, key=gpk, fcm=fcm, pcm=pcm):
        proof = key.create_proof(_cols(f), seed=9, instances=_inst(f))
        return CV.verify_proof(proof, f["circuit"], VK_REPR, fx["s"], f["tables"], len(TABLE), n, instances=f["instances"],
                               fixed_commitments=to_pts(fcm), perm_commitments=to_pts(pcm))

    assert _gpu(gpk, fx) == (0, []) and accepted(fx)
    bad_gate, _ = WC.wrong_c(k)
    assert _gpu(gpk, bad_gate)[0] == 3 and not accepted(bad_gate)
    bad_perm, _ = WC.wrong_instance(k)
    assert _gpu(gpk, bad_perm)[0] == 2 and not accepted(bad_perm)


def test_proof_bytes_do_not_depend_on_a_check(ctx):
    """create_proof(seed) before and after check_witness on the same context: a used one and a fresh one."""
    from sha2_on_cq_halo2_amd import Context

    for kw in (dict(with_lookup=True), dict(plookup=True)):
        fx = chain_circuit(5, **kw)
        cols, inst = _cols(fx), _inst(fx)
        gpk = _backend_pk(ctx, fx)
        before = gpk.create_proof(cols, seed=11, instances=inst)
        assert _gpu(gpk, fx) == (0, [])
        assert gpk.create_proof(cols, seed=11, instances=inst) == before
        fresh = Context(0)
        fpk = _backend_pk(fresh, fx)
        assert _gpu(fpk, fx) == (0, [])  # the first thing this context ever runs on the key
        assert fpk.create_proof(cols, seed=11, instances=inst) == before
        fresh.close()


# ---- 6. multi-phase -----------------------------------------------------------------------------------------------------------
def test_multi_phase_challenges(ctx):
    fx, told, expected = WC.wrong_challenges(5)
    gpk = _backend_pk(ctx, fx)
    assert _gpu(gpk, fx, WC.phase_challenges()) == (0, [])
    assert _model(fx, told) == (len(expected), expected)
    assert _gpu(gpk, fx, told) == (len(expected), expected)
    assert _gpu(gpk, fx, [B.to_mont_limbs([c])[0] for c in told]) == (len(expected), expected)  # Montgomery limbs


# ---- 7. size: k = 18, the witness on the device as the workloads leave it ----------------------------------------------------
def _overwrite(ctx, buf, row, value):
    from sha2_on_cq_halo2_amd.api import fr_to_mont

    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    ctx._chk(ctx.lib.cq_dev_upload(ctx.h, buf.ptr + 32 * row, v.ctypes.data, 32))


def test_sha_cq_workload_k18(ctx):
    from sha2_on_cq_halo2_amd.sha_circuit import TABLE_BITS, ShaCqWorkload

    wl = ShaCqWorkload(ctx, 18)
    ptrs = [c.ptr for c in wl.cols]
    assert wl.pk.check_witness(ptrs) == (0, [])
    row = 123457
    assert row < wl.pk.usable_rows
    _overwrite(ctx, wl.cols[0], row, 1 << TABLE_BITS)
    total, fails = wl.pk.check_witness(ptrs)
    assert (total, [tuple(f) for f in fails]) == (1, [(4, 0, row, 0)])
    wl.close()


@pytest.mark.parametrize("legacy", [False, True], ids=["static", "static+legacy"])
def test_sha_plonk_workload_k18(ctx, legacy):
    """sha_circuit.py ShaPlonkWorkload: gate 0 "recompose" q (a0 + 2^16 a2 - w), gate 1 "shift" q (w2 - w@next), copies
    (w2, r) == (w, r + 1); permutation columns 0 = w, 1 = w2.  Overwriting w on row r breaks recompose on r, shift on
    r - 1 and the copy between (w, r) and (w2, r - 1): four findings.  With the legacy lookup, column 0 = 4096 on row r0
    also fails the legacy lookup 0 (the fixed table holds 0 .. 4095), static lookup 0 (not in the dense table) and
    recompose on r0."""
    from sha2_on_cq_halo2_amd.sha_circuit import ShaPlonkWorkload

    cls = type("ShaPlonkLegacy", (ShaPlonkWorkload,), dict(legacy_lookup=True)) if legacy else ShaPlonkWorkload
    wl = cls(ctx, 18)
    ptrs = [c.ptr for c in wl.cols]
    assert wl.pk.check_witness(ptrs) == (0, [])
    r = 200001
    assert 0 < r < wl.rows
    _overwrite(ctx, wl.cols[2 * wl.pairs], r, 0xABCDEF12345)
    expected = [(1, 0, r, 0), (1, 1, r - 1, 0), (5, 0, r, 0), (5, 1, r - 1, 0)]
    if legacy:
        r0 = 777
        _overwrite(ctx, wl.cols[0], r0, 4096)
        expected = sorted(expected + [(1, 0, r0, 0), (3, 0, r0, 0), (4, 0, r0, 0)])
    total, fails = wl.pk.check_witness(ptrs)
    print("check_witness:", total, fails)
    assert (total, [tuple(f) for f in fails]) == (len(expected), expected)
    wl.close()
