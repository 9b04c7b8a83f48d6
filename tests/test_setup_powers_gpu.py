"""GPU: the trapdoor-free setup path -- `ParamsKZG.from_powers`, `TableConfig.from_srs`, `StaticTable.new_fk(srs_dev=)` and the
fixed-window G1 FFT under them (`g1_fft_windowed`, csrc/g1fft.hip) -- byte for byte against the toxic-waste constructors, the
double-and-add FFT (`cq_g_to_lagrange_dev`) and, at small sizes, the oracle.  Every object here is built from the monomial
powers [s^i]_1 alone; s is used to make those powers and the objects they are compared with."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle import kzg
from tests import g1_structured as S

pytestmark = pytest.mark.gpu
P = B.R_MOD
S_INT = B.fr_random(B.Xoshiro256ss(0x706F77))


def _sm(s=S_INT):
    return B.to_mont_limbs([s])[0]


@pytest.fixture(scope="module")
def powers(ctx):
    """[s^i]_1 for i < 4096 (host array), the stand-in for a ceremony file; read-only."""
    from sha2_on_cq_halo2_amd import ParamsKZG

    p = ParamsKZG.setup_from_toxic_waste(ctx, 12, _sm())
    g = p.download()[0]
    p.close()
    g.setflags(write=False)
    return g


def _inputs(powers, k):
    """(name, uint64[2^k, 8]) inputs of the FFT comparison"""
    n = 1 << k
    g = np.array(powers[:n])
    holes = g.copy()
    for i in {0, n // 2, n - 1}:
        holes[i] = 0  # the identity, (0, 0)
    out = [("powers", g), ("identities", holes), ("all_equal", np.tile(powers[1:2], (n, 1)))]
    # a_j = w^j and w^j + 3 w^((1 + n/2) j): every stage doubles or cancels (tests/g1_structured.py)
    fams = ("character", "two_characters", "antisym") if k <= 7 else ("two_characters",)  # (scalar by scalar on the CPU)
    out += [(cid, S.point_bytes(a)) for fam in fams for cid, a in S.family(fam, k)]
    return out


# 0 and 1 have no twiddle other than 1; 6 is a partial 64-lane block of butterflies and 7 exactly one; 10 is eight blocks
@pytest.mark.parametrize("k", [0, 1, 2, 3, 6, 7, 10])
def test_windowed_fft_equals_double_and_add_fft(ctx, powers, k):
    for name, pts in _inputs(powers, k):
        got = ctx.g_to_lagrange_windowed(pts, k)
        exp = ctx.g_to_lagrange(pts, k)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, "%s k=%d: %d of %d points differ, first at %s" % (name, k, bad.size, 1 << k, bad[:8])
        if k <= 4:
            ref = kzg.g_to_lagrange(B.points_from_mont_limbs(pts), k)
            assert np.array_equal(got, B.points_to_mont_limbs(ref)), "%s k=%d against the oracle" % (name, k)


def test_windowed_fft_rejects_a_wrong_length(ctx, powers):
    from sha2_on_cq_halo2_amd import CqError

    with pytest.raises(CqError):
        ctx.g_to_lagrange_windowed(powers[:3], 2)


@pytest.mark.parametrize("N", [1, 2, 4, 64, 128, 4096])
def test_table_config_from_srs_equals_toxic_waste_setup(ctx, powers, N):
    from sha2_on_cq_halo2_amd import TableConfig

    exp = TableConfig.setup_from_toxic_waste(ctx, N, _sm())
    got = TableConfig.from_srs(ctx, N, powers)  # more powers than it needs: the first N are used
    a0, b0 = exp.download()
    a1, b1 = got.download()
    assert np.array_equal(a0, a1), "g1_lagrange N=%d" % N
    assert np.array_equal(b0, b1), "g_lagrange_opening_at_0 N=%d" % N
    dev = ctx.to_device(np.array(powers[:N]))
    a2, b2 = TableConfig.from_srs(ctx, N, dev, srs_len=N).download()
    assert np.array_equal(a0, a2) and np.array_equal(b0, b2), "device powers N=%d" % N
    if N <= 16:
        o = kzg.TableSRS(N - 1, S_INT)
        assert np.array_equal(a1, B.points_to_mont_limbs(o.g1_lagrange))
        assert np.array_equal(b1, B.points_to_mont_limbs(o.g_lagrange_opening_at_0))


def test_table_config_from_srs_rejects_bad_sizes(ctx, powers):
    from sha2_on_cq_halo2_amd import CqError, TableConfig

    for size, srs in [(8, powers[:7]), (6, powers[:8]), (0, powers[:8])]:
        with pytest.raises(CqError) as ei:
            TableConfig.from_srs(ctx, size, srs)
        assert ei.value.code == -1
    dev = ctx.to_device(np.array(powers[:8]))
    with pytest.raises(CqError) as ei:
        TableConfig.from_srs(ctx, 16, dev, srs_len=8)
    assert ei.value.code == -1


@pytest.mark.parametrize("k", [1, 5, 10])
def test_params_from_powers_equals_toxic_waste_setup(ctx, powers, k):
    from sha2_on_cq_halo2_amd import ParamsKZG

    n = 1 << k
    g0, gl0 = ParamsKZG.setup_from_toxic_waste(ctx, k, _sm()).download()
    assert np.array_equal(g0, powers[:n])
    host = ParamsKZG.from_powers(ctx, k, np.array(powers[:n]))
    g1, gl1 = host.download()
    assert np.array_equal(g0, g1) and np.array_equal(gl0, gl1)
    buf = ctx.to_device(np.array(powers[:n]))
    g2, gl2 = ParamsKZG.from_powers(ctx, k, buf).download()
    g3, gl3 = ParamsKZG.from_powers(ctx, k, host.g_dev).download()  # a bare device address
    assert np.array_equal(g0, g2) and np.array_equal(gl0, gl2)
    assert np.array_equal(g0, g3) and np.array_equal(gl0, gl3)
    # the window tables registered for the new arrays commit like the toxic-waste ones
    from oracle import cbind as OC
    from tests.util import random_scalars

    a = B.to_mont_limbs(random_scalars(n, 3 + k))
    ref = ParamsKZG.setup_from_toxic_waste(ctx, k, _sm())
    assert np.array_equal(OC.g1_to_affine(host.commit_lagrange(a)), OC.g1_to_affine(ref.commit_lagrange(a)))
    assert np.array_equal(OC.g1_to_affine(host.commit(a)), OC.g1_to_affine(ref.commit(a)))


@pytest.mark.parametrize("N", [2, 64, 1024])
def test_static_table_new_fk_from_resident_powers(ctx, powers, N):
    from sha2_on_cq_halo2_amd import CqError, StaticTable

    vm = B.to_mont_limbs(S.values_random(N))
    exp = StaticTable.new_fk(ctx, vm, np.array(powers[:N])).download_qs()
    dev = ctx.to_device(np.array(powers))  # longer than N: only read
    got = StaticTable.new_fk(ctx, vm, srs_dev=dev).download_qs()
    assert np.array_equal(got, exp)
    assert np.array_equal(StaticTable.new_fk(ctx, vm, srs_dev=dev.ptr).download_qs(), exp)
    with pytest.raises(CqError):
        StaticTable.new_fk(ctx, vm)


def _spread(x):
    r = 0
    for i in range(16):
        r |= ((x >> i) & 1) << (2 * i)
    return r


def test_cq_circuit_keyed_from_powers_proves_the_same_bytes(ctx, powers):
    """k = 8, two (dense, spread) lookups over tables of 2^6: the key built from [s^i]_1 alone gives the proof of the
    toxic-waste key for the same witness and seed, and the verifying key's table commitments (G2) are the same points."""
    from sha2_on_cq_halo2_amd import G2Srs, ParamsKZG, ProvingKey, StaticTable, TableConfig

    k, pairs, N = 8, 2, 64
    n = 1 << k
    dense, spread = list(range(N)), [_spread(i) for i in range(N)]
    vk_repr = B.to_mont_limbs([0xC0FFEE + k])[0]

    def key(params, cfg, td, ts):
        lookups = [[(2 * p, td), (2 * p + 1, ts)] for p in range(pairs)]
        return ProvingKey(ctx, params, k, 2 * pairs, lookups, cfg, params.g_dev + 64, vk_repr)

    tparams = ParamsKZG.setup_from_toxic_waste(ctx, k, _sm())
    ttables = [StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(v), _sm()) for v in (dense, spread)]
    tpk = key(tparams, TableConfig.setup_from_toxic_waste(ctx, N, _sm()), *ttables)

    pparams = ParamsKZG.from_powers(ctx, k, np.array(powers[:n]))
    ptables = [StaticTable.new_fk(ctx, B.to_mont_limbs(v), srs_dev=pparams.g_dev) for v in (dense, spread)]
    ppk = key(pparams, TableConfig.from_srs(ctx, N, pparams), *ptables)

    rng = B.Xoshiro256ss(k)
    u = tpk.usable_rows
    cols = []
    for _ in range(pairs):
        vals = [rng.next_u64() % N for _ in range(u - 3)] + [0] * (n - u + 3)
        cols += [B.to_mont_limbs(vals), B.to_mont_limbs([_spread(v) for v in vals])]
    proof = tpk.create_proof(cols, seed=11)
    assert len(proof) > 0 and ppk.create_proof(cols, seed=11) == proof

    g2 = G2Srs.setup_from_toxic_waste(ctx, n + 1, _sm())  # the ceremony's G2 stream
    for t0, t1 in zip(ttables, ptables):
        for a, b in zip(t0.commit(g2, n, n), t1.commit(g2, n, n)):
            assert np.array_equal(a, b)


def test_sha_workload_set_up_from_powers_proves_the_same_bytes(ctx):
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    toxic = ShaCqWorkload(ctx, 10, setup="toxic")
    proof = toxic.prove(seed=5)
    a0, b0 = toxic.cfg.download()
    qs0 = [toxic.dense.download_qs(), toxic.spread.download_qs()]
    g0 = toxic.params.download()
    toxic.close()
    pw = ShaCqWorkload(ctx, 10, setup="powers")
    a1, b1 = pw.cfg.download()
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
    for q0, t in zip(qs0, (pw.dense, pw.spread)):
        assert np.array_equal(q0, t.download_qs())
    for x, y in zip(g0, pw.params.download()):
        assert np.array_equal(x, y)
    assert pw.prove(seed=5) == proof
    pw.close()
