"""GPU: [b_0] and [p] from per-table-row bucket sums ("b's commitments by table row").

  * the bucket-sum launch on its own (cq_msm_bucket_sums_dev), every bucket of every array against host sums of the same
    points: a skewed index vector at the size and shape of a k = 18 proof's launch (2^18 rows, 90 % of them on one bucket,
    eight arrays sharing one list: three combine levels and the wave-per-long-list path) and a uniform one;
  * [b_0] and [p] assembled from the bucket sums of the key's own row bases against the coefficient-path MSMs of the same
    key (cq_cq_round2_dev);
  * whole proofs byte for byte against the C restatement of the reference prover on the witness shapes that stress the
    launch: every row on one table row, every one of the 4096 table rows in use, uniform indices, the SHA witness's mix."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cbind as OC

pytestmark = pytest.mark.gpu


def _host_bucket_sums(points, index, buckets):
    """sum of points[i] over index[i] == b, per bucket: the C oracle's multiexp with unit scalars over the bucket's points"""
    one = B.to_mont_limbs([1])[0]
    order = np.argsort(index, kind="stable")
    sorted_idx = index[order]
    out = np.zeros((buckets, 8), dtype=np.uint64)
    lo = np.searchsorted(sorted_idx, np.arange(buckets), side="left")
    hi = np.searchsorted(sorted_idx, np.arange(buckets), side="right")
    for b in range(buckets):
        if hi[b] > lo[b]:
            pts = points[order[lo[b]:hi[b]]]
            out[b] = OC.g1_to_affine(OC.best_multiexp(np.tile(one, (len(pts), 1)), pts))
    return out


@pytest.mark.parametrize("shape", ["skewed", "uniform"])
def test_bucket_sums_equal_host_sums(ctx, shape):
    from sha2_on_cq_halo2_amd import ParamsKZG

    k, buckets = 18, 4097
    n = 1 << k
    params = ParamsKZG.setup_from_toxic_waste(ctx, k, B.to_mont_limbs([B.fr_random(B.Xoshiro256ss(18))])[0])
    g, gl = params.download()
    rs = np.random.RandomState(3)
    if shape == "skewed":  # 90.6 % of the rows on bucket 0, the rest spread, bucket 77 empty, the last bucket a handful of rows
        index = np.where(rs.rand(n) < 0.906, 0, rs.randint(1, buckets - 1, size=n)).astype(np.uint32)
        index[index == 77] = 78
        index[n - 6:] = buckets - 1
    else:  # no skew; a few rows name no bucket at all
        index = rs.randint(0, buckets, size=n).astype(np.uint32)
        index[::1000] = 0xFFFFFFFF
        index[5::1000] = buckets
    assert (np.bincount(index[index < buckets], minlength=buckets) > 0).sum() > buckets * 9 // 10  # (the input itself: most buckets in use)
    ptrs = [params.g_dev, params.g_lagrange_dev] * (4 if shape == "skewed" else 1)  # eight arrays on one list, as a proof's launch
    got = ctx.msm_bucket_sums(ptrs, index, buckets)
    want = [_host_bucket_sums(g, index, buckets), _host_bucket_sums(gl, index, buckets)]
    params.close()
    if shape == "skewed":
        assert not want[0][77].any() and not got[0][77].any()  # an empty bucket is the identity
    for a in range(len(ptrs)):
        bad = np.nonzero((got[a] != want[a % 2]).any(axis=1))[0]
        assert bad.size == 0, "array %d: buckets %s differ" % (a, bad[:8])


def test_b0_and_p_from_row_bases_equal_the_coefficient_path(ctx):
    """Same key, same f, m, theta, beta: (a, q_a, a_0, b_0, p) of cq_cq_round2_dev -- MSMs over b's coefficients -- against
    sum_j b_j S_j over the bucket sums of the key's row bases."""
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, spread16

    k, pairs = 13, 2
    n = 1 << k
    wl = ShaCqWorkload(ctx, k, pairs=pairs)
    N, u = wl.cfg.size, wl.pk.usable_rows
    rng = B.Xoshiro256ss(44)
    theta_i, beta_i = B.fr_random(rng), B.fr_random(rng)
    theta, beta = B.to_mont_limbs([theta_i])[0], B.to_mont_limbs([beta_i])[0]
    f, m, _ = wl.pk.cq_round1([c.ptr for c in wl.cols], theta)
    _, _, cm2, _ = wl.pk.cq_round2(f, m, theta, beta)
    mh = m.download((pairs, N), dtype=np.uint32)
    P = B.R_MOD
    for l in range(pairs):
        dense = np.array(B.from_mont_limbs(wl.cols[2 * l].download((n, 4))[:u]), dtype=np.int64)  # the dense table is the identity map
        index = np.concatenate([dense, np.full(n - u, N)]).astype(np.uint32)  # rows from u on: the extra bucket
        assert np.array_equal(np.bincount(dense, minlength=N), mh[l])
        sums = ctx.msm_bucket_sums([wl.pk.b_row_bases(0), wl.pk.b_row_bases(1)], index, N + 1, packed=True)
        sp = spread16(np.arange(N))
        vals = [pow((theta_i * j + int(sp[j]) + beta_i) % P, P - 2, P) if mh[l][j] else 0 for j in range(N)] + [pow(beta_i, P - 2, P)]
        sc = B.to_mont_limbs(vals)
        for q in range(2):
            assert np.array_equal(OC.g1_to_affine(OC.best_multiexp(sc, sums[q])), cm2[l][3 + q]), ("b0", "p")[q]
    wl.close()


def _witness(kind, u, N, pair, rs):
    if kind == "one_row":  # every usable row looks up table row 3
        return np.full(u, 3, dtype=np.int64)
    if kind == "all_rows":  # every table row, the lower ones twice or more
        return (np.arange(u) * (1 + 2 * pair)) % N
    if kind == "uniform":
        return rs.randint(0, N, size=u)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["one_row", "all_rows", "uniform", "sha"])
def test_proof_bytes_equal_the_coefficient_path(ctx, kind):
    from sha2_on_cq_halo2_amd.api import fr_to_mont
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, small_to_mont, spread16

    k, pairs = 13, 2
    n = 1 << k
    wl = ShaCqWorkload(ctx, k, pairs=pairs)
    N, u = wl.cfg.size, wl.pk.usable_rows
    assert N == 4096 and u > N
    if kind != "sha":
        rs = np.random.RandomState(5)
        for p in range(pairs):
            rows = _witness(kind, u, N, p, rs)
            if kind == "all_rows":
                assert len(set(rows.tolist())) == N
            for col, vals in ((2 * p, rows), (2 * p + 1, spread16(rows))):
                full = np.zeros((n, 4), dtype=np.uint64)
                full[:u] = small_to_mont(vals)
                wl.cols[col].upload(full)
    proof = wl.prove(seed=9)
    assert proof == wl.prove(seed=9)
    g, gl = wl.params.download()
    tl, t0 = wl.cfg.download()
    idx = np.arange(N)
    cproof = OC.create_proof(k, 2 * pairs, [[(2 * p, 0), (2 * p + 1, 1)] for p in range(pairs)],
                             [small_to_mont(idx), small_to_mont(spread16(idx))], [wl.dense.download_qs(), wl.spread.download_qs()],
                             g, gl, tl, t0, g[1:], OC.keygen_l_active(k, 5), fr_to_mont(0xC0FFEE + k),
                             [c.download((n, 4)) for c in wl.cols], 9)
    wl.close()
    assert proof == cproof
