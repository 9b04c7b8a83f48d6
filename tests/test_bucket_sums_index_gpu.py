"""GPU: the index front of the bucket-sum launch (msm_sort.hip: msm_index_count_kernel / msm_index_place_kernel).

Context.msm_bucket_sums hands uint32 bucket indices straight to the launch; every bucket of every array is checked against
host sums of the same points (the C oracle's multiexp with unit scalars).  The shapes are the smallest at which the two
kernels take another path: a lone lane, a ragged last wave, a ragged last tile (a tile is 2048 rows), several tiles; one
bucket up to the 2^14 of a bucket set; one to eight arrays.  Through this entry point every array of a call shares the one
index list (the ABI has a single index pointer); launches with several lists are the proofs at the end of the file, whose
two lookups bring a list each.

The index patterns aim at the ranking: every row on one bucket (one LDS atomic per wave, one device atomic per tile), two
buckets alternating lane by lane (the second ballot round), 64 distinct buckets per wave (every lane sends its own atomic),
every row its own bucket (a full tile table), runs whose ends fall on wave and tile boundaries, nothing in range, and the
SHA witness's mix."""
import ctypes as C

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cbind as OC

pytestmark = pytest.mark.gpu

K = 13
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def srs(ctx):
    from sha2_on_cq_halo2_amd import ParamsKZG

    params = ParamsKZG.setup_from_toxic_waste(ctx, K, B.to_mont_limbs([B.fr_random(B.Xoshiro256ss(13))])[0])
    g, gl = params.download()
    yield params, (g, gl)
    params.close()


def _host_bucket_sums(points, index, buckets):
    """sum of points[i] over index[i] == b, per bucket: the C oracle's multiexp with unit scalars over the bucket's points"""
    one = B.to_mont_limbs([1])[0]
    out = np.zeros((buckets, 8), dtype=np.uint64)
    rows = np.nonzero(index < buckets)[0]
    order = rows[np.argsort(index[rows], kind="stable")]
    sorted_idx = index[order]
    used = np.unique(sorted_idx)
    lo = np.searchsorted(sorted_idx, used, side="left")
    hi = np.searchsorted(sorted_idx, used, side="right")
    for b, l, h in zip(used, lo, hi):
        pts = points[order[l:h]]
        out[b] = OC.g1_to_affine(OC.best_multiexp(np.tile(one, (len(pts), 1)), pts))
    return out


def _check(ctx, srs, index, buckets, arrays):
    params, host = srs
    index = np.ascontiguousarray(index, dtype=np.uint32)
    n = len(index)
    ptrs = [(params.g_dev, params.g_lagrange_dev)[a % 2] for a in range(arrays)]
    got = ctx.msm_bucket_sums(ptrs, index, buckets)
    want = [_host_bucket_sums(host[q][:n], index, buckets) for q in range(min(arrays, 2))]
    for a in range(arrays):
        bad = np.nonzero((got[a] != want[a % 2]).any(axis=1))[0]
        assert bad.size == 0, "array %d: buckets %s differ" % (a, bad[:8])
    return got


def _runs(n, ends, buckets):
    """runs of equal indices: a new bucket starts at every row of `ends`"""
    return (np.searchsorted(np.array(sorted(ends)), np.arange(n), side="right") * 7 % buckets).astype(np.uint32)


def _sparse_2_14(n, rs):
    """rows on buckets 0, 127, 128, 2^14 - 1 and fifty random ones only"""
    pool = np.concatenate([[0, 127, 128, (1 << 14) - 1], rs.choice(np.arange(129, (1 << 14) - 1), size=50, replace=False)])
    index = pool[rs.randint(0, len(pool), size=n)]
    index[: min(n, 4)] = pool[: min(n, 4)]
    return index.astype(np.uint32)


def _sha_mix(n, buckets, rs):
    index = np.where(rs.rand(n) < 0.9, 0, rs.randint(0, buckets, size=n)).astype(np.uint32)
    index[7::500] = NONE
    index[11::500] = buckets
    return index


WAVE_TILE_ENDS = [1, 63, 64, 65, 128, 2047, 2048, 2049, 4095, 4096, 4097, 4100, 6144]

CASES = {
    # id: (n, buckets, arrays, index(n, buckets, rs))
    "lone_row": (1, 1, 1, lambda n, b, rs: np.zeros(n)),
    "lone_row_last_bucket": (1, 1 << 14, 2, lambda n, b, rs: np.full(n, b - 1)),
    "one_bucket_ragged_wave": (63, 2, 2, lambda n, b, rs: np.ones(n)),
    "one_bucket_full_wave": (64, 1, 3, lambda n, b, rs: np.zeros(n)),
    "one_bucket_first_ragged_tile": (4096 + 37, 129, 2, lambda n, b, rs: np.zeros(n)),
    "one_bucket_last_tiles": (8192, 4097, 1, lambda n, b, rs: np.full(n, b - 1)),
    "one_bucket_last_of_2_14": (4096 + 37, 1 << 14, 8, lambda n, b, rs: np.full(n, b - 1)),
    "alternating_two": (65, 2, 1, lambda n, b, rs: np.arange(n) % 2),
    "alternating_two_tiles": (4096 + 37, 129, 3, lambda n, b, rs: np.where(np.arange(n) % 2, 128, 5)),
    "alternating_127_128": (300, 1 << 14, 2, lambda n, b, rs: 127 + np.arange(n) % 2),
    "distinct_per_wave": (65, 129, 1, lambda n, b, rs: np.arange(n) % 64 + 64 * (np.arange(n) // 64 % 2)),
    "distinct_per_wave_tiles": (4096 + 37, 129, 2, lambda n, b, rs: np.arange(n) % 64 + 64 * (np.arange(n) // 64 % 2)),
    "own_bucket_small": (300, 4097, 2, lambda n, b, rs: np.arange(n) * 13 % b),
    "own_bucket_full_tiles": (4096 + 37, 1 << 14, 1, lambda n, b, rs: (np.arange(n) * 3 + 1) % b),
    "own_bucket_4097": (4096, 4097, 1, lambda n, b, rs: rs.permutation(b)[:n]),
    "runs_on_boundaries": (8192, 129, 2, lambda n, b, rs: _runs(n, WAVE_TILE_ENDS, b)),
    "runs_on_boundaries_ragged": (4096 + 37, 4097, 3, lambda n, b, rs: _runs(n, WAVE_TILE_ENDS, b)),
    "none_in_range_ffff": (300, 129, 2, lambda n, b, rs: np.full(n, NONE)),
    "none_in_range_equal_buckets": (4096 + 37, 4097, 1, lambda n, b, rs: np.full(n, b)),
    "none_in_range_2_14": (8192, 1 << 14, 8, lambda n, b, rs: np.where(np.arange(n) % 2, NONE, b)),
    "sha_mix": (8192, 4097, 8, _sha_mix),
    "sha_mix_ragged": (4096 + 37, 129, 3, _sha_mix),
    "sha_mix_two_buckets": (8192, 2, 2, _sha_mix),
    "sparse_2_14": (8192, 1 << 14, 2, lambda n, b, rs: _sparse_2_14(n, rs)),
    "sparse_2_14_ragged_wave": (63, 1 << 14, 3, lambda n, b, rs: _sparse_2_14(n, rs)),
    "uniform_300": (300, 129, 8, lambda n, b, rs: rs.randint(0, b, size=n)),
    "uniform_64": (64, 4097, 2, lambda n, b, rs: rs.randint(0, b, size=n)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bucket_sums_equal_host_sums(ctx, srs, case):
    n, buckets, arrays, make = CASES[case]
    index = np.asarray(make(n, buckets, np.random.RandomState(len(case) + n))).astype(np.int64)
    assert len(index) == n
    got = _check(ctx, srs, index.astype(np.uint32), buckets, arrays)
    in_range = index[(index >= 0) & (index < buckets)]
    if case.startswith("none_in_range"):
        assert in_range.size == 0 and not got.any()  # every output is the identity
    if case.startswith("own_bucket"):
        assert len(set(in_range.tolist())) == n
    if case.startswith("sparse_2_14"):
        used = np.zeros(buckets, dtype=bool)
        used[in_range] = True
        assert used.sum() <= 54 and not got[:, ~used].any()  # all other buckets come back as the identity


def test_second_call_on_the_same_buffers_gives_its_own_result(ctx, srs):
    """The front is a captured graph, replayed when workspace, index pointer, bases and output are the same: the second
    call, with other contents in the same index buffer, must not see the first call's counts or cursors."""
    params, host = srs
    n, buckets = 4096 + 37, 129
    rs = np.random.RandomState(21)
    first = _sha_mix(n, buckets, rs)
    second = np.where(np.arange(n) % 3 == 0, 128, rs.randint(0, buckets, size=n)).astype(np.uint32)
    second[:2048] = NONE  # a tile that names nothing where the first call filled bucket 0
    idx = ctx.to_device(first)
    out = ctx.alloc(2 * buckets * 64)
    arr = (C.c_void_p * 2)(params.g_dev, params.g_lagrange_dev)
    try:
        for index in (first, second, first):
            idx.upload(index)
            ctx._chk(ctx.lib.cq_msm_bucket_sums_dev(ctx.h, arr, 2, 0, idx.ptr, n, buckets, out.ptr))
            got = out.download((2, buckets, 8))
            for q in range(2):
                assert np.array_equal(got[q], _host_bucket_sums(host[q][:n], index, buckets))
    finally:
        idx.close()
        out.close()


def test_proofs_repeat_and_a_bad_row_fails_without_leaving_traces(ctx):
    """k = 13, two lookups (two index lists, two arrays each).  Same seed, same bytes; a usable row whose value is not in the
    table makes round 1 store "no bucket" and the proof fail with the lookup error; the good witness then proves as before."""
    from sha2_on_cq_halo2_amd._lib import CqError
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, small_to_mont

    n = 1 << K
    wl = ShaCqWorkload(ctx, K, pairs=2)
    try:
        N, u = wl.cfg.size, wl.pk.usable_rows
        proof = wl.prove(seed=9)
        assert proof == wl.prove(seed=9)
        good = wl.cols[0].download((n, 4))
        bad = good.copy()
        bad[u // 2] = small_to_mont(np.array([N + 5]))[0]  # the dense table holds 0 .. N - 1
        wl.cols[0].upload(bad)
        with pytest.raises(CqError) as e:
            wl.prove(seed=9)
        assert e.value.code == -4 and "not in table" in str(e.value)  # CQ_ERR_LOOKUP
        wl.cols[0].upload(good)
        assert wl.prove(seed=9) == proof
    finally:
        wl.close()
