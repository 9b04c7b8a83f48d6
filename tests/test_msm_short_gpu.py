"""GPU parity of the short plain-mode MSM path (msm_short_kernel: one workgroup per MSM and 8-bit window) against the C
oracle's `best_multiexp`, through the library's own entry points: lengths around the bucket count and the cut-over, the
batch shapes of a proof ([b_0] / [p]: one scalar vector under two base arrays), the digit and carry edges of the biased
bytes, hot buckets, and the special cases of the additions inside a bucket."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cbind as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HPP = open(os.path.join(ROOT, "sha2_on_cq_halo2_amd", "csrc", "msm.hpp")).read()
MSM_SHORT_MAX = int(re.search(r"#define CQ_MSM_SHORT_MAX (\d+)", _HPP).group(1))
MSM_MAX_BATCH = int(re.search(r"MSM_MAX_BATCH = (\d+)", _HPP).group(1))
# cq_msm_multi_v(ctx, scalars, bases, lens, count, out) has C++ linkage and no Python wrapper
MULTI_V = "_Z14cq_msm_multi_vP6cq_ctxPKPKN2cq2FpINS1_3FrPEEEPKPKNS1_8G1AffineEPKmmPm"


@pytest.fixture(scope="module")
def srs(ctx):
    """8192 SRS points as a host array (the params' own device arrays carry window tables: the tests upload copies)."""
    from sha2_on_cq_halo2_amd import ParamsKZG
    from sha2_on_cq_halo2_amd.api import fr_to_mont

    params = ParamsKZG.setup_from_toxic_waste(ctx, 13, fr_to_mont(0x5EED5EED5EED))
    g, _ = params.download()
    return g


def _bases(srs, n, shift=0):
    """n points: the SRS rotated by `shift`, repeated when n is larger than it"""
    idx = (np.arange(n) + shift) % srs.shape[0]
    return np.ascontiguousarray(srs[idx])


def _uniform(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)  # any words below r are a valid Montgomery form of some scalar
    return a


def _affine(jac):
    return OC.g1_to_affine(jac)


def _check_one(ctx, sc, bases):
    got = _affine(ctx.best_multiexp(sc, bases))
    assert np.array_equal(got, _affine(OC.best_multiexp(sc, bases)))
    return got


def _multi_v(ctx, pairs, n):
    """cq_msm_multi_v over (scalar DevBuf, base DevBuf) pairs of n terms each"""
    fn = getattr(ctx.lib, MULTI_V)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
    count = len(pairs)
    sp = (C.c_void_p * count)(*[s.ptr for s, _ in pairs])
    bp = (C.c_void_p * count)(*[b.ptr for _, b in pairs])
    lens = (C.c_size_t * count)(*([n] * count))
    out = np.zeros((count, 12), dtype=np.uint64)
    ctx._chk(fn(ctx.h, sp, bp, lens, count, out.ctypes.data))
    return out


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 4097, MSM_SHORT_MAX, MSM_SHORT_MAX + 1])
def test_lengths_uniform_scalars(ctx, srs, n):
    """... MSM_SHORT_MAX + 1: the generic pipeline still answers"""
    _check_one(ctx, _uniform(n, 100 + n), _bases(srs, n))


def test_batch_of_two_over_one_base_array(ctx, srs):
    n = 129
    bases = _bases(srs, n, 5)
    scs = [_uniform(n, 7), _uniform(n, 8)]
    db = ctx.to_device(bases)
    ds = [ctx.to_device(s) for s in scs]
    got = ctx.msm_batch_dev([d.ptr for d in ds], db.ptr, n)
    for j in range(2):
        assert np.array_equal(_affine(got[j]), _affine(OC.best_multiexp(scs[j], bases)))


def test_batch_of_eight_with_shared_scalar_vectors(ctx, srs):
    """four scalar vectors, each under two different base arrays: [b_0] and [p] of four lookups"""
    n = 4097
    scs = [_uniform(n, 20 + l) for l in range(4)]
    bss = [_bases(srs, n, 17 * q + 1) for q in range(8)]
    ds = [ctx.to_device(s) for s in scs]
    db = [ctx.to_device(b) for b in bss]
    got = _multi_v(ctx, [(ds[q // 2], db[q]) for q in range(8)], n)
    for q in range(8):
        assert np.array_equal(_affine(got[q]), _affine(OC.best_multiexp(scs[q // 2], bss[q])))


def test_full_batch_of_distinct_base_arrays(ctx, srs):
    n = 129
    scs = [_uniform(n, 40 + j) for j in range(MSM_MAX_BATCH)]
    bss = [_bases(srs, n, 131 * j) for j in range(MSM_MAX_BATCH)]
    ds = [ctx.to_device(s) for s in scs]
    db = [ctx.to_device(b) for b in bss]
    got = _multi_v(ctx, list(zip(ds, db)), n)
    for j in range(MSM_MAX_BATCH):
        assert np.array_equal(_affine(got[j]), _affine(OC.best_multiexp(scs[j], bss[j])))


def test_digit_and_carry_edges(ctx, srs):
    n = 4097
    r = B.R_MOD
    edge = [0, 1, r - 1, r - 2, int("7f" * 32, 16) % r, int("80" * 32, 16) % r, int("ff" * 32, 16) % r,
            int("7f80" * 16, 16) % r, int("807f" * 16, 16) % r, (1 << 253) + 0x80, (1 << 248) - 1, 128, 127, 129, 255, 256]
    sc = _uniform(n, 60)
    sc[:len(edge)] = B.to_mont_limbs(edge)
    sc[n - len(edge):] = B.to_mont_limbs(edge)
    _check_one(ctx, sc, _bases(srs, n, 3))


def test_all_zero_scalars_give_the_identity(ctx, srs):
    n = 4097
    got = _check_one(ctx, np.zeros((n, 4), dtype=np.uint64), _bases(srs, n))
    assert not got.any()


@pytest.mark.parametrize("value", [1, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % B.R_MOD])
def test_equal_scalars_one_bucket_per_window(ctx, srs, value):
    """every entry of a window in ONE bucket: the longest list and the hot histogram bin"""
    n = 4097
    sc = np.repeat(B.to_mont_limbs([value]), n, axis=0)
    _check_one(ctx, sc, _bases(srs, n, 9))


def test_special_cases_of_the_additions_inside_a_bucket(ctx, srs):
    n = 300
    bases = _bases(srs, n, 11)
    sc = _uniform(n, 70)
    bases[0:n:7] = 0                  # the identity, as an empty bucket sum is written, under non-zero scalars
    bases[50:120] = bases[50]         # one point repeated under equal scalars: the doubling case of the mixed addition
    sc[50:120] = B.to_mont_limbs([5])
    neg = bases[131].copy()           # P and -P under equal scalars: the bucket cancels, later additions start from the identity
    neg[4:] = B.to_mont_limbs([(B.Q_MOD - y) % B.Q_MOD for y in B.from_mont_limbs(bases[131][4:].reshape(1, 4), B.Q_MOD)], B.Q_MOD)[0]
    bases[130] = neg
    sc[130] = sc[131] = sc[132] = B.to_mont_limbs([9])[0]
    _check_one(ctx, sc, bases)
    # ... and a whole vector of one point under one scalar
    same = np.repeat(bases[1:2], 200, axis=0)
    _check_one(ctx, np.repeat(B.to_mont_limbs([77]), 200, axis=0), same)
