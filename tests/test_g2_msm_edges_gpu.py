"""The G2 Pippenger (csrc/msm_g2.hip) where such code goes wrong, against [k]_2 of the C oracle: the crafted scalars of
tests/msm_digits_model.py at every window width the engine has (c = 4..16, each reached through n as callers reach it),
one digit at a time around the lane boundaries of the window reduction at every depth of its tree, one bucket holding
all entries on either side of every change of the level count, short buckets beside ragged and exact lanes, doubling and
cancellation in every addition of the engine (the mixed addition of level 1, the XYZZ addition of the later levels, the
window reduction's `acc += run`, the host fold), and the fixed-base kernel of the SRS at one table row, alternating signs
and sparse bytes.  tests/g2_msm_model.py says what the kernels do for each n; tests/test_g2_msm_model_cpu.py holds the
inputs built here to the events they are named for.

Every base has a known discrete log, so every expected value is ONE [k]_2 with k summed in Python integers mod r; the
comparison is exact."""
import functools

import numpy as np
import pytest

from oracle import bn254 as B
from sha2_on_cq_halo2_amd import G2Srs
from sha2_on_cq_halo2_amd._lib import load
from tests import g2_msm_model as G
from tests import msm_digits_model as D
from tests.g2_helpers import R, fr_mont, g2_mul_limbs

pytestmark = pytest.mark.gpu

S_TOXIC = 0x1B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
N_SRS = (1 << 20) + 1
R256_INV = pow(1 << 256, -1, R)
P_LOG, Q_LOG = 0x5EED0001C0FFEE, 0x7A11F00D5EED0002   # discrete logs of the host-side bases P and Q


def _affine(jac24):
    out = np.zeros(16, dtype=np.uint64)
    j = np.ascontiguousarray(jac24, dtype=np.uint64)
    assert load().cq_g2_to_affine(j.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.fixture(scope="module")
def powers():
    """s^i mod r for i < N_SRS: (list of Python integers, the same as an object array)"""
    out, v = [1] * N_SRS, 1
    for i in range(1, N_SRS):
        v = v * S_TOXIC % R
        out[i] = v
    return out, np.array(out, dtype=object)


@pytest.fixture(scope="module")
def srs(ctx, powers):
    """[s^i]_2 for i <= 2^20 on the device.  Every expected value below rests on it: sampled above 2^18 here
    (test_g2_gpu.py samples below)"""
    p = G2Srs.setup_from_toxic_waste(ctx, N_SRS, fr_mont([S_TOXIC])[0])
    pts = p.download()
    rng = B.Xoshiro256ss(0x62D0)
    idx = {(1 << 18) + 1, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20}
    while len(idx) < 16:
        idx.add((1 << 18) + 1 + int(B.fr_random(rng) % (N_SRS - (1 << 18) - 1)))
    for i in sorted(idx):
        assert i > 1 << 18 and np.array_equal(pts[i], g2_mul_limbs(powers[0][i])), i
    del pts
    yield p
    p.close()


def _uniform(n, seed):
    """random words below r, taken as Montgomery forms: the scalar of a row is its words * 2^-256"""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def _uniform_dot(limbs, pw):
    """sum_i (scalar of row i) * pw[i] mod r for rows of _uniform"""
    words = sum(int(np.dot(limbs[:, j].astype(object), pw)) << (64 * j) for j in range(4))
    return words * R256_INV % R


def _mont_rows(scalars):
    """Montgomery limbs of a list with few distinct values"""
    uniq = sorted(set(scalars))
    at = {k: i for i, k in enumerate(uniq)}
    return np.ascontiguousarray(fr_mont(uniq)[[at[k] for k in scalars]])


def _run_srs(ctx, srs, sc):
    """sum_i sc[i] * [s^i]_2, affine; the scalar buffer is freed again"""
    dsc = ctx.to_device(sc)
    try:
        return _affine(ctx.best_multiexp_g2_dev(dsc, srs.dev, sc.shape[0]))
    finally:
        dsc.free()


@functools.lru_cache(maxsize=None)
def _point(log):
    p = g2_mul_limbs(log)
    p.setflags(write=False)
    return p


def _run_host(ctx, scalars, logs):
    """sum_i scalars[i] * [logs[i]]_2 over host bases, checked against the oracle; returns the affine result"""
    uniq = sorted({v % R for v in logs})
    at = {v: i for i, v in enumerate(uniq)}
    bases = np.ascontiguousarray(np.array([_point(v) for v in uniq], dtype=np.uint64)[[at[v % R] for v in logs]])
    got = _affine(ctx.best_multiexp_g2(_mont_rows(scalars), bases))
    expect = sum(k * v for k, v in zip(scalars, logs)) % R
    assert np.array_equal(got, g2_mul_limbs(expect))
    assert got.any() == (expect != 0)
    return got


# ---- a. digit edges at every width ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(4, 17))
def test_digit_edges_at_every_width(ctx, srs, powers, c):
    """the whole edge set at the first rows and again at the last ones, uniform scalars between, at the smallest n of
    each width (the largest for c = 4).  c = 5 and 15 have W c = 255: the top window ends at the scalars' last bit"""
    n = G.edges_n(c)
    assert G.window_bits(n) == c
    edges = D.edge_values(c)
    m = len(edges)
    assert 2 * m <= n
    sc = _uniform(n, 0x6300 + c)
    sc[:m] = sc[n - m:] = fr_mont(edges)
    pw, pw_obj = powers
    expect = _uniform_dot(sc[m:n - m], pw_obj[m:n - m])
    expect += sum(k * (pw[i] + pw[n - m + i]) for i, k in enumerate(edges))
    got = _run_srs(ctx, srs, sc)
    assert np.array_equal(got, g2_mul_limbs(expect))


# ---- b. one digit at a time -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [4, 6, 10, 13, 14])
def test_one_digit_at_a_time(ctx, srs, powers, c):
    """all scalars zero but one row per (window, digit at a lane boundary of the window reduction), each on a base of its
    own: a wrong top bucket, a wrong g R multiple or a tree pass that reads the neighbouring window changes the sum.
    G = 1, 2, 32, 256, 512 lanes per window: no tree and its one, two, two and three passes.  Then, on the same context,
    no digit at all and a single term on the last row."""
    pw, _ = powers
    n, rows = G.one_digit_case(c)
    sc = np.zeros((n, 4), dtype=np.uint64)
    order = sorted(rows)
    sc[order] = fr_mont([rows[i] for i in order])
    got = _run_srs(ctx, srs, sc)
    assert np.array_equal(got, g2_mul_limbs(sum(k * pw[i] for i, k in rows.items())))
    sc[:] = 0
    assert not _run_srs(ctx, srs, sc).any(), "all scalars zero"
    sc[n - 1] = fr_mont([R - 1])[0]
    assert np.array_equal(_run_srs(ctx, srs, sc), g2_mul_limbs((R - 1) * pw[n - 1])), "one term on the last row"


# ---- c. level thresholds ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.LEVEL_SIZES)
def test_one_bucket_of_n_entries_at_level_thresholds(ctx, srs, powers, n):
    """one scalar on every row: each window has ONE bucket of n entries, summed in L = 1, 2, 2, 3, 3, 4, 4, 5 levels; past
    a threshold the last level adds one item that came up alone"""
    assert G.levels(n) == {32: 1, 33: 2, 512: 2, 513: 3, 8192: 3, 8193: 4, 131072: 4, 131073: 5}[n]
    k = 0x1F2E3D4C5B6A79880123456789ABCDEF ^ n
    got = _run_srs(ctx, srs, np.repeat(fr_mont([k]), n, axis=0))
    assert np.array_equal(got, g2_mul_limbs(k * sum(powers[0][:n])))


def test_short_ragged_and_exact_buckets_through_four_levels(ctx, srs, powers):
    """n = 8193 (L = 4): groups of 1, 31, 32, 33, 511, 512, 513, 1025 rows and the remaining 5535 under a scalar each: a
    bucket of one entry is carried through three levels beside ragged and exact lanes"""
    rng = B.Xoshiro256ss(0x62E0)
    sc = G.mixed_case([B.fr_random(rng) for _ in range(len(G.MIXED_GROUPS) + 1)])
    assert G.levels(len(sc)) == 4
    got = _run_srs(ctx, srs, _mont_rows(sc))
    assert np.array_equal(got, g2_mul_limbs(sum(k * p for k, p in zip(sc, powers[0]))))


# ---- d. special cases of every addition -------------------------------------------------------------------------------------

def test_level_one_doubles_cancels_and_skips_the_identity(ctx):
    k = 0x0123456789ABCDEF0FEDCBA987654321
    _run_host(ctx, [k] * 64, [P_LOG] * 64)                         # one base 64 times: a lane's second entry doubles
    _run_host(ctx, [k] * 3, [P_LOG, R - P_LOG, Q_LOG])             # P, -P, Q in one bucket
    assert not _run_host(ctx, [k] * 2, [P_LOG, R - P_LOG]).any()
    logs = [(P_LOG, Q_LOG, 3 * P_LOG, 5 * Q_LOG, 7 * P_LOG)[i % 5] for i in range(100)]
    for i in (0, 1, 31, 32, 33, 50, 63, 64, 99):                   # identity bases at the ends of level 1's lanes and between
        logs[i] = 0
    _run_host(ctx, [k] * 100, logs)
    n = 600                                                        # only identity bases, under uniform scalars
    got = ctx.best_multiexp_g2(_uniform(n, 0x6350), np.zeros((n, 16), dtype=np.uint64))
    assert not _affine(got).any()


@pytest.mark.parametrize("n", [1024, 8192])
@pytest.mark.parametrize("kind", G.LONG_KINDS)
def test_long_lists_double_and_cancel_above_level_one(ctx, kind, n):
    """n rows over P and -P (c = 6 and 9, L = 3): the lane sums of level 1 are the identity ("alternate"), +32 P and -32 P
    in turn ("runs": the XYZZ addition of level 2 cancels) or all 32 P ("pair-low", "pair-high": it doubles, on level 3
    too at n = 8192)"""
    sc, signs, identity = G.long_case(kind, n, 0x2B3C4D5E6F708192A3B4C5D6E7F8091A)
    got = _run_host(ctx, sc, [s * P_LOG for s in signs])
    assert got.any() != identity


@pytest.mark.parametrize("c", [6, 10])
def test_window_reduction_meets_its_own_running_sum(ctx, c):
    """P under digit d and [-2]P under digit d - 1 of one window, nothing else: `acc += run` adds -P to P, and the buckets
    below add to an identity accumulator.  d in the first lane and at the top of the last one"""
    n = G.smallest_n(c)
    for d in G.reduce_cancel_digits(c):
        for w in (0, D.below_top(c) // 2):
            sc, logs = [0] * n, [Q_LOG] * n
            for row, (k, m) in zip((7, n - 2), G.reduce_cancel_case(c, w, d)):
                sc[row], logs[row] = k, m * P_LOG
            _run_host(ctx, sc, logs)


@pytest.mark.parametrize("c,n", [(4, 2), (6, 1024)])
def test_host_fold_adds_equal_and_opposite_window_sums(ctx, c, n):
    """[2^c]P under 1 and P under 2^c: window sum 1 doubled c times meets window sum 0, the same point; with -[2^c]P its
    opposite"""
    assert G.window_bits(n) == c
    for sign in (1, -1):
        sc, logs = [0] * n, [Q_LOG] * n
        for row, (k, m) in zip((0, n - 1), G.fold_case(c, sign)):
            sc[row], logs[row] = k, m * P_LOG
        assert _run_host(ctx, sc, logs).any() == (sign == 1)


# ---- e. the fixed-base kernel of the SRS ------------------------------------------------------------------------------------

FIXED_BASE_S = {"1": 1, "r-1": R - 1, "2^8": 1 << 8, "2^248+1": (1 << 248) + 1}


@functools.lru_cache(maxsize=None)
def _srs_expected(name):
    s = FIXED_BASE_S[name]
    return np.array([g2_mul_limbs(pow(s, i, R)) for i in range(129)], dtype=np.uint64)


@pytest.mark.parametrize("count", [1, 127, 128, 129])
@pytest.mark.parametrize("name", list(FIXED_BASE_S))
def test_srs_powers_at_the_fixed_base_kernels_edges(ctx, name, count):
    """s = 1: one table row only; r - 1: G and -G in turn; 2^8: a single byte moving up the rows until it wraps mod r;
    2^248 + 1: for i = 1 all rows but two are skipped.  One block less a lane, one block, one block and a lane: every
    point is compared"""
    p = G2Srs.setup_from_toxic_waste(ctx, count, fr_mont([FIXED_BASE_S[name]])[0])
    try:
        pts = p.download()
    finally:
        p.close()
    assert pts.shape == (count, 16) and np.array_equal(pts, _srs_expected(name)[:count])
