"""GPU parity of the generic Pippenger pipeline (msm_digits_kernel / msm_scatter_kernel / msm_accumulate_kernel and the combine
levels) and of every table-mode sorting front (digits with pre = 1, the partition sort at c = 15, its 256-bucket form at
c = 16 and 17, the refinement pass of c = 18..20) against the C oracle's `best_multiexp`, on the inputs where such code goes
wrong: the crafted scalars of tests/msm_digits_model.py (a digit exactly M, a zero digit that still carries, a carry chain
into the top window, one digit at a time in every window), identity / repeated / opposite bases, bucket lists that cancel
or double all the way through the combine levels, a nearly empty launch on a workspace full of old bucket sums, and one
launch of MSMs with very different loads.  tests/test_msm_digits_cpu.py holds the inputs to their events and asserts which
front each (mode, c) below reaches.

Everything runs on a context of the module's own: the tables registered here go away with it."""
import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cbind as OC
from tests import msm_digits_model as D

pytestmark = pytest.mark.gpu

N_FORCED = 600                    # plain launches with a forced window (any length reaches the generic pipeline)
N_UNFORCED = D.MSM_SHORT_MAX + 1  # the shortest plain launch that leaves the short kernel on its own
N_TABLE = 4097                    # 17 scatter blocks of 256 scalars, the last one ragged
N_LONG = 8192


@pytest.fixture(scope="module")
def own():
    from sha2_on_cq_halo2_amd import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(own):
    """8192 distinct points as a host array (an SRS's own device arrays carry tables: the tests upload copies)"""
    from sha2_on_cq_halo2_amd import ParamsKZG
    from sha2_on_cq_halo2_amd.api import fr_to_mont

    params = ParamsKZG.setup_from_toxic_waste(own, 13, fr_to_mont(0xED6E5ED6E5))
    g, _ = params.download()
    params.close()
    g.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def plain_bases(own, srs):
    """2^15 + 1 points on the device, never registered: (host array, DevBuf)"""
    n = (1 << 15) + 1
    host = np.ascontiguousarray(srs[np.arange(n) % srs.shape[0]])
    host.setflags(write=False)
    return host, own.to_device(host)


class _Tables:
    """`pts` uploaded and registered with c-bit window tables; freeing the buffer forgets them"""

    def __init__(self, ctx, pts, c):
        self.ctx, self.n = ctx, pts.shape[0]
        self.buf = ctx.to_device(pts)
        ctx.set_msm_table_window(c)
        try:
            ctx.msm_precompute(self.buf.ptr, self.n)
        finally:
            ctx.set_msm_table_window(0)
        assert ctx.msm_table_width(self.buf.ptr, self.n) == c

    def __enter__(self):
        return self.buf

    def __exit__(self, *exc):
        ptr = self.buf.ptr
        self.buf.free()
        assert self.ctx.msm_table_width(ptr, self.n) == 0


class _Window:
    """cq_msm_set_window(c) for the duration of a block (c = 0: leave the automatic width)"""

    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c

    def __enter__(self):
        if self.c:
            self.ctx.set_msm_window(self.c)

    def __exit__(self, *exc):
        if self.c:
            self.ctx.set_msm_window(0)


def _uniform(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)  # any words below r are a valid Montgomery form of some scalar
    return a


def _mont(values):
    return B.to_mont_limbs([int(v) for v in values])


def _repeat(value, n):
    return np.repeat(_mont([value]), n, axis=0)


def _negated(p):
    """-P of an affine point in Montgomery limbs"""
    q = p.copy()
    q[4:] = B.to_mont_limbs([(B.Q_MOD - y) % B.Q_MOD for y in B.from_mont_limbs(p[4:].reshape(1, 4), B.Q_MOD)], B.Q_MOD)[0]
    return q


def _expect(sc, pts):
    return OC.g1_to_affine(OC.best_multiexp(np.ascontiguousarray(sc), np.ascontiguousarray(pts)))


def _edge_vector(c, n, seed):
    """the whole edge set of c-bit windows at the head and again at the tail (the ragged last block) of a uniform vector"""
    edges = _mont(D.edge_values(c))
    assert 2 * len(edges) <= n
    sc = _uniform(n, seed)
    sc[:len(edges)] = edges
    sc[n - len(edges):] = edges
    return sc


def _run(ctx, sc, dbases, n):
    """one MSM over the first n points of a device array; the scalar buffer is freed again"""
    dsc = ctx.to_device(sc)
    try:
        return OC.g1_to_affine(ctx.best_multiexp_dev(dsc, dbases, n))
    finally:
        dsc.free()


def _batch(ctx, vecs, order, dbases, n):
    dev = [ctx.to_device(v) for v in vecs]
    try:
        res = ctx.msm_batch_dev([dev[i].ptr for i in order], dbases.ptr, n)
        return [OC.g1_to_affine(r) for r in res]
    finally:
        for d in dev:
            d.free()


# ---- digit edges, every front ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [2, 3, 5, 8, 11, 13, 15])
def test_digit_edges_plain_forced_window(own, plain_bases, c):
    """msm_digits_kernel / msm_scatter_kernel in plain mode (one bucket set per window) at every forced width"""
    host, dev = plain_bases
    n = N_FORCED
    assert D.plain_path(n, c) == ("digits", c)
    sc = _edge_vector(c, n, 900 + c)
    with _Window(own, c):
        got = _run(own, sc, dev, n)
    assert np.array_equal(got, _expect(sc, host[:n]))


@pytest.mark.parametrize("n", [N_UNFORCED, (1 << 15) + 1])
def test_digit_edges_plain_automatic_window(own, plain_bases, n):
    """the generic pipeline as a caller gets it: the first length past the short kernel (c = 10) and the first at c = 15"""
    host, dev = plain_bases
    front, c = D.plain_path(n)
    assert front == "digits" and c == {N_UNFORCED: 10, (1 << 15) + 1: 15}[n]
    sc = _edge_vector(c, n, 950 + c)
    got = _run(own, sc, dev, n)
    assert np.array_equal(got, _expect(sc, host[:n]))


@pytest.mark.parametrize("c", [8, 14, 15, 16, 17, 18, 19, 20])
def test_digit_edges_table_mode(own, srs, c):
    """One launch of three MSMs over registered tables: the edge vector, one family alone on every row (all_full: a digit
    -1, then only zero digits that carry, then +1), and the edge vector again -- which reads the first one's lists
    (msm_alias_counts_kernel).  c = 8, 14: digits front with pre = 1; 15: partition sort; 16, 17: 256-bucket partitions;
    18..20: refinement pass."""
    assert D.front_of(True, c) == {8: "digits", 14: "digits", 15: "part", 16: "part-wide", 17: "part-wide"}.get(c, "part-refine")
    n = N_TABLE
    pts = srs[:n]
    edges = _edge_vector(c, n, 1000 + c)
    alone = _repeat(D.edge_scalars(c)["all_full"][0], n)
    with _Tables(own, pts, c) as dev:
        got = _batch(own, [edges, alone], [0, 1, 0], dev, n)
    exp = [_expect(edges, pts), _expect(alone, pts)]
    for j, i in enumerate([0, 1, 0]):
        assert np.array_equal(got[j], exp[i]), "MSM %d of the launch differs from the oracle at c = %d" % (j, c)


# ---- one digit at a time --------------------------------------------------------------------------------------------------

def _one_digit_sequence(ctx, dev, pts, n, c):
    """a full uniform launch, then -- on the workspace it leaves behind -- one non-zero digit per row over all (window, d),
    then no digit at all, then a single term"""
    uni = _uniform(n, 1100 + c)
    assert np.array_equal(_run(ctx, uni, dev, n), _expect(uni, pts))
    keys = D.single_keys(c)
    assert n >= 2 * len(keys)
    sc = _mont([D.single(c, *keys[i % len(keys)]) for i in range(n)])
    assert np.array_equal(_run(ctx, sc, dev, n), _expect(sc, pts)), "one digit per row"
    sparse = np.zeros((n, 4), dtype=np.uint64)  # ... and with every other row zero: buckets of one entry next to empty ones
    sparse[::len(keys) + 1] = sc[::len(keys) + 1]
    assert np.array_equal(_run(ctx, sparse, dev, n), _expect(sparse, pts)), "one digit on few rows"
    zero = np.zeros((n, 4), dtype=np.uint64)
    got = _run(ctx, zero, dev, n)
    assert not got.any() and np.array_equal(got, _expect(zero, pts)), "all-zero scalars"
    last = _mont([D.R - 1])
    assert np.array_equal(_run(ctx, last, dev, 1), _expect(last, pts[:1])), "n = 1, scalar r - 1"


@pytest.mark.parametrize("c", [15, 17, 20])
def test_one_digit_at_a_time_table_mode(own, srs, c):
    """catches a wrong table row T[w], a wrong last bucket (d = M) and a reduction that reads a stale bucket"""
    n = N_TABLE
    with _Tables(own, srs[:n], c) as dev:
        _one_digit_sequence(own, dev, srs[:n], n, c)


def test_one_digit_at_a_time_plain(own, plain_bases):
    host, dev = plain_bases
    with _Window(own, 15):
        _one_digit_sequence(own, dev, host[:N_FORCED], N_FORCED, 15)


# ---- special cases of the additions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,c,n", [("plain", 15, N_FORCED), ("plain", 0, N_UNFORCED), ("table", 15, N_TABLE), ("table", 18, N_TABLE)])
def test_special_cases_of_the_additions_inside_a_bucket(own, srs, mode, c, n):
    """The short suite's test of the same name on the generic accumulate kernel (bases converted on the fly) and in table
    mode: the identity as a base, one point many times in one bucket (doubling), P and -P in one bucket with a third entry
    behind them, and the cancellation only equal bases give: +d and -d of ONE base in window w (the cancel pairs)."""
    if mode == "plain":
        front, cw = D.plain_path(n, c)  # c = 0: the automatic width of this length
        assert front == "digits"
    else:
        cw = c
        assert D.front_of(True, c) == {15: "part", 18: "part-refine"}[c]
    pts = np.ascontiguousarray(srs[np.arange(n) % srs.shape[0]])
    sc = _uniform(n, 1200 + cw)
    pts[0] = 0                        # the identity, as an empty bucket sum is written, under non-zero scalars
    pts[n - 1] = 0
    pts[300:370] = 0
    pts[50:120] = pts[50]             # one point on 70 rows under one scalar: the doubling case of the mixed addition
    sc[50:120] = _mont([5])
    pts[130] = _negated(pts[131])     # P and -P under equal scalars: the bucket cancels, the next addition starts from the identity
    sc[130:133] = _mont([9])
    row = 140                         # +d and -d of one base in one bucket, +1 of it in the next window
    for w, d in D.cancel_keys(cw):
        pts[row + 1] = pts[row]
        sc[row:row + 2] = _mont(D.cancel(cw, w, d))
        row += 2
    exp = _expect(sc, pts)
    if mode == "plain":
        dev = own.to_device(pts)
        try:
            with _Window(own, c):
                got = _run(own, sc, dev, n)
        finally:
            dev.free()
    else:
        with _Tables(own, pts, c) as dev:
            got = _run(own, sc, dev, n)
    assert np.array_equal(got, exp)


# ---- long cancelling lists ------------------------------------------------------------------------------------------------

def _long_case(kind, c, srs):
    """(scalars, bases, must_be_identity) of N_LONG rows over one point P"""
    n = N_LONG
    p = srs[7]
    pts = np.repeat(p.reshape(1, 8), n, axis=0)
    i = np.arange(n)
    if kind == "alternate":           # P, -P, P, -P, .. under one scalar
        pts[i % 2 == 1] = _negated(p)
        return _repeat(B.fr_random(B.Xoshiro256ss(1300 + c)), n), pts, True
    if kind == "runs":                # twelve P, four -P, ..: sub-list sums are equal or opposite multiples of P, n / 2 P remain
        pts[i % 16 >= 12] = _negated(p)
        return _repeat(B.fr_random(B.Xoshiro256ss(1301 + c)), n), pts, False
    w, d = {"pair-low": (0, 1), "pair-high": (D.below_top(c) - 1, (1 << (c - 1)) - 1)}[kind]
    assert (w, d) in D.cancel_keys(c)
    sc = np.tile(_mont(D.cancel(c, w, d)), (n // 2, 1))  # rows alternate a, b: +d / -d cancel, n / 2 times +1 one window up
    return sc, pts, False


@pytest.mark.parametrize("kind", ["alternate", "runs", "pair-low", "pair-high"])
@pytest.mark.parametrize("mode", ["table", "plain"])
def test_long_lists_that_cancel_or_double(own, srs, mode, kind):
    """8192 rows over P and -P: every bucket list has 4096 entries or more -- hundreds of accumulate sub-lists, two combine
    levels -- whose partial sums are equal or opposite multiples of P: the mixed addition and the combine levels' XYZZ +
    XYZZ addition see doubling and cancellation at every step.  c = 15 in both modes.  "alternate" sums to the identity by
    cancellation alone; "runs" and the two cancel pairs also need every doubling to be right (their sums are n / 2 times a
    multiple of P)."""
    c, n = 15, N_LONG
    sc, pts, identity = _long_case(kind, c, srs)
    exp = _expect(sc, pts)
    if mode == "plain":
        assert D.plain_path(n, c) == ("digits", c)
        dev = own.to_device(pts)
        try:
            with _Window(own, c):
                got = _run(own, sc, dev, n)
        finally:
            dev.free()
    else:
        with _Tables(own, pts, c) as dev:
            got = _run(own, sc, dev, n)
    assert np.array_equal(got, exp)
    assert got.any() != identity


# ---- mixed launch ---------------------------------------------------------------------------------------------------------

def test_mixed_launch_of_very_different_loads(own, srs):
    """One table-mode launch (c = 15) whose MSMs share the plan and the scans: an ordinary one, an empty one, one whose
    entries all sit in the LAST bucket (all_M on every row: 16 x 4097 entries), and one whose lists cancel to the identity
    (rows 2k and 2k + 1 hold P_k and -P_k under one scalar)."""
    c, n = 15, N_TABLE
    pts = srs[:n].copy()
    for k in range(1024):
        pts[2 * k + 1] = _negated(pts[2 * k])
    uni = _uniform(n, 1400)
    zero = np.zeros((n, 4), dtype=np.uint64)
    hot = _repeat(D.edge_scalars(c)["all_M"][0], n)
    pairs = np.zeros((n, 4), dtype=np.uint64)
    pairs[:2048] = _mont([B.fr_random(B.Xoshiro256ss(1401))])
    vecs = [uni, zero, hot, pairs]
    with _Tables(own, pts, c) as dev:
        got = _batch(own, vecs, [0, 1, 2, 3], dev, n)
    for j, v in enumerate(vecs):
        assert np.array_equal(got[j], _expect(v, pts)), "MSM %d of the launch differs from the oracle" % j
    assert not got[1].any() and not got[3].any() and got[0].any() and got[2].any()
