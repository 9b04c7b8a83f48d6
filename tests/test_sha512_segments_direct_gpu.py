"""GPU: cq_sha512_synthesize_segments_dev called directly on bare columns (no key), following tests/sha512_direct.py: 67
one-block segments in three levels at n = 2^17 -- level 0 has 65 lanes, one past a workgroup; segment 65 reads words of
segments 0, 63 and 64 and starts from the final state of segment 1; segment 66 reads segment 65 -- against the pure-Python
model cell for cell over all 18 columns and all n rows, the guard rows behind n untouched.  Then the all-private
description against cq_sha512_synthesize_dev column for column, a level of exactly 64 lanes, the table widths 11 and 16,
two calls queued back to back, a SHA-256 segment synthesis queued just before (the staging's event), and every argument
the entry point refuses."""
import hashlib
import random
import struct

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC256
from sha2_on_cq_halo2_amd import sha256_segments as SS256
from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from sha2_on_cq_halo2_amd._lib import constants
from tests import sha256_direct as D256
from tests import sha512_direct as D
from tests import sha512_segments_model as SM

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
N = 1 << 17
P16 = (SS.PRIVATE,) * 16
V512, V384 = SC.VARIANT_512, SC.VARIANT_384
DW = SS.DigestWord


class Job:
    """A plan and one witness for it, lowered and uploaded."""

    def __init__(self, ctx, plan, values, shared=()):
        self.ctx, self.plan, self.values, self.shared = ctx, plan, values, list(shared)
        self.low = low = SS.lower(plan)
        self._words = ctx.to_device(SS.word_buffer(low, values, shared))
        self._digests = ctx.alloc(64 * len(low.seg_blocks))
        self.rows = SS.rows_for(plan)

    def launch(self, columns, n, table_bits=12, **change):
        """The entry point alone -> its status; nothing here waits for the stream.  `change`: arguments to replace."""
        ctx, low = self.ctx, self.low
        a = dict(table_bits=table_bits, seg_blocks=low.seg_blocks, segments=len(low.seg_blocks), seg_variant=low.seg_variant, sources=low.sources,
                 init_sources=low.init_sources if SS.has_init(self.plan) else None, words=self._words.ptr, words_len=low.words_len, n=n,
                 cols=columns.arr, digests=self._digests.ptr)
        a.update(change)
        ptr = lambda x: None if x is None else x.ctypes.data
        return ctx.lib.cq_sha512_synthesize_segments_dev(ctx.h, a["table_bits"], ptr(a["seg_blocks"]), a["segments"], ptr(a["seg_variant"]),
                                                         ptr(a["sources"]), ptr(a["init_sources"]), a["words"], a["words_len"], a["n"], a["cols"],
                                                         a["digests"])

    def states(self):
        """The final state of every segment as the device left it (waits for the stream)."""
        return [[int(x) for x in s] for s in self._digests.download((len(self.low.seg_blocks), 8), np.uint64)]

    def close(self):
        self._words.close()
        self._digests.close()


def three_levels():
    """The 67 segments: 65 of level 0 -- about a third SHA-384, some with a Const or a Var among their words -- then the two
    that read digests."""
    rng = random.Random(3)
    segs = []
    for j in range(65):
        src = list(P16)
        if j % 7 == 2:
            src[rng.randrange(16)] = SS.Const(rng.choice((0, (1 << 64) - 1, 1 << 63)))
        if j % 9 == 4:
            src[rng.randrange(16)] = SS.Var(j % 2)
        segs.append(SS.Segment(1, tuple(src), None, V384 if rng.random() < 0.35 else V512))
    segs[1] = segs[1]._replace(variant=V384)  # words 6 and 7 of a SHA-384 state are read below
    src65 = (DW(0, 0), DW(63, 7), DW(64, 3), SS.PRIVATE, DW(0, 5), SS.Const(7), DW(64, 6), SS.Var(0)) + (SS.PRIVATE,) * 7 + (DW(63, 0),)
    segs.append(SS.Segment(1, src65, tuple(DW(1, i) for i in range(8))))
    segs.append(SS.Segment(1, tuple(DW(65, 7 - i) for i in range(8)) + (SS.Const(1 << 63),) + (SS.Const(0),) * 6 + (SS.Const(512),)))
    return SS.Plan(tuple(segs), ((66, 8),))


def random_values(plan, seed):
    rng = random.Random(seed)
    edgy = lambda: rng.choice((0, (1 << 64) - 1, 1 << 63, 1)) if rng.random() < 0.1 else rng.getrandbits(64)
    return [[edgy() for _ in range(count)] for count in SS.lower(plan).private_counts], [edgy() for _ in range(SS.var_count(plan))]


class Case:
    """A plan, a witness and -- computed once, never changed -- the model's columns at n."""

    def __init__(self, plan, seed, n=None, table_bits=12):
        self.plan, self.table_bits = plan, table_bits
        self.values, self.shared = random_values(plan, seed)
        self.rows = SS.rows_for(plan)
        self.n = self.rows + 5 if n is None else n
        self.want, self.states, self.inits, _ = SM.plan_witness(plan, self.values, self.shared, table_bits, self.n)

    def job(self, ctx):
        return Job(ctx, self.plan, self.values, self.shared)


@pytest.fixture(scope="module")
def big():
    return Case(three_levels(), 5, N)


@pytest.fixture(scope="module")
def columns(ctx):
    cols = D.Columns(ctx, N)
    yield cols
    cols.close()


@pytest.fixture
def fresh(columns):
    columns.fill()
    return columns


def small_plan():
    """Three levels in four segments of 1, 2, 1 and 1 blocks."""
    seg2 = SS.Segment(1, (DW(0, 1), DW(1, 6)) + P16[2:], tuple(DW(1, 7 - i) for i in range(4)) + (SS.PRIVATE, SS.Const(9), SS.Var(0), DW(0, 0)))
    seg3 = SS.Segment(1, P16[:15] + (DW(2, 7),), (SS.Const(3),) * 8, V384)
    return SS.Plan((SS.Segment(1, P16), SS.Segment(2, P16 + (SS.Var(0),) + P16[1:], None, V384), seg2, seg3), ((3, 6),))


def test_67_segments_in_three_levels(ctx, big, fresh):
    assert SM.levels(big.plan) == [0] * 65 + [1, 2] and big.rows == 67 * SC.rows_for(1) < N
    assert {s.variant for s in big.plan.segments[:64]} == {V512, V384}
    job = big.job(ctx)
    try:
        assert job.launch(fresh, N) == 0
        fresh.assert_equals(big.want, N)
        assert job.states() == big.states
        # the wiring holds in the model's own states: segment 65 starts from the state of segment 1, segment 66 hashes its digest
        assert big.inits[65] == big.states[1] and big.inits[0] == SM.M.IV[big.plan.segments[0].variant]
        data = struct.pack(">8Q", *reversed(big.states[65]))
        assert struct.pack(">8Q", *big.states[66]) == hashlib.sha512(data).digest()
    finally:
        job.close()


def test_two_calls_queued_back_to_back(ctx, big, fresh):
    """Another witness of the same plan first, then the case on the same columns with nothing between them."""
    values, shared = random_values(big.plan, 6)
    other, job = Job(ctx, big.plan, values, shared), big.job(ctx)
    try:
        assert other.launch(fresh, N) == 0 and job.launch(fresh, N) == 0
        fresh.assert_equals(big.want, N)
        assert job.states() == big.states and other.states() != big.states
    finally:
        other.close()
        job.close()


def test_all_private_is_the_unwired_entry_point_column_for_column(ctx, fresh):
    rng = random.Random(8)
    blocks = [1, 2, 1] + [1] * 63 + [3]
    variants = [V384 if rng.random() < 0.4 else V512 for _ in blocks]
    plan = SS.batch(blocks, variants)
    values, _ = random_values(plan, 9)
    n = SS.rows_for(plan) + 5
    rc, states = D.synthesize(ctx, fresh, blocks, variants, [w for v in values for w in v], n)
    assert rc == 0
    want = fresh.download()
    fresh.fill()
    job = Job(ctx, plan, values)
    try:
        assert SM.levels(plan) == [0] * 67 and job.launch(fresh, n) == 0
        got = fresh.download()
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and job.states() == states
        assert not (want[0][:n] == D.PATTERN).all(axis=1).any() and (want[0][n:] == D.PATTERN).all()
    finally:
        job.close()


def test_a_level_of_exactly_64_lanes(ctx, big, fresh):
    """The first 64 segments of the big case and one that reads the first and the last of them: the model's columns are the
    big case's rows with one more segment behind them."""
    seg = SS.Segment(1, (DW(63, 7), DW(0, 0)) + P16[2:], tuple(DW(63, i) for i in range(8)))
    plan = SS.Plan(big.plan.segments[:64] + (seg,), ((64, 8),))
    assert SM.levels(plan) == [0] * 64 + [1]
    own = [random.Random(10).getrandbits(64) for _ in range(14)]
    values = big.values[:64] + [own]
    rows = SS.rows_for(plan)
    n = rows + 5
    words = [big.states[63][7], big.states[0][0]] + own
    part, chaining = SM.cells_of(words, 1, 12, big.states[63])
    want = [list(col[:64 * SC.rows_for(1)]) + p + [0] * 5 for col, p in zip(big.want, part)]
    job = Job(ctx, plan, values, big.shared)
    try:
        assert job.launch(fresh, n) == 0
        fresh.assert_equals(want, n)
        assert job.states() == big.states[:64] + [chaining[-1]]
    finally:
        job.close()


@pytest.mark.parametrize("table_bits", [11, 16])
def test_table_widths(ctx, fresh, table_bits):
    case = Case(small_plan(), table_bits, table_bits=table_bits)
    assert SM.levels(case.plan) == [0, 0, 1, 2]
    job = case.job(ctx)
    try:
        assert job.launch(fresh, case.n, table_bits) == 0
        fresh.assert_equals(case.want, case.n)
        assert job.states() == case.states
    finally:
        job.close()


def test_behind_a_sha256_segment_synthesis(ctx, fresh):
    """A SHA-256 segment synthesis is queued first, on columns of its own; this call's tables go through the same pinned
    staging, which must wait for that call's copy out of it and for nothing else."""
    case = Case(small_plan(), 12)
    rng = random.Random(13)
    messages = [bytes(rng.randrange(256) for _ in range(rng.randrange(56))) for _ in range(40)]
    job256 = D256.SegmentsJob(ctx, SS256.batch([1] * len(messages)), [SC256.pad(m, 1) for m in messages])
    cols256 = D256.Columns(ctx, job256.rows)
    job = case.job(ctx)
    try:
        assert job256.launch(cols256, job256.rows) == 0 and job.launch(fresh, case.n) == 0
        fresh.assert_equals(case.want, case.n)
        assert job.states() == case.states
        assert [struct.pack(">8I", *d) for d in job256.digest_words()] == [hashlib.sha256(m).digest() for m in messages]
    finally:
        job.close()
        job256.close()
        cols256.close()


def test_bad_arguments_are_refused_and_nothing_is_written(ctx, fresh):
    case = Case(small_plan(), 14)
    job = case.job(ctx)
    low, n = job.low, case.n
    D_ = SS.SOURCE_DIGEST

    def sources(at, value):
        out = low.sources.copy()
        out[at] = value
        return out

    def inits(at, value):
        out = low.init_sources.copy()
        out[at] = value
        return out

    u32 = lambda *xs: np.array(xs, dtype=np.uint32)
    bad = [
        (dict(seg_blocks=None), ""), (dict(seg_variant=None), ""), (dict(sources=None), ""), (dict(cols=None), ""), (dict(digests=None), ""),
        (dict(words=None), ""),
        (dict(segments=0), ""),
        (dict(seg_blocks=u32(1, 0, 1, 1)), "segment 1"),
        (dict(seg_variant=u32(0, 1, 2, 1)), "segment 2"),
        (dict(table_bits=SC.MIN_TABLE_BITS - 1), "table_bits"), (dict(table_bits=SC.MAX_TABLE_BITS + 1), "table_bits"),
        (dict(n=case.rows - 1), "segment 3"), (dict(n=SC.rows_for(1)), "segment 1"),
        (dict(sources=sources(5, low.words_len)), "segment 0, word 5"),
        (dict(words_len=low.words_len - 1), "segment 1, word 16"),             # the buffer's last word, the Var: its first reader
        (dict(sources=sources(16 + 20, D_ + 8)), "segment 1, word 20"),        # its own digest
        (dict(sources=sources(3, D_ + 8 * 2 + 1)), "segment 0, word 3"),       # a later one's
        (dict(sources=sources(48 + 2, D_ + 8 * 4)), "segment 2, word 2"),      # a segment that does not exist
        (dict(sources=sources(48 + 7, SS.SOURCE_IV)), "segment 2, word 7"),
        (dict(init_sources=inits(16 + 4, low.words_len)), "segment 2, initial word 4"),
        (dict(init_sources=inits(16 + 1, D_ + 8 * 2 + 1)), "segment 2, initial word 1"),
        (dict(init_sources=inits(3, D_)), "segment 0, initial word 3"),
    ]
    try:
        for change, names in bad:
            rest = {name: v for name, v in change.items() if name not in ("n", "table_bits")}
            assert job.launch(fresh, change.get("n", n), change.get("table_bits", 12), **rest) == ERR_ARG, change
            message = ctx.lib.cq_last_error(ctx.h).decode()
            assert names in message, (change, message)
        fresh.assert_untouched()
        assert job.launch(fresh, case.rows) == 0  # n = rows exactly is enough
        assert job.states() == case.states
        # the sentinel among other initial sources is the variant's own word at that position: segment 3 is SHA-384
        assert job.launch(fresh, n, init_sources=inits(24 + 2, SS.SOURCE_IV)) == 0
        init = [3, 3, SM.M.IV[V384][2]] + [3] * 5
        assert job.states() == case.states[:3] + [SM.compress(case.values[3] + [case.states[2][7]], 1, init)[1][-1]]
    finally:
        job.close()
