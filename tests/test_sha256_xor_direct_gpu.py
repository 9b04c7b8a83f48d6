"""GPU, keyless: cq_sha256_synthesize_xors_dev called directly on bare columns (tests/sha256_direct.py) at n <= 2^12 with
table_bits 11 and 12.  Every comparison is against the XOR model over all 18 columns and all n rows, with the guard rows
behind untouched, and the units' result words behind the digests; a bad description is refused on the host before
anything is launched, which is what is asserted."""
import random

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd._lib import constants
from tests import sha256_direct as D
from tests import sha256_states_model as IM
from tests import sha256_xor_model as XM

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
N = 1 << 12
P16 = (SS.PRIVATE,) * 16


class XorsJob(D.SegmentsJob):
    """A plan without a Choice and one witness for it: cq_sha256_synthesize_xors_dev.  `extra`: Xor units behind the plan's
    own that no word reads, their operands Vars or DigestWords of any segment."""

    def __init__(self, ctx, plan, values, shared=(), extra=()):
        super().__init__(ctx, plan, values, shared)
        low = self.low
        first_var = low.words_len - sum(low.shared_counts)
        src = lambda o: first_var + o.index if isinstance(o, SS.Var) else SS.SOURCE_DIGEST + 8 * o.segment + o.word
        rows = [list(r) for r in low.xors] + [[src(u.x), src(u.y), 0, 0] for u in extra]
        self.xors = np.array(rows, dtype=np.uint32).reshape(-1, SC.XOR_WORDS)
        self.init = low.init_sources if SS.has_init(plan) else None
        self._digests.close()
        self._digests = ctx.alloc(32 * len(low.seg_blocks) + 4 * max(len(self.xors), 1))
        self.rows = SS.rows_for(plan) + SC.XOR_REGIONS * SC.REGION_ROWS * len(extra)

    def launch(self, cols, n, table_bits=12, xors=None, sources=None, n_xors=None, null_xors=False):
        ctx, low = self.ctx, self.low
        xors = self.xors if xors is None else xors
        sources = low.sources if sources is None else sources
        return ctx.lib.cq_sha256_synthesize_xors_dev(ctx.h, table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks), sources.ctypes.data, None, 0,
                                                     None if self.init is None else self.init.ctypes.data,
                                                     None if null_xors else xors.ctypes.data, len(xors) if n_xors is None else n_xors,
                                                     self._words.ptr, low.words_len, n, cols.arr, self._digests.ptr)

    def results(self):
        """Every unit's result word as the device left it behind the digests (waits for the stream)."""
        return self._digests.download(8 * len(self.seg_blocks) + len(self.xors), np.uint32)[8 * len(self.seg_blocks):].tolist()


@pytest.fixture(scope="module")
def columns(ctx):
    sets = [D.Columns(ctx, N) for _ in range(2)]
    yield sets
    for s in sets:
        s.close()


@pytest.fixture
def fresh(columns):
    for s in columns:
        s.fill()
    return columns


def check(ctx, cols, plan, values, shared, n, table_bits=12, extra=()):
    job = XorsJob(ctx, plan, values, shared, extra)
    try:
        assert job.rows <= n <= N
        job.run(cols, n, table_bits)
        want, digests, operands = XM.plan_witness(plan, values, shared, table_bits, n, extra)
        cols.assert_equals(want, n)
        assert job.digest_words() == digests
        assert job.results() == [x ^ y for x, y in operands] and len(operands) == len(job.xors)
        return want, digests, operands
    finally:
        job.close()


@pytest.mark.parametrize("x, y, table_bits", [(0x6A09E667, 0x6A09E667, 12), (0xFFFFFFFF, 0, 11), (0, 0, 12), (0x80000001, 0x7FFFFFFE, 11)])
def test_one_unit_of_two_buffer_words(ctx, fresh, x, y, table_bits):
    plan = SS.Plan((SS.Segment(1, P16[:7] + (SS.Xor(SS.Var(0), SS.Var(1)),) + P16[8:]),), (0,))
    values = [[(0x01010101 * i) & 0xFFFFFFFF for i in range(15)]]
    want, _, operands = check(ctx, fresh[0], plan, values, [x, y], SS.rows_for(plan) + 5, table_bits)
    assert operands == [(x, y)] and SS.rows_for(plan) == 576 + 16
    assert want[XM.X][SC.REGION_ROWS * (4 + 7) + XM.ROW["W"]] == x ^ y == want[XM.X][XM.unit_rows(plan, 0)[1] + XM.ROW["W"]]


def test_one_unit_of_one_buffer_word_twice_and_of_a_constant(ctx, fresh):
    plan = SS.Plan((SS.Segment(1, (SS.Xor(SS.Var(0), SS.Var(0)), SS.Xor(SS.Const(0xFFFFFFFF), SS.Var(0))) + P16[2:]),), (0,))
    _, _, operands = check(ctx, fresh[0], plan, [list(range(14))], [0xDEADBEEF], SS.rows_for(plan) + 5)
    assert operands == [(0xDEADBEEF, 0xDEADBEEF), (0xFFFFFFFF, 0xDEADBEEF)]


def wired_case():
    """Unit 0 = Var 1 ^ Const (level 0), read by segment 0 (level 0) and segment 1; unit 1 = digest word 3 of segment 0 ^
    Var 0 (level 1), read by two words of segment 1 (level 1), whose initial state is wired too.  Extra units that no word
    reads: one over buffer words, one over a digest word of segment 1 -- the last level's, so the launch behind the chains."""
    a, b = SS.Xor(SS.DigestWord(0, 3), SS.Var(0)), SS.Xor(SS.Var(1), SS.Const(0x36363636))
    plan = SS.Plan((SS.Segment(1, P16[:15] + (b,)),
                    SS.Segment(2, (a,) + P16[1:5] + (b,) + P16[6:16] + (a,) + SS.PAD_64_BYTES[1:], (SS.Var(1),) + tuple(SS.DigestWord(0, i) for i in range(1, 8)))),
                   (1,))
    extra = (SS.Xor(SS.Var(0), SS.Var(1)), SS.Xor(SS.DigestWord(1, 7), SS.DigestWord(0, 0)))
    rng = random.Random(5)
    values = [[rng.randrange(1 << 32) for _ in range(15)], [rng.randrange(1 << 32) for _ in range(14)]]
    return plan, values, [0x0BADF00D, 0xCAFEBABE], extra


@pytest.mark.parametrize("table_bits", [11, 12])
def test_digest_operands_shared_units_and_the_trailing_launch(ctx, fresh, table_bits):
    plan, values, shared, extra = wired_case()
    n = SS.rows_for(plan) + 32 + 5
    want, digests, operands = check(ctx, fresh[0], plan, values, shared, n, table_bits, extra)
    assert operands == [(shared[1], 0x36363636), (digests[0][3], shared[0]), (shared[0], shared[1]), (digests[1][7], digests[0][0])]
    assert digests[0] == IM.compress(values[0] + [shared[1] ^ 0x36363636], 1)[1][-1]
    readers = [SC.REGION_ROWS * (72 + 4 + t) + XM.ROW["W"] for t in (0, SC.BLOCK_REGIONS)]  # words 0 and 16 of segment 1
    assert [want[XM.X][r] for r in readers] == [digests[0][3] ^ shared[0]] * 2


def many_units_case():
    """65 units whose levels are 0, 1 and 2 in turn: Var ^ Var, digest of segment 0 ^ Var, digest of segment 1 ^ digest of
    segment 0 (segment 1 reads a level-1 unit, so it runs at level 1).  Segments 2 and 3 read 16 each -- whatever their
    level, so both run at level 2 -- and 33 are read by no word; the last of those reads segment 3's digest: level 3."""
    def unit(t):
        return (SS.Xor(SS.Var(t % 8), SS.Var(8 + t % 56)), SS.Xor(SS.DigestWord(0, t % 8), SS.Var(t % 64)),
                SS.Xor(SS.DigestWord(1, t % 8), SS.DigestWord(0, (t // 8) % 8)))[t % 3]

    units = [unit(t) for t in range(64)] + [SS.Xor(SS.DigestWord(3, 7), SS.Var(63))]
    assert len(set(units)) == 65
    segs = (SS.Segment(1, P16[:15] + (SS.Var(63),)), SS.Segment(1, (units[1],) + P16[1:]), SS.Segment(1, tuple(units[:16])), SS.Segment(1, tuple(units[16:32])))
    rng = random.Random(7)
    values = [[rng.randrange(1 << 32) for _ in range(15)], [rng.randrange(1 << 32) for _ in range(15)], [], []]
    return SS.Plan(segs, (3,)), values, [rng.randrange(1 << 32) for _ in range(64)], units


def test_65_units_of_mixed_levels(ctx, fresh):
    plan, values, shared, units = many_units_case()
    own = SS.xor_units(plan)
    assert own == [units[1]] + [u for u in units[:32] if u != units[1]]
    extra = units[32:]
    assert len(own) + len(extra) == 65 > 64 and SS.rows_for(plan) + 16 * len(extra) == 4 * 576 + 65 * 16 <= N - 5
    _, digests, operands = check(ctx, fresh[0], plan, values, shared, N - 5, 12, extra)
    assert operands[-1] == (digests[3][7], shared[63])


def test_no_units_is_the_states_entry_point(ctx, fresh):
    rng = random.Random(23)
    plan = SS.Plan((SS.Segment(1, P16), SS.Segment(2, P16 + tuple(SS.DigestWord(0, i) for i in range(8)) + P16[8:]),
                    SS.Segment(1, P16, tuple(SS.DigestWord(1, i) for i in range(4)) + (SS.PRIVATE, SS.Const(9), SS.Var(0), SS.Var(0)))), (2,))
    values = [[rng.randrange(1 << 32) for _ in range(n_)] for n_ in (16, 24, 17)]
    job = XorsJob(ctx, plan, values, [77])
    try:
        low, n = job.low, job.rows + 5
        assert job.init is not None and len(job.xors) == 0
        rc = ctx.lib.cq_sha256_synthesize_states_dev(ctx.h, 12, low.seg_blocks.ctypes.data, 3, low.sources.ctypes.data, None, 0, job.init.ctypes.data,
                                                     job._words.ptr, low.words_len, n, fresh[0].arr, job._digests.ptr)
        assert rc == 0
        want, digests = fresh[0].download(), job.digest_words()
        for null in (True, False):
            fresh[1].fill()
            assert job.launch(fresh[1], n, null_xors=null) == 0
            for i, (a, b) in enumerate(zip(want, fresh[1].download())):
                assert np.array_equal(a, b), f"advice column {i}"
            assert job.digest_words() == digests
        model, model_digests, _ = XM.plan_witness(plan, values, [77], 12, n)
        fresh[0].assert_equals(model, n, got=want)
        assert digests == model_digests
    finally:
        job.close()


def test_refusals_write_nothing(ctx, fresh):
    plan, values, shared, extra = wired_case()
    job = XorsJob(ctx, plan, values, shared, extra)
    try:
        low, xors, D_ = job.low, job.xors, SS.SOURCE_DIGEST
        n = job.rows + 5
        assert len(xors) == 4 and len(low.seg_blocks) == 2 and low.sources[15] == D_ + 16  # segment 0, word 15 reads unit 0

        def with_unit(u, o, value):
            out = xors.copy()
            out[u, o] = value
            return {"xors": out}

        def with_source(at, value):
            out = low.sources.copy()
            out[at] = value
            return {"sources": out}

        cases = ((with_unit(2, 0, low.words_len), ("xor unit 2, operand x", f"word {low.words_len} of a buffer")),
                 (with_unit(3, 1, low.words_len + 5), ("xor unit 3, operand y", "of a buffer")),
                 (with_unit(0, 1, D_ + 8 * 2), ("xor unit 0, operand y", "segment 2 of 2")),          # a segment that does not exist
                 (with_unit(2, 0, D_ + 8 * 2 + 1), ("xor unit 2, operand x", "segment 2 of 2")),      # ... which a unit's result is
                 (with_unit(0, 0, D_ + 5), ("segment 0, word 15", "xor unit 0, operand x", "segment 0, which does not come before")),
                 (with_unit(1, 1, D_ + 8 + 2), ("segment 1, word 0", "xor unit 1, operand y", "segment 1, which does not come before")),
                 (with_source(16 + 3, D_ + 16 + 4), ("segment 1, word 3", "xor unit 4 of 4")),
                 ({"n_xors": 1}, ("segment 1, word 0", "xor unit 1 of 1")),
                 ({"n": job.rows - 1}, ("4 xor units", "does not fit the rows")),
                 ({"n": SS.rows_for(plan) - 1}, ("4 xor units", "does not fit the rows")),
                 ({"null_xors": True}, ("null xor table",)))
        for kw, names in cases:
            kw = dict(kw)
            assert job.launch(fresh[0], kw.pop("n", n), **kw) == ERR_ARG
            message = ctx.lib.cq_last_error(ctx.h).decode()
            assert all(name in message for name in names), message
        ctx.sync()
        fresh[0].assert_untouched()
        assert job.launch(fresh[1], job.rows) == 0  # the area fits exactly
        ctx.sync()
    finally:
        job.close()
