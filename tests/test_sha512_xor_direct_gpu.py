"""GPU, keyless: cq_sha512_synthesize_xors_dev called directly on bare columns (tests/sha512_direct.py) at n <= 2^13 with
table_bits 11 and 12.  Every comparison is against the XOR model over all 18 columns and all n rows, with the guard rows
behind untouched, and the units' result words behind the final states; a bad description is refused on the host before
anything is launched, which is what is asserted."""
import random

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from sha2_on_cq_halo2_amd import sha512_xor as SX
from sha2_on_cq_halo2_amd._lib import constants
from sha2_on_cq_halo2_amd.sha2_segments import Xor
from tests import sha512_direct as D
from tests import sha512_segments_model as SM
from tests import sha512_xor_model as XM

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
N = 1 << 13
P16 = (SS.PRIVATE,) * 16
ONES = (1 << 64) - 1
V384 = SC.VARIANT_384
Var, Const, DW = SS.Var, SS.Const, SS.DigestWord
EDGES = [(0, 0), (ONES, 0), (0x6A09E667F3BCC908, 0x6A09E667F3BCC908), (0x8000000000000001, 0x7FFFFFFFFFFFFFFE)]


class XorsJob:
    """A plan and one witness for it, lowered and uploaded: cq_sha512_synthesize_xors_dev.  `extra`: Xor units behind the
    plan's own that no word reads, their operands Vars or DigestWords of any segment."""

    def __init__(self, ctx, plan, values, shared=(), extra=()):
        self.ctx, self.plan = ctx, plan
        self.low = low = SX.lower(plan)
        first_var = low.words_len - sum(low.shared_counts)
        src = lambda o: first_var + o.index if isinstance(o, Var) else SS.SOURCE_DIGEST + 8 * o.segment + o.word
        rows = [list(r) for r in low.xors] + [[src(u.x), src(u.y), 0, 0] for u in extra]
        self.xors = np.array(rows, dtype=np.uint32).reshape(-1, SC.XOR_WORDS)
        self._words = ctx.to_device(SS.word_buffer(low, values, shared))
        self._digests = ctx.alloc(64 * len(low.seg_blocks) + 8 * max(len(self.xors), 1))
        self.rows = SX.rows_for(plan) + SC.XOR_REGIONS * SC.REGION_ROWS * len(extra)

    def launch(self, columns, n, table_bits=12, null_xors=False, **change):
        """The entry point alone -> its status; nothing here waits for the stream.  `change`: arguments to replace."""
        ctx, low = self.ctx, self.low
        a = dict(seg_blocks=low.seg_blocks, segments=len(low.seg_blocks), seg_variant=low.seg_variant, sources=low.sources,
                 init_sources=low.init_sources if SS.has_init(self.plan) else None, xors=self.xors, n_xors=len(self.xors), words_len=low.words_len)
        a.update(change)
        ptr = lambda x: None if x is None else x.ctypes.data
        return ctx.lib.cq_sha512_synthesize_xors_dev(ctx.h, table_bits, ptr(a["seg_blocks"]), a["segments"], ptr(a["seg_variant"]), ptr(a["sources"]),
                                                     ptr(a["init_sources"]), None if null_xors else ptr(a["xors"]), a["n_xors"], self._words.ptr,
                                                     a["words_len"], n, columns.arr, self._digests.ptr)

    def launch_segments(self, columns, n, table_bits=12):
        ctx, low = self.ctx, self.low
        return ctx.lib.cq_sha512_synthesize_segments_dev(ctx.h, table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks), low.seg_variant.ctypes.data,
                                                         low.sources.ctypes.data, low.init_sources.ctypes.data if SS.has_init(self.plan) else None,
                                                         self._words.ptr, low.words_len, n, columns.arr, self._digests.ptr)

    def states(self):
        """The final state of every segment as the device left it (waits for the stream)."""
        return [[int(x) for x in s] for s in self._digests.download((len(self.low.seg_blocks), 8), np.uint64)]

    def results(self):
        """Every unit's result word as the device left it behind the final states (waits for the stream)."""
        segments = len(self.low.seg_blocks)
        return [int(x) for x in self._digests.download(8 * segments + len(self.xors), np.uint64)[8 * segments:]]

    def close(self):
        self._words.close()
        self._digests.close()


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
        ctx._chk(job.launch(cols, n, table_bits))
        want, states, operands = XM.plan_witness(plan, values, shared, table_bits, n, extra)
        cols.assert_equals(want, n)
        assert job.states() == states
        assert job.results() == [x ^ y for x, y in operands] and len(operands) == len(job.xors)
        return want, states, operands
    finally:
        job.close()


@pytest.mark.parametrize("table_bits", [11, 12])
@pytest.mark.parametrize("x, y", EDGES)
def test_one_unit_of_two_buffer_words(ctx, fresh, x, y, table_bits):
    plan = SS.Plan((SS.Segment(1, P16[:7] + (Xor(Var(0), Var(1)),) + P16[8:]),), ((0, 8),))
    values = [[(0x0101010101010101 * i) & ONES for i in range(15)]]
    want, _, operands = check(ctx, fresh[0], plan, values, [x, y], SX.rows_for(plan) + 5, table_bits)
    assert operands == [(x, y)] and SX.rows_for(plan) == 1408 + 32
    assert want[XM.X][SM.message_row(0, 7)] == x ^ y == want[XM.X][XM.unit_rows(plan, 0)[1] + XM.ROW["W"]]


def test_one_unit_of_one_buffer_word_twice_and_of_a_constant(ctx, fresh):
    plan = SS.Plan((SS.Segment(1, (Xor(Var(0), Var(0)), Xor(Const(ONES), Var(0))) + P16[2:]),), ((0, 8),))
    _, _, operands = check(ctx, fresh[0], plan, [list(range(14))], [0xDEADBEEF00C0FFEE], SX.rows_for(plan) + 5)
    assert operands == [(0xDEADBEEF00C0FFEE, 0xDEADBEEF00C0FFEE), (ONES, 0xDEADBEEF00C0FFEE)]


def wired_case():
    """Unit 0 = Var 1 ^ Const (level 0), read by segment 0 (level 0, SHA-384) and segment 1; unit 1 = word 3 of segment 0's
    final state ^ Var 0 (level 1), read by two words of segment 1 (level 1), whose initial state is wired too.  Extra units
    that no word reads: one over buffer words, one over a word of segment 1's state -- the last level's, so the launch
    behind the chains."""
    a, b = Xor(DW(0, 3), Var(0)), Xor(Var(1), Const(XM.IPAD))
    plan = SS.Plan((SS.Segment(1, P16[:15] + (b,), None, V384),
                    SS.Segment(2, (a,) + P16[1:5] + (b,) + P16[6:16] + (a,) + SS.PAD_128_BYTES[1:], (Var(1),) + tuple(DW(0, i) for i in range(1, 8)))),
                   ((1, 8),))
    extra = (Xor(Var(0), Var(1)), Xor(DW(1, 7), DW(0, 0)))
    rng = random.Random(5)
    values = [[rng.getrandbits(64) for _ in range(15)], [rng.getrandbits(64) for _ in range(14)]]
    return plan, values, [0x0BADF00DDEADBEEF, 0xCAFEBABE8BADF00D], extra


@pytest.mark.parametrize("table_bits", [11, 12])
def test_digest_operands_shared_units_and_the_trailing_launch(ctx, fresh, table_bits):
    plan, values, shared, extra = wired_case()
    n = SX.rows_for(plan) + 64 + 5
    want, states, operands = check(ctx, fresh[0], plan, values, shared, n, table_bits, extra)
    assert operands == [(shared[1], XM.IPAD), (states[0][3], shared[0]), (shared[0], shared[1]), (states[1][7], states[0][0])]
    assert states[0] == SM.compress(values[0] + [shared[1] ^ XM.IPAD], 1, XM.M.IV[V384])[1][-1]
    readers = [SM.message_row(88, t) for t in (0, 16)]
    assert [want[XM.X][r] for r in readers] == [states[0][3] ^ shared[0]] * 2


def many_units_case():
    """65 units whose levels are 0, 1 and 2 in turn: Var ^ Var, a word of segment 0 ^ Var, a word of segment 1 ^ a word of
    segment 0 (segment 1 reads a level-1 unit, so it runs at level 1).  Segments 2 and 3 read 16 each -- whatever their
    level, so both run at level 2 -- and 33 are read by no word; the last of those reads segment 3's state: level 3."""
    def unit(t):
        return (Xor(Var(t % 8), Var(8 + t % 56)), Xor(DW(0, t % 8), Var(t % 64)), Xor(DW(1, t % 8), DW(0, (t // 8) % 8)))[t % 3]

    units = [unit(t) for t in range(64)] + [Xor(DW(3, 7), Var(63))]
    assert len(set(units)) == 65
    segs = (SS.Segment(1, P16[:15] + (Var(63),)), SS.Segment(1, (units[1],) + P16[1:], None, V384), SS.Segment(1, tuple(units[:16])),
            SS.Segment(1, tuple(units[16:32])))
    rng = random.Random(7)
    values = [[rng.getrandbits(64) for _ in range(15)], [rng.getrandbits(64) for _ in range(15)], [], []]
    return SS.Plan(segs, ((3, 8),)), values, [rng.getrandbits(64) for _ in range(64)], units


def test_65_units_of_mixed_levels(ctx, fresh):
    plan, values, shared, units = many_units_case()
    own = SX.xor_units(plan)
    assert own == [units[1]] + [u for u in units[:32] if u != units[1]] and XM.M2.levels(plan) == [0, 1, 2, 2]
    extra = units[32:]
    assert len(own) + len(extra) == 65 > 64 and SX.rows_for(plan) + 32 * len(extra) == 4 * 1408 + 65 * 32 == 7712 <= N - 5
    _, states, operands = check(ctx, fresh[0], plan, values, shared, N - 5, 12, extra)
    assert operands[-1] == (states[3][7], shared[63])


def test_no_units_is_the_segments_entry_point(ctx, fresh):
    rng = random.Random(23)
    plan = SS.Plan((SS.Segment(1, P16), SS.Segment(2, P16 + tuple(DW(0, i) for i in range(8)) + P16[8:], None, V384),
                    SS.Segment(1, P16, tuple(DW(1, i) for i in range(4)) + (SS.PRIVATE, Const(9), Var(0), Var(0)))), ((2, 8),))
    values = [[rng.getrandbits(64) for _ in range(n_)] for n_ in (16, 24, 17)]
    job = XorsJob(ctx, plan, values, [77])
    try:
        n = job.rows + 5
        assert SS.has_init(plan) and len(job.xors) == 0 and job.rows == SS.rows_for(plan)
        assert job.launch_segments(fresh[0], n) == 0
        want, states = fresh[0].download(), job.states()
        for null in (True, False):
            fresh[1].fill()
            assert job.launch(fresh[1], n, null_xors=null) == 0
            for i, (a, b) in enumerate(zip(want, fresh[1].download())):
                assert np.array_equal(a, b), f"advice column {i}"
            assert job.states() == states
        model, model_states, _ = XM.plan_witness(plan, values, [77], 12, n)
        fresh[0].assert_equals(model, n, got=want)
        assert states == model_states
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

        def with_init(at, value):
            out = low.init_sources.copy()
            out[at] = value
            return {"init_sources": out}

        u32 = lambda *xs: np.array(xs, dtype=np.uint32)
        cases = ((with_unit(2, 0, low.words_len), ("xor unit 2, operand x", f"word {low.words_len} of a buffer")),
                 (with_unit(3, 1, low.words_len + 5), ("xor unit 3, operand y", "of a buffer")),
                 (with_unit(0, 1, D_ + 8 * 2), ("xor unit 0, operand y", "segment 2 of 2")),          # a segment that does not exist
                 (with_unit(2, 0, D_ + 8 * 2 + 1), ("xor unit 2, operand x", "segment 2 of 2")),      # ... which a unit's result is
                 (with_unit(0, 0, D_ + 5), ("segment 0, word 15", "xor unit 0, operand x", "segment 0, which does not come before")),
                 (with_unit(1, 1, D_ + 8 + 2), ("segment 1, word 0", "xor unit 1, operand y", "segment 1, which does not come before")),
                 (with_source(16 + 3, D_ + 16 + 4), ("segment 1, word 3", "xor unit 4 of 4")),
                 ({"n_xors": 1}, ("segment 1, word 0", "xor unit 1 of 1")),
                 ({"n": job.rows - 1}, ("4 xor units", "does not fit the rows")),
                 ({"n": SX.rows_for(plan) - 1}, ("4 xor units", "does not fit the rows")),
                 ({"null_xors": True}, ("null xor table",)),
                 # the checks of cq_sha512_synthesize_segments_dev
                 ({"seg_blocks": None}, ("null array",)), ({"seg_variant": None}, ("null array",)), ({"sources": None}, ("null array",)),
                 ({"segments": 0}, ("no segment",)),
                 ({"seg_blocks": u32(1, 0)}, ("segment 1 has no block",)),
                 ({"seg_variant": u32(0, 2)}, ("segment 1 has variant 2",)),
                 ({"table_bits": SC.MIN_TABLE_BITS - 1}, ("table_bits",)), ({"table_bits": SC.MAX_TABLE_BITS + 1}, ("table_bits",)),
                 ({"n": SC.rows_for(1) + SC.rows_for(2) - 1}, ("segment 1", "do not fit the rows")),
                 (with_source(5, low.words_len), ("segment 0, word 5", "of a buffer")),
                 ({"words_len": low.words_len - 1}, ("of a buffer",)),
                 (with_source(16 + 20, D_ + 8), ("segment 1, word 20", "does not come before")),      # its own state
                 (with_source(3, D_ + 8 + 1), ("segment 0, word 3", "does not come before")),         # a later one's
                 (with_source(16 + 7, SS.SOURCE_IV), ("segment 1, word 7", "sentinel")),
                 (with_init(8 + 4, low.words_len), ("segment 1, initial word 4", "of a buffer")),
                 (with_init(8 + 1, D_ + 8 + 1), ("segment 1, initial word 1", "does not come before")),
                 (with_init(8 + 2, D_ + 16), ("segment 1, initial word 2", "does not come before")))  # a unit's result as an initial word
        for kw, names in cases:
            kw = dict(kw)
            assert job.launch(fresh[0], kw.pop("n", n), kw.pop("table_bits", 12), **kw) == ERR_ARG, names
            message = ctx.lib.cq_last_error(ctx.h).decode()
            assert all(name in message for name in names), message
        ctx.sync()
        fresh[0].assert_untouched()
        assert job.launch(fresh[1], job.rows) == 0  # the area fits exactly
        want, states, operands = XM.plan_witness(plan, values, shared, 12, job.rows, extra)
        fresh[1].assert_equals(want, job.rows)
        assert job.states() == states and job.results() == [x ^ y for x, y in operands]
    finally:
        job.close()
