"""GPU: SHA-256 witness synthesis past one workgroup -- the four entry points called directly on bare columns (no key), so
that the chain kernel runs more than one workgroup, more than three levels and a level order that is not the row order,
the padding and fill kernels run several workgroups whose blocks straddle segments, two syntheses are queued back to
back, and the table width is not 12.  Every comparison is against the pure-Python models, cell for cell over all 18
columns and all n rows, with n = rows + 5 (no multiple of 8 or 256: the rows behind the last region come back zero) and
the guard rows behind n untouched; every digest the device returns is compared with hashlib's."""
import hashlib
import random

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd._lib import constants
from tests import sha256_choice_model as CM
from tests import sha256_circuit_model as M
from tests import sha256_direct as D
from tests import sha256_segments_model as SM
from tests import sha256_varlen_model as VM
from tests.sha2_model import words_of

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
PAD_32_BYTES = (SS.Const(0x80000000),) + (SS.Const(0),) * 6 + (SS.Const(256),)  # behind 8 words: sha256_segments.double_sha256


def edgy_bytes(rng, length):
    """Bytes among which 0x00, 0x80 and 0xff are common: a pad byte in the wrong place next to them would show."""
    return bytes(rng.choice((0x00, 0x80, 0xFF)) if rng.random() < 0.5 else rng.randrange(256) for _ in range(length))


# ---- a. variable length: 72 segments, 96 blocks -------------------------------------------------------------------------

def varlen_case(seed=3):  # a seed whose bytes reach every carry value (test_varlen_72_segments_in_one_call asserts it)
    """(max_blocks per segment, messages, data, offsets): one-block segments of every length 0 .. 55, two-block segments at
    the lengths around the spill into the second block, three-block segments around the third -- and 0, 55 and 64, which
    leave blocks behind the final one -- in a fixed shuffled order.  The messages are packed back to back, so at unaligned
    offsets, in another order; the three-block message of 55 bytes is the one-block one's bytes (one offset, two
    segments), and one empty message sits at the very end of the buffer."""
    rng = random.Random(seed)
    shape = [(1, length) for length in range(56)] + [(2, length) for length in (56, 57, 59, 60, 63, 64, 65, 119)]
    shape += [(3, length) for length in (120, 121, 127, 128, 183, 0, 55, 64)]
    rng.shuffle(shape)
    shared_by, shares = shape.index((3, 55)), shape.index((1, 55))
    packing = [j for j in range(len(shape)) if j != shared_by]
    rng.shuffle(packing)
    packing.remove(shape.index((1, 0)))
    packing.append(shape.index((1, 0)))  # the empty message of the one-block segment: offset == len(data)
    data, offsets = b"", [None] * len(shape)
    for j in packing:
        offsets[j] = len(data)
        data += edgy_bytes(rng, shape[j][1])
    offsets[shared_by] = offsets[shares]
    messages = [data[o: o + length] for o, (_, length) in zip(offsets, shape)]
    assert offsets[shape.index((1, 0))] == len(data) and any(o % 4 for o in offsets) and offsets != sorted(offsets)
    return [b for b, _ in shape], messages, data, offsets


class Varlen:
    """The case, its job on the device and -- computed once, never changed -- the model's witness at n = rows + 5."""

    def __init__(self, ctx):
        self.max_blocks, self.messages, data, offsets = varlen_case()
        self.job = D.VarlenJob(ctx, self.max_blocks, data, offsets, [len(m) for m in self.messages])
        self.n = self.job.rows + 5
        self.want, self.digests = VM.witness(self.messages, self.max_blocks, 12, self.n)

    def check(self, cols):
        cols.assert_equals(self.want, self.n)
        got = self.job.digest_words()
        assert got == self.digests and got == [words_of(hashlib.sha256(m).digest()) for m in self.messages]


@pytest.fixture(scope="module")
def varlen(ctx):
    v = Varlen(ctx)
    yield v
    v.job.close()


@pytest.fixture(scope="module")
def columns(ctx):
    """Two column sets of the largest case's rows, refilled with the pattern before every test that takes them."""
    rows = max(sum(SC.rows_for(b) for b in varlen_case()[0]), SS.rows_for(wired_case()[0]), SS.rows_for(choice_case()[0])) + 5
    sets = [D.Columns(ctx, rows) for _ in range(2)]
    yield sets
    for s in sets:
        s.close()


@pytest.fixture
def fresh(columns):
    for s in columns:
        s.fill()
    return columns


def carries(want, name):
    """The values the model's columns hold in the cell of carry `name`, over all regions."""
    cell = next(c for c in SC.layout() if c.kind == SC.SRC[name])
    return set(want[cell.column][cell.row:: SC.REGION_ROWS])


def test_varlen_72_segments_in_one_call(varlen, fresh):
    v = varlen
    assert len(v.max_blocks) == 72 and sum(v.max_blocks) == 96 and v.n == 54528 + 5 and v.n % 8 and v.n % 256
    # 6 workgroups of the padding kernel, 12 of the fill kernel, 2 of the chain kernel; neighbours in a wave differ in blocks
    assert (16 * 96 + 255) // 256 == 6 and (32 * 96 + 255) // 256 == 12 and (72 + 63) // 64 == 2
    first_block = np.cumsum([0] + v.max_blocks[:-1])
    assert set(v.max_blocks[:64]) == {1, 2, 3} and any(f % 8 + b > 8 for f, b in zip(first_block, v.max_blocks))  # a fill workgroup over two segments
    assert all(x in b"".join(v.messages) for x in (0x00, 0x80, 0xFF))
    # the inputs reach every carry the layout holds: a later change of inputs that loses an edge shows here
    assert carries(v.want, "CARRY_A") == set(range(7)) and carries(v.want, "CARRY_E") == set(range(6))
    assert carries(v.want, "CARRY_W") == set(range(4))
    v.job.run(fresh[0], v.n)
    v.check(fresh[0])


# ---- b. wired segments: 68 lanes in level 0, 7 levels, level order != row order -------------------------------------------

def wired_case(seed=5):
    """(plan, values): 68 private one-block segments (level 0) in row order, and between them a chain of one-block segments
    that each hash the digest of an earlier segment (levels 1 .. 5), a second level-1 segment, and two two-block segments
    that hash two digests: one of two private segments (level 1; its right operand is level 0's lane 65), one of the
    chain's end and lane 66 (level 6).  The level order is far from the row order."""
    rng = random.Random(seed)
    segs, values, private = [], [], []  # private: segment index of private message i

    def hash_of(*earlier):
        words = tuple(SS.DigestWord(s, w) for s in earlier for w in range(8))
        segs.append(SS.Segment(len(earlier), words + (PAD_32_BYTES if len(earlier) == 1 else SS.PAD_64_BYTES)))
        values.append([])
        return len(segs) - 1

    chain = None
    for i in range(68):
        private.append(len(segs))
        segs.append(SS.Segment(1, (SS.PRIVATE,) * 16))
        values.append(SC.pad(edgy_bytes(rng, rng.randrange(56)), 1))
        if i == 3:
            chain = hash_of(private[1])
        elif i in (10, 20, 30, 40):
            chain = hash_of(chain)
        elif i == 50:
            hash_of(private[45])
        elif i == 65:
            hash_of(private[2], private[65])
        elif i == 66:
            top = hash_of(chain, private[66])
    return SS.Plan(tuple(segs), (top,)), values


def levels_of(plan):
    """Every segment's dependency level, as the entry point derives it: one more than the highest level it reads."""
    out = []
    for seg in plan.segments:
        reads = [o.segment for s in seg.sources for o in ((s.zero, s.one) if isinstance(s, SS.Choice) else (s,)) if isinstance(o, SS.DigestWord)]
        out.append(1 + max((out[r] for r in reads), default=-1))
    return out


def test_wired_segments_levels_against_row_order(ctx, fresh):
    plan, values = wired_case()
    levels = levels_of(plan)
    assert levels.count(0) == 68 and max(levels) == 6 and levels.count(1) == 3 and levels != sorted(levels)
    assert {plan.segments[j].blocks for j in range(len(levels)) if levels[j] == 1} == {1, 2}  # a wave whose lanes differ in blocks
    job = D.SegmentsJob(ctx, plan, values)
    try:
        assert len(job.low.choices) == 0
        n = job.rows + 5
        job.run(fresh[0], n)
        fresh[0].assert_equals(SM.witness(plan, values, 12, n), n)
        got = job.digest_words()
        assert got == SM.digests(plan, values)
        assert got == [words_of(hashlib.sha256(m).digest()) for m in SM.messages(plan, values)]
    finally:
        job.close()


# ---- c. choices: 66 choice-reading lanes in one level ---------------------------------------------------------------------

def choice_case(seed=7):
    """(plan, values, shared, bits): two private segments, then 66 one-block segments that hash 8 chosen words -- word t of
    segment j is Choice(bit j, x, y) with one operand a Var and the other a digest word of a private segment, which is
    which alternating with t -- all in level 1, with bits that alternate from lane to lane; and one segment in level 2
    whose operands are digest words of two of those."""
    rng = random.Random(seed)
    segs = [SS.Segment(1, (SS.PRIVATE,) * 16)] * 2
    values = [SC.pad(edgy_bytes(rng, 55), 1), SC.pad(edgy_bytes(rng, 31), 1)]
    for j in range(66):
        pairs = [(SS.Var(8 * (j % 4) + t), SS.DigestWord(j // 2 % 2, (t + j) % 8)) for t in range(8)]
        segs.append(SS.Segment(1, tuple(SS.Choice(j, *(p if t % 2 else p[::-1])) for t, p in enumerate(pairs)) + PAD_32_BYTES))
    segs.append(SS.Segment(1, tuple(SS.Choice(66, SS.DigestWord(2 + 64, t), SS.DigestWord(2 + 65, t)) for t in range(8)) + PAD_32_BYTES))
    values += [[]] * 67
    shared = [rng.choice((0, 0x80000000, 0xFFFFFFFF, rng.randrange(1 << 32))) for _ in range(32)]
    bits = [j % 2 for j in range(66)] + [1]
    return SS.Plan(tuple(segs), (len(segs) - 1,)), values, shared, bits


def test_choices_66_lanes_in_one_level(ctx, fresh):
    plan, values, shared, bits = choice_case()
    levels = levels_of(plan)
    assert levels.count(1) == 66 and levels[-1] == 2 and all(bits[j] != bits[j + 1] for j in range(65))
    job = D.SegmentsJob(ctx, plan, values, shared, bits)
    try:
        assert len(job.low.choices) == 8 * 67
        n = job.rows + 5
        job.run(fresh[0], n)
        want = CM.witness(plan, values, shared, bits, 12, n)
        y = want[2 * SC.PAIRS + 1]
        assert any(y[r] for r in range(SC.CHOICE_ROW_ZERO, n, SC.REGION_ROWS)) and any(y[r] for r in range(SC.CHOICE_ROW_BIT, n, SC.REGION_ROWS))
        fresh[0].assert_equals(want, n)
        got = job.digest_words()
        plain, plain_values, _ = CM.resolve(plan, values, shared, bits)
        assert got == CM.digests(plan, values, shared, bits)
        assert got == [words_of(hashlib.sha256(m).digest()) for m in SM.messages(plain, plain_values)]
    finally:
        job.close()


# ---- d. the host chain against the model and the device chain ---------------------------------------------------------------

def test_host_chain_of_five_blocks_is_the_device_chain(ctx, fresh):
    msg = edgy_bytes(random.Random(11), 64 * 5 - 9)
    words, n = SC.pad(msg, 5), SC.rows_for(5) + 5
    rc, digest = D.synthesize(ctx, fresh[0], words, 5, n)
    assert rc == 0 and digest == words_of(hashlib.sha256(msg).digest())
    want, model_digest = M.witness(msg, 5, 12, n)
    assert model_digest == digest
    host = fresh[0].assert_equals(want, n)
    job = D.SegmentsJob(ctx, SS.batch([5]), [words])
    try:
        job.run(fresh[1], n)
        for i, (a, b) in enumerate(zip(host, fresh[1].download())):
            assert np.array_equal(a, b), f"advice column {i}"
        assert job.digest_words() == [digest]
    finally:
        job.close()


# ---- e. two syntheses queued back to back ---------------------------------------------------------------------------------

def test_back_to_back_calls_share_the_staging(ctx, varlen, fresh):
    """Nothing between two launches waits for the stream: the second call fills the pinned staging buffer and the two
    scratch entries the first one's copy and kernels still read, behind the event that guards the staging."""
    a, b = fresh
    small_messages = [b"\x80" * 57, b""]
    data = b"\xff" + small_messages[0]
    small = D.VarlenJob(ctx, [2, 1], data, [1, len(data)], [57, 0])
    five = SC.pad(edgy_bytes(random.Random(13), 64 * 5 - 9), 5)
    wired = D.SegmentsJob(ctx, SS.batch([5]), [five])
    try:
        small_n, wired_n = small.rows + 5, wired.rows + 5
        small_want, small_digests = VM.witness(small_messages, [2, 1], 12, small_n)
        wired_want = SM.witness(SS.batch([5]), [five], 12, wired_n)
        ctx.sync()
        # the large variable-length call, then a small one
        assert varlen.job.launch(a, varlen.n) == 0 and small.launch(b, small_n) == 0
        ctx.sync()
        varlen.check(a)
        b.assert_equals(small_want, small_n)
        assert small.digest_words() == small_digests == [words_of(hashlib.sha256(m).digest()) for m in small_messages]
        # a segments call, then the large variable-length call into the set that holds the small result
        a.fill()
        assert wired.launch(a, wired_n) == 0 and varlen.job.launch(b, varlen.n) == 0
        ctx.sync()
        a.assert_equals(wired_want, wired_n)
        assert wired.digest_words() == SM.digests(SS.batch([5]), [five])
        varlen.check(b)
    finally:
        small.close()
        wired.close()


# ---- f. refusals at these shapes -------------------------------------------------------------------------------------------

def test_refusals_with_72_segments_write_nothing(ctx, varlen, fresh):
    job = varlen.job
    lens = job.lens.copy()
    try:
        job.lens = lens.copy()
        job.lens[70] = 64 * varlen.max_blocks[70] - 8  # one byte more than the segment's blocks hold
        assert job.launch(fresh[0], varlen.n) == ERR_ARG
        assert "segment 70:" in ctx.lib.cq_last_error(ctx.h).decode()
        job.lens = lens
        # one region short: the last segment is the first that does not fit
        assert job.launch(fresh[0], varlen.n - SC.REGION_ROWS) == ERR_ARG
        assert "up to segment 71 " in ctx.lib.cq_last_error(ctx.h).decode()
        # short by the last segment's regions and one more: the one before it
        short = SC.rows_for(varlen.max_blocks[71]) + SC.REGION_ROWS
        assert job.launch(fresh[0], varlen.n - short) == ERR_ARG
        assert "up to segment 70 " in ctx.lib.cq_last_error(ctx.h).decode()
        ctx.sync()
        fresh[0].assert_untouched()
    finally:
        job.lens = lens


# ---- table width -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table_bits", [11, 13, 16])
def test_host_chain_at_other_table_widths(ctx, fresh, table_bits):
    """Chunk c of an even / odd word starts at bit c * table_bits: at 11 the top chunk has 10 bits, at 16 it starts at bit 32
    and is zero."""
    msg = edgy_bytes(random.Random(table_bits), 119)
    n = SC.rows_for(2) + 5
    rc, digest = D.synthesize(ctx, fresh[0], SC.pad(msg, 2), 2, n, table_bits)
    assert rc == 0 and digest == words_of(hashlib.sha256(msg).digest())
    want, _ = M.witness(msg, 2, table_bits, n)
    top = [c for c in SC.layout() if c.per_table_bits == 2]
    assert len(top) == 14 and any(want[c.column][r] for c in top for r in range(c.row, n, SC.REGION_ROWS)) == (table_bits != 16)
    fresh[0].assert_equals(want, n)


@pytest.mark.parametrize("table_bits", [13, 16])
def test_varlen_at_other_table_widths(ctx, fresh, table_bits):
    rng = random.Random(table_bits)
    messages = [edgy_bytes(rng, 57), b"", edgy_bytes(rng, 55)]
    data = b"\x00" + messages[0] + messages[2]
    job = D.VarlenJob(ctx, [2, 1, 1], data, [1, len(data), 58], [57, 0, 55])
    try:
        n = job.rows + 5
        job.run(fresh[0], n, table_bits)
        want, digests = VM.witness(messages, [2, 1, 1], table_bits, n)
        fresh[0].assert_equals(want, n)
        assert job.digest_words() == digests == [words_of(hashlib.sha256(m).digest()) for m in messages]
    finally:
        job.close()


@pytest.mark.parametrize("table_bits", [10, 17])
def test_a_table_width_outside_the_range_is_refused(ctx, fresh, table_bits):
    words = SC.pad(b"abc", 1)
    n = SC.rows_for(1) + 5
    wired = D.SegmentsJob(ctx, SS.batch([1]), [words])
    plan, values, shared, bits = choice_case()
    chosen = D.SegmentsJob(ctx, plan, values, shared, bits)
    var = D.VarlenJob(ctx, [1], b"abc", [0], [3])
    try:
        calls = (lambda: D.synthesize(ctx, fresh[0], words, 1, n, table_bits)[0], lambda: wired.launch(fresh[0], n, table_bits),
                 lambda: chosen.launch(fresh[0], chosen.rows + 5, table_bits), lambda: var.launch(fresh[0], n, table_bits))
        for call in calls:
            assert call() == ERR_ARG
            assert "table_bits" in ctx.lib.cq_last_error(ctx.h).decode()
        ctx.sync()
        fresh[0].assert_untouched()
    finally:
        for job in (wired, chosen, var):
            job.close()
