"""GPU, keyless: cq_sha256_synthesize_states_dev and cq_sha256_synthesize_varlen_from_dev called directly on bare columns
(tests/sha256_direct.py).  The row count is 2^16 where a case has more than 64 segments -- 70 one-block segments alone take
40320 rows -- and the segments' rows + 5 elsewhere.  Every comparison is against the initial-state model over all 18 columns and all n
rows, with the guard rows behind untouched; digests are held to hashlib wherever a segment's words spell a message."""
import hashlib
import random
import struct

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd._lib import constants
from tests import sha256_direct as D
from tests import sha256_states_model as IM
from tests.sha2_model import words_of

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
N = 1 << 16
P16 = (SS.PRIVATE,) * 16


class StatesJob(D.SegmentsJob):
    """A plan with initial states and one witness for it: cq_sha256_synthesize_states_dev.  `init_sources`: None for the
    lowered plan's, "null" for a NULL pointer, else an array."""

    def launch(self, cols, n, table_bits=12, init_sources=None, sources=None):
        ctx, low = self.ctx, self.low
        init = low.init_sources if init_sources is None else init_sources
        sources = low.sources if sources is None else sources
        return ctx.lib.cq_sha256_synthesize_states_dev(ctx.h, table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks), sources.ctypes.data,
                                                       low.choices.ctypes.data if len(low.choices) else None, len(low.choices),
                                                       None if isinstance(init, str) else init.ctypes.data, self._words.ptr, low.words_len,
                                                       n, cols.arr, self._digests.ptr)


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


def levels_of(plan):
    out = []
    for seg in plan.segments:
        reads = [o.segment for s in tuple(seg.sources) + tuple(seg.init or ()) for o in ((s.zero, s.one) if isinstance(s, SS.Choice) else (s,))
                 if isinstance(o, SS.DigestWord)]
        out.append(1 + max((out[r] for r in reads), default=-1))
    return out


# ---- 4. one call of cq_sha256_synthesize_states_dev -------------------------------------------------------------------------

MESSAGE = bytes((11 * i + 5) % 256 for i in range(64 * 6 - 9))  # 6 blocks: the split message


def states_case(seed=17):
    """(plan, values, shared): 70 one-block segments in level 0 that alternate between the IV and Const / Private states, two
    of them with one Var initial word; segment 0 holds block 0 of MESSAGE, and three one-block segments (levels 1 .. 3) and
    one two-block segment (level 4) carry it on, each wired to the one before by its initial state alone."""
    rng = random.Random(seed)
    blocks = SC.pad(MESSAGE, 6)
    segs, values = [SS.Segment(1, P16)], [blocks[:16]]
    for j in range(1, 70):
        words = [rng.randrange(1 << 32) for _ in range(16)]
        if j % 2 == 0:
            segs.append(SS.Segment(1, P16))
            values.append(words)
        elif j % 4 == 1:
            state = tuple(SS.Const(rng.choice((0, 0xFFFFFFFF, 0x80000000, rng.randrange(1 << 32)))) for _ in range(8))
            segs.append(SS.Segment(1, P16, state[:5] + (SS.Var(0),) + state[6:] if j in (5, 9) else state))
            values.append(words)
        else:
            segs.append(SS.Segment(1, P16, (SS.PRIVATE,) * 8))
            values.append([rng.randrange(1 << 32) for _ in range(8)] + words)
    prev = 0
    for b in (1, 2, 3):
        segs.append(SS.Segment(1, P16, tuple(SS.DigestWord(prev, i) for i in range(8))))
        values.append(blocks[16 * b: 16 * b + 16])
        prev = len(segs) - 1
    segs.append(SS.Segment(2, P16 * 2, tuple(SS.DigestWord(prev, i) for i in range(8))))
    values.append(blocks[64:])
    return SS.Plan(tuple(segs), (len(segs) - 1,)), values, [0x9E3779B9]


def test_states_in_one_call(ctx, fresh):
    plan, values, shared = states_case()
    levels = levels_of(plan)
    assert levels[:70] == [0] * 70 and levels[70:] == [1, 2, 3, 4] and SS.rows_for(plan) <= N
    kinds = [None if s.init is None else type(s.init[0]) for s in plan.segments[:64]]
    assert {None, SS.Const, SS.Private} == set(kinds) and all((k is None) != (kinds[i + 1] is None) for i, k in enumerate(kinds[:-1]))
    job = StatesJob(ctx, plan, values, shared)
    try:
        assert len(job.low.choices) == 0 and (job.low.init_sources == SS.SOURCE_IV).sum() == 8 * 35
        job.run(fresh[0], N)
        want, digests, inits = IM.plan_witness(plan, values, shared, (), 12, N)
        fresh[0].assert_equals(want, N)
        got = job.digest_words()
        assert got == digests and inits[5][5] == inits[9][5] == shared[0]
        assert got[-1] == words_of(hashlib.sha256(MESSAGE).digest())
        assert got[0] == IM.state_after(struct.pack(">16I", *values[0]))
        # the two-block segment: the state regions of its first block are no chain regions -- their carry cells are zero
        first = SS.first_regions(plan)[-1]
        carries = [c for c in SC.layout() if c.kind in (SC.SRC["CARRY_A"], SC.SRC["CARRY_E"])]
        assert all(want[c.column][SC.REGION_ROWS * (first + g) + c.row] == 0 for c in carries for g in range(4))
    finally:
        job.close()


def choice_states_case(seed=19):
    """Two private segments; 66 one-block segments in level 1 whose message words 0 .. 7 are choices between a Var and a digest
    word and whose state is, in turn, the IV, the first segment's digest, and a mix of Var, Const and digest words; one
    segment in level 2 that starts from the digest of one of those."""
    rng = random.Random(seed)
    pad = (SS.Const(0x80000000),) + (SS.Const(0),) * 6 + (SS.Const(256),)
    segs = [SS.Segment(1, P16), SS.Segment(1, P16, tuple(SS.Const(v) for v in SS.IV224))]
    values = [SC.pad(bytes(rng.randrange(256) for _ in range(55)), 1), SC.pad(bytes(rng.randrange(256) for _ in range(31)), 1)]
    states = (None, tuple(SS.DigestWord(0, i) for i in range(8)),
              (SS.Var(0), SS.Const(5), SS.DigestWord(1, 7), SS.Var(31), SS.Const(0xFFFFFFFF), SS.DigestWord(0, 0), SS.Var(1), SS.Const(5)))
    for j in range(66):
        words = tuple(SS.Choice(j, SS.Var(8 * (j % 4) + t), SS.DigestWord(j % 2, (t + j) % 8)) for t in range(8))
        segs.append(SS.Segment(1, words + pad, states[j % 3]))
    segs.append(SS.Segment(1, tuple(SS.Choice(66, SS.DigestWord(66, t), SS.DigestWord(67, t)) for t in range(8)) + pad,
                           tuple(SS.DigestWord(65, i) for i in range(8))))
    values += [[]] * 67
    return SS.Plan(tuple(segs), (len(segs) - 1,)), values, [rng.randrange(1 << 32) for _ in range(32)], [j % 2 for j in range(66)] + [1]


def test_choices_and_states_in_one_wave(ctx, fresh):
    plan, values, shared, bits = choice_states_case()
    levels = levels_of(plan)
    assert levels.count(1) == 66 and levels[-1] == 2
    job = StatesJob(ctx, plan, values, shared, bits)
    try:
        assert len(job.low.choices) == 8 * 67 and SS.rows_for(plan) <= N
        job.run(fresh[0], N)
        want, digests, _ = IM.plan_witness(plan, values, shared, bits, 12, N)
        fresh[0].assert_equals(want, N)
        assert job.digest_words() == digests
        assert struct.pack(">8I", *digests[1])[:28] == hashlib.sha224(bytes(struct.pack(">16I", *values[1])[:31])).digest()
    finally:
        job.close()


# ---- 5. the old entry points ---------------------------------------------------------------------------------------------------

def test_null_and_all_sentinel_states_are_the_segments_entry_point(ctx, fresh):
    rng = random.Random(23)
    plan = SS.Plan(tuple(SS.Segment(1 + j % 2, P16 * (1 + j % 2)) for j in range(5)) +
                   (SS.Segment(1, tuple(SS.DigestWord(4, i) for i in range(8)) + (SS.Const(0x80000000),) + (SS.Const(0),) * 6 + (SS.Const(256),)),), (5,))
    values = [[rng.randrange(1 << 32) for _ in range(16 * s.blocks)] for s in plan.segments[:5]] + [[]]
    old, new = D.SegmentsJob(ctx, plan, values), StatesJob(ctx, plan, values)
    try:
        assert (new.low.init_sources == SS.SOURCE_IV).all()
        n = old.rows + 5
        old.run(fresh[0], n)
        want = fresh[0].download()
        for init in ("null", None):
            fresh[1].fill()
            assert new.launch(fresh[1], n, init_sources=init) == 0
            for i, (a, b) in enumerate(zip(want, fresh[1].download())):
                assert np.array_equal(a, b), f"advice column {i}"
            assert new.digest_words() == old.digest_words()
        model, digests, _ = IM.plan_witness(plan, values, (), (), 12, n)
        fresh[0].assert_equals(model, n, got=want)
    finally:
        old.close()
        new.close()


# ---- 6. cq_sha256_synthesize_varlen_from_dev ---------------------------------------------------------------------------------

class VarlenFromJob(D.VarlenJob):
    def __init__(self, ctx, max_blocks_list, data, offsets, lens, states, bases):
        super().__init__(ctx, max_blocks_list, data, offsets, lens)
        self._states = ctx.to_device(np.array(states, dtype=np.uint32))
        self.bases = np.array(bases, dtype=np.uint64)

    def launch(self, cols, n, table_bits=12):
        ctx = self.ctx
        return ctx.lib.cq_sha256_synthesize_varlen_from_dev(ctx.h, table_bits, self.seg_blocks.ctypes.data, len(self.seg_blocks), self._bytes.ptr,
                                                            self.bytes_len, self.offsets.ctypes.data, self.lens.ctypes.data, self._states.ptr,
                                                            self.bases.ctypes.data, n, cols.arr, self._digests.ptr)

    def close(self):
        super().close()
        self._states.close()


PREFIX = bytes((13 * i + 1) % 256 for i in range(64 * 3))
LENGTHS = (0, 1, 55, 56, 63, 119, 183)


def continued_case():
    """One segment per (max_blocks, tail length, base) of the issue's grid that fits: 66 segments, tails packed back to back.
    A base of 64 or 192 is PREFIX's own length, so prefix || tail is a message hashlib knows; at 2^29 - 64 * max_blocks the
    state is any state and the model alone is the reference."""
    shape = [(mb, length, base) for mb in (1, 3) for length in LENGTHS if length <= 64 * mb - 9
             for base in (64, 192, (1 << 29) - 64 * mb)]
    shape += [(1, length, 64) for length in range(2, 66 - len(shape) + 2)]
    data, offsets, states, messages = b"", [], [], []
    for j, (mb, length, base) in enumerate(shape):
        tail = bytes((j + 3 * i) % 256 for i in range(length))
        offsets.append(len(data))
        data += tail
        messages.append(tail)
        states.append(IM.state_after(PREFIX[:base]) if base <= len(PREFIX) else [(0x01010101 * (j + 1) + i) & 0xFFFFFFFF for i in range(8)])
    return shape, messages, data, offsets, states


def test_continued_varlen_66_segments(ctx, fresh):
    shape, messages, data, offsets, states = continued_case()
    blocks, bases = [mb for mb, _, _ in shape], [base for _, _, base in shape]
    assert len(shape) == 66 and {(mb, ln) for mb, ln, _ in shape} >= {(1, 0), (1, 1), (1, 55), (3, 56), (3, 63), (3, 119), (3, 183)}
    assert sum(SC.rows_for(b) for b in blocks) <= N and any(8 * (b + len(m)) >> 31 for b, m in zip(bases, messages))
    job = VarlenFromJob(ctx, blocks, data, offsets, [len(m) for m in messages], states, bases)
    try:
        job.run(fresh[0], N)
        want, digests = IM.varlen_witness(messages, blocks, 12, N, states, bases)
        fresh[0].assert_equals(want, N)
        got = job.digest_words()
        assert got == digests
        for (mb, length, base), m, d in zip(shape, messages, got):
            if base <= len(PREFIX):
                assert d == words_of(hashlib.sha256(PREFIX[:base] + m).digest())
    finally:
        job.close()


def test_all_iv_states_and_no_base_are_the_varlen_entry_point(ctx, fresh):
    messages = [b"\x80" * 57, b"", bytes(range(183))]
    data = b"".join(messages)
    args = ([2, 1, 3], data, [0, 57, 57], [57, 0, 183])
    old, new = D.VarlenJob(ctx, *args), VarlenFromJob(ctx, *args, [SC.IV256] * 3, [0] * 3)
    try:
        n = old.rows + 5
        old.run(fresh[0], n)
        new.run(fresh[1], n)
        for i, (a, b) in enumerate(zip(fresh[0].download(), fresh[1].download())):
            assert np.array_equal(a, b), f"advice column {i}"
        assert new.digest_words() == old.digest_words() == [words_of(hashlib.sha256(m).digest()) for m in messages]
    finally:
        old.close()
        new.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(ctx, fresh):
    plan, values, shared, bits = choice_states_case()
    job = StatesJob(ctx, plan, values, shared, bits)
    var = VarlenFromJob(ctx, [1, 3], b"abc", [0, 0], [3, 3], [SC.IV256] * 2, [64, 64])
    try:
        low = job.low

        def with_init(at, value):
            init = low.init_sources.copy()
            init[at] = value
            return init

        for init, names in ((with_init(8 * 5 + 2, SS.SOURCE_DIGEST + 8 * 5 + 1), ("segment 5, initial word 2", "does not come before")),
                            (with_init(8 * 5 + 2, SS.SOURCE_DIGEST + 8 * 40), ("segment 5, initial word 2", "segment 40")),
                            (with_init(8 * 67 + 7, low.words_len), ("segment 67, initial word 7", f"word {low.words_len} of a buffer")),
                            (with_init(8 * 3, SS.SOURCE_CHOICE + 1), ("segment 3, initial word 0", "choice"))):
            assert job.launch(fresh[0], N, init_sources=init) == ERR_ARG
            message = ctx.lib.cq_last_error(ctx.h).decode()
            assert all(name in message for name in names), message
        for bases, names in (([64, 32], ("segment 1", "multiple of 64")), ([(1 << 29) - 64 + 64, 64], ("segment 0", "2^29")),
                             ([64, (1 << 29) - 192 + 64], ("segment 1", "2^29"))):
            var.bases = np.array(bases, dtype=np.uint64)
            assert var.launch(fresh[0], N) == ERR_ARG
            message = ctx.lib.cq_last_error(ctx.h).decode()
            assert all(name in message for name in names), message
        var.bases = np.array([(1 << 29) - 64, (1 << 29) - 192], dtype=np.uint64)  # the bound itself is inside
        assert var.launch(fresh[1], N) == 0
        ctx.sync()
        fresh[0].assert_untouched()
    finally:
        job.close()
        var.close()
