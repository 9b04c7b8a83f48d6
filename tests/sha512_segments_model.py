"""Pure-Python model of wired SHA-512 segments (sha512_segments.Plan): tests/sha2_model.py's compression and cells at 64
bits for any 16 * blocks words and any initial state, the rows of a segment's wired cells, and a plan-level witness that
resolves every source, the initial words included, from the model's own final states, level by level.  The SHA-512/256
initial hash value is generated there as FIPS 180-4, 5.3.6 says.  hashlib is the reference the tests hold all of it to."""
import struct

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd import sha512_segments as SS
from tests import sha2_model as M2
from tests import sha512_circuit_model as M
from tests.sha2_model import levels  # noqa: F401

W = M.W
M64 = M.M64
X = 2 * SC.PAIRS
IV512_256 = W.iv["sha512/256"]


def layout():
    return [c for c, _ in M2.layout(W)]


def compress(words, blocks, init):
    """(per region (a, e, W, round or None, chained), the chaining values H_0 = `init` .. H_blocks)."""
    return M2.compress(W, words, blocks, init)


def cells_of(words, blocks, table_bits, init):
    """(18 columns over the segment's rows, the chaining values): the compression circuit's cells for any 16 * blocks
    words from any state."""
    return M2.cells_of(W, words, blocks, table_bits, init)


def state_row(first_region: int, word: int) -> int:
    """The row of initial word `word` in column X: region 3 - word % 4 of the first block, the A row or the E row."""
    return M2.state_row(W, first_region, word)


def tail_row(first_region: int, blocks: int, word: int) -> int:
    """The row of word `word` of the final state in column X."""
    return state_row(first_region + SC.BLOCK_REGIONS * blocks, word)


def message_row(first_region: int, t: int) -> int:
    """The row of message word t's W cell in column X."""
    return SC.REGION_ROWS * M2.message_region(W, first_region, t) + M2.word_row(W, "W")


P16 = (SS.PRIVATE,) * 16


def mixed_plan():
    """Every kind of wired cell in two one-block segments and one of two blocks: Const, DigestWord and Var message words,
    a Var that stands three times, a digest-wired, a Var, a Const and a Private initial word, a SHA-384 segment."""
    seg0 = SS.Segment(1, (SS.Var(1), SS.Const(5)) + P16[2:])
    seg1 = SS.Segment(1, P16, None, SC.VARIANT_384)
    init = (SS.DigestWord(0, 7), SS.DigestWord(1, 6), SS.Var(0), SS.Const(1 << 63), SS.PRIVATE, SS.DigestWord(1, 0), SS.Var(1), SS.Const(5))
    seg2 = SS.Segment(2, (SS.DigestWord(1, 7), SS.Var(1), SS.Const((1 << 64) - 1)) + P16[3:] + P16[:15] + (SS.DigestWord(0, 3),), init)
    return SS.Plan((seg0, seg1, seg2), ((2, 5), (1, 6), (0, 1)), (2,))


def plan_witness(plan, values, shared, table_bits, n):
    """(18 advice columns of n integers, every segment's 8 final words, every segment's 8 initial words, the instance
    words): Private words come from `values` (a segment's initial ones first), everything else is resolved from `shared`
    and the model's own final states.  The segments are evaluated level by level, as the device runs them."""
    cols, states, inits, _ = M2.plan_witness(W, plan, SS.first_regions(plan), lambda seg: M.IV[seg.variant], values, shared, (), table_bits, n)
    instance = [x for s, words in plan.public for x in states[s][:words]] + [x for q in plan.public_init for x in inits[q]]
    return cols, states, inits, instance


def digest_bytes(state, words=8):
    return struct.pack(f">{words}Q", *state[:words])
