"""Pure-Python model of SHA-256 segments that start from a given state (sha256_segments.Segment.init, the continued
sha256_varlen circuit): tests/sha2_model.py's compression and cells at 32 bits with the initial state as an argument, the
rows of a segment's initial words, and a plan-level witness that resolves every source, the initial words included, from the
model's own chaining values and writes a Choice's three cells to column Y.  The variable-length cells from a state and a
base length are sha256_varlen_model's.  hashlib is the reference the tests hold all of it to."""
from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from tests import sha2_model as M2
from tests import sha256_circuit_model as M
from tests import sha256_varlen_model as VM

W = M.W
M32 = M.M32
X, Y = 2 * SC.PAIRS, 2 * SC.PAIRS + 1
VAR = SC.VAR


def compress(words, blocks, init=None):
    """(per region (a, e, W, round or None, chained), the chaining values H_0 (`init`, or the IV) .. H_blocks)."""
    return M2.compress(W, words, blocks, M.IV if init is None else init)


def state_after(data: bytes, init=None):
    """The chaining value behind the whole 64-byte blocks of `data`."""
    assert len(data) % 64 == 0
    return compress(M2.words_of(data), len(data) // 64, init)[1][-1]


def cells_of(words, blocks, table_bits, init=None):
    """(18 columns over the segment's rows, the chaining values): the compression circuit's cells for any 16 * blocks words."""
    return M2.cells_of(W, words, blocks, table_bits, M.IV if init is None else init)


def state_row(first_region: int, word: int) -> int:
    """The row of initial word `word` in column X: region 3 - word % 4 of the first block, the A row or the E row."""
    return M2.state_row(W, first_region, word)


def plan_witness(plan, values, shared, bits, table_bits, n):
    """(18 advice columns of n integers, every segment's 8 digest words, every segment's 8 initial words) of a plan whose
    segments may have an `init`: Private words come from `values` (a segment's initial ones first), everything else is
    resolved from `shared`, `bits` and the model's own digests; a Choice's three cells go to column Y."""
    firsts = SS.first_regions(plan)
    cols, digests, inits, choices = M2.plan_witness(W, plan, firsts, lambda seg: M.IV, values, shared, bits, table_bits, n)
    for first, chosen in zip(firsts, choices):
        for t, zero, one, bit in chosen:
            base = SC.REGION_ROWS * M2.message_region(W, first, t)
            cols[Y][base + SC.CHOICE_ROW_ZERO], cols[Y][base + SC.CHOICE_ROW_ONE], cols[Y][base + SC.CHOICE_ROW_BIT] = zero, one, bit
    return cols, digests, inits


varlen_cells = VM.segment_cells  # (message, max_blocks, table_bits, init, base)
varlen_witness = VM.witness  # (messages, max_blocks_list, table_bits, n, inits, bases)
