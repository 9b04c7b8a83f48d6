"""The SHA-512 / SHA-384 witness-synthesis entry point called directly on bare device columns: no key, table or SRS, so any
row count and any table width the entry point takes can be reached.  The columns are those of tests/sha256_direct.py:
`GUARD` rows longer than the row count a call is given and prefilled with a pattern no synthesis writes.  A cell here may
exceed 64 bits (the spread form of a 64-bit word has 128), so the model's integers are encoded one by one where they do."""
import numpy as np

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from tests import sha256_direct as D
from tests.sha_oracle import mont_column  # noqa: F401

GUARD, PATTERN = D.GUARD, D.PATTERN


class Columns(D.Columns):
    def assert_equals(self, want, n: int, got=None):
        """Rows [0, n) of all 18 columns are the model's integers `want` (18 sequences of n) in Montgomery form, and every
        row from n on -- the guard rows and whatever of the allocation a smaller call leaves unused -- holds PATTERN."""
        assert len(want) == len(self.bufs) == SC.ADVICE_COLUMNS and n <= self.rows
        got = self.download() if got is None else got
        for i, (g, w) in enumerate(zip(got, want)):
            assert len(w) == n
            exp = mont_column(w)
            if not np.array_equal(g[:n], exp):
                row = int(np.nonzero((g[:n] != exp).any(axis=1))[0][0])
                raise AssertionError(f"advice column {i}, row {row} (region {row // SC.REGION_ROWS}, row {row % SC.REGION_ROWS} of it): "
                                     f"{g[row].tolist()}, the model has {int(w[row])}")
            assert (g[n:] == PATTERN).all(), f"advice column {i}: a row at or behind n = {n} was written"
        return got


def synthesize(ctx, cols, blocks_list, variants, message_words, n: int, table_bits: int = 12):
    """cq_sha512_synthesize_dev -> (status, the 8 words of every segment's final state)."""
    seg_blocks, seg_variant = np.array(blocks_list, dtype=np.uint32), np.array(variants, dtype=np.uint32)
    words = np.array(message_words, dtype=np.uint64)
    states = np.zeros(8 * len(seg_blocks), dtype=np.uint64)
    rc = ctx.lib.cq_sha512_synthesize_dev(ctx.h, table_bits, seg_blocks.ctypes.data, len(seg_blocks), seg_variant.ctypes.data,
                                          words.ctypes.data, n, cols.arr, states.ctypes.data)
    return rc, [[int(x) for x in states[8 * j: 8 * j + 8]] for j in range(len(seg_blocks))]
