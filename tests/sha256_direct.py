"""The four SHA-256 witness-synthesis entry points called directly on bare device columns: no key, table or SRS, so any
row count and any table width the entry points take can be reached.  The columns are `GUARD` rows longer than the row
count a call is given and prefilled with a pattern no synthesis writes; a comparison against a model's integer columns
covers every row of every column and then the rows behind, which must still hold the pattern.

Uploads, downloads and allocations wait for the stream; a job's `launch` does not, so two launches with nothing between
them are queued back to back."""
import ctypes as C

import numpy as np

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS

GUARD = 16
# every limb 0xA5..A5: above the field's modulus, so the Montgomery form of nothing -- and not zero
PATTERN = np.full(4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)


class Columns:
    """18 device columns of `rows + GUARD` field elements, prefilled with PATTERN."""

    def __init__(self, ctx, rows: int):
        self.ctx, self.rows = ctx, rows
        self.bufs = [ctx.alloc(32 * (rows + GUARD)) for _ in range(SC.ADVICE_COLUMNS)]
        self.arr = (C.c_void_p * SC.ADVICE_COLUMNS)(*[b.ptr for b in self.bufs])
        self.fill()

    def fill(self):
        pattern = np.tile(PATTERN, (self.rows + GUARD, 1))
        for b in self.bufs:
            b.upload(pattern)

    def download(self):
        """uint64[rows + GUARD, 4] per column (waits for the stream)."""
        return [b.download((self.rows + GUARD, 4)) for b in self.bufs]

    def assert_equals(self, want, n: int, got=None):
        """Rows [0, n) of all 18 columns are the model's integers `want` (18 sequences of n) in Montgomery form, and every
        row from n on -- the guard rows and whatever of the allocation a smaller call leaves unused -- holds PATTERN."""
        assert len(want) == len(self.bufs) == SC.ADVICE_COLUMNS and n <= self.rows
        got = self.download() if got is None else got
        for i, (g, w) in enumerate(zip(got, want)):
            assert len(w) == n
            exp = SC._mont_column(np.array(w, dtype=np.uint64))
            if not np.array_equal(g[:n], exp):
                row = int(np.nonzero((g[:n] != exp).any(axis=1))[0][0])
                raise AssertionError(f"advice column {i}, row {row} (region {row // SC.REGION_ROWS}, row {row % SC.REGION_ROWS} of it): "
                                     f"{g[row].tolist()}, the model has {int(w[row])}")
            assert (g[n:] == PATTERN).all(), f"advice column {i}: a row at or behind n = {n} was written"
        return got

    def assert_untouched(self):
        for i, g in enumerate(self.download()):
            assert (g == PATTERN).all(), f"advice column {i} was written"

    def close(self):
        for b in self.bufs:
            b.close()


def synthesize(ctx, cols: Columns, message_words, blocks: int, n: int, table_bits: int = 12):
    """cq_sha256_synthesize_dev (the chain on the host) -> (status, the 8 digest words)."""
    words = np.array(message_words, dtype=np.uint32)
    digest = (C.c_uint32 * 8)()
    rc = ctx.lib.cq_sha256_synthesize_dev(ctx.h, table_bits, words.ctypes.data, blocks, n, cols.arr, digest)
    return rc, [int(x) for x in digest]


class _Job:
    def run(self, cols: Columns, n: int, table_bits: int = 12):
        self.ctx._chk(self.launch(cols, n, table_bits))

    def digest_words(self):
        """The digest words of every segment as the device left them (waits for the stream)."""
        return self._digests.download((len(self.seg_blocks), 8), np.uint32).tolist()


class SegmentsJob(_Job):
    """A plan and one witness for it, lowered and uploaded: cq_sha256_synthesize_segments_dev, or _choices_dev for a plan
    with a Choice."""

    def __init__(self, ctx, plan, values, shared=(), bits=()):
        self.ctx, self.plan = ctx, plan
        self.low = low = SS.lower(plan)
        self.seg_blocks = low.seg_blocks
        self._words = ctx.to_device(SS.word_buffer(low, values, shared, bits))
        self._digests = ctx.alloc(32 * len(low.seg_blocks))
        self.rows = SS.rows_for(plan)

    def launch(self, cols: Columns, n: int, table_bits: int = 12) -> int:
        """The entry point alone -> its status; nothing here waits for the stream."""
        ctx, low = self.ctx, self.low
        if len(low.choices):
            return ctx.lib.cq_sha256_synthesize_choices_dev(ctx.h, table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks),
                                                            low.sources.ctypes.data, low.choices.ctypes.data, len(low.choices),
                                                            self._words.ptr, low.words_len, n, cols.arr, self._digests.ptr)
        return ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, table_bits, low.seg_blocks.ctypes.data, len(low.seg_blocks),
                                                         low.sources.ctypes.data, self._words.ptr, low.words_len, n, cols.arr,
                                                         self._digests.ptr)

    def close(self):
        self._words.close()
        self._digests.close()


class VarlenJob(_Job):
    """Segments of `max_blocks_list` blocks whose messages are bytes [offsets[j], offsets[j] + lens[j]) of `data`, uploaded:
    cq_sha256_synthesize_varlen_dev."""

    def __init__(self, ctx, max_blocks_list, data: bytes, offsets, lens):
        self.ctx = ctx
        self.seg_blocks = np.array(max_blocks_list, dtype=np.uint32)
        self.offsets, self.lens = np.array(offsets, dtype=np.uint64), np.array(lens, dtype=np.uint64)
        self.bytes_len = len(data)
        self._bytes = ctx.to_device(np.frombuffer(bytes(data), dtype=np.uint8))
        self._digests = ctx.alloc(32 * len(self.seg_blocks))
        self.rows = sum(SC.rows_for(int(b)) for b in self.seg_blocks)

    def launch(self, cols: Columns, n: int, table_bits: int = 12) -> int:
        """The entry point alone -> its status; nothing here waits for the stream."""
        ctx = self.ctx
        return ctx.lib.cq_sha256_synthesize_varlen_dev(ctx.h, table_bits, self.seg_blocks.ctypes.data, len(self.seg_blocks), self._bytes.ptr,
                                                       self.bytes_len, self.offsets.ctypes.data, self.lens.ctypes.data, n, cols.arr,
                                                       self._digests.ptr)

    def close(self):
        self._bytes.close()
        self._digests.close()
