"""GPU: `ProvingKey.check_witness` where its bookkeeping is used -- the ordered compaction of the verdict bitmap past one
256-block spine tile, the cut at `cap` on word, block and tile boundaries, dense findings, and the two hash paths with
long runs of equal tuples, many broken cycles and a corrupt key.  Exact equality of (total, list) throughout.

The large case is k = 14 with 320 gate polynomials (tests/witness_check_wide.py LARGE_K, LARGE_GATES): 2^14 rows are the
fewest with which the key reaches three tiles (646 blocks; tests/test_witness_check_wide_cpu.py pins the geometry), and
one check is exactly one 256-word block, so block and tile boundaries fall on check boundaries.  320 polynomials, not
256: with 256 the failed-gate section would end with tile 0 and tile 1 would hold only poisoned-gate checks, which no
witness of this circuit sets -- with 320, failed-gate checks 256 .. 319 put findings into tile 1 and the carry into the
last tile is the sum of two non-empty tiles.  The key is built once for the module and the advice stays on the device.

The expected lists at k = 14 are written down from the planted positions (tests/witness_check_wide.py), which the CPU
tests hold against the model at k = 6 and 7; the model itself runs here at k <= 11 only."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import kzg
from tests import witness_check_wide as W
from tests.plonk_fixtures import to_backend_cs
from tests.test_witness_check_gpu import VK_REPR, _backend_pk, _cols, _gpu, _inst, _model, _overwrite

pytestmark = pytest.mark.gpu
P = B.R_MOD


class _Large:
    """The k = 14 key and its valid witness on the device."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.fx = W.wide_circuit(W.LARGE_K, W.LARGE_GATES)
        self.n, self.u = 1 << W.LARGE_K, W.usable(self.fx)
        self.pk = _backend_pk(ctx, self.fx)
        self.valid = _cols(self.fx)
        self.dev = [ctx.to_device(c) for c in self.valid]
        self.inst = _inst(self.fx)

    @contextlib.contextmanager
    def planted(self, cells):
        """The fixture with `cells` overwritten, on the host (the yielded copy) and on the device; put back on leaving."""
        work = W.fresh(self.fx)
        W.overwrite(work, cells)
        columns = {c for c, _ in cells}
        try:
            if len(cells) > 64:
                for c in columns:
                    self.dev[c].upload(B.to_mont_limbs(work["advice"][c] + [0] * (self.n - self.u)))
            else:
                for c, row in cells:
                    _overwrite(self.ctx, self.dev[c], row, work["advice"][c][row])
            yield work
        finally:
            for c in columns:
                self.dev[c].upload(self.valid[c])

    def check(self, cap=1 << 16):
        total, fails = self.pk.check_witness(self.dev, self.inst, max_failures=cap)
        print("check_witness:", total, [tuple(f) for f in fails[:8]])
        return total, [tuple(f) for f in fails]

    def check_array(self, cap):
        """cq_pk_check_witness into a uint32[cap, 4] array: a list of a million findings without a Python object each."""
        from sha2_on_cq_halo2_amd._marshal import _instance_columns, _ptr_array

        iptr, ilen, keep = _instance_columns(self.inst)
        out = np.zeros((max(cap, 1), 4), dtype=np.uint32)
        total = C.c_size_t()
        self.ctx._chk(self.ctx.lib.cq_pk_check_witness(self.pk.h, _ptr_array([d.ptr for d in self.dev], False), 1, iptr, ilen, None,
                                                       out.ctypes.data, cap, C.byref(total)))
        del keep
        return total.value, out[: min(cap, total.value)]


@pytest.fixture(scope="module")
def large(ctx):
    return _Large(ctx)


def _three_rows(fx, col, skip=0):
    """Three adjacent rows of one 64-row word in advice column `col`, the first (where the word allows) a cell that a copy
    constraint names."""
    row = [r for c, r in fx["copy_cells"] if c == col][skip]
    row = min(row - max(0, row % 64 - 61), W.usable(fx) - 3)
    assert row // 64 == (row + 2) // 64
    return [(col, row), (col, row + 1), (col, row + 2)]


# ---- a. b.  the valid witness; sparse findings in all three tiles -----------------------------------------------------------
def test_large_valid_witness_has_no_findings(large):
    assert large.check() == (0, [])


def test_large_sparse_findings_span_three_tiles(large):
    fx = large.fx
    cells = W.sparse_cells(fx)
    with large.planted(cells) as work:
        expected = W.findings(work, cells)
        blocks = {W.place(fx, f)[1] for f in expected}
        assert 0 in blocks and W.LARGE_GATES - 1 in blocks and any(256 < b < W.LARGE_GATES - 1 for b in blocks)
        assert {W.place(fx, f)[2] for f in expected} == {0, 1, 2}
        assert {W.place(fx, f)[2] for f in expected if f[0] == W.PERMUTATION} == {2}
        assert len(expected) < 1 << 16
        assert large.check() == (len(expected), expected)
    assert large.check() == (0, [])


# ---- c.  cap on every kind of boundary -----------------------------------------------------------------------------------------
def test_large_cap_on_word_block_and_tile_boundaries(large):
    fx = large.fx
    cells = _three_rows(fx, 0) + _three_rows(fx, 2, skip=40)
    with large.planted(cells) as work:
        expected = W.findings(work, cells)
        total = len(expected)
        at = [W.place(fx, f) for f in expected]
        tile0 = sum(t == 0 for _, _, t in at)
        tile01 = sum(t <= 1 for _, _, t in at)
        assert 0 < tile0 < tile01 < total, "findings in each of the three tiles"
        # the second word that holds three findings: a cut after its first and after its second bit
        starts = [i for i in range(total - 2) if at[i][0] == at[i + 2][0] and (i == 0 or at[i - 1][0] != at[i][0])]
        assert len(starts) > 2 and starts[0] == 0
        mid_word = starts[1]
        # the last finding of a block: the first block's and one in the middle of the list
        ends = [i for i in range(total - 1) if at[i][1] != at[i + 1][1]]
        caps = [0, 1, mid_word + 1, mid_word + 2, ends[0] + 1, ends[len(ends) // 2] + 1, tile0, tile0 + 1, tile01, tile01 + 1,
                total - 1, total, total + 5]
        assert at[tile0 - 1][2] == 0 and at[tile0][2] == 1 and at[tile01 - 1][2] == 1 and at[tile01][2] == 2
        for cap in caps:
            assert large.check(cap) == (total, expected[:cap]), cap


# ---- d.  dense: a whole column wrong -------------------------------------------------------------------------------------------
def test_large_dense_column(large):
    """Column 1 wrong on every usable row: every fourth failed-gate block is all ones but its six blinding rows -- block
    sums of 16378, 64 of them in tile 0 and 16 in tile 1 -- and the permutation findings come after a carry of 80 u."""
    fx, u = large.fx, large.u
    col = 1
    gates = list(range(col, W.LARGE_GATES, 4))
    with large.planted([(col, row) for row in range(u)]) as work:
        perms = W.perm_findings(work)
        assert perms and all(W.place(fx, f)[2] == 2 for f in perms)
        total = len(gates) * u + len(perms)
        assert len(gates) * u == (W.LARGE_GATES // 4) * u > 1 << 16
        prefix = lambda cap: [(W.GATE, g, row, 0) for g in gates[: cap // u + 1] for row in range(u)][:cap]
        assert large.check() == (total, prefix(1 << 16))  # the default cap is exceeded
        for cap in (64, 3 * u + 17):
            assert large.check(cap) == (total, prefix(cap)), cap
        # the whole list, across both tile boundaries, as an array: the first of them lies 64 u findings in
        want = np.zeros((total, 4), dtype=np.uint32)
        want[: len(gates) * u, 0] = W.GATE
        want[: len(gates) * u, 1] = np.repeat(gates, u)
        want[: len(gates) * u, 2] = np.tile(np.arange(u), len(gates))
        want[len(gates) * u:] = perms
        got_total, got = large.check_array(total)
        assert got_total == total and np.array_equal(got, want)
        got_total, got = large.check_array(64 * u + 1)  # the first finding of tile 1 is the last one kept
        assert got_total == total and np.array_equal(got, want[: 64 * u + 1])


# ---- e.  the scratch bitmap, block sums and counters are reused ---------------------------------------------------------------------
def test_large_repeat_and_sparse_after_dense(large):
    cells = W.sparse_cells(large.fx)
    with large.planted(cells) as work:
        sparse = W.findings(work, cells)
        assert large.check() == large.check() == (len(sparse), sparse)
    with large.planted([(3, row) for row in range(large.u)]) as work:
        dense_total = (W.LARGE_GATES // 4) * large.u + len(W.perm_findings(work))
        first = large.check(200)
        assert first[0] == dense_total and large.check(200) == first
    with large.planted(cells):
        assert large.check() == (len(sparse), sparse)
        assert large.check(3) == (len(sparse), sparse[:3])
    assert large.check() == (0, [])


# ---- f.  small domains: one, two and four words per check ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 7, 8])
def test_small_domains_sparse(ctx, k):
    fx = W.wide_circuit(k, 12)
    gpk = _backend_pk(ctx, fx)
    assert _gpu(gpk, fx) == (0, [])
    expected = W.plant(fx, W.sparse_cells(fx))
    assert _model(fx) == (len(expected), expected)
    assert _gpu(gpk, fx) == (len(expected), expected)
    for cap in (1, len(expected) - 1):
        assert _gpu(gpk, fx, cap=cap) == (len(expected), expected[:cap])


# ---- g.  a legacy table that is mostly duplicates; a poisoned input component ------------------------------------------------------------
def test_legacy_table_of_duplicates_k11(ctx):
    fx = W.wide_circuit(11, 4, legacy=True)
    u = W.usable(fx)
    gpk = _backend_pk(ctx, fx)
    poisoned = (1, [(W.LOOKUP, 1, u - 1, 0)])  # lookup 1 reads p0 @ next on the last usable row
    assert _model(fx) == poisoned
    assert _gpu(gpk, fx) == poisoned
    expected = W.plant_half_matching_tuples(fx, 50)
    assert sum(f[1] == 0 for f in expected) == 50 and len(expected) == 101
    assert _model(fx) == (len(expected), expected)
    assert _gpu(gpk, fx) == (len(expected), expected)


# ---- h.  many broken cycles over every permutation column ---------------------------------------------------------------------------------
def test_permutation_at_scale_k11(ctx):
    fx = W.wide_circuit(11, 8, copies=1200)
    expected = W.break_cycles(fx, 200)
    perms = [f for f in expected if f[0] == W.PERMUTATION]
    assert len(perms) > 300 and {f[1] for f in perms} == set(range(6))
    assert _model(fx) == (len(expected), expected)
    assert _gpu(_backend_pk(ctx, fx), fx) == (len(expected), expected)


# ---- i.  a corrupt key: sigma values that are no identity value -----------------------------------------------------------------------------
def test_corrupt_sigma_values_are_findings_on_their_cells(ctx):
    """The key's raw bytes (plonk.rs:349-362 as pk.hip writes them) with two sigma values replaced: 0 in a cell that maps
    to itself, and 1 + its value in a cell of a copy cycle.  Neither is a delta^c omega^r, so `perm_check_kernel` finds
    no cell for them: a finding on exactly those two cells, whatever the witness."""
    from sha2_on_cq_halo2_amd import ProvingKey
    from sha2_on_cq_halo2_amd.api import fr_to_mont

    k = 7
    fx = W.wide_circuit(k, 8)
    n, nf, pc = 1 << k, fx["circuit"].num_fixed, len(fx["circuit"].perm_columns)
    gpk = _backend_pk(ctx, fx)
    raw = bytearray(gpk.to_bytes())
    # k, fixed count | commitments | l0, l_last, l_active_row (extended) | fixed values, polys, cosets | sigma values, ...
    poly_n = 4 + 32 * n
    poly_ext, rest = divmod(len(raw) - 8 - 64 * (nf + pc) - 24 - 2 * poly_n * (nf + pc), 3 + nf + pc)
    assert rest == 0 and (poly_ext - 4) % (32 * n) == 0
    sigma0 = 8 + 64 * (nf + pc) + 3 * poly_ext + 12 + nf * (2 * poly_n + poly_ext) + 4
    at = lambda c, r: sigma0 + c * poly_n + 4 + 32 * r
    omega = kzg._root_for(k)
    ident = lambda c, r: pow(B.FR_DELTA, int(c), P) * pow(omega, int(r), P) % P
    mont = lambda v: fr_to_mont(v).astype("<u8").tobytes()

    named = set(fx["copy_cells"])
    alone = next((2, row) for row in range(40, W.usable(fx)) if (2, row) not in named)
    cycled = next(cell for cell in fx["copy_cells"] if cell[0] == 1 and tuple(fx["mapping"][cell[0]][cell[1]]) != cell)
    assert tuple(fx["mapping"][alone[0]][alone[1]]) == alone
    for c, r in (alone, cycled, (0, 0), (5, n - 1)):  # the offsets are the sigma values' own
        assert bytes(raw[at(c, r): at(c, r) + 32]) == mont(ident(*fx["mapping"][c][r]))
    identities = {ident(c, r) for c in range(pc) for r in range(n)}
    bad = 1 + ident(*fx["mapping"][cycled[0]][cycled[1]])
    assert 0 not in identities and bad not in identities
    raw[at(*alone): at(*alone) + 32] = mont(0)
    raw[at(*cycled): at(*cycled) + 32] = mont(bad)

    cs = to_backend_cs(fx["circuit"], {})
    rpk = ProvingKey(ctx, gpk.params, k, 0, [], None, None, B.to_mont_limbs([VK_REPR])[0], cs=cs, raw=bytes(raw))
    expected = sorted([(W.PERMUTATION,) + alone + (0,), (W.PERMUTATION,) + cycled + (0,)])
    assert _gpu(gpk, fx) == (0, [])
    assert _gpu(rpk, fx) == (2, expected)
    more = W.plant(fx, W.sparse_cells(fx))  # and next to the findings of a planted witness (which may name `cycled` too)
    both = sorted(set(more) | set(expected))
    assert (W.PERMUTATION,) + alone + (0,) not in more and _gpu(rpk, fx) == (len(both), both)
