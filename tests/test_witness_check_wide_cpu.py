"""CPU: what licenses tests/test_witness_check_wide_gpu.py.  The findings tests/witness_check_wide.py writes down from
the planted positions equal the model's (tests/witness_check_model.py) at k = 6 and 7, where the model is cheap; and the
bitmap geometry of every size the GPU tests use is pinned here, the large case reaching three spine tiles."""
import pytest

from tests import witness_check_model as M
from tests import witness_check_wide as W


def _model(fx):
    return M.check_witness(fx["circuit"], fx["fixed"], fx["advice"], fx["instances"], fx["mapping"], fx["tables"])


@pytest.fixture(scope="module", params=[6, 7])
def small(request):
    return W.wide_circuit(request.param, 12)


def test_valid_witness_has_no_findings(small):
    assert _model(small) == (0, [])
    assert W.perm_findings(small) == []


def test_copies_cover_every_column_and_the_row_range(small):
    u = W.usable(small)
    named = set(small["copy_cells"])
    assert {c for c, _ in named} == set(range(6))
    for j in range(4):
        rows = sorted(r for c, r in named if c == j)
        assert rows[0] < u // 8 and rows[-1] >= u - u // 8
    assert max(_cycle_length(small["mapping"], cell) for cell in named) > 2, "some cycles are longer than two cells"


def _cycle_length(mapping, cell):
    at, steps = tuple(mapping[cell[0]][cell[1]]), 1
    while at != cell:
        at, steps = tuple(mapping[at[0]][at[1]]), steps + 1
    return steps


def _plantings(fx):
    u = W.usable(fx)
    named = [cell for cell in fx["copy_cells"] if cell[0] < 4]
    c, r = named[7]
    r3 = min(r, u - 3)
    return {
        "single cell": [named[0]],
        "single cell no copy names": [next((1, row) for row in range(u) if (1, row) not in set(fx["copy_cells"]))],
        "three adjacent rows": [(c, r3), (c, r3 + 1), (c, r3 + 2)],
        "whole column": [(2, row) for row in range(u)],
        "sparse": W.sparse_cells(fx),
    }


@pytest.mark.parametrize("which", ["single cell", "single cell no copy names", "three adjacent rows", "whole column", "sparse"])
def test_analytic_findings_equal_the_model(small, which):
    fx = W.fresh(small)
    cells = _plantings(fx)[which]
    expected = W.plant(fx, cells)
    assert expected == sorted(expected) and len(set(expected)) == len(expected)
    assert sum(f[0] == W.GATE for f in expected) == 3 * len(cells)  # 12 gates over 4 columns
    if which != "single cell no copy names":
        assert any(f[0] == W.PERMUTATION for f in expected)
    assert _model(fx) == (len(expected), expected)
    assert _model(small) == (0, []), "the shared fixture is left alone"


def test_broken_cycles_equal_the_model(small):
    """Advice, instance and kc cells of the copy constraints changed: both ends of a 2-cycle, and of a longer cycle the
    cells whose partner differs."""
    fx = W.fresh(small)
    expected = W.break_cycles(fx, 20)
    assert {f[1] for f in expected if f[0] == W.PERMUTATION} == set(range(6))
    assert _model(fx) == (len(expected), expected)


def test_legacy_hand_list_equals_the_model():
    fx = W.wide_circuit(7, 4, legacy=True)
    u = W.usable(fx)
    assert len({(fx["fixed"][6][r], fx["fixed"][7][r]) for r in range(u)}) == 8
    assert len({(fx["fixed"][8][r], fx["fixed"][9][r]) for r in range(u)}) == 8
    assert _model(fx) == (1, [(W.LOOKUP, 1, u - 1, 0)])  # the poisoned tuple of the last usable row
    expected = W.plant_half_matching_tuples(fx, 10)
    assert sum(f[1] == 0 for f in expected) == 10
    assert _model(fx) == (len(expected), expected)


# ---- the bitmap geometry of the sizes the GPU tests use --------------------------------------------------------------------
def test_geometry_of_the_small_domains():
    """12 gates: 24 gate checks + 6 permutation columns; one, two and four words per check, all in one block."""
    assert [W.geometry(k, 30) for k in (6, 7, 8)] == [(1, 30, 1, 1), (2, 60, 1, 1), (4, 120, 1, 1)]
    assert W.num_checks(W.wide_circuit(6, 12)) == 30


def test_geometry_of_the_hash_path_cases():
    """k = 11: 32 words per check.  Permutation at scale: 8 gates -> 22 checks, 3 blocks; legacy: 4 gates, 2 lookups -> 16
    checks, 2 blocks."""
    assert W.geometry(11, 22) == (32, 704, 3, 1)
    assert W.geometry(11, 16) == (32, 512, 2, 1)
    assert W.num_checks(W.wide_circuit(7, 4, legacy=True)) == 16


def test_geometry_of_the_largest_case_before_these_tests():
    """test_sha_plonk_workload_k18 (ShaPlonkWorkload, pairs = 4): 2 gate polynomials (failed and poisoned: 4 checks), 4
    static lookups, 2 permutation columns, and one legacy lookup in its second case: 10 and 11 checks of 4096 words --
    160 and 176 blocks, one tile."""
    assert W.geometry(18, 10) == (4096, 40960, 160, 1)
    assert W.geometry(18, 11) == (4096, 45056, 176, 1)


def test_geometry_of_the_large_case():
    """2^14 rows are the fewest that give three tiles with a block-aligned check: nblocks >= 513 needs 1025 checks of 128
    words at k = 13.  The sparse planting reaches all three tiles, the first block, the interior of tile 1, the last
    block of the failed-gate section and the permutation section in the last tile."""
    fx = W.wide_circuit(W.LARGE_K, W.LARGE_GATES)
    checks = W.num_checks(fx)
    words, nwords, nblocks, tiles = W.geometry(W.LARGE_K, checks)
    assert (checks, words, nwords, nblocks, tiles) == (646, 256, 165376, 646, 3) and nblocks >= 513
    assert W.geometry(13, checks)[2] < 513
    assert W.perm_findings(fx) == []
    expected = W.plant(W.fresh(fx), W.sparse_cells(fx))
    blocks = {W.place(fx, f)[1] for f in expected}
    assert 0 in blocks and W.LARGE_GATES - 1 in blocks
    assert any(256 < b < W.LARGE_GATES - 1 for b in blocks)
    assert {W.place(fx, f)[2] for f in expected} == {0, 1, 2}
    assert {W.place(fx, f)[2] for f in expected if f[0] == W.PERMUTATION} == {2}
    assert W.place(fx, (W.GATE, 0, 5, 0)) == (0, 0, 0) and W.place(fx, (W.PERMUTATION, 0, 64, 0)) == (640 * 256 + 1, 640, 2)
