"""GPU: Assigned (rational) witness columns -- cq_batch_invert_assigned(_dev) against tests/assigned_model.py at the
edges of the batch-inversion kernel, bad row lists as errors, cq_create_proof_assigned byte for byte against the dense
path, check_witness on Assigned columns, the keygen call site and one SHA-shaped proof at k = 14."""
import numpy as np
import pytest

from oracle import bn254 as B
from sha2_on_cq_halo2_amd import CqError
from sha2_on_cq_halo2_amd.plonk import Assigned, AssignedColumn
from tests import assigned_model as M
from tests.plonk_fixtures import TABLE, chain_circuit, plonk_api_circuit, to_backend_cs

pytestmark = pytest.mark.gpu
P = B.R_MOD
VK_REPR = 424242
N_SMALL, COLS_SMALL = 1 << 11, 3
# poly_batch_invert (csrc/poly.hip, batch_invert_per_lane): 4 elements per lane up to 5 * 2^16, 8 up to 3 * 2^20, 16 beyond
PER_LANE_STEPS = (5 << 16, 3 << 20)


def _split(total, n, ncols):
    """den_count per column: a column WITHOUT rational cells between two that have some whenever the total fits the outer
    two, a full outer pair otherwise."""
    assert ncols == 3 and total <= 3 * n
    if total <= 2 * n:
        return [(total + 1) // 2, 0, total // 2]
    return [n, total - 2 * n, n]


def _small_case(total, pattern, seed):
    """3 columns of 2^11 cells with `total` Rational cells at seeded rows.  By position in the concatenated list: zero
    denominators at the first and last element of the 1024-element blocks of the 4-per-lane kernel and at the very end,
    every 97th; denominators 1 and r - 1; zero numerators over non-zero denominators; pattern "zero_block": the whole
    first block's denominators are zero."""
    rng = np.random.RandomState(seed)
    pr = B.Xoshiro256ss(seed)
    cols, at = [], 0
    for cnt in _split(total, N_SMALL, COLS_SMALL):
        rows = set(int(r) for r in rng.choice(N_SMALL, cnt, replace=False))
        cells = []
        for r in range(N_SMALL):
            if r not in rows:
                cells.append(M.Z if r % 5 == 0 else M.T(B.fr_random(pr)))
                continue
            den = B.fr_random(pr)
            if at in (0, 1023, 1024, 2047, total - 1) or at % 97 == 0 or (pattern == "zero_block" and at < 1024):
                den = 0
            elif at % 97 == 1:
                den = 1
            elif at % 97 == 2:
                den = P - 1
            cells.append(M.R(0 if at % 89 == 3 else B.fr_random(pr), den))
            at += 1
        cols.append(cells)
    assert at == total
    return cols


def _columns(model_cols, n):
    out = []
    for cells in model_cols:
        num, rows, den = M.to_arrays(cells, n)
        out.append(AssignedColumn(B.to_mont_limbs(num), rows, B.to_mont_limbs(den) if den else np.zeros((0, 4), dtype=np.uint64)))
    return out


def _resolve_dev(ctx, columns, in_place, poison=None):
    """through cq_batch_invert_assigned_dev; returns the downloaded outputs (and frees everything)"""
    n = columns[0].n
    bufs, descr, outs = [], [], []
    for col in columns:
        num = ctx.to_device(col.num)
        m = col.den_rows.shape[0]
        rows = ctx.to_device(col.den_rows) if m else None
        den = ctx.to_device(col.den) if m else None
        out = num if in_place else ctx.to_device(poison if poison is not None else np.full((n, 4), 0xAB, dtype=np.uint64))
        bufs += [b for b in (num, rows, den, None if in_place else out) if b is not None]
        descr.append((num.ptr, rows.ptr if m else None, den.ptr if m else None, m))
        outs.append(out)
    try:
        ctx.batch_invert_assigned_dev(descr, n, [o.ptr for o in outs])
        return [o.download((n, 4)) for o in outs]
    finally:
        res = [o.download((n, 4)) for o in outs]
        for b in bufs:
            b.free()
        _resolve_dev.last_outputs = res


SMALL_TOTALS = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.mark.parametrize("entry", ["host", "dev_in_place", "dev_out_of_place"])
@pytest.mark.parametrize("total", SMALL_TOTALS)
def test_resolve_matches_the_model_at_the_kernel_edges(ctx, total, entry):
    for pattern in ("mixed", "zero_block"):
        model_cols = _small_case(total, pattern, seed=1000 + total)
        want = [B.to_mont_limbs(c) for c in M.batch_invert_assigned_ref(model_cols)]
        columns = _columns(model_cols, N_SMALL)
        assert sum(c.den_rows.shape[0] for c in columns) == total
        if entry == "host":
            got = ctx.batch_invert_assigned(columns)
        else:
            got = _resolve_dev(ctx, columns, in_place=entry == "dev_in_place")
        for c in range(COLS_SMALL):
            bad = np.nonzero((got[c] != want[c]).any(axis=1))[0]
            assert bad.size == 0, (total, entry, pattern, c, bad[:8])


def _pool_case(n, ncols, total, seed):
    """A large case whose expectation needs no big-integer pass: every Rational cell is drawn from a pool of 4096
    (numerator, denominator, quotient) triples worked out by the model -- zero, 1 and r - 1 denominators and zero
    numerators among them -- so that the expected column is an index into the pool."""
    pr = B.Xoshiro256ss(seed)
    pool = []
    for i in range(4096):
        den = 0 if i % 61 == 0 else 1 if i % 61 == 1 else P - 1 if i % 61 == 2 else B.fr_random(pr)
        pool.append(M.R(0 if i % 53 == 3 else B.fr_random(pr), den))
    p_num = B.to_mont_limbs([c[1] for c in pool])
    p_den = B.to_mont_limbs([c[2] for c in pool])
    p_val = B.to_mont_limbs([M.evaluate(c) for c in pool])
    rng = np.random.RandomState(seed)
    counts = [min(n, max(0, total - c * n)) for c in range(ncols)]
    assert sum(counts) == total
    columns, want = [], []
    for cnt in counts:
        rows = np.sort(rng.choice(n, cnt, replace=False)).astype(np.uint32) if cnt < n else np.arange(n, dtype=np.uint32)
        pick = rng.randint(0, 4096, size=cnt)
        num = rng.randint(0, 2**62, size=(n, 4), dtype=np.int64).astype(np.uint64)
        num[:, 3] &= np.uint64((1 << 60) - 1)  # below r: any canonical Montgomery word is a Trivial cell
        exp = num.copy()
        num[rows] = p_num[pick]
        exp[rows] = p_val[pick]
        columns.append(AssignedColumn(num, rows, p_den[pick]))
        want.append(exp)
    return columns, want


@pytest.mark.parametrize("total", [t + d for t in PER_LANE_STEPS for d in (-1, 0, 1)])
def test_resolve_where_the_elements_per_lane_change(ctx, total):
    """One below, at and above the counts where poly_batch_invert goes from 4 to 8 and from 8 to 16 elements per lane
    (more cells than 3 columns of 2^11 hold: 3 x 2^17 and 4 x 2^20 here), device entry point, in place."""
    n, ncols = (1 << 17, 3) if total < (1 << 19) else (1 << 20, 4)
    columns, want = _pool_case(n, ncols, total, seed=total)
    got = _resolve_dev(ctx, columns, in_place=True)
    for c in range(ncols):
        bad = np.nonzero((got[c] != want[c]).any(axis=1))[0]
        assert bad.size == 0, (total, c, bad[:8])


@pytest.mark.parametrize("kind", ["row_equals_n", "descending", "duplicate"])
def test_bad_device_lists_are_errors_and_write_nothing(ctx, kind):
    n = N_SMALL
    model_cols = _small_case(300, "mixed", seed=7)
    columns = _columns(model_cols, n)
    good = [AssignedColumn(c.num, c.den_rows.copy(), c.den) for c in columns]
    rows = columns[2].den_rows  # column 2 holds 150 entries
    entry = 77
    if kind == "row_equals_n":
        entry = rows.shape[0] - 1
        rows[entry] = n
    elif kind == "descending":
        rows[entry - 1], rows[entry] = rows[entry], rows[entry - 1]  # entry - 1 still ascends from entry - 2
    else:
        rows[entry] = rows[entry - 1]
    poison = np.full((n, 4), 0x5A5A5A5A, dtype=np.uint64)
    with pytest.raises(CqError) as e:
        _resolve_dev(ctx, columns, in_place=False, poison=poison)
    print(e.value)
    assert e.value.code == -1 and "column 2" in str(e.value) and "entry %d" % entry in str(e.value)
    assert all((o == poison).all() for o in _resolve_dev.last_outputs)
    # the host entry point names the same entry
    with pytest.raises(CqError) as e2:
        ctx.batch_invert_assigned(columns)
    assert e2.value.code == -1 and "column 2" in str(e2.value) and "entry %d" % entry in str(e2.value)
    # and the context goes on working
    want = [B.to_mont_limbs(c) for c in M.batch_invert_assigned_ref(model_cols)]
    got = _resolve_dev(ctx, good, in_place=False)
    assert all((g == w).all() for g, w in zip(got, want))


# ---- proofs ------------------------------------------------------------------------------------------------------------
def _backend_pk(ctx, fx, fixed=None):
    from sha2_on_cq_halo2_amd import ParamsKZG, ProvingKey, StaticTable, TableConfig

    k = fx["circuit"].k
    sm = B.to_mont_limbs([B.fr_random(B.Xoshiro256ss(k))])[0]
    gparams = ParamsKZG.setup_from_toxic_waste(ctx, k, sm)
    gtables, gcfg, b0 = {}, None, None
    if fx["tables"]:
        gcfg = TableConfig.setup_from_toxic_waste(ctx, len(TABLE), sm)
        gtables = {name: StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(v), sm) for name, v in fx["tables"].items()}
        b0 = gparams.g_dev + 64
    cs = to_backend_cs(fx["circuit"], gtables)
    return ProvingKey(ctx, gparams, k, 0, [], gcfg, b0, B.to_mont_limbs([VK_REPR])[0], cs=cs,
                      fixed=fixed if fixed is not None else [B.to_mont_limbs(c) for c in fx["fixed"]],
                      permutation=np.array(fx["mapping"], dtype=np.uint32))


def _rationalise(values, n, seed, zero_column=False):
    """A seeded half of the cells v as Rational(v d, d) with random d; in `zero_column` every zero cell as Rational(a, 0)
    with random a; the rest Trivial, or Zero where the value is zero."""
    pr = B.Xoshiro256ss(seed)
    cells = []
    for v in list(values) + [0] * (n - len(values)):
        if zero_column and v == 0:
            cells.append(Assigned.rational(B.fr_random(pr), 0))
        elif pr.next_u64() & 1:
            d = B.fr_random(pr) or 1
            cells.append(Assigned.rational(v * d, d))
        else:
            cells.append(Assigned.trivial(v) if v else Assigned.zero())
    return cells


def _dense(fx):
    n = 1 << fx["circuit"].k
    return [B.to_mont_limbs(list(c) + [0] * (n - len(c))) for c in fx["advice"]]


@pytest.mark.parametrize("which", ["chain5", "chain11_lookup", "plonk_api"])
def test_create_proof_assigned_is_the_dense_proof(ctx, which):
    fx = {"chain5": lambda: chain_circuit(5), "chain11_lookup": lambda: chain_circuit(11, with_lookup=True),
          "plonk_api": lambda: plonk_api_circuit()}[which]()
    n = 1 << fx["circuit"].k
    gpk = _backend_pk(ctx, fx)
    u = gpk.usable_rows
    inst = [B.to_mont_limbs(i) for i in fx["instances"]]
    dense = gpk.create_proof(_dense(fx), seed=31, instances=inst)
    cells = [_rationalise(col[:u], u, 50 + j, zero_column=j == 1) + [Assigned.zero()] * (n - u) for j, col in enumerate(fx["advice"])]
    assert any(c.kind == Assigned.RATIONAL and c.den == 0 for c in cells[1])
    columns = [AssignedColumn.from_cells(c, n) for c in cells]
    assert [[c.evaluate() for c in col[:u]] for col in cells] == [list(col[:u]) + [0] * (u - len(col[:u])) for col in fx["advice"]]
    assert gpk.create_proof_assigned(columns, seed=31, instances=inst) == dense
    # a listed row in the blinding range (and a numerator there) changes nothing: those cells are overwritten (:346-349)
    blind = [c[:] for c in cells]
    blind[0][u] = Assigned.rational(5, 7)
    blind[2][n - 1] = Assigned.rational(9, 0)
    assert gpk.create_proof_assigned([AssignedColumn.from_cells(c, n) for c in blind], seed=31, instances=inst) == dense
    # the witness checker takes the same columns
    assert gpk.check_witness(columns, inst) == (0, [])
    bad = [c[:] for c in cells]
    row = 3
    old = bad[2][row]
    bad[2][row] = Assigned.rational(old.num + 1, old.den) if old.kind == Assigned.RATIONAL else Assigned.trivial(old.numerator() + 1)
    resolved = [B.to_mont_limbs([c.evaluate() for c in col]) for col in bad]
    want = gpk.check_witness(resolved, inst)
    assert want[0] > 0
    assert gpk.check_witness([AssignedColumn.from_cells(c, n) for c in bad], inst) == want
    gpk.close()


def test_keygen_fixed_columns_from_rational_form(ctx):
    """keygen.rs:244,320: `batch_invert_assigned(assembly.fixed)` before the fixed columns enter the key."""
    fx = chain_circuit(5)
    n = 1 << fx["circuit"].k
    dense_pk = _backend_pk(ctx, fx)
    want = dense_pk.vk_commitments()
    columns = [AssignedColumn.from_cells(_rationalise(col, n, 90 + j, zero_column=j == 0), n) for j, col in enumerate(fx["fixed"])]
    assert sum(c.den_rows.shape[0] for c in columns) > n
    resolved = ctx.batch_invert_assigned(columns)
    assert all((r == B.to_mont_limbs(col)).all() for r, col in zip(resolved, fx["fixed"]))
    pk2 = _backend_pk(ctx, fx, fixed=resolved)
    got = pk2.vk_commitments()
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and want[0].shape[0] == len(fx["fixed"])
    dense_pk.close()
    pk2.close()


def test_sha_shaped_proof_k14_from_assigned_columns(ctx):
    """The smallest BASELINE size: 8 columns of 2^14 cells, an eighth of them Rational."""
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    wl = ShaCqWorkload(ctx, 14, pairs=4)
    n = 1 << 14
    dense = wl.prove(seed=9)
    cols = [c.download((n, 4)) for c in wl.cols]
    pr = B.Xoshiro256ss(14)
    columns, rational = [], 0
    for col in cols:
        vals = list(B.from_mont_limbs(col))
        rows = [r for r in range(n) if pr.next_u64() % 8 == 0]
        dens = [B.fr_random(pr) or 1 for _ in rows]
        for r, d in zip(rows, dens):
            vals[r] = vals[r] * d % P
        rational += len(rows)
        columns.append(AssignedColumn(B.to_mont_limbs(vals), rows, B.to_mont_limbs(dens)))
    assert n * 8 // 10 < rational < n * 8 // 6
    assert wl.pk.create_proof_assigned(columns, seed=9) == dense
    wl.close()
