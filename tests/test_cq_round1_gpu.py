"""GPU: round 1 of the static-lookup argument (`table_insert_kernel`, `cq_round1_kernel` of csrc/cq.hip, `table_find` of
csrc/tablehash.hpp) and the witness checker's static lookups (csrc/check.hip) on tables whose values collide under the
slot hash on purpose (tests/tablehash_model.py; tests/test_cq_round1_cpu.py checks that they do) and on witnesses that are
index patterns through those tables.  The reference is numpy over the integer witness: `m` is a bincount of the indices.

Keys are built on the GPU alone (toxic-waste setup, b0 bases from the params' own g[1..]); no oracle key is needed for
round 1."""
import types

import numpy as np
import pytest

from oracle import bn254 as B
from tests import tablehash_model as M
from tests import witness_check_model as WM

pytestmark = pytest.mark.gpu
P = B.R_MOD
BF = 5  # blinding factors of a CQ-only key: u = n - 6
STATIC, NOT_IN_TABLE, DIFFERENT_ROWS = WM.STATIC_LOOKUP, WM.NOT_IN_TABLE, WM.DIFFERENT_ROWS


class _Env:
    """params per k, table config per N, tables per (N, name) and keys per shape, built once for the module"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.s = B.to_mont_limbs([B.fr_random(B.Xoshiro256ss(0xC011))])[0]
        self._params, self._cfg, self._tables, self._keys = {}, {}, {}, {}

    def params(self, k):
        from sha2_on_cq_halo2_amd import ParamsKZG

        if k not in self._params:
            self._params[k] = ParamsKZG.setup_from_toxic_waste(self.ctx, k, self.s)
        return self._params[k]

    def cfg(self, N):
        from sha2_on_cq_halo2_amd import TableConfig

        if N not in self._cfg:
            self._cfg[N] = TableConfig.setup_from_toxic_waste(self.ctx, N, self.s)
        return self._cfg[N]

    def table(self, N, name):
        """(StaticTable, its values as uint64[N, 4] Montgomery limbs)"""
        from sha2_on_cq_halo2_amd import StaticTable

        if (N, name) not in self._tables:
            limbs = B.to_mont_limbs(M.tables_for(N)[name])
            self._tables[N, name] = (StaticTable.setup_from_toxic_waste(self.ctx, limbs, self.s), limbs)
        return self._tables[N, name]

    def key(self, k, N, lookups):
        """lookups: tuple of lookups, each a tuple of (advice column, table name)"""
        from sha2_on_cq_halo2_amd import ProvingKey

        if (k, N, lookups) not in self._keys:
            params = self.params(k)
            num_advice = 1 + max(c for lk in lookups for c, _ in lk)
            self._keys[k, N, lookups] = ProvingKey(self.ctx, params, k, num_advice,
                                                   [[(c, self.table(N, t)[0]) for c, t in lk] for lk in lookups], self.cfg(N),
                                                   params.g_dev + 64, B.to_mont_limbs([0xC0FFEE + k])[0])
        return self._keys[k, N, lookups]

    def close(self):
        for group in (self._keys, self._tables, self._cfg, self._params):
            for obj in group.values():
                (obj[0] if isinstance(obj, tuple) else obj).close()


@pytest.fixture(scope="module")
def env(ctx):
    e = _Env(ctx)
    yield e
    e.close()


def _patterns(N, n):
    """name -> index per row (int64[n]); lane t of block b looks up rows (4 b + r) 256 + t, r = 0..3"""
    i = np.arange(n)
    strip = (i // 256) % 4
    a, b = 3, N - 2
    rng = np.random.RandomState(N + n)
    pat = {
        "constant": np.full(n, N - 1),                             # m[N - 1] = u
        "lane4": (i % 256) % N,                                    # a lane's four rows are equal: the held count reaches 4
        "ABAB": np.where(strip % 2 == 0, a, b),                    # the held pair is flushed three times
        "ABBA": np.where((strip == 0) | (strip == 3), a, b),
        "AABB": np.where(strip < 2, a, b),
        "runs": i * N // n,                                        # neighbouring lanes equal
        "uniform": rng.randint(0, N, n),
        "three": np.array([0, N // 2, N - 1])[rng.randint(0, 3, n)],
    }
    for d in (1, 2, 4, 5, 8, 64):  # distinct indices per wave: the leader loop ends in <= 4 rounds, leaves one value, leaves 60
        pat["wave%d" % d] = (i % 64) % d % N
    return pat


def _blinding(seed, count, avoid):
    rng = B.Xoshiro256ss(seed)
    out = []
    while len(out) < count:
        v = B.fr_random(rng)
        if v not in avoid:
            out.append(v)
    return B.to_mont_limbs(out)


def _column(table_limbs, idx, u, blind):
    """value = table[idx(i)] on the usable rows, the given field elements (not in the table) on the rows from u on"""
    col = table_limbs[idx]
    col[u:] = blind
    return col


def _theta(seed):
    v = B.fr_random(B.Xoshiro256ss(seed))
    return v, B.to_mont_limbs([v])[0]


def _round1(gpk, bufs, theta, L, n, N):
    """(f uint64[L, n, 4], m uint32[L, N]) of the stand-alone round-1 call"""
    f, m, _ = gpk.cq_round1([b.ptr for b in bufs], theta)
    fh, mh = f.download((L, n, 4)), m.download((L, N), dtype=np.uint32)
    f.free()
    m.free()
    return fh, mh


def _findings(gpk, bufs):
    total, fails = gpk.check_witness(bufs)
    return total, [tuple(f) for f in fails]


def _model_findings(k, lookups, advice, tables):
    circuit = types.SimpleNamespace(k=k, blinding_factors=lambda: BF, gates=[], plookups=[], lookups=[list(lk) for lk in lookups],
                                    perm_columns=[])
    return WM.check_witness(circuit, [], advice, [], [], tables)


# ---- multiplicities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap", "adjacent", "random"])
@pytest.mark.parametrize("N", [64, 512])
@pytest.mark.parametrize("k", [5, 10, 11])
def test_multiplicities_equal_a_bincount(ctx, env, k, N, name):
    """Two width-1 lookups on the same table per call (blockIdx.y separates their m arrays), every pattern of `_patterns`.
    k = 5: u = 26, one partial wave; k = 10: u = 1018, one block whose strip r = 3 is partly out of range; k = 11:
    u = 2042, two blocks, the last wave partial.  N = 512 is more than n at k = 5."""
    n, u = 1 << k, (1 << k) - BF - 1
    gpk = env.key(k, N, (((0, name),), ((1, name),)))
    assert gpk.usable_rows == u
    _, limbs = env.table(N, name)
    pats = _patterns(N, n)
    names = sorted(pats)
    blind = _blinding(k * 1000 + N, 2 * (n - u), set(M.tables_for(N)[name]))
    bufs = [ctx.alloc(n * 32), ctx.alloc(n * 32)]
    _, theta = _theta(k)
    for pa, pb in zip(names[0::2], names[1::2]):
        cols = [_column(limbs, pats[pa], u, blind[: n - u]), _column(limbs, pats[pb], u, blind[n - u:])]
        for buf, col in zip(bufs, cols):
            buf.upload(col)
        f, m = _round1(gpk, bufs, theta, 2, n, N)
        for l, p in enumerate((pa, pb)):
            want = np.bincount(pats[p][:u], minlength=N)
            assert want.sum() == u
            assert np.array_equal(m[l], want), (p, np.nonzero(m[l] != want)[0][:8], m[l][m[l] != want][:8], want[m[l] != want][:8])
            assert np.array_equal(f[l, :u], cols[l][:u]), p  # width 1: f is the column
        assert _findings(gpk, bufs) == (0, [])
    assert len(names) == 14
    for buf in bufs:
        buf.free()


def test_width_two_fold_and_multiplicities(ctx, env):
    """One width-2 lookup over two different colliding tables, both columns on the same index: m is the bincount and
    f = theta e_0 + e_1 (static_lookup/prover.rs:108-116) on Python integers."""
    k, N = 10, 64
    n, u = 1 << k, (1 << k) - BF - 1
    lookups = (((0, "wrap"), (1, "wrap2")),)
    gpk = env.key(k, N, lookups)
    t = M.tables_for(N)
    idx = _patterns(N, n)["uniform"]
    blind = _blinding(99, 2 * (n - u), set(t["wrap"]) | set(t["wrap2"]))
    cols = [_column(env.table(N, "wrap")[1], idx, u, blind[: n - u]), _column(env.table(N, "wrap2")[1], idx, u, blind[n - u:])]
    bufs = [ctx.to_device(c) for c in cols]
    tv, theta = _theta(4242)
    f, m = _round1(gpk, bufs, theta, 1, n, N)
    assert np.array_equal(m[0], np.bincount(idx[:u], minlength=N))
    want_f = [(tv * t["wrap"][j] + t["wrap2"][j]) % P for j in idx[:u]]
    assert np.array_equal(f[0, :u], B.to_mont_limbs(want_f))
    assert _findings(gpk, bufs) == (0, [])
    for buf in bufs:
        buf.free()


# ---- failures: one kind per call, the error word is a last-writer-wins flag ----------------------------------------------------
def _expect_lookup_error(gpk, bufs, theta, text):
    from sha2_on_cq_halo2_amd import CqError

    with pytest.raises(CqError) as e:
        gpk.cq_round1([b.ptr for b in bufs], theta)
    assert e.value.code == -4 and text in str(e.value), str(e.value)


@pytest.mark.parametrize("k,N", [(10, 64), (10, 512), (11, 512)])
def test_values_outside_a_colliding_table_are_reported(ctx, env, k, N):
    """Row 0, a row of strip 3 in block 0 and row u - 1, each with: a value that walks the whole cluster and the wrap to the
    first empty slot; a value whose home slot is empty; values that equal an entry in all but the top / the lowest word."""
    n, u = 1 << k, (1 << k) - BF - 1
    lookups = (((0, "wrap"),),)
    gpk = env.key(k, N, lookups)
    _, limbs = env.table(N, "wrap")
    t = M.tables_for(N)
    idx = _patterns(N, n)["uniform"]
    good = _column(limbs, idx, u, _blinding(7 * k + N, n - u, set(t["wrap"])))
    buf = ctx.to_device(good)
    _, theta = _theta(k + N)
    want_m = np.bincount(idx[:u], minlength=N)
    absent = M.absent_values(N)
    rows = (0, 3 * 256 + 37, u - 1)
    for name in ("head", "empty", "top", "low"):
        value = B.to_mont_limbs([absent[name]])[0]
        for row in rows:
            bad = good.copy()
            bad[row] = value
            buf.upload(bad)
            _expect_lookup_error(gpk, [buf], theta, "not in table")
            assert _findings(gpk, [buf]) == (1, [(STATIC, 0, row, NOT_IN_TABLE)]), (name, row)
            buf.upload(good)  # the same witness with that row repaired
            f, m = _round1(gpk, [buf], theta, 1, n, N)
            assert np.array_equal(m[0], want_m) and np.array_equal(f[0, :u], good[:u])
    # all four at once, against the model of the checker
    bad = good.copy()
    advice = [t["wrap"][j] for j in idx[:u]]
    for name, row in zip(("head", "empty", "top", "low"), (0, 3 * 256 + 37, 3 * 256 + 38, u - 1)):
        bad[row] = B.to_mont_limbs([absent[name]])[0]
        advice[row] = absent[name]
    buf.upload(bad)
    want = (4, [(STATIC, 0, row, NOT_IN_TABLE) for row in (0, 3 * 256 + 37, 3 * 256 + 38, u - 1)])
    assert _model_findings(k, lookups, [advice], t) == want
    assert _findings(gpk, [buf]) == want
    assert "static lookup 0, row %d: the value is not in the table" % (u - 1) in str(gpk.check_witness([buf])[1][-1])
    buf.free()


@pytest.mark.parametrize("N", [64, 512])
def test_vector_lookup_on_different_table_rows_is_reported(ctx, env, N):
    """Width 2 over two different colliding tables: both values present but at different indices -> "same table row"
    (static_lookup/prover.rs:148); the second (or the first) column's value absent -> "not in table" (:141)."""
    k = 10
    n, u = 1 << k, (1 << k) - BF - 1
    lookups = (((0, "wrap"), (1, "wrap2")),)
    gpk = env.key(k, N, lookups)
    t = M.tables_for(N)
    l0, l1 = env.table(N, "wrap")[1], env.table(N, "wrap2")[1]
    idx = _patterns(N, n)["three"]
    blind = _blinding(5 + N, 2 * (n - u), set(t["wrap"]) | set(t["wrap2"]))
    good = [_column(l0, idx, u, blind[: n - u]), _column(l1, idx, u, blind[n - u:])]
    bufs = [ctx.to_device(c) for c in good]
    _, theta = _theta(N)
    want_m = np.bincount(idx[:u], minlength=N)
    absent = B.to_mont_limbs([M.absent_values(N)["head"]])[0]
    rows = (0, 3 * 256 + 37, u - 1)
    cases = [(row, 1, "same table row", DIFFERENT_ROWS) for row in rows]
    cases += [(rows[1], 1, "not in table", NOT_IN_TABLE), (rows[2], 0, "not in table", NOT_IN_TABLE)]
    for row, col, text, detail in cases:
        bad = good[col].copy()
        bad[row] = l1[(idx[row] + 1) % N] if detail == DIFFERENT_ROWS else absent  # in table 2, but at another index
        bufs[col].upload(bad)
        _expect_lookup_error(gpk, bufs, theta, text)
        assert _findings(gpk, bufs) == (1, [(STATIC, 0, row, detail)]), (col, row, text)
        bufs[col].upload(good[col])
        f, m = _round1(gpk, bufs, theta, 1, n, N)
        assert np.array_equal(m[0], want_m)
    # one of each kind at once, against the model of the checker
    advice = [[t["wrap"][j] for j in idx[:u]], [t["wrap2"][j] for j in idx[:u]]]
    b0, b1 = good[0].copy(), good[1].copy()
    b1[rows[0]], advice[1][rows[0]] = l1[(idx[rows[0]] + 1) % N], t["wrap2"][(idx[rows[0]] + 1) % N]
    b1[rows[1]], advice[1][rows[1]] = absent, M.absent_values(N)["head"]
    b0[rows[2]], advice[0][rows[2]] = absent, M.absent_values(N)["head"]
    bufs[0].upload(b0)
    bufs[1].upload(b1)
    want = (3, [(STATIC, 0, rows[0], DIFFERENT_ROWS), (STATIC, 0, rows[1], NOT_IN_TABLE), (STATIC, 0, rows[2], NOT_IN_TABLE)])
    assert _model_findings(k, lookups, advice, dict(wrap=t["wrap"], wrap2=t["wrap2"])) == want
    assert _findings(gpk, bufs) == want
    assert "row 0: the values are on different table rows" in str(gpk.check_witness(bufs)[1][0])
    for buf in bufs:
        buf.free()


@pytest.mark.parametrize("N,src,dst", [(512, 0, 511), (512, 255, 256), (64, 0, 1)], ids=["two_blocks", "block_edge", "adjacent"])
def test_duplicates_inside_a_cluster_are_refused(ctx, env, N, src, dst):
    """Entry `dst` replaced by a copy of entry `src` in a table that is one cluster: the insert that comes second walks the
    cluster up to its twin.  (512, 0, 511): the twins are inserted by different blocks."""
    from sha2_on_cq_halo2_amd import CqError, StaticTable

    _, limbs = env.table(N, "wrap")  # the same table without the copy builds
    dup = limbs.copy()
    dup[dst] = dup[src]
    with pytest.raises(CqError) as e:
        StaticTable.setup_from_toxic_waste(ctx, dup, env.s)
    assert e.value.code == -1 and "not unique" in str(e.value), str(e.value)
