"""The model behind the G2 MSM edge tests (tests/g2_msm_model.py), held to what it promises -- no GPU needed: the routing
table (which n gives which window width, how many windows and buckets, how many lanes per window in the reduction, which
tree passes, how many bucket-sum levels) is written out here, so a change of a threshold in csrc/msm_g2.hip shows up; the
edge scalars leave no carry after the top window at any width; and every scalar family of
tests/test_g2_msm_edges_gpu.py produces the bucket lengths, digits and equal or opposite partial sums it is named for."""
import pytest

from oracle import bn254 as B
from tests import g2_msm_model as G
from tests import msm_digits_model as D

WIDTHS = list(range(4, 17))

# c: (smallest n, W, M, G, tree passes)
ROUTING = {
    4: (1, 64, 8, 1, []),
    5: (512, 51, 16, 1, []),
    6: (1024, 43, 32, 2, [2]),
    7: (2048, 37, 64, 4, [4]),
    8: (4096, 32, 128, 8, [8]),
    9: (8192, 29, 256, 16, [16]),
    10: (16384, 26, 512, 32, [16, 2]),
    11: (32768, 24, 1024, 64, [16, 4]),
    12: (65536, 22, 2048, 128, [16, 8]),
    13: (131072, 20, 4096, 256, [16, 16]),
    14: (262144, 19, 8192, 512, [16, 16, 2]),
    15: (524288, 17, 16384, 1024, [16, 16, 4]),
    16: (1048576, 16, 32768, 2048, [16, 16, 8]),
}


def _nonzero(ds):
    return [(w, d) for w, d in enumerate(ds) if d]


# ---- routing ---------------------------------------------------------------------------------------------------------------

def test_constants_as_the_source_states_them():
    assert (G.G2_S1, G.G2_S, G.G2_RED, G.G2_MAX_LEVELS) == (32, 16, 16, 8)
    assert (G.LG_LOW, G.C_MIN, G.LG_HIGH, G.C_MAX, G.LG_SHIFT) == (8, 4, 20, 16, 4)


@pytest.mark.parametrize("c", WIDTHS)
def test_routing_table(c):
    n, W, M, lanes, passes = ROUTING[c]
    assert G.smallest_n(c) == n and G.window_bits(n) == c
    if c > 4:
        assert G.window_bits(n - 1) == c - 1
    assert G.window_bits(2 * n - 1) == c
    assert (D.windows(c), 1 << (c - 1)) == (W, M)
    r, g, p = G.reduce_shape(c)
    assert (r, g, p) == (min(16, M), lanes, passes) and r * g == M
    prod = 1
    for s in p:
        prod *= s
    assert prod == g
    assert G.window_bits(G.edges_n(c)) == c


def test_widths_at_the_ends():
    assert [G.window_bits(n) for n in (1, 2, 255, 256, 511)] == [4] * 5
    assert [G.window_bits(n) for n in ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 21, 1 << 24, (1 << 31) - 1)] == [15, 16, 16, 16, 16, 16]
    assert W_times_c_255() == [5, 15]


def W_times_c_255():
    """the widths whose top window ends at bit 254 exactly"""
    return [c for c in WIDTHS if D.windows(c) * c == 255]


def test_level_counts_at_every_threshold():
    assert [G.levels(n) for n in (32, 33, 512, 513, 8192, 8193, 131072, 131073, 1 << 20)] == [1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert [G.levels(n) for n in G.LEVEL_SIZES] == [1, 2, 2, 3, 3, 4, 4, 5]
    assert G.levels(1) == 1 and G.levels((1 << 31) - 1) == 8


def test_lane_edge_digits():
    assert G.lane_edge_digits(4) == [1, 7, 8] and G.lane_edge_digits(5) == [1, 15, 16]   # one lane: R = M
    assert G.lane_edge_digits(6) == [1, 16, 17, 31, 32]                                    # two lanes
    assert G.lane_edge_digits(10) == [1, 16, 17, 496, 497, 511, 512]
    for c in WIDTHS:
        r, g, _ = G.reduce_shape(c)
        M = 1 << (c - 1)
        ds = G.lane_edge_digits(c)
        assert ds == sorted(set(ds)) and ds[0] == 1 and ds[-1] == M
        lanes = {(d - 1) // r for d in ds}
        assert lanes == {0, g - 1} | ({1, g - 2} if g > 1 else set())


# ---- edge scalars ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS)
def test_edge_scalars_leave_no_carry_after_the_top_window(c):
    M = 1 << (c - 1)
    W = D.windows(c)
    for v in D.edge_values(c):
        assert 0 <= v < D.R
        ds, carry = D.digits(v, c)
        assert carry == 0 and len(ds) == W and all(-M < d <= M for d in ds)
        assert sum(d << (c * w) for w, d in enumerate(ds)) == v
    # r - 1 has the largest raw top window of all scalars: even with a carry coming in it stays positive.  It stays below M
    # too, so in the top window "M stays positive" never decides anything: recoding a digit M as -M with a carry gives the
    # same sum in every window below (the carry is added one window up), and the top window never holds one
    top = (D.R - 1) >> (c * (W - 1))
    assert top + 1 < M
    if c == 15:
        assert top == 12388
    assert 2 * len(D.edge_values(c)) <= G.edges_n(c)


# ---- the families of the GPU tests ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [4, 6, 10, 13, 14])
def test_one_digit_case_touches_one_bucket_per_row(c):
    assert G.reduce_shape(c)[1] == {4: 1, 6: 2, 10: 32, 13: 256, 14: 512}[c]
    n, rows = G.one_digit_case(c)
    keys = G.lane_edge_keys(c)
    J = D.below_top(c)
    assert G.window_bits(n) == c and len(rows) == len(keys)
    assert {(w, d) for w in range(J) for d in G.lane_edge_digits(c)} <= set(keys) and any(w == J for w, _ in keys)
    assert min(rows) == 0 and max(rows) == n - 1 and (n - 1) // G.SCATTER_BLOCK == (n + G.SCATTER_BLOCK - 1) // G.SCATTER_BLOCK - 1
    assert len({r // G.SCATTER_BLOCK for r in rows}) > 1
    seen = []
    for row in sorted(rows):
        (key,) = _nonzero(D.digits(rows[row], c)[0])
        seen.append(key)
    assert seen == keys


@pytest.mark.parametrize("n", [32, 33, 512, 513, 8192, 8193])
def test_one_scalar_on_every_row_fills_one_bucket_per_window(n):
    """(the two largest sizes of the GPU test differ only in n: left out here for the time a Python walk takes)"""
    k = 0x1F2E3D4C5B6A79880123456789ABCDEF
    walk = G.Walk([k] * n, list(range(1, n + 1)))
    assert walk.L == G.levels(n)
    assert walk.bucket_len and set(walk.bucket_len.values()) == {n}
    last = n % (G.G2_S1 * G.G2_S ** (walk.L - 2)) if walk.L > 1 else 0  # entries under the last lane of the last level
    assert (last == 1) == (n in (33, 513, 8193))      # just past a threshold: one entry carried up alone
    assert walk.value == k * n * (n + 1) // 2 % D.R


def test_mixed_case_has_short_ragged_and_exact_buckets():
    rng = B.Xoshiro256ss(0x62E0)
    ks = [B.fr_random(rng) for _ in range(len(G.MIXED_GROUPS) + 1)]
    sc = G.mixed_case(ks)
    assert len(sc) == G.MIXED_N == 8193 and G.levels(len(sc)) == 4
    walk = G.Walk(sc, list(range(1, len(sc) + 1)))
    lens = set(walk.bucket_len.values())
    assert set(G.MIXED_GROUPS) | {G.MIXED_N - sum(G.MIXED_GROUPS)} <= lens
    # a bucket of one entry stays one item on every level; 33 and 513 leave a ragged last lane on levels 1 / 2
    one = next(b for b, m in walk.bucket_len.items() if m == 1)
    assert [len(level[one]) for level in walk.lane_sums] == [1, 1, 1, 1]
    b33 = next(b for b, m in walk.bucket_len.items() if m == 33)
    assert [len(level[b33]) for level in walk.lane_sums] == [2, 1, 1, 1]
    b513 = next(b for b, m in walk.bucket_len.items() if m == 513)
    assert [len(level[b513]) for level in walk.lane_sums] == [17, 2, 1, 1]
    assert walk.value == sum(k * (i + 1) for i, k in enumerate(sc)) % D.R


def test_level_one_special_cases():
    k, e, q = 0x1234567, 0xABCDEF, 0x13579B
    walk = G.Walk([k] * 64, [e] * 64)                # one base 64 times: the second entry of each lane doubles
    assert walk.c == 4 and walk.L == 2
    nz = len(_nonzero(D.digits(k, 4)[0]))
    assert walk.events[("level1", "double")] == 2 * nz and walk.events[("levels", "double")] == nz
    assert walk.value == 64 * k * e % D.R
    walk = G.Walk([k] * 3, [e, D.R - e, q])           # P, -P, Q: cancels, then Q lands on the identity
    assert walk.events[("level1", "cancel")] == nz and walk.value == k * q % D.R
    walk = G.Walk([k, k], [e, D.R - e])
    assert walk.value == 0


@pytest.mark.parametrize("n", [1024, 8192])
@pytest.mark.parametrize("kind", G.LONG_KINDS)
def test_long_cases_double_and_cancel_above_level_one(kind, n):
    k = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A
    c = G.window_bits(n)
    assert (c, G.levels(n), G.reduce_shape(c)[1]) == {1024: (6, 3, 2), 8192: (9, 3, 16)}[n]
    sc, signs, identity = G.long_case(kind, n, k)
    walk = G.Walk(sc, signs)
    ev = walk.events
    assert (walk.value == 0) == identity
    level1 = {v for sums in walk.lane_sums[0].values() for v in sums}
    if kind == "alternate":
        assert level1 == {0} and ev[("level1", "cancel")] > 0
    elif kind == "runs":                                          # equal entries inside a lane, opposite lane sums
        assert level1 == {32, D.R - 32}
        assert ev[("level1", "double")] > 0 and ev[("level1", "cancel")] == 0 and ev[("levels", "cancel")] > 0
        assert {v for sums in walk.lane_sums[1].values() for v in sums} == {0}
    else:
        w, d = {"pair-low": (0, 1), "pair-high": (D.below_top(c) - 1, (1 << (c - 1)) - 1)}[kind]
        assert set(walk.bucket_len) == {(w, d), (w + 1, 1)} and walk.bucket_len[(w + 1, 1)] == n // 2
        assert set(walk.lane_sums[0][(w, d)]) == {0} and set(walk.lane_sums[0][(w + 1, 1)]) == {32}
        assert ev[("levels", "double")] > 0
        assert walk.value == (n // 2 << (c * (w + 1))) % D.R
        if n == 8192:   # 8 sums of 512 P meet on level 3 as well
            assert len(walk.lane_sums[1][(w + 1, 1)]) == 8 and set(walk.lane_sums[1][(w + 1, 1)]) == {512}


@pytest.mark.parametrize("c", [6, 10])
def test_window_reduction_cancels_at_the_intended_step_only(c):
    n = G.smallest_n(c)
    r, lanes, _ = G.reduce_shape(c)
    first, last = G.reduce_cancel_digits(c)
    assert (first - 1) // r == 0 and (last - 1) // r == lanes - 1 and lanes > 1
    for d in (first, last):
        for w in (0, D.below_top(c) // 2):
            (k1, m1), (k2, m2) = G.reduce_cancel_case(c, w, d)
            assert _nonzero(D.digits(k1, c)[0]) == [(w, d)] and _nonzero(D.digits(k2, c)[0]) == [(w, d - 1)]
            sc, logs = [0] * n, [1] * n
            sc[7], logs[7] = k1, m1
            sc[n - 2], logs[n - 2] = k2, m2
            walk = G.Walk(sc, logs)
            assert walk.c == c and walk.cancel_steps == [(w, d - 1)]
            assert walk.events[("reduce-acc", "cancel")] == 1
            assert walk.value == (2 - d) * (1 << (c * w)) % D.R


@pytest.mark.parametrize("c,n", [(4, 2), (6, 1024)])
def test_fold_cases_add_equal_and_opposite_window_sums(c, n):
    for sign, kind in ((1, "double"), (-1, "cancel")):
        pairs = G.fold_case(c, sign)
        sc, logs = [0] * n, [1] * n
        (sc[0], logs[0]), (sc[n - 1], logs[n - 1]) = pairs
        walk = G.Walk(sc, logs)
        assert walk.c == c
        assert walk.window_sums[:2] == [sign * (1 << c) % D.R, 1] and not any(walk.window_sums[2:])
        assert walk.events[("fold", kind)] == 1 and sum(walk.events.values()) == 1
        assert walk.value == (2 << c if sign == 1 else 0)
