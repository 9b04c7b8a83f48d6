"""The model behind the MSM edge tests (tests/msm_digits_model.py), held to what it promises -- no GPU needed: every crafted
scalar is canonical, recodes with a final carry of 0 into digits that spell its value, and produces the digit event it is
named for (counted, so that a later edit of the families cannot quietly lose an edge); and the routing table says which
sorting front each launch of tests/test_msm_edges_gpu.py reaches."""
import pytest

from tests import msm_digits_model as D

WIDTHS = list(range(2, 21))


def _nonzero(ds):
    return [(w, d) for w, d in enumerate(ds) if d]


@pytest.mark.parametrize("c", WIDTHS)
def test_every_family_is_canonical_and_its_digits_spell_the_value(c):
    M = 1 << (c - 1)
    fams = D.edge_scalars(c)
    assert len(fams) == 4 + len(D.single_keys(c)) + len(D.cancel_keys(c)) + len(D.CONSTANTS)
    for name, vals in fams.items():
        for v in vals:
            assert 0 <= v < D.R, name
            ds, carry = D.digits(v, c)
            assert carry == 0, name
            assert len(ds) == D.windows(c) and all(-M < d <= M for d in ds), name
            assert sum(d << (c * w) for w, d in enumerate(ds)) == v, name
    assert D.edge_values(c) == [v for vals in fams.values() for v in vals]


@pytest.mark.parametrize("c", WIDTHS)
def test_carry_families_produce_their_events(c):
    M = 1 << (c - 1)
    J = D.below_top(c)
    fams = D.edge_scalars(c)
    assert J >= 2 and c * J <= 253 < c * (J + 1)

    (v,) = fams["all_M"]  # J digits equal to M (the last bucket, not negated), none negative
    ds, _ = D.digits(v, c)
    assert ds[:J] == [M] * J and not any(ds[J:]) and D.carries_on_zero(v, c) == 0

    (v,) = fams["all_M_plus_1"]  # every digit negative, the carry chain ends as +1 in the top window
    ds, _ = D.digits(v, c)
    assert ds[:J] == [-(M - 1)] + [-(M - 2)] * (J - 1) and ds[J] == 1 and not any(ds[J + 1:])
    if c > 2:
        assert all(d < 0 for d in ds[:J])
    else:  # M + 1 = 2^c - 1: the width at which this family is all_full
        assert v == fams["all_full"][0]

    (v,) = fams["all_full"]  # one digit -1, then J - 1 zero digits that still carry, then +1
    ds, _ = D.digits(v, c)
    assert ds[0] == -1 and ds[1:J] == [0] * (J - 1) and ds[J] == 1 and not any(ds[J + 1:])
    assert D.carries_on_zero(v, c) == J - 1

    (v,) = fams["one_then_M_minus_1"]  # a digit that becomes M only through the carry
    ds, _ = D.digits(v, c)
    assert ds[0] == -(M - 1) and ds[1] == M and not any(ds[2:])
    assert (v >> c) & ((1 << c) - 1) == M - 1


@pytest.mark.parametrize("c", WIDTHS)
def test_single_and_cancel_families_touch_one_bucket_at_a_time(c):
    M = 1 << (c - 1)
    J = D.below_top(c)
    fams = D.edge_scalars(c)
    keys = D.single_keys(c)
    # every window below the top one with every d, the last bucket (d = M) included; above, whatever stays below r
    for w in range(J):
        for d in {1, M - 1, M}:
            assert (w, d) in keys
    assert any(w == J for w, _ in keys)
    for w, d in keys:
        (v,) = fams["single(%d,%d)" % (w, d)]
        assert _nonzero(D.digits(v, c)[0]) == [(w, d)]
    ck = D.cancel_keys(c)
    assert {w for w, _ in ck} == {0, J // 2, J - 1} and {d for _, d in ck} == {1, M - 1}
    for w, d in ck:
        assert 0 < d < M  # d = M would give b == a: no cancellation
        a, b = fams["cancel(%d,%d)" % (w, d)]
        assert _nonzero(D.digits(a, c)[0]) == [(w, d)]
        assert _nonzero(D.digits(b, c)[0]) == [(w, -d), (w + 1, 1)]
        assert a + b == 1 << (c * (w + 1))


@pytest.mark.parametrize("c", WIDTHS)
def test_constants_cover_limb_boundaries_and_both_signs(c):
    fams = D.edge_scalars(c)
    for name in ("0", "1", "2", "r-1", "r-2", "2^253+1", "2^128-1"):
        assert "const:" + name in fams
    for j in range(1, 8):
        assert fams["const:2^%d-1" % (32 * j)] == ((1 << (32 * j)) - 1,) and fams["const:2^%d" % (32 * j)] == (1 << (32 * j),)
    assert not any(D.digits(0, c)[0])
    assert D.digits(D.R - 1, c)[0][-1] != 0 or D.windows(c) * c - c >= 254  # r - 1 reaches the top window
    # a window that straddles two 32-bit limbs with set bits on both sides of the boundary
    straddling = [w for w in range(D.windows(c)) if (c * w) % 32 + c > 32 and c * w + c <= 256]
    if straddling:
        hit = 0
        for v in D.edge_values(c):
            for w in straddling:
                edge = 32 * ((c * w) // 32 + 1)
                lo = (v >> (c * w)) & ((1 << (edge - c * w)) - 1)
                hi = (v >> edge) & ((1 << (c * w + c - edge)) - 1)
                hit += bool(lo and hi)
        assert hit > 0
    # both signs occur (the sign travels in bit 31 of a sorted entry)
    alld = [d for v in D.edge_values(c) for d in D.digits(v, c)[0]]
    assert min(alld) < 0 < max(alld) and max(alld) == 1 << (c - 1)


def test_model_digits_on_small_cases():
    # c = 2, M = 2: raw digits 2, 1 -> 2 stays (not negated), 1 stays
    assert D.digits(0b0110, 2)[0][:3] == [2, 1, 0]
    # raw 3 > M -> -1 and a carry; 3 + 1 = 4 = 2^c -> 0 and a carry; then +1
    assert D.digits(0b1111, 2)[0][:4] == [-1, 0, 1, 0]
    assert D.carries_on_zero(0b1111, 2) == 1
    # c = 15: the examples the families were designed on
    f = D.edge_scalars(15)
    assert D.digits(f["all_M"][0], 15)[0].count(16384) == 16
    ds = D.digits(f["all_full"][0], 15)[0]
    assert [d for d in ds if d < 0] == [-1] and ds.count(0) == 15 and ds[16] == 1


def test_routing_table_the_gpu_tests_rely_on():
    assert D.MSM_TABLE_C_MIN == 8 and D.MSM_TABLE_C_MAX == 20
    for c in range(2, 16):  # plain launches with a forced window
        assert D.front_of(False, c) == "digits"
        assert D.plain_path(600, c) == ("digits", c)
    for c in range(8, 15):
        assert D.windows(c) > D.PSC_MAX_WIN and D.front_of(True, c) == "digits"
    assert D.front_of(True, 15) == "part"
    assert D.front_of(True, 16) == "part-wide" and D.front_of(True, 17) == "part-wide"
    for c in (18, 19, 20):
        assert D.front_of(True, c) == "part-refine"
    # every table width behind the partition sort has its compile-time form of the first pass (the run-time form is what a
    # width without one would take)
    assert D.PART_SPECIALISED == [(c, D.windows(c)) for c in range(15, 21)]
    assert (D.PART_BITS, D.PART_BITS_WIDE) == (7, 8)


def test_driver_overview_quotes_the_layout():
    """msm.hip's overview quotes the layout's routing lines for the reader of the driver: the quotation says what msm_layout.hpp says"""
    assert D.routing_constants(D._HIP) == D.routing_constants(D._LAYOUT)


def test_short_cut_over_and_automatic_widths():
    assert D.MSM_SHORT_MAX == 16384
    assert D.plain_path(D.MSM_SHORT_MAX) == ("short", 8)
    assert D.plain_path(D.MSM_SHORT_MAX + 1) == ("digits", 10)
    assert D.plain_path((1 << 15) + 1) == ("digits", 15)
    # the older edge tests of tests/test_msm_gpu.py: all on the short kernel today
    for n in (300, 200, 512, 4096, 6000):
        assert D.plain_path(n)[0] == "short"
    assert D.plain_path(6000, 9) == ("digits", 9) and D.plain_path(700, 2) == ("digits", 2)
