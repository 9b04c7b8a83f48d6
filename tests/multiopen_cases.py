"""Case tables of tests/test_multiopen_shapes_cpu.py and tests/test_multiopen_shapes_gpu.py: polynomials, queries and
scripted challenges for cq_multiopen_dev at the sizes, counts and point sets where its parts change path.  The CPU file
pins the oracles (oracle.shplonk.shplonk_prove, stages_helpers.gwc_prove) on every table from the verifier side; the
GPU file compares the device with those oracles on the same tables.

A case id is a tuple; `build(case_id)` gives the case (cached: the tables are read-only).

Launch counts, from prover_support.hip / poly.hip: eval_many evaluates 40 polynomials per launch (EVAL_MAX_BATCH) at
ceil(log_4096(len)) levels; lincomb_many takes 40 terms in its first launch and 39 new ones in each later launch
(LINCOMB_MAX = 40, `out` fed back as term 0), and lincomb_kernel reduces a launch's terms in groups of 6."""
import functools
import itertools
import random
from typing import NamedTuple

from oracle import bn254 as B
from oracle.poly import eval_polynomial

P = B.R_MOD


def key_secret(k):
    """The toxic waste of the key that the GPU file builds for k (as test_stages_gpu._cq_env draws it)."""
    return B.fr_random(B.Xoshiro256ss(700 + k))


class Case(NamedTuple):
    k: int
    polys: dict      # key -> coefficients, at most n
    queries: list    # (key, point, evaluation), in the order the opener receives them
    script: tuple    # (y, v, u): SHPLONK squeezes all three in this order, GWC squeezes v alone
    shplonk_refuses: bool = False


def _fr(rnd):
    return rnd.getrandbits(320) % P


def _poly(rnd, length):
    return [_fr(rnd) for _ in range(length)]


def _case(k, polys, kp, rnd, yv=None, shplonk_refuses=False):
    y, v, u = _fr(rnd), _fr(rnd), _fr(rnd)
    if yv is not None:
        y, v = yv
    assert all(u != pt for _, pt in kp)  # the reference asserts on a zero z_0 difference: never scripted
    queries = [(key, pt, eval_polynomial(polys[key], pt)) for key, pt in kp]
    return Case(k, polys, queries, (y, v, u), shplonk_refuses)


# ---- 1. poly_kate_division's threshold (block-scan path from 4096 coefficients on) and block_eval_kernel's second level
THRESHOLD = [("threshold", 12), ("threshold", 13)]


def _threshold(k):
    """Polynomial 0 at all 8 points: SHPLONK's div_by_vanishing divides at lengths n .. n - 7 (k = 12: the first
    division on the block path with 4 blocks, the other seven recursive; k = 13: all on the block path, 8 blocks whose
    last is partial), ping-ponging between its two buffers.  Polynomials 1 and 2 at the same two points in opposite
    order: one rotation set.  The rest at one point each, sharing points: at k = 13 the evaluations at x0 mix second-level
    lengths 2, 2, 1 (n, 4097, 4096) and those at x3 mix 2, 1, 1 (n, 4095, 257)."""
    n = 1 << k
    rnd = random.Random(1200 + k)
    lens = (n, n, n - 1, 4097 if k == 13 else n - 2, 4096, 4095, 257, 1)
    polys = {i: _poly(rnd, ln) for i, ln in enumerate(lens)}
    x = [_fr(rnd) for _ in range(8)]
    kp = [(0, pt) for pt in x] + [(1, x[1]), (1, x[2]), (2, x[2]), (2, x[1]), (3, x[0]), (4, x[0]), (5, x[3]), (6, x[3]), (7, x[5])]
    return _case(k, polys, kp, rnd)


# ---- 2. count boundaries: m polynomials at one point
# m polynomials make m lincomb terms for GWC and m + 1 for SHPLONK (its remainder term in the quotient, its h_x term in
# the linearisation), so
#   m        1  5  6  7  12  13  39  40  41  78  79  80  81
#   GWC      terms = m:      groups of 6 per launch 1 1 1 2 2 3; launches 1 up to m = 40, 2 up to 79, 3 from 80
#   SHPLONK  terms = m + 1:  groups 1 1 2 2 3 3;                 launches 1 up to m = 39, 2 up to 78, 3 from 79
#   eval_many launches: 1 up to m = 40, 2 up to 80, 3 for 81.
# Lengths cycle through n, n - 1, 7, 1, so every group of 6 skips terms at the high coefficients.
COUNTS = [("count", 5, m) for m in (1, 5, 6, 7, 12, 13, 39, 40, 41, 78, 79, 80, 81)] + [("count", 13, 41)]  # k = 13: two batches at two levels


def _count(k, m):
    n = 1 << k
    rnd = random.Random(100 * k + m)
    polys = {i: _poly(rnd, (n, n - 1, 7, 1)[i % 4]) for i in range(m)}
    x0 = _fr(rnd)
    return _case(k, polys, [(i, x0) for i in range(m)], rnd)


# ---- 3. SHPLONK's limits: at most 64 rotation sets of at most 8 points
SET_LIMITS = [("sets", "64"), ("sets", "65"), ("sets", "9-points")]


def _subsets():
    small = [c for size in range(1, 8) for c in itertools.combinations(range(8), size)]
    return small[:63] + [tuple(range(8))], small[63]


def _sets(kind):
    """"64": 64 polynomials over 8 points, each with a point set of its own -- the first 63 subsets of at most 7 points in
    itertools.combinations order, the full set last, so the last set's 8 remainder coefficients are the last 8 elements
    of the opener's scratch.  "65": one more distinct subset.  "9-points": one polynomial at 9 points."""
    k = 5
    n = 1 << k
    rnd = random.Random(64)
    if kind == "9-points":
        polys = {0: _poly(rnd, n)}
        return _case(k, polys, [(0, _fr(rnd)) for _ in range(9)], rnd, shplonk_refuses=True)
    subsets, extra = _subsets()
    if kind == "65":
        subsets = subsets + [extra]
    polys = {i: _poly(rnd, (n, n - 1, 7, 1)[i % 4]) for i in range(len(subsets))}
    x = [_fr(rnd) for _ in range(8)]
    kp = [(i, x[j]) for i, sub in enumerate(subsets) for j in sub]
    return _case(k, polys, kp, rnd, shplonk_refuses=kind == "65")


# ---- 4. challenge and operand edges: y, v in {0, 1, p - 1} against coefficients p - 1
EDGE_SCRIPTS = {"minus-one": (P - 1, P - 1), "zero-one": (0, 1), "one-zero": (1, 0), "random": None}
EDGES = [("edge", k, name) for k in (5, 12) for name in EDGE_SCRIPTS]


def _edge(k, name):
    """40 polynomials of n coefficients p - 1 (equal contents, 40 buffers), one of zeros, one [1].  At x0, in this order:
    A_0, zeros, A_1 .. A_39, [1]; A_39 and [1] also at x1.  GWC's first launch at x0 then holds 40 terms, 39 of them
    p - 1 throughout; SHPLONK's first set {x0} has 40 members (41 terms), its second {x0, x1} two.  The zeros polynomial
    in second place keeps the alternating sum for y or v = p - 1 from cancelling (the A's get the exponents 0, 2 .. 40),
    so no commitment is the identity; the CPU file asserts that for every script."""
    n = 1 << k
    rnd = random.Random(400 + k)
    a = [P - 1] * n
    polys = {i: a for i in range(40)}
    polys["zeros"], polys["one"] = [0] * n, [1]
    x0, x1 = _fr(rnd), _fr(rnd)
    kp = [(0, x0), ("zeros", x0)] + [(i, x0) for i in range(1, 40)] + [(39, x1), ("one", x0), ("one", x1)]
    return _case(k, polys, kp, rnd, yv=EDGE_SCRIPTS[name])


# ---- 5. the same polynomial at the same point twice: GWC counts the query twice, SHPLONK's sets count it once
DUPLICATE = [("duplicate",)]
SMALL = ("small",)  # the valid call after a refusal


def _few(seed, duplicate):
    k = 5
    n = 1 << k
    rnd = random.Random(seed)
    polys = {0: _poly(rnd, n), 1: _poly(rnd, n - 1), 2: _poly(rnd, 7)}
    x0, x1 = _fr(rnd), _fr(rnd)
    kp = [(0, x0), (1, x0), (0, x0), (2, x1), (1, x1)] if duplicate else [(0, x0), (1, x0), (1, x1)]
    return _case(k, polys, kp, rnd)


ALL = THRESHOLD + COUNTS + SET_LIMITS + EDGES + DUPLICATE + [SMALL]


@functools.lru_cache(maxsize=None)
def build(case_id):
    kind, args = case_id[0], case_id[1:]
    return {"threshold": _threshold, "count": _count, "sets": _sets, "edge": _edge, "duplicate": lambda: _few(55, True),
            "small": lambda: _few(56, False)}[kind](*args)


def case_name(case_id):
    return "-".join(str(part) for part in case_id)
