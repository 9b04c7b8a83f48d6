"""CPU model of the G2 Pippenger (csrc/msm_g2.hip): what the kernels do for a given n -- the window width, the number of
bucket-sum levels, the shape of the window reduction and of its tree -- and a walk through the whole algorithm over
discrete logs, which says which additions meet equal or opposite operands.  The recoding is the G1 engine's (a digit of
exactly M stays positive), so the digits and the crafted scalars come from tests/msm_digits_model.py.
tests/test_g2_msm_model_cpu.py holds the model to a routing table written out there, and the scalar families below to the
events they are named for; tests/test_g2_msm_edges_gpu.py runs them through the kernels against the C oracle.

The constants are read from the source, so a change of a threshold there shows up in the CPU test's routing table."""
import os
import re
from collections import Counter

from tests.msm_digits_model import R, below_top, cancel, digits, edge_scalars, edge_values, single, windows  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HIP = open(os.path.join(ROOT, "sha2_on_cq_halo2_amd", "csrc", "msm_g2.hip")).read()


def _const(name):
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, _HIP).group(1))


G2_S1 = _const("G2_S1")                  # entries per lane, level 1
G2_S = _const("G2_S")                    # partial sums per lane, levels >= 2 and the window tree
G2_RED = _const("G2_RED")                # buckets per lane of the window reduction
G2_MAX_LEVELS = _const("G2_MAX_LEVELS")
# g2_msm_window_bits: lg = floor(log2 n); return lg < LG_LOW ? C_MIN : lg > LG_HIGH ? C_MAX : lg - LG_SHIFT
_body = re.search(r"uint32_t g2_msm_window_bits\(size_t n\) \{(.*?)\n\}", _HIP, re.S).group(1)
assert re.search(r"while \(\(\(size_t\)1 << \(lg \+ 1\)\) <= n\) lg\+\+;", _body)
LG_LOW, C_MIN, LG_HIGH, C_MAX, LG_SHIFT = (int(g) for g in re.search(
    r"return lg < (\d+) \? (\d+) : lg > (\d+) \? (\d+) : lg - (\d+);", _body).groups())
SCATTER_BLOCK = 256                      # threads per block of the canon / count / scatter kernels
assert len(re.findall(r"<<<nb, %d, 0, st>>>" % SCATTER_BLOCK, _HIP)) == 3 and "nb = (n + 255) / 256" in _HIP


def window_bits(n):
    """g2_msm_window_bits: the width is a function of n alone"""
    lg = max(n, 1).bit_length() - 1
    return C_MIN if lg < LG_LOW else C_MAX if lg > LG_HIGH else lg - LG_SHIFT


def levels(n):
    """L: the divisor D_L = G2_S1 * G2_S^(L-1) grows until it covers a bucket holding all n entries"""
    d, L = G2_S1, 0
    while True:
        L += 1
        if d >= n or L == G2_MAX_LEVELS:
            return L
        d *= G2_S


def reduce_shape(c):
    """(R, G, [group sizes of the tree passes]): R buckets per lane of the window reduction, G lanes per window"""
    M = 1 << (c - 1)
    r = min(G2_RED, M)
    G = M // r
    passes, g = [], G
    while g > 1:
        s = min(G2_S, g)
        passes.append(s)
        g //= s
    return r, G, passes


def smallest_n(c):
    """the smallest n whose width is c"""
    return 1 if c == C_MIN else 1 << (c + LG_SHIFT)


def lane_edge_digits(c):
    """the digits around the lane boundaries of g2_window_reduce_kernel: the first lane's two ends (1, R), the first
    bucket of the second lane, the last bucket of the lane before the last, and the last lane's first, second-last and top
    bucket (d = M)"""
    M = 1 << (c - 1)
    r = min(G2_RED, M)
    return sorted(d for d in {1, r, r + 1, M - r, M - r + 1, M - 1, M} if 1 <= d <= M)


def lane_edge_keys(c):
    """every (w, d), d in lane_edge_digits(c), whose scalar d * 2^(cw) is below r"""
    return [(w, d) for w in range(windows(c)) for d in lane_edge_digits(c) if single(c, w, d) < R]


# ---- the algorithm over discrete logs ------------------------------------------------------------------------------

class Walk:
    """g2_msm over bases given by their discrete logs (base i = [logs[i]]_2, 0 = the identity), entries of a bucket in
    row order (the kernels store them in order of arrival: the sum does not depend on it, which operands meet does).
    Every addition goes through `add`, which counts under (stage, "double") / (stage, "cancel") the ones whose operands
    are equal / opposite.  Kept after the run: `lane_sums[l][(w, d)]`, the partial sums of bucket d of window w after
    level l + 1; `window_sums`; `events`; `value`, the log of the result."""

    def __init__(self, scalars, logs):
        n = len(scalars)
        assert n == len(logs) and n > 0
        self.n, self.c = n, window_bits(n)
        self.W, self.M, self.L = windows(self.c), 1 << (self.c - 1), levels(n)
        self.events = Counter()
        self.cancel_steps = []          # (w, d) of every cancelling `acc += run` of the window reduction
        buckets = {}
        for i, k in enumerate(scalars):
            if not k:
                continue
            ds, carry = digits(k, self.c)
            assert carry == 0
            for w, d in enumerate(ds):
                if d:
                    buckets.setdefault((w, abs(d)), []).append(logs[i] % R if d > 0 else -logs[i] % R)
        self.bucket_len = {b: len(v) for b, v in buckets.items()}
        self.lane_sums = []
        size = G2_S1
        for l in range(self.L):
            stage = "level1" if l == 0 else "levels"
            buckets = {b: [self._sum(stage, v[j:j + size]) for j in range(0, len(v), size)] for b, v in buckets.items()}
            self.lane_sums.append(buckets)
            size = G2_S
        assert all(len(v) == 1 for v in buckets.values())
        r, G, passes = reduce_shape(self.c)
        self.window_sums = []
        for w in range(self.W):
            lanes = []
            for g in range(G):
                run = acc = 0
                for d in range((g + 1) * r, g * r, -1):
                    if (w, d) in buckets:
                        run = self.add("reduce-run", run, buckets[(w, d)][0])
                    before = self.events[("reduce-acc", "cancel")]
                    acc = self.add("reduce-acc", acc, run)
                    if self.events[("reduce-acc", "cancel")] != before:
                        self.cancel_steps.append((w, d))
                k = g * r
                while k:
                    if k & 1:
                        acc = self.add("reduce-offset", acc, run)
                    if k > 1:
                        run = 2 * run % R
                    k >>= 1
                lanes.append(acc)
            for s in passes:
                lanes = [self._sum("tree", lanes[j:j + s]) for j in range(0, len(lanes), s)]
            assert len(lanes) == 1
            self.window_sums.append(lanes[0])
        acc = 0
        for w in reversed(range(self.W)):
            acc = self.add("fold", acc << self.c, self.window_sums[w])
        self.value = acc

    def add(self, stage, a, b):
        a %= R
        b %= R
        if a and b:
            if a == b:
                self.events[(stage, "double")] += 1
            elif a + b == R:
                self.events[(stage, "cancel")] += 1
        return (a + b) % R

    def _sum(self, stage, vals):
        acc = 0
        for v in vals:
            acc = self.add(stage, acc, v)
        return acc


# ---- the scalar and base families of the GPU tests ------------------------------------------------------------------
# bases as multiples of one point P: +1 / -1 / 0 stand for P, -P and the identity

LONG_KINDS = ["alternate", "runs", "pair-low", "pair-high"]


def long_case(kind, n, k):
    """(scalars, signs, sums_to_identity) of n rows over P and -P, the kinds of test_msm_edges_gpu._long_case on this
    engine's lane sizes:
    "alternate"  P, -P, P, -P, .. under the scalar k: every level-1 lane cancels pair by pair;
    "runs"       G2_S1 times P, G2_S1 times -P, .. under k: level-1 lane sums +32 P and -32 P, which cancel one level up;
    "pair-low", "pair-high"  rows alternate the cancel pair (a, b) of window w: +d and -d of P cancel in bucket d of window
                 w, and n / 2 times +1 in window w + 1 give equal lane sums 32 P, which double one level up."""
    c = window_bits(n)
    assert n % (2 * G2_S1) == 0
    if kind == "alternate":
        return [k] * n, [1 - 2 * (i % 2) for i in range(n)], True
    if kind == "runs":
        return [k] * n, [1 - 2 * (i // G2_S1 % 2) for i in range(n)], True
    w, d = {"pair-low": (0, 1), "pair-high": (below_top(c) - 1, (1 << (c - 1)) - 1)}[kind]
    a, b = cancel(c, w, d)
    return [a, b] * (n // 2), [1] * n, False


def reduce_cancel_case(c, w, d):
    """{row scalar: base multiple} of the window reduction's `acc == -run`: P under digit d and [-2]P under digit d - 1 of
    window w.  Walking down, run = acc = P at bucket d; at bucket d - 1 run becomes -P and `acc += run` cancels; the
    buckets below add -P to an accumulator that starts from the identity.  The sum is (2 - d) 2^(cw) P."""
    r = min(G2_RED, 1 << (c - 1))
    assert d <= 1 << (c - 1) and (d - 1) // r == (d - 3) // r  # d, d - 1 and a bucket below them in one lane
    return [(single(c, w, d), 1), (single(c, w, d - 1), -2)]


def reduce_cancel_digits(c):
    """one d in the first lane of the reduction and one in the last (its top bucket d = M)"""
    return [5, 1 << (c - 1)]


def fold_case(c, sign):
    """[(scalar, base multiple)]: [sign 2^c]P under 1 and P under 2^c -- the host fold doubles window sum 1 c times and
    adds window sum 0, an equal (sign = 1) or opposite (sign = -1) point"""
    return [(1, sign * (1 << c)), (1 << c, 1)]


def edges_n(c):
    """the length at which the edge tests reach width c: the largest n of the narrowest width (its smallest, 1, holds no
    edge set), else the smallest n of the width"""
    return (1 << (LG_LOW + 1)) - 1 if c == C_MIN else smallest_n(c)


def spread_rows(count, n):
    """`count` distinct rows from 0 to n - 1 at even distances: the first block of the 256-thread kernels, the last one
    and those between"""
    assert 2 <= count <= n
    return [j * (n - 1) // (count - 1) for j in range(count)]


def one_digit_case(c):
    """(n, {row: scalar}): one row per (window, lane-edge digit), nothing else"""
    n = edges_n(c)
    keys = lane_edge_keys(c)
    return n, dict(zip(spread_rows(len(keys), n), (single(c, w, d) for w, d in keys)))


LEVEL_SIZES = [32, 33, 512, 513, 8192, 8193, 131072, 131073]   # either side of every change of the level count
MIXED_N = 8193
MIXED_GROUPS = [1, 31, 32, 33, 511, 512, 513, 1025]            # rows per scalar; the rest of MIXED_N under one more


def mixed_case(scalars):
    """per-row scalars of the mixed case: consecutive groups of MIXED_GROUPS rows under scalars[0], scalars[1], .. and the
    remainder under the last one"""
    sizes = MIXED_GROUPS + [MIXED_N - sum(MIXED_GROUPS)]
    assert len(scalars) == len(sizes) and sizes[-1] > 0
    return [k for k, m in zip(scalars, sizes) for _ in range(m)]
